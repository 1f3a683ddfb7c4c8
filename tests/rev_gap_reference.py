"""TEST INFRASTRUCTURE: the cases of the gap-aware reverse-mode gradient kernels and their stored reference.  The reference
itself is ``grad_gap_reference.reference`` (unchanged: Richardson differences of the numpy oracle).  The five ``grad_gap_reference.CASES`` are read
from that module's file; this module names three more - 64-group tracks of a 4-state model, and K = D = 2 and K = D = 3 at frame_len 4 - and keeps
their arrays in a file of their own, tests/golden/rev_gap_reference.npz (same array names), written by running this file.  Not a conftest; imported
by tests/test_emul_rev_gaps.py and tests/test_hip_rev_gaps.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
if __name__ == "__main__":  # run as a script (regenerating the golden file): the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(HERE))

import gap_reference as R  # noqa: E402
import grad_gap_reference as GR  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "rev_gap_reference.npz")
NEW_CASES = [(4, 2, "global1", 4), (4, 2, "globalD", 4), (3, 3, "peak", 4)]  # (S, D, layout, frame_len) of gap_reference.make_case
CASES = list(GR.CASES) + NEW_CASES
ARRAYS = ("ll", "fd", "est", "gfd", "gest")


def golden(case, key):
    """``grad_gap_reference.reference(case, key, golden=True)``: the five old cases from that module's file, the new ones from this module's."""
    if tuple(key) in GR.CASES:
        return GR.reference(case, tuple(key), golden=True)
    with np.load(GOLDEN) as z:
        ref = {a: z[GR._key(tuple(key)) + "." + a] for a in ARRAYS}
    ref["dirs"] = GR.directions(case)
    return ref


def assert_golden_is_current(case, key, ref):
    """``grad_gap_reference.assert_golden_is_current`` for either file: same inputs (LL to 1e-12), same differences up to their own estimates."""
    gold = golden(case, key)
    np.testing.assert_allclose(gold["ll"], ref["ll"], rtol=1e-12, atol=1e-10)
    for a, e in (("fd", "est"), ("gfd", "gest")):
        assert np.all(np.abs(gold[a] - ref[a]) <= 2 * (gold[e] + ref[e]) + 1e-7 * np.abs(ref[a])), (key, a)


if __name__ == "__main__":  # regenerate the golden file
    out = {}
    for key in NEW_CASES:
        ref = GR.reference(R.make_case(*key), key)
        GR.assert_condition("%s" % (key,), ref["gfd"], ref["gest"])
        for a in ARRAYS:
            out[GR._key(key) + "." + a] = ref[a]
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
