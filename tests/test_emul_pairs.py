"""CPU check of the PAIRS instantiations of the fixed-window body (xt_kernel.h) on CPU threads (tests/emul/emul_pairs.cpp) against the pair
reference built from the oracle's pieces (tests/pair_reference.py): the buckets of the GPU test (L = 2, 3, frame_len + 1, frame_len + 2, 14,
40; ragged N) launched longest first through the bucket-descriptor table with min_len 3 and the longest bucket isBL = 0.  Tolerance: the
project's posterior tolerance (tests/test_hip_parity.py, tests/test_hip_gaps.py), 1e-9 absolute; counts against the sum of the pairs over t at
1e-12 * L."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))

import gap_reference as R
import pair_reference as PR
from oracle import oracle_np as O

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

TOL_PRED = 1e-9
# (S, D, layout, frame_len, tracks per block override): every state count; frame_len 2 (S threads per track write S^2 values), 3 and 5 (more
# than one wavefront per track at 3 states); the per-peak and affine errors; D = 3 with K = 3 (globalD); two tracks per block.  4 states at
# frame_len >= 5 (256 CPU threads per track in lock-step) are left to the GPU test.
_CASES = [(2, 2, "global1", 2, 0), (3, 1, "global1", 2, 0), (4, 2, "peak", 2, 0), (2, 2, "affine", 3, 2), (3, 3, "globalD", 3, 0),
          (4, 2, "global1", 3, 2), (2, 3, "peak", 5, 0), (3, 2, "affine", 5, 0), (2, 1, "global1", 6, 2)]


def _emulate(case, gaps=True, buckets=None, sigmas=None, tpb=0, pairs=True, counts=True):
    import run_emul_pairs as E
    Ds, Tm, Fs = R.MODELS[case["S"]]
    ds = np.sqrt(2 * Ds * R.DT)
    bk = case["buckets"] if buckets is None else buckets
    sg = case["sig"] if sigmas is None else sigmas
    order = list(range(len(bk)))[::-1]  # longest first
    pr, ct, info = E.run_pairs([bk[i] for i in order], case["le"] if case["le"] is not None else [0.0], ds, Fs, Tm, R.PBL,
                               O.p_stay_table(ds, case["S"], 1, R.CELL), case["F"], R.MIN_LEN, max(b.shape[1] for b in bk),
                               sigmas=None if sg is None else [sg[i] for i in order], slope_offset=case["slope_offset"], gaps=gaps, tpb=tpb,
                               pairs=pairs, counts=counts)
    back = lambda got: None if got is None else [got[order.index(i)] for i in range(len(bk))]
    return back(pr), back(ct), info


def _check(case, got_pairs, got_counts, ref, what):
    for i, (g, c, (_, r)) in enumerate(zip(got_pairs, got_counts, ref)):
        assert np.all(np.isfinite(r)), (what, i)
        err = np.abs(g - r).max()
        assert err <= TOL_PRED, "%s bucket %d (L = %d): max |pairs - reference| = %.3e" % (what, i, g.shape[1] + 1, err)
        L = g.shape[1] + 1
        assert np.abs(c - g.sum(axis=1)).max() <= 1e-12 * L, (what, i)


@pytest.mark.parametrize("S,D,layout,F,tpb", _CASES)
def test_emulated_pair_body(S, D, layout, F, tpb):
    case = PR.make_case(S, D, layout, F)
    assert any(m.any() for m in case["masks"]) and any(b.shape[1] == F + 2 for b in case["buckets"])
    pr, ct, info = _emulate(case, gaps=True, tpb=tpb)
    assert tpb == 0 or info[0] == min(tpb, info[0])
    _check(case, pr, ct, PR.case_reference(case, gaps=True), "gaps")
    # the same buckets with their missed rows filled in, through the instantiation without GAPS
    pr, ct, _ = _emulate(case, gaps=False, buckets=PR.plain_buckets(case), sigmas=PR.plain_sigmas(case), tpb=tpb)
    _check(case, pr, ct, PR.case_reference(case, gaps=False), "plain")


def test_emulated_pairs_gap_free_data_through_the_gap_body():
    case = PR.make_case(3, 2, "global1", 3)
    full = PR.plain_buckets(case)
    a, ca, _ = _emulate(case, gaps=True, buckets=full)
    b, cb, _ = _emulate(case, gaps=False, buckets=full)
    assert all(np.abs(x - y).max() <= 1e-13 for x, y in zip(a, b)) and all(np.abs(x - y).max() <= 1e-12 for x, y in zip(ca, cb))


def test_emulated_pairs_counts_only_and_nan_track():
    """With the per-step pointer null only the counts are written, and they are those of the call with both outputs; a NaN coordinate
    (a partial row under GAPS, any NaN without) makes its track NaN everywhere, counts included, and no other track."""
    case = PR.make_case(2, 2, "global1", 3)
    pr, ct, _ = _emulate(case)
    none, ct2, _ = _emulate(case, pairs=False)
    assert none is None and all(np.array_equal(x, y) for x, y in zip(ct, ct2))
    dirty = [b.copy() for b in case["buckets"]]
    dirty[4][6, 5, 1] = np.nan  # L = 14, track 6: a partial row
    dirty[4][9, 0] = np.nan     # a missed first row
    dpr, dct, _ = _emulate(case, buckets=dirty)
    keep = np.ones(len(dirty[4]), bool)
    keep[[6, 9]] = False
    assert np.all(np.isnan(dpr[4][~keep])) and np.all(np.isnan(dct[4][~keep]))
    assert np.array_equal(dpr[4][keep], pr[4][keep]) and np.array_equal(dct[4][keep], ct[4][keep]) and np.all(np.isfinite(pr[4]))
    plain = PR.plain_buckets(case)
    plain[2][1, 2, 0] = np.nan
    ppr, pct, _ = _emulate(case, gaps=False, buckets=plain)
    assert np.all(np.isnan(ppr[2][1])) and np.all(np.isnan(pct[2][1])) and np.all(np.isfinite(ppr[2][0])) and np.all(np.isfinite(ppr[2][2]))
