"""CPU check of the gap-aware fixed-window body (xt_kernel.h, GAPS = true) on CPU threads (tests/emul/emul_gap.cpp) against the reference
built from the unchanged oracle (tests/gap_reference.py): the buckets of the GPU test (L = 2, 3 with its only interior row missing,
frame_len + 1, 14 with gaps at t = 1 / L - 2 / a run longer than the window / every interior row, 40 with gaps across the staging boundary;
ragged N), launched longest first through the bucket-descriptor table with min_len 3 and the longest bucket isBL = 0.
Tolerances: those of tests/test_hip_parity.py (per-track LL rtol 1e-13 / atol 1e-10, total 1e-12 relative, posteriors 1e-9)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))

import gap_reference as R
from oracle import oracle_np as O

TOL_PRED = 1e-9
# every state count, dimensionality and error layout at frame_len 3 (2 .. 16 groups per track, many tracks per emulated workgroup), and at
# frame_len 5 for 2 and 3 states (up to 81 groups: more than one wavefront per track).  4 states at frame_len 5 (256 CPU threads per track in
# lock-step: 20 s a case) are left to the GPU test.
_CASES = [(S, D, lay, F) for F in (3, 5) for S in (2, 3, 4) for D in (1, 2, 3) for lay in R.LAYOUTS
          if not (D == 1 and lay == "globalD") and not (S == 4 and F == 5)]


def _emulate(case, preds, gaps=True, buckets=None):
    import run_emul_gap as E
    Ds, Tm, Fs = R.MODELS[case["S"]]
    ds = np.sqrt(2 * Ds * R.DT)
    bk = case["buckets"] if buckets is None else buckets
    order = list(range(len(bk)))[::-1]  # longest first
    got, tot, info = E.run_gap([bk[i] for i in order], case["le"] if case["le"] is not None else [0.0], ds, Fs, Tm, R.PBL,
                               O.p_stay_table(ds, case["S"], 1, R.CELL), case["F"], R.MIN_LEN, max(b.shape[1] for b in bk),
                               sigmas=None if case["sig"] is None else [case["sig"][i] for i in order], slope_offset=case["slope_offset"],
                               preds=preds, gaps=gaps)
    out = [None] * len(bk)
    for j, i in enumerate(order):
        out[i] = got[j]
    return out, tot


@pytest.mark.parametrize("S,D,layout,F", _CASES)
def test_emulated_gap_body(S, D, layout, F):
    case = R.make_case(S, D, layout, F)
    assert any(m.any() for m in case["masks"])
    ref = R.case_reference(case, False)
    got, tot = _emulate(case, False)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert np.all(np.isfinite(r))
        np.testing.assert_allclose(g, r, rtol=1e-13, atol=1e-10, err_msg="LL bucket %d" % i)
    rt = sum(r.sum() for r in ref)
    assert abs(tot - rt) <= 1e-12 * abs(rt), (tot, rt)
    refp = R.case_reference(case, True)
    gotp, _ = _emulate(case, True)
    for i, (g, r) in enumerate(zip(gotp, refp)):
        np.testing.assert_allclose(g, r, rtol=0, atol=TOL_PRED, err_msg="posteriors bucket %d" % i)


def test_emulated_gap_body_without_gaps_is_the_plain_body():
    """Gap-free data: the flag changes nothing - the likelihood bit for bit (the same operations in the same order), the posteriors up to the
    order of their atomic sums (1e-13 on a probability)."""
    case = R.make_case(3, 2, "global1", 3)
    from extrack_amd import synth
    Ds, Tm, Fs = R.MODELS[3]
    full = [synth.brownian_tracks(len(b), b.shape[1], list(Ds), Tm.tolist(), list(Fs), dt=R.DT, dims=2, seed=3 + i) for i, b in enumerate(case["buckets"])]
    a, ta = _emulate(case, False, gaps=True, buckets=full)
    b, tb = _emulate(case, False, gaps=False, buckets=full)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and ta == tb
    a, _ = _emulate(case, True, gaps=True, buckets=full)
    b, _ = _emulate(case, True, gaps=False, buckets=full)
    assert all(np.abs(x - y).max() <= 1e-13 for x, y in zip(a, b))


def test_emulated_gap_poison_rules():
    """A row with some NaN coordinates, a NaN first row and a NaN last row poison their track and nothing else; without the flag every NaN does."""
    case = R.make_case(2, 2, "global1", 3)
    clean, _ = _emulate(case, False)
    dirty = [b.copy() for b in case["buckets"]]
    dirty[3][6, 5, 1] = np.nan   # partial row
    dirty[3][9, 0] = np.nan      # first row
    dirty[4][5, -1] = np.nan     # last row
    got, _ = _emulate(case, False, buckets=dirty)
    bad = {3: [6, 9], 4: [5]}
    for i in range(len(dirty)):
        keep = np.ones(len(dirty[i]), bool)
        keep[bad.get(i, [])] = False
        assert np.all(np.isnan(got[i][~keep])) and np.array_equal(got[i][keep], clean[i][keep]) and np.all(np.isfinite(clean[i]))
    gotp, _ = _emulate(case, True, buckets=dirty)
    assert np.all(np.isnan(gotp[3][6])) and np.all(np.isnan(gotp[3][9])) and np.all(np.isnan(gotp[4][5])) and np.all(np.isfinite(gotp[3][7]))
    plain, _ = _emulate(case, False, gaps=False)
    for m, p in zip(case["masks"], plain):
        assert np.array_equal(np.isnan(p), m.any(axis=1))
