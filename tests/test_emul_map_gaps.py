"""CPU check of the gap-aware state-path decoder body (xt_map.h, GAPS = true) on CPU threads (tests/emul/emul_map_gap.cpp) against the numpy
restatement of the gap rule (tests/map_gap_reference.py): the five buckets of ``gap_reference.make_case`` (L = 2, 3, frame_len + 1, 14, 40;
gaps at t = 1 and t = L - 2, a run longer than the window, every interior row missing, gaps across the staging boundary, a ragged last
batch) in ONE emulated launch through the bucket-descriptor table, longest first, min_len 3, the longest bucket isBL = 0.  Scores within
1e-10 (the tolerance of tests/test_hip_map.py), paths under the gap comparison rule of tests/map_gap_reference.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))

import gap_reference as G
import map_gap_reference as MG
from oracle import oracle_np as O

SCORE_TOL = 1e-10
# every state count, dimensionality and error layout at frame_len 3, and 2 / 3 states at frame_len 5 (up to 81 groups: more than one
# wavefront per track); 4 states at frame_len 5 (256 CPU threads per track in lock-step) are left to the GPU test.  The back-pointer
# placement alternates from case to case: both are covered at every state count and frame_len.
_CASES = [(S, D, lay, F) for F in (3, 5) for S in (2, 3, 4) for D in (1, 2, 3) for lay in G.LAYOUTS if not (S == 4 and F == 5)]


def _emulate(case, gaps=True, buckets=None, sigmas=None, **kw):
    import run_emul_map_gap as E
    Ds, Tm, Fs = G.MODELS[case["S"]]
    ds = np.sqrt(2 * Ds * G.DT)
    bk = case["buckets"] if buckets is None else buckets
    sg = case["sig"] if sigmas is None else sigmas
    order = list(range(len(bk)))[::-1]  # longest first
    got = E.run_map([bk[i] for i in order], case["le"] if case["le"] is not None else [0.0], ds, Fs, Tm, G.PBL,
                    O.p_stay_table(ds, case["S"], 1, G.CELL), case["F"], G.MIN_LEN, max(b.shape[1] for b in bk),
                    sigmas=None if sg is None else [sg[i] for i in order], slope_offset=case["slope_offset"], gaps=gaps, **kw)
    out = [None] * len(bk)
    for j, i in enumerate(order):
        out[i] = got[j]
    return out


def _reference(case, buckets=None, effs=None):
    Ds, Tm, Fs = G.MODELS[case["S"]]
    ds = np.sqrt(2 * Ds * G.DT)
    bk = case["buckets"] if buckets is None else buckets
    ef = case["eff"] if effs is None else effs
    Lmax = max(b.shape[1] for b in bk)
    refs, models = [], []
    for b, eff in zip(bk, ef):
        isBL = int(b.shape[1] != Lmax)
        refs.append(MG.map_path(b, eff, ds, Fs, Tm, G.PBL, isBL, G.CELL, case["F"], G.MIN_LEN))
        models.append((ds, Fs, Tm, G.PBL, isBL, G.CELL, G.MIN_LEN))
    return refs, models


@pytest.mark.parametrize("n,S,D,layout,F", [(n,) + c for n, c in enumerate(_CASES)])
def test_emulated_gap_decoder(n, S, D, layout, F):
    case = G.make_case(S, D, layout, F)
    assert any(m.any() for m in case["masks"])
    refs, models = _reference(case)
    got = _emulate(case, bp_global=bool(n % 2))
    left = [MG.compare_paths(st, sc, ref, b, eff, model, SCORE_TOL, "S=%d D=%d %s F=%d bucket %d" % (S, D, layout, F, i))
            for i, ((st, sc), ref, b, eff, model) in enumerate(zip(got, refs, case["buckets"], case["eff"], models))]
    MG.check_exclusions(left, case["masks"], what="S=%d D=%d %s F=%d" % (S, D, layout, F))


def test_emulated_gap_decoder_placements_agree():
    """Back-pointer words in LDS and in the global region give the same bits; two tracks per block and four give the same bits."""
    case = G.make_case(3, 2, "peak", 3)
    a = _emulate(case, bp_global=False, tpb=2)
    b = _emulate(case, bp_global=True, tpb=4, blocks_per_bucket=[1] * 5)
    for (s0, c0), (s1, c1) in zip(a, b):
        assert np.array_equal(s0, s1) and np.array_equal(c0, c1)


@pytest.mark.parametrize("S,D,layout,F", [(3, 2, "global1", 3), (2, 3, "peak", 5), (4, 1, "affine", 3)])
def test_emulated_gap_decoder_without_gaps_is_the_plain_body(S, D, layout, F):
    """Gap-free data: the flag changes nothing, states and scores bit for bit."""
    from extrack_amd import synth
    case = G.make_case(S, D, layout, F)
    Ds, Tm, Fs = G.MODELS[S]
    full = [synth.brownian_tracks(len(b), b.shape[1], list(Ds), Tm.tolist(), list(Fs), dt=G.DT, dims=D, seed=3 + i) for i, b in enumerate(case["buckets"])]
    sig = None if case["sig"] is None else [np.where(np.isnan(s) | (s > 100), 0.03, s) for s in case["sig"]]
    a = _emulate(case, gaps=True, buckets=full, sigmas=sig)
    b = _emulate(case, gaps=False, buckets=full, sigmas=sig)
    for (s0, c0), (s1, c1) in zip(a, b):
        assert np.array_equal(s0, s1) and np.array_equal(c0, c1) and not np.any(s0 < 0) and np.all(np.isfinite(c0))


def test_emulated_gap_decoder_poison_rules():
    """A row with some NaN coordinates, a NaN first row, a NaN last row and a NaN error at an observed row each poison their own track
    (states -1, score NaN) and leave every other track's bits unchanged; the error of a gap row is never read; without the flag every NaN
    row poisons."""
    case = G.make_case(2, 2, "peak", 3)
    clean = _emulate(case)
    dirty = [b.copy() for b in case["buckets"]]
    sig = [s.copy() for s in case["sig"]]
    dirty[3][6, 5, 1] = np.nan   # partial row
    dirty[3][9, 0] = np.nan      # first row
    dirty[4][5, -1] = np.nan     # last row
    obs = np.nonzero(~case["masks"][3][12])[0]
    sig[3][12, obs[1], 1] = np.nan  # NaN error at an observed row
    for s, m in zip(sig, case["masks"]):
        s[m] = np.nan               # ... and at every gap row: never read
    got = _emulate(case, buckets=dirty, sigmas=sig)
    bad = {3: [6, 9, 12], 4: [5]}
    for i in range(len(dirty)):
        keep = np.ones(len(dirty[i]), bool)
        keep[bad.get(i, [])] = False
        assert np.all(got[i][0][~keep] == -1) and np.all(np.isnan(got[i][1][~keep]))
        assert np.array_equal(got[i][0][keep], clean[i][0][keep]) and np.array_equal(got[i][1][keep], clean[i][1][keep])
        assert not np.any(clean[i][0] < 0) and np.all(np.isfinite(clean[i][1]))
    # (one batch per block: the plain body clears its flag after a batch's last barrier, which CPU threads of the next batch can overtake)
    plain = _emulate(case, gaps=False, blocks_per_bucket=[(len(b) + 1) // 2 for b in case["buckets"][::-1]])
    for m, (st, sc) in zip(case["masks"], plain):
        assert np.array_equal(np.isnan(sc), m.any(axis=1)) and np.array_equal((st == -1).all(axis=1), m.any(axis=1))
