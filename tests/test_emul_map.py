"""CPU check of the state-path decoder body (xt_map.h) on CPU threads (tests/emul/emul_map.cpp): three length buckets in upload order
(L, N) = (2, 4), (3, 5), (9, 14), launched longest first through the bucket-descriptor table at frame_len 4 (no merge, no merge, four
merges), two blocks per bucket and two tracks per block so that a block walks several batches - against the numpy restatement of the
recursion (tests/map_reference.py): paths identical under its tie rule, scores within 1e-10 (the kernel carries linear-domain weights
with <= 1 ulp reciprocals and a 3e-16 exponential over at most 9 positions: ~1e-14 on a log density of magnitude <= 100)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))

import map_reference as R
from extrack_amd import synth
from oracle import oracle_np as O

_DT, _PBL, _CELL, _F = 0.02, 0.1, [1.0], 4
_SHAPES = ((2, 4), (3, 5), (9, 14))  # (L, N) in upload order
_MODELS = {
    2: (np.array([0.0005, 0.25]), np.array([[0.9, 0.1], [0.15, 0.85]]), np.array([0.55, 0.45])),
    3: (np.array([0.0005, 0.04, 0.25]), np.array([[0.85, 0.1, 0.05], [0.08, 0.85, 0.07], [0.05, 0.1, 0.85]]), np.array([0.3, 0.3, 0.4])),
}


def _data(S, dims, seed):
    Ds, Tm, Fs = _MODELS[S]
    return [synth.brownian_tracks(N, L, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=_DT, dims=dims, seed=seed + i)
            for i, (L, N) in enumerate(_SHAPES)]


def _reference(S, parts, le_of):
    Ds, Tm, Fs = _MODELS[S]
    ds = np.sqrt(2 * Ds * _DT)
    Lmax = max(L for L, _ in _SHAPES)
    return [R.map_path(p, le_of(i, p), ds, Fs, Tm, _PBL, int(p.shape[1] != Lmax), _CELL, _F, 2) for i, p in enumerate(parts)]


def _emulate(S, parts, le, **kw):
    import run_emul_map as E
    Ds, Tm, Fs = _MODELS[S]
    ds = np.sqrt(2 * Ds * _DT)
    order = [2, 1, 0]  # longest first
    sig = kw.pop("sigmas", None)
    got = E.run_map([parts[i] for i in order], le, ds, Fs, Tm, _PBL, O.p_stay_table(ds, S, 1, _CELL), _F, 2, 9,
                    sigmas=None if sig is None else [sig[i] for i in order], **kw)
    out = [None] * 3
    for j, i in enumerate(order):
        out[i] = got[j]
    return out


def _check(got, ref, what):
    for i, ((st, sc), (rst, rsc, mg)) in enumerate(zip(got, ref)):
        R.compare_paths(st, sc, rst, rsc, mg, 1e-10, "%s bucket %d" % (what, i))


@pytest.mark.parametrize("S,dims,le,bp_global", [(2, 2, [0.02], False), (3, 2, [0.02], True), (2, 3, [0.02, 0.03, 0.05], False),
                                                 (3, 1, [0.025], False)])
def test_emulated_decoder_global_error(S, dims, le, bp_global):
    parts = _data(S, dims, 40 + S)
    ref = _reference(S, parts, lambda i, p: np.asarray(le, float)[None, None])
    _check(_emulate(S, parts, le, bp_global=bp_global), ref, "S=%d D=%d K=%d" % (S, dims, len(le)))


@pytest.mark.parametrize("KS,affine", [(2, False), (1, True)])
def test_emulated_decoder_per_peak_error(KS, affine):
    S = 2
    parts = _data(S, 2, 50)
    rng = np.random.default_rng(7)
    sig = [rng.uniform(0.01, 0.05, p.shape[:2] + (KS,)) for p in parts]
    so = (1.3, 0.004) if affine else None
    eff = [np.maximum(s * so[0] + so[1], 1e-6) for s in sig] if affine else sig
    ref = _reference(S, parts, lambda i, p: eff[i])
    _check(_emulate(S, parts, [0.0], sigmas=sig, slope_offset=so, bp_global=True), ref, "per-peak KS=%d affine=%d" % (KS, affine))


def test_emulated_decoder_nan_track():
    S = 2
    parts = _data(S, 2, 60)
    clean = _emulate(S, parts, [0.02])
    dirty_parts = [p.copy() for p in parts]
    dirty_parts[2][3, 5, 1] = np.nan
    dirty_parts[0][1, 0, 0] = np.nan
    dirty = _emulate(S, dirty_parts, [0.02])
    for i, row in ((2, 3), (0, 1)):
        assert np.all(dirty[i][0][row] == -1) and np.isnan(dirty[i][1][row])
    for i in range(3):
        keep = np.ones(len(parts[i]), bool)
        if i == 2:
            keep[3] = False
        if i == 0:
            keep[1] = False
        assert np.array_equal(dirty[i][0][keep], clean[i][0][keep]) and np.array_equal(dirty[i][1][keep], clean[i][1][keep])
        assert not np.any(clean[i][0] < 0) and np.all(np.isfinite(clean[i][1]))


def test_emulated_decoder_placements_agree():
    """Back-pointer words in LDS and in the global region give the same bits; one track per block and four give the same bits."""
    parts = _data(3, 2, 70)
    a = _emulate(3, parts, [0.02], bp_global=False, tpb=2)
    b = _emulate(3, parts, [0.02], bp_global=True, tpb=4, blocks_per_bucket=[1, 1, 1])
    for (s0, c0), (s1, c1) in zip(a, b):
        assert np.array_equal(s0, s1) and np.array_equal(c0, c1)
