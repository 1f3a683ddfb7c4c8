"""CPU check of the fixed-state smoother body (xt_cond.h) on CPU threads (tests/emul/emul_cond.cpp) against the dense solve of
tests/cond_reference.py.  Buckets (L, N) = (2, 5) - smaller than a wave -, (3, 70) - a partial last wave - and (9, 130) - three batches
of 64 tracks walked by two blocks -, with RANDOM state paths so that every entry of the step-variance table is used.

Tolerances (cond_reference.compare): mu 1e-12 absolute (positions are O(1)), sigma 1e-12 relative, logdens 1e-10.  A numpy version of the
same recursion differs from the dense solve by at most 1.8e-14 / 7.4e-15 relative / 5.1e-13 on these models for tracks up to 200
positions; the tolerances leave 50 - 200 x for the kernel's operation order, its reciprocal and its product-carried log."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))

import cond_reference as R
from extrack_amd import synth

_DT = 0.02
_SHAPES = ((2, 5), (3, 70), (9, 130))  # (L, N)
_MODELS = {
    2: (np.array([0.0005, 0.25]), np.array([[0.9, 0.1], [0.15, 0.85]]), np.array([0.55, 0.45])),
    3: (np.array([0.0005, 0.04, 0.25]), np.array([[0.85, 0.1, 0.05], [0.08, 0.85, 0.07], [0.05, 0.1, 0.85]]), np.array([0.3, 0.3, 0.4])),
}


def _ds(S):
    return np.sqrt(2 * _MODELS[S][0] * _DT)


def _data(S, dims, seed):
    """[(tracks [N, L, dims], random paths int8 [N, L])] per bucket."""
    Ds, Tm, Fs = _MODELS[S]
    rng = np.random.default_rng(seed)
    return [(synth.brownian_tracks(N, L, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=_DT, dims=dims, seed=seed + i),
             rng.integers(0, S, (N, L)).astype(np.int8)) for i, (L, N) in enumerate(_SHAPES)]


def _emulate(S, Cs, st, le, **kw):
    import run_emul_cond as E
    return E.run_cond(Cs, st, le, _ds(S), **kw)


@pytest.mark.parametrize("S,dims,le,ws_global", [(2, 2, [0.02], False), (3, 1, [0.025], True), (2, 3, [0.02, 0.03, 0.05], False),
                                                 (3, 2, [0.02, 0.035], True), (3, 3, [0.03], False), (2, 1, [0.02], False)])
def test_emulated_smoother_global_error(S, dims, le, ws_global):
    for Cs, st in _data(S, dims, 40 + S):
        got = _emulate(S, Cs, st, le, ws_global=ws_global)
        R.compare(got, R.refine(Cs, st, _ds(S), le=le), "S=%d D=%d K=%d L=%d" % (S, dims, len(le), Cs.shape[1]))
        assert np.unique(st).size == S or Cs.shape[1] == 2


@pytest.mark.parametrize("S,dims,KS,affine", [(2, 2, 2, False), (2, 2, 1, True), (3, 3, 1, False), (3, 3, 3, True), (2, 1, 1, True)])
def test_emulated_smoother_per_peak_error(S, dims, KS, affine):
    rng = np.random.default_rng(7)
    so = (1.3, 0.004) if affine else None
    for Cs, st in _data(S, dims, 50 + S):
        sig = rng.uniform(0.01, 0.05, Cs.shape[:2] + (KS,))
        if affine:
            sig[0, 0, 0] = -1.0  # below the 1e-6 floor after slope / offset
        got = _emulate(S, Cs, st, [0.0], sigma=sig, slope_offset=so, ws_global=(KS == 1))
        R.compare(got, R.refine(Cs, st, _ds(S), sigma=sig, slope_offset=so), "per-peak S=%d D=%d KS=%d affine=%d L=%d" % (S, dims, KS, affine, Cs.shape[1]))


@pytest.mark.parametrize("ws_global", [False, True])
def test_emulated_smoother_special_rows(ws_global):
    """A NaN position, a NaN error and a -1 path each poison exactly their own track; every other row keeps its bits."""
    S = 2
    rng = np.random.default_rng(3)
    for Cs, st in _data(S, 2, 60):
        N, L = st.shape
        sig = rng.uniform(0.01, 0.05, (N, L, 1))
        clean = _emulate(S, Cs, st, [0.0], sigma=sig, ws_global=ws_global)
        Cd, sd, gd = Cs.copy(), st.copy(), sig.copy()
        rows = [1, 3, 4] if N < 64 else [3, 63, 64 + 5]
        Cd[rows[0], L - 1, 1] = np.nan
        sd[rows[1], 0] = -1
        gd[rows[2], L // 2, 0] = np.nan
        dirty = _emulate(S, Cd, sd, [0.0], sigma=gd, ws_global=ws_global)
        R.compare(dirty, R.refine(Cd, sd, _ds(S), sigma=gd), "special rows L=%d" % L)
        keep = np.ones(N, bool)
        keep[rows] = False
        for x, y in zip(clean, dirty):
            assert np.all(np.isnan(y[rows])) and np.array_equal(x[keep], y[keep]) and np.all(np.isfinite(x))


def test_emulated_smoother_placements_agree():
    """Rows in LDS and rows in the output arrays give the same bits; 64 and 128 tracks per block and 1 - 3 blocks give the same bits;
    without a logdens output the other two are unchanged."""
    S = 3
    for Cs, st in _data(S, 2, 70):
        a = _emulate(S, Cs, st, [0.02, 0.03], ws_global=False, tpb=64, nblocks=2)
        b = _emulate(S, Cs, st, [0.02, 0.03], ws_global=True, tpb=64, nblocks=3)
        c = _emulate(S, Cs, st, [0.02, 0.03], ws_global=False, tpb=128, nblocks=1)
        d = _emulate(S, Cs, st, [0.02, 0.03], ws_global=True, tpb=128, nblocks=2, logdens=False)
        for x, y, z, w in zip(a, b, c, d):
            assert np.array_equal(x, y) and np.array_equal(x, z) and (w is None or np.array_equal(x, w))
        assert d[2] is None
