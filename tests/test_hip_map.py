"""GPU tests of the most-likely state path (extrack_map_states, csrc/xt_map.h; tracking.predict_states), all through the C ABI or
``predict_states``.  References: fixtures taken from the reference's own sequence matrix (tests/golden/map_cases.*, exact MAP for tracks of
at most frame_len + 1 positions) and the numpy restatement of the windowed recursion (tests/map_reference.py), under its tie rule; scores
within 1e-10 (linear-domain weights, <= 1 ulp reciprocals and a 3e-16 exponential per position: ~1e-13 on log densities of magnitude
<= 300 at the longest tracks used here)."""
import json
import os

import numpy as np
import pytest

import map_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
_DT, _PBL, _CELL = 0.02, 0.1, [1.0]
_D = {2: [0.0005, 0.25], 3: [0.0005, 0.04, 0.25], 4: [0.0005, 0.02, 0.08, 0.3]}
_F = {2: [0.55, 0.45], 3: [0.3, 0.3, 0.4], 4: [0.2, 0.3, 0.3, 0.2]}


def _params(S, le=(0.02,), so=None):
    """Parameters of an S-state model; ``le``: global error(s) (1 or one per dimension); ``so``: slope / offset of per-peak errors."""
    from extrack_amd.lmfit_compat import Parameters
    p = Parameters()
    for s in range(S):
        p.add("D%d" % s, value=_D[S][s])
        p.add("F%d" % s, value=_F[S][s])
        for t in range(S):
            if s != t:
                p.add("p%d%d" % (s, t), value=0.06 + 0.02 * ((s + 2 * t) % 3))
    if len(le) == 1:
        p.add("LocErr", value=le[0])
    else:
        for i, v in enumerate(le):
            p.add("LocErr%d" % i, value=v)
    if so is not None:
        p.add("slope_LocErr", value=so[0])
        p.add("offset_LocErr", value=so[1])
    p.add("pBL", value=_PBL)
    return p


def _arrays(p):
    from extrack_amd import tracking
    le, Ds, Fs, Tm, pBL, so = tracking._extract_arrays(p, _DT, 1, 1)
    return le, np.sqrt(2 * Ds * _DT), Fs, Tm, pBL, so


def _dataset(S, shapes, dims, seed):
    from extrack_amd import synth
    Tm = np.full((S, S), 0.1 / (S - 1)) + np.eye(S) * (0.9 - 0.1 / (S - 1))
    return {str(L): synth.brownian_tracks(N, L, _D[S], Tm.tolist(), _F[S], LocErr=0.02, dt=_DT, dims=dims, seed=seed + i)
            for i, (L, N) in enumerate(shapes)}


def _reference(tracks, p, F, sig=None):
    """{key: (states, score, margin)} of the restatement, with min_len / max_len / isBL from all keys as predict_states takes them."""
    le, ds, Fs, Tm, pBL, so = _arrays(p)
    lens = sorted(int(k) for k in tracks)
    out = {}
    for k, Cs in tracks.items():
        if len(Cs) == 0:
            continue
        if sig is None:
            LE = le[None, None]
        else:
            LE = np.asarray(sig[k], float)
            if so is not None:
                LE = np.maximum(LE * so[0] + so[1], 1e-6)
        out[k] = R.map_path(Cs, LE, ds, Fs, Tm, pBL, int(int(k) != lens[-1]), _CELL, F, max(lens[0], 2))
    return out


def _check_dataset(tracks, p, F, sig=None, what=""):
    from extrack_amd import tracking
    st, sc = tracking.predict_states(tracks, _DT, p, cell_dims=_CELL, frame_len=F, input_LocErr=sig, return_scores=True)
    ref = _reference(tracks, p, F, sig)
    assert set(st) == set(tracks) and set(sc) == set(tracks)
    for k in ref:
        R.compare_paths(st[k], sc[k], ref[k][0], ref[k][1], ref[k][2], 1e-10, "%s L=%s" % (what, k))
    return st, sc


# ---- 1. every golden case: exact MAP of the reference's own sequence matrix ----------------------------------------------------------
def test_golden_exact_map_cases():
    from extrack_amd import tracking as T
    with open(os.path.join(GOLDEN, "map_cases.json")) as f:
        meta = json.load(f)
    data = np.load(os.path.join(GOLDEN, "map_cases.npz"))
    worst = 0.0
    for c in meta:
        pre = "m%04d_" % c["id"]
        ts, le = T._one_bucket(data[pre + "Cs"], data[pre + "LE"], c["isBL"], c["min_len"], 0)
        try:
            model = ts.make_model(le, data[pre + "ds"], data[pre + "Fs"], data[pre + "T"], c["pBL"], c["cell_dims"], 1, c["F"])
            (st, sc), = ts.map_states(model, scores=True)
        finally:
            ts.close()
        worst = max(worst, np.abs(sc - data[pre + "logp"]).max())
        R.compare_paths(st, sc, data[pre + "path"], data[pre + "logp"], data[pre + "margin"], 1e-10, "golden case %d %s" % (c["id"], c))
    print("golden map cases: %d, worst |score - reference| = %.3e" % (len(meta), worst))


# ---- 2. windowed regime against the restatement: three buckets per dataset (isBL 1 and 0 side by side) -------------------------------
@pytest.mark.parametrize("S,F,lens,dims,err", [
    (2, 2, (4, 9, 30), 1, "scalar"),
    (2, 4, (6, 9, 30), 2, "peak"),
    (2, 6, (8, 9, 30), 3, "dim"),
    (3, 4, (6, 20), 2, "affine"),
    (4, 3, (5, 12), 2, "scalar"),
    (3, 4, (6, 20), 3, "peak1"),
])
def test_windowed_paths_match_restatement(S, F, lens, dims, err):
    tracks = _dataset(S, [(L, 300) for L in lens], dims, 11 * S + F)
    rng = np.random.default_rng(5)
    sig, p = None, _params(S)
    if err == "dim":
        p = _params(S, le=(0.02, 0.03, 0.045)[:dims])
    elif err in ("peak", "peak1", "affine"):
        sig = {k: rng.uniform(0.01, 0.05, v.shape[:2] + ((1,) if err == "peak1" else (dims,))) for k, v in tracks.items()}
        p = _params(S, so=(1.2, 0.003) if err == "affine" else None)
    _check_dataset(tracks, p, F, sig, "S=%d F=%d %s" % (S, F, err))


# ---- 3. batch loop and scratch sizing -----------------------------------------------------------------------------------------------
def test_block_serves_several_batches(monkeypatch):
    from extrack_amd import engine, tracking
    monkeypatch.setenv("EXTRACK_MAP_MAX_BLOCKS", "16")
    tracks = _dataset(2, [(9, 20000)], 2, 77)
    p = _params(2)
    _check_dataset(tracks, p, 4, None, "20000 x 9")
    # the launch really looped: fewer track slots than tracks
    le, ds, Fs, Tm, pBL, _ = _arrays(p)
    ts = engine.TrackSet([tracks["9"]])
    try:
        ts.map_states(ts.make_model(le[None, None], ds, Fs, Tm, pBL, _CELL, 1, 4))
        info = ts.ctx.last_launch_info()
    finally:
        ts.close()
    assert info["blocks"] <= 16 and info["blocks"] * info["tracks_per_block"] * 4 <= 20000, info


def test_global_back_pointer_scratch_is_sized_by_the_grid(monkeypatch):
    monkeypatch.setenv("EXTRACK_MAP_BP", "global")
    monkeypatch.setenv("EXTRACK_MAP_MAX_BLOCKS", "24")
    tracks = _dataset(2, [(8, 5000), (13, 5000), (27, 5000)], 2, 91)
    _check_dataset(tracks, _params(2), 4, None, "global scratch")


def test_back_pointer_placements_agree(monkeypatch):
    from extrack_amd import tracking
    tracks = _dataset(3, [(7, 200), (25, 200)], 2, 17)
    p = _params(3)
    res = {}
    for where in ("lds", "global"):
        monkeypatch.setenv("EXTRACK_MAP_BP", where)
        res[where] = tracking.predict_states(tracks, _DT, p, cell_dims=_CELL, frame_len=4, return_scores=True)
    for k in tracks:
        assert np.array_equal(res["lds"][0][k], res["global"][0][k]) and np.array_equal(res["lds"][1][k], res["global"][1][k])


# ---- 4. edge lengths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,F", [(2, 4), (3, 3)])
@pytest.mark.parametrize("lens", [(2, 3, "F+1", "F+2"), (5, "F+2", 9)])
def test_edge_lengths_and_min_len(S, F, lens):
    """L = 2, 3, frame_len + 1 (no merge), frame_len + 2 (first merge); min_len 2 (first tuple) and 5 (second)."""
    lens = sorted(set(F + int(l[2:]) if isinstance(l, str) else l for l in lens))
    tracks = _dataset(S, [(L, 64) for L in lens], 2, 300 + S)
    _check_dataset(tracks, _params(S), F, None, "edge S=%d F=%d lens=%s" % (S, F, lens))


# ---- 5. contract of predict_states --------------------------------------------------------------------------------------------------
def test_predict_states_contract():
    from extrack_amd import tracking
    tracks = _dataset(2, [(5, 37), (12, 41)], 2, 5)
    tracks["12"][7, 3, 0] = np.nan
    tracks["8"] = np.empty((0, 8, 2))
    p = _params(2)
    only = tracking.predict_states(tracks, _DT, p, cell_dims=_CELL, frame_len=4)
    st, sc = tracking.predict_states(tracks, _DT, p, cell_dims=_CELL, frame_len=4, return_scores=True)
    assert isinstance(only, dict) and set(only) == {"5", "8", "12"} == set(st) == set(sc)
    for k in tracks:
        assert st[k].dtype == np.int8 and st[k].shape == tracks[k].shape[:2] and np.array_equal(only[k], st[k])
        assert sc[k].dtype == np.float64 and sc[k].shape == (len(tracks[k]),)
    assert np.all(st["12"][7] == -1) and np.isnan(sc["12"][7])
    ref = _reference(tracks, p, 4)
    for k in ("5", "12"):
        R.compare_paths(st[k], sc[k], ref[k][0], ref[k][1], ref[k][2], 1e-10, "contract L=%s" % k)
        assert np.all((st[k] >= 0) & (st[k] < 2) | np.isnan(sc[k])[:, None])
    # rows in input order: the reversed input gives the reversed output, bit for bit
    rev = {k: v[::-1].copy() for k, v in tracks.items()}
    st2, sc2 = tracking.predict_states(rev, _DT, p, cell_dims=_CELL, frame_len=4, return_scores=True)
    for k in tracks:
        assert np.array_equal(st2[k], st[k][::-1]) and np.array_equal(sc2[k], sc[k][::-1], equal_nan=True)


# ---- 6 / 7. determinism; the other entry points are untouched ----------------------------------------------------------------------
@pytest.mark.parametrize("S,F", [(2, 6), (4, 4), (3, 4)])
def test_repeatable_and_leaves_other_entry_points_alone(S, F):
    """Posteriors are compared bit for bit where extrack_predict itself is repeatable: its per-position sums go through LDS atomics, whose
    order is fixed only when a track's groups are one aligned power-of-two lane range (2 states; 4 states at frame_len 4: 64 groups).  With
    3 states (27 groups) two extrack_predict calls differ in the last bits with or without this entry point (measured 3.3e-16), so there the
    posteriors are held to the reordering bound of a 27-term sum and its normalisation, 2 * 26 * eps; the likelihood is bit-identical
    everywhere."""
    from extrack_amd import engine
    tracks = _dataset(S, [(7, 150), (19, 170)], 2, 23)
    le, ds, Fs, Tm, pBL, _ = _arrays(_params(S))
    ts = engine.TrackSet([tracks["7"], tracks["19"]])
    try:
        model = ts.make_model(le[None, None], ds, Fs, Tm, pBL, _CELL, 1, F)
        pred0 = ts.predict(model)
        ll0, per0 = ts.loglik(model, per_track=True)
        a = ts.map_states(model, scores=True)
        b = ts.map_states(model, scores=True)
        for (s0, c0), (s1, c1) in zip(a, b):
            assert np.array_equal(s0, s1) and np.array_equal(c0, c1)
        assert ts.ctx.last_kernel_ms() > 0.0
        pred1 = ts.predict(model)
        ll1, per1 = ts.loglik(model, per_track=True)
        assert ll0 == ll1 and np.array_equal(per0, per1)
        if S != 3:
            assert all(np.array_equal(x, y) for x, y in zip(pred0, pred1))
        else:
            assert all(np.abs(x - y).max() <= 2 * 26 * np.finfo(float).eps for x, y in zip(pred0, pred1))
        # score <= the track's log-likelihood where nothing is fused (L = 7 <= F + 1 only for F = 6)
        if F == 6:
            assert np.all(a[0][1] <= per0[:150] + 1e-12 * np.abs(per0[:150]))
    finally:
        ts.close()


# ---- 8. unsupported requests are refused on the host --------------------------------------------------------------------------------
def test_unsupported_requests():
    from extrack_amd import _lib, engine, tracking
    tracks = _dataset(2, [(6, 8)], 2, 3)
    p = _params(2)
    with pytest.raises(NotImplementedError):
        tracking.predict_states(tracks, {"6": np.full((8, 6), _DT)}, p)
    with pytest.raises(NotImplementedError):
        tracking.predict_states(tracks, _DT, p, fusion="threshold")
    for S, F in ((5, 3), (2, 12), (4, 7)):  # five states; 2048 and 4096 groups per track
        ts = engine.TrackSet([tracks["6"]])
        try:
            ds = np.sqrt(2 * np.linspace(0.001, 0.3, S) * _DT)
            Tm = np.full((S, S), 0.05) + np.eye(S) * (1 - 0.05 * S)
            model = ts.make_model(np.array([[[0.02]]]), ds, np.full(S, 1.0 / S), Tm, _PBL, _CELL, 1, F)
            with pytest.raises(_lib.ExtrackError) as ei:
                ts.map_states(model)
            assert ei.value.code == _lib.E_UNSUPPORTED
            with pytest.raises(_lib.ExtrackError):  # nothing was launched to find that out
                ts.ctx.last_kernel_ms()
        finally:
            ts.close()
