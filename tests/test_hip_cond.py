"""GPU tests of the fixed-state position refinement (extrack_refine_fixed_states, csrc/xt_cond.h; refined_localization.get_pos_PDF_fixedBs
and refine_along_states), through the C ABI and the two Python functions, against the dense solve of tests/cond_reference.py with the
tolerances of the emulation test (tests/test_emul_cond.py): mu 1e-12 absolute, sigma 1e-12 relative, logdens 1e-10."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cond_reference as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
_DT, _PBL, _CELL = 0.02, 0.1, [1.0]
_D = {2: [0.0005, 0.25], 3: [0.0005, 0.04, 0.25], 4: [0.0005, 0.02, 0.08, 0.3]}
_F = {2: [0.55, 0.45], 3: [0.3, 0.3, 0.4], 4: [0.2, 0.3, 0.3, 0.2]}
_SMALL = ((2, 5), (3, 70), (9, 130))  # (L, N): less than a wave, a partial last wave, more than one block
_LE = {1: (0.02,), 2: (0.02, 0.035), 3: (0.02, 0.03, 0.045)}


def _params(S, le=(0.02,), so=None):
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


def _tm(S):
    return np.full((S, S), 0.1 / (S - 1)) + np.eye(S) * (0.9 - 0.1 / (S - 1))


def _ds(S):
    return np.sqrt(2 * np.array(_D[S]) * _DT)


def _dataset(S, shapes, dims, seed):
    """({key: tracks}, {key: random paths int8}): random, not decoded, so that every step-variance entry is used."""
    from extrack_amd import synth
    rng = np.random.default_rng(seed)
    tracks = {str(L): synth.brownian_tracks(N, L, _D[S], _tm(S).tolist(), _F[S], LocErr=0.02, dt=_DT, dims=dims, seed=seed + i)
              for i, (L, N) in enumerate(shapes)}
    return tracks, {k: rng.integers(0, S, v.shape[:2]).astype(np.int8) for k, v in tracks.items()}


def _tab_bytes(S):
    return 8 * ((S * S + 1) & ~1)


def _run_abi(S, tracks, states, le=None, sig=None, so=None, logdens=True):
    """Through engine.TrackSet / _lib.Context.refine_fixed_states.  Returns ({key: (mu, sigma, logdens)}, {key: launch info})."""
    from extrack_amd import engine
    keys = sorted(tracks, key=int)
    ts = engine.TrackSet([tracks[k] for k in keys], None if sig is None else [sig[k] for k in keys])
    out, info = {}, {}
    try:
        model = ts.make_model(None if sig is not None else np.asarray(le, float)[None, None], _ds(S), _F[S], _tm(S), _PBL, _CELL, 1, 4, slope_offset=so)
        for i, k in enumerate(keys):
            out[k] = ts.ctx.refine_fixed_states(model, i, states[k], logdens=logdens)
            info[k] = ts.ctx.last_launch_info()
            assert ts.ctx.last_kernel_ms() > 0.0
    finally:
        ts.close()
    return out, info


# ---- 1. the C ABI on the three small buckets: states, dimensions, error channels and error modes -----------------------------------------
@pytest.mark.parametrize("S,dims,err", [(2, 2, "scalar"), (3, 1, "scalar"), (2, 3, "dim"), (3, 2, "dim"), (3, 3, "scalar"), (2, 1, "peak"),
                                        (2, 2, "peak"), (2, 2, "peak1_affine"), (3, 3, "peak_affine"), (3, 3, "peak1")])
def test_small_buckets_match_dense_solve(S, dims, err):
    tracks, states = _dataset(S, _SMALL, dims, 10 * S + dims)
    rng = np.random.default_rng(5)
    le, sig, so = None, None, None
    if err in ("scalar", "dim"):
        le = _LE[dims] if err == "dim" else (0.02,)
    else:
        sig = {k: rng.uniform(0.01, 0.05, v.shape[:2] + ((1,) if "peak1" in err else (dims,))) for k, v in tracks.items()}
        so = (1.2, 0.003) if "affine" in err else None
    got, info = _run_abi(S, tracks, states, le, sig, so)
    for k in tracks:
        ref = R.refine(tracks[k], states[k], _ds(S), le=le, sigma=None if sig is None else sig[k], slope_offset=so)
        R.compare(got[k], ref, "S=%d D=%d %s L=%s" % (S, dims, err, k))
        assert info[k]["lds_bytes"] > _tab_bytes(S) and info[k]["threads"] == info[k]["tracks_per_block"] == 64, info[k]  # rows in LDS
    assert info["9"]["blocks"] == 3 and info["3"]["blocks"] == 2 and info["2"]["blocks"] == 1


# ---- 2. long / wide tracks: the placements the library chooses by itself ---------------------------------------------------------------------
@pytest.mark.parametrize("S,dims,err,L,N,placement", [(4, 3, "dim", 60, 200, "global"), (2, 2, "scalar", 400, 70, "global"),
                                                      (4, 2, "scalar", 60, 130, "lds")])
def test_long_tracks_and_placement(S, dims, err, L, N, placement):
    """(60, 200) at 4 states, 3 dimensions, 3 error channels: 64 rows of 361 doubles exceed the 160 KiB of a CU; (400, 70): far beyond;
    (60, 130) at 2 dimensions, one channel: 64 rows of 181 doubles = 97 KiB, LDS beyond the 64 KiB a kernel gets without asking.  The
    placement shows in the launch's LDS bytes: the global one keeps only the step-variance table there (include/extrack_hip.h)."""
    tracks, states = _dataset(S, [(L, N)], dims, 77 + L)
    le = _LE[dims] if err == "dim" else (0.02,)
    got, info = _run_abi(S, tracks, states, le)
    k = str(L)
    if placement == "global":
        assert info[k]["lds_bytes"] == _tab_bytes(S), info[k]
    else:
        assert 64 * 1024 < info[k]["lds_bytes"] <= 160 * 1024, info[k]
    R.compare(got[k], R.refine(tracks[k], states[k], _ds(S), le=le), "S=%d D=%d %s L=%d" % (S, dims, err, L))


# ---- 3. the global placement forced in a fresh process equals the LDS placement bit for bit ---------------------------------------------------
_CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
from extrack_amd import engine
d = np.load(sys.argv[1])
out = {}
for k in ("2", "3", "9"):
    ts = engine.TrackSet([d["c" + k]], [d["g" + k]])
    try:
        model = ts.make_model(None, d["ds"], d["Fs"], d["T"], 0.1, [1.0], 1, 4, slope_offset=(1.2, 0.003))
        mu, sg, ld = ts.ctx.refine_fixed_states(model, 0, d["s" + k], logdens=True)
        out["lds" + k] = np.array(ts.ctx.last_launch_info()["lds_bytes"])
    finally:
        ts.close()
    out["mu" + k], out["sg" + k], out["ld" + k] = mu, sg, ld
np.savez(sys.argv[2], **out)
"""


def test_forced_global_placement_in_child_process(tmp_path):
    S, dims = 3, 2
    tracks, states = _dataset(S, _SMALL, dims, 31)
    rng = np.random.default_rng(9)
    sig = {k: rng.uniform(0.01, 0.05, v.shape[:2] + (dims,)) for k, v in tracks.items()}
    got, info = _run_abi(S, tracks, states, None, sig, (1.2, 0.003))
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, ds=_ds(S), Fs=np.array(_F[S]), T=_tm(S), **{"c" + k: v for k, v in tracks.items()}, **{"g" + k: v for k, v in sig.items()},
             **{"s" + k: v for k, v in states.items()})
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, inp, outp], env=dict(os.environ, EXTRACK_COND_WS="global"), cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = np.load(outp)
    for k in tracks:
        assert int(d["lds" + k]) == _tab_bytes(S) < info[k]["lds_bytes"]
        assert np.array_equal(d["mu" + k], got[k][0]) and np.array_equal(d["sg" + k], got[k][1]) and np.array_equal(d["ld" + k], got[k][2])


# ---- 4. the Python functions ------------------------------------------------------------------------------------------------------------------
def test_get_pos_PDF_fixedBs():
    from extrack_amd import refined_localization as RL
    S = 3
    tracks, states = _dataset(S, [(9, 130)], 2, 41)
    Cs, Bs = tracks["9"], states["9"]
    ds, Fs, T = _ds(S), _F[S], _tm(S)
    mus, sigs = RL.get_pos_PDF_fixedBs(Cs, 0.02, ds, Fs, T, Bs[:, None, :])  # the reference's [n, 1, len]
    assert mus.shape == (130, 9, 2) and sigs.shape == (130, 9)
    ref = R.refine(Cs, Bs, ds, le=[0.02])
    R.compare((mus, sigs[:, :, None], None), ref, "get_pos_PDF_fixedBs float")
    mus2, sigs2 = RL.get_pos_PDF_fixedBs(Cs, np.array([[[0.02]]]), ds, Fs, T, Bs.astype(np.int64))
    assert np.array_equal(mus, mus2) and np.array_equal(sigs, sigs2)
    mus, sigs = RL.get_pos_PDF_fixedBs(Cs, [0.02, 0.035], ds, Fs, T, Bs)
    assert sigs.shape == (130, 9, 2)
    R.compare((mus, sigs, None), R.refine(Cs, Bs, ds, le=[0.02, 0.035]), "get_pos_PDF_fixedBs per dimension")
    sig = np.random.default_rng(2).uniform(0.01, 0.05, (130, 9, 1))
    mus, sigs = RL.get_pos_PDF_fixedBs(Cs, sig, ds, Fs, T, Bs)
    assert sigs.shape == (130, 9)
    R.compare((mus, sigs[:, :, None], None), R.refine(Cs, Bs, ds, sigma=sig), "get_pos_PDF_fixedBs per peak")


def test_refine_along_states_decodes_first_and_nan_flows_through():
    from extrack_amd import refined_localization as RL
    from extrack_amd import tracking
    S = 2
    tracks, _ = _dataset(S, [(5, 37), (12, 141)], 2, 5)
    tracks["12"][7, 3, 0] = np.nan
    tracks["8"] = np.empty((0, 8, 2))
    p = _params(S)
    mus, sigs, lds = RL.refine_along_states(tracks, _DT, p, frame_len=4, cell_dims=_CELL, return_logdensity=True)
    st = tracking.predict_states(tracks, _DT, p, cell_dims=_CELL, frame_len=4)
    assert np.all(st["12"][7] == -1)
    mus2, sigs2, lds2 = RL.refine_along_states(tracks, _DT, p, states=st, return_logdensity=True)
    two = RL.refine_along_states(tracks, _DT, p, states=st)
    assert set(mus) == set(sigs) == set(lds) == {"5", "8", "12"} and len(two) == 2
    for k in tracks:
        assert mus[k].shape == tracks[k].shape and sigs[k].shape == tracks[k].shape[:2] and lds[k].shape == (len(tracks[k]),)
        for a, b in ((mus, mus2), (sigs, sigs2), (lds, lds2), (mus, two[0]), (sigs, two[1])):
            assert np.array_equal(a[k], b[k], equal_nan=True)
    for k in ("5", "12"):
        R.compare((mus[k], sigs[k][:, :, None], lds[k]), R.refine(tracks[k], st[k], _ds(S), le=[0.02]), "refine_along_states L=%s" % k)
    nan_rows = np.nonzero(np.isnan(mus["12"]).any(axis=(1, 2)))[0]
    assert list(nan_rows) == [7] and not np.isnan(mus["5"]).any()


def test_refine_along_states_per_peak_errors():
    from extrack_amd import refined_localization as RL
    S = 3
    tracks, states = _dataset(S, [(3, 70), (9, 130)], 3, 8)
    rng = np.random.default_rng(4)
    sig = {k: rng.uniform(0.01, 0.05, v.shape) for k, v in tracks.items()}
    states["9"][5, 2] = -1
    mus, sigs, lds = RL.refine_along_states(tracks, _DT, _params(S, so=(1.2, 0.003)), states=states, nb_states=S, input_LocErr=sig,
                                            return_logdensity=True)
    for k in tracks:
        assert sigs[k].shape == tracks[k].shape
        R.compare((mus[k], sigs[k], lds[k]), R.refine(tracks[k], states[k], _ds(S), sigma=sig[k], slope_offset=(1.2, 0.003)),
                  "refine_along_states per peak L=%s" % k)
    assert np.isnan(lds["9"][5]) and np.isnan(lds["9"]).sum() == 1


# ---- 5. determinism; the other entry points are untouched ---------------------------------------------------------------------------------------
def test_repeatable_and_leaves_the_likelihood_alone(monkeypatch):
    from extrack_amd import engine
    S = 2
    tracks, states = _dataset(S, [(7, 150), (19, 170)], 2, 23)
    ts = engine.TrackSet([tracks["7"], tracks["19"]])
    try:
        model = ts.make_model(np.array([[[0.02]]]), _ds(S), _F[S], _tm(S), _PBL, _CELL, 1, 5)
        ll0, per0 = ts.loglik(model, per_track=True)
        a = ts.refine_fixed_states(model, [states["7"], states["19"]], logdens=True)
        b = ts.refine_fixed_states(model, [states["7"], states["19"]], logdens=True)
        c = ts.refine_fixed_states(model, [states["7"], states["19"]])
        monkeypatch.setenv("EXTRACK_COND_MAX_BLOCKS", "1")  # one block walks every batch
        d = ts.refine_fixed_states(model, [states["7"], states["19"]], logdens=True)
        assert ts.ctx.last_launch_info()["blocks"] == 1
        for x, y, z, w in zip(a, b, c, d):
            assert len(z) == 2 and all(np.array_equal(x[i], y[i]) and np.array_equal(x[i], w[i]) for i in range(3))
            assert np.array_equal(x[0], z[0]) and np.array_equal(x[1], z[1])
        ll1, per1 = ts.loglik(model, per_track=True)
        assert ll0 == ll1 and np.array_equal(per0, per1)
    finally:
        ts.close()


# ---- 6. refusals, each decided on the host with nothing launched ---------------------------------------------------------------------------------
def test_refusals():
    from extrack_amd import _lib, engine
    S = 2
    tracks, states = _dataset(S, [(6, 8)], 2, 3)
    Cs, st = tracks["6"], states["6"]

    def refused(ts, model, st, code):
        with pytest.raises(_lib.ExtrackError) as ei:
            ts.ctx.refine_fixed_states(model, 0, st)
        assert ei.value.code == code
        with pytest.raises(_lib.ExtrackError):  # nothing was launched to find that out
            ts.ctx.last_kernel_ms()

    ts = engine.TrackSet([Cs])
    try:
        model = ts.make_model(np.array([[[0.02]]]), _ds(S), _F[S], _tm(S), _PBL, _CELL, 1, 4)
        bad = st.copy()
        bad[5, 3] = S
        refused(ts, model, bad, _lib.E_INVALID)  # a state >= n_states
        model2 = ts.make_model(np.array([[[0.02]]]), _ds(S), _F[S], _tm(S), _PBL, _CELL, 2, 4)
        refused(ts, model2, st, _lib.E_INVALID)  # nb_substeps 2
        with pytest.raises(ValueError):
            ts.ctx.refine_fixed_states(model, 0, st.astype(np.int32))
    finally:
        ts.close()
    ts = engine.TrackSet([Cs], dts=[np.full((8, 6), _DT)])
    try:
        model = ts.make_model(np.array([[[0.02]]]), np.sqrt(2 * np.array(_D[S])), _F[S], _tm(S), _PBL, _CELL, 1, 4, dt_chunk=2000)
        refused(ts, model, st, _lib.E_UNSUPPORTED)  # per-track time steps
    finally:
        ts.close()
