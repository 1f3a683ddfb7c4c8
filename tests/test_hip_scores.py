"""GPU tests of the per-track scores and their outer-product sum (extrack_loglik_scores, csrc/xt_opg.h) and of the standard errors built on
them (extrack_amd.uncertainty).  Everything goes through the C ABI.  Reference for a score: Richardson-extrapolated central differences
of the pinned oracle's PER-TRACK log-likelihood (the unsummed form of test_grad_cpu.oracle_fd_gradient), with the project's gradient
tolerance applied per track: |s - fd| <= 1e-6 max(|fd|, 1e-3 max_p |fd_n|)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, case_inputs
from test_grad_cpu import _richardson, model_directions

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
OPG_TILE = 1024  # EXTRACK_OPG_TILE (include/extrack_hip.h): rows per first-stage workgroup of the OPG reduction


def oracle_fd_scores(Cs, LEfun, ds2, Fs, T, pBL, isBL, cell, ns, F, min_len, dirs):
    """[N, n_dir]: d LL_n / d theta by Richardson central differences of oracle_np.proba_cs.  LEfun(x, d) -> the LocErr array of the model
    displaced by x along direction d (global error [1, 1, K] or per-peak [N, L, K])."""
    from oracle import oracle_np as O

    def per_track(x, d):
        return O.proba_cs(Cs, LEfun(x, d), np.sqrt(ds2 + x * d.get("ds2", 0.0)), Fs + x * d.get("Fs", 0.0), T + x * d.get("T", 0.0),
                          pBL + x * d.get("pBL", 0.0), isBL, cell, ns, F, min_len)

    return np.stack([_richardson(lambda x: per_track(x, d), h) for _, _, d, h in dirs], axis=1)


def assert_scores_match(sc, fd, what=""):
    tol = 1e-6 * np.maximum(np.abs(fd), 1e-3 * np.abs(fd).max(axis=1, keepdims=True))
    bad = np.abs(sc - fd) > tol
    print("%s scores vs oracle differences: worst |s - fd| / tol = %.3g over %s" % (what, (np.abs(sc - fd) / tol).max(), sc.shape))
    assert not bad.any(), (what, np.argwhere(bad)[:5], sc[bad][:5], fd[bad][:5])


def assert_consistent(ll, g, B, sc, what=""):
    """Derived bounds: the kernels and numpy add the same N numbers per column in different orders - each sum carries at most
    (N - 1) eps sum|x| of rounding, so the two differ by less than 2 N eps sum|x|; 4 N eps sum|x| leaves room for the fused multiply-adds
    of the device's products."""
    N = len(sc)
    tol_g = 4 * N * EPS * np.abs(sc).sum(0)
    assert np.all(np.abs(sc.sum(0) - g) <= tol_g), (what, sc.sum(0) - g, tol_g)
    tol_B = 4 * N * EPS * (np.abs(sc).T @ np.abs(sc))
    assert np.all(np.abs(sc.T @ sc - B) <= tol_B), (what, np.abs(sc.T @ sc - B).max())
    assert np.array_equal(B, B.T), what


# ---- 3. scores against the oracle on golden kernel cases ------------------------------------------------------------------------------
# (path = EXTRACK_GRAD_PATH, golden case id, localisation error: "global" | "peak" (per-peak sigma) | "affine" (clip(sigma slope + offset)))
_GOLDEN_CASES = [
    (None, 189, "global"),     # xt_reg2.h: 2 states, 10 directions = two passes, pBL rides along as a uniform direction
    (None, 191, "global"),     # xt_reg2.h: one error per dimension (11 directions)
    (None, 101, "global"),     # xt_reg2.h: frame_len 4
    (None, 329, "global"),     # 3 states by default: forward mode (xt_gradr.h) although loglik_grad would take the reverse-mode kernels
    ("gradr", 253, "global"),  # xt_gradr.h: 3 states
    ("gradr", 673, "global"),  # xt_gradr.h: 2 states, nb_substeps 2
    ("gradr", 393, "global"),  # xt_gradr.h: 4 states
    ("lds", 189, "global"),    # xt_grad.h
    ("lds", 253, "global"),    # xt_grad.h: 3 states
    ("lds", 877, "global"),    # xt_grad.h: 2 states, nb_substeps 3
    (None, 192, "peak"),       # per-peak errors (xt_gradr.h: the 2-state register kernel takes a global error only)
    ("lds", 196, "affine"),    # per-peak errors through slope / offset, 3 dims
]


@pytest.mark.parametrize("path,cid,errmode", _GOLDEN_CASES)
def test_scores_vs_oracle_on_golden_models(kernel_cases, path, cid, errmode, monkeypatch):
    from extrack_amd import tracking as T
    if path:
        monkeypatch.setenv("EXTRACK_GRAD_PATH", path)  # read when a context is created
    meta, data = kernel_cases
    row = meta[cid]
    assert row["id"] == cid
    x = case_inputs(row, data)
    Cs, LE = x["Cs"], x["LE"]
    S, ns, F = len(x["ds"]), row["ns"], row["F"]
    # the selection rule of test_gradient_vs_oracle_central_differences_on_golden_models
    assert S <= 4 and S ** F <= 300 and Cs.shape[1] >= 3 and not np.any(x["ds"] <= 0)
    ds2, cell = np.asarray(x["ds"], float) ** 2, row["cell_dims"]
    Fs, Tm, pBL = np.asarray(x["Fs"], float), np.asarray(x["T"], float), row["pBL"]
    if errmode == "global":
        assert LE.shape[1] == 1
        K = LE.shape[2]
        le = LE[0, 0].astype(float)
        dirs = model_directions(S, K, ns, ds2, Tm, le, cell)
        LEfun = lambda xx, d: (le + xx * d.get("le", 0.0))[None, None]
        sigma, so = LE, None
    else:
        assert LE.shape[1] == Cs.shape[1]
        dirs = model_directions(S, 0, ns, ds2, Tm, np.zeros(0), cell)
        if errmode == "peak":
            LEfun = lambda xx, d: LE
            sigma, so = LE, None
        else:
            so = (1.15, 0.003)
            dirs = dirs + [("slope", dict(slope=1.0), dict(slope=1.0), 1e-3), ("offset", dict(offset=1.0), dict(offset=1.0), 1e-5)]
            LEfun = lambda xx, d: np.clip(LE * (so[0] + xx * d.get("slope", 0.0)) + so[1] + xx * d.get("offset", 0.0), 1e-6, None)
            sigma = LE
    ts, _ = T._one_bucket(Cs, sigma, row["isBL"], row["min_len"], 0)
    try:
        if errmode == "global":
            model = ts.make_model(LE, x["ds"], Fs, Tm, pBL, cell, ns, F)
        else:
            model = ts.make_model(None, x["ds"], Fs, Tm, pBL, cell, ns, F, slope_offset=so)
        ll, g, B, sc = ts.ctx.loglik_scores(model, [d[1] for d in dirs], scores=True)
        ll_pt = ts.loglik(model, per_track=True)[1]
    finally:
        ts.close()
    if errmode != "affine":
        assert abs(ll - x["LPC"].sum()) < 1e-10 * max(1.0, abs(ll))
    assert abs(ll - ll_pt.sum()) < 1e-10 * max(1.0, abs(ll))
    assert sc.shape == (len(Cs), len(dirs))
    fd = oracle_fd_scores(Cs, LEfun, ds2, Fs, Tm, pBL, row["isBL"], cell, ns, F, row["min_len"], dirs)
    assert_scores_match(sc, fd, "golden %d %s %s:" % (cid, path, errmode))
    assert_consistent(ll, g, B, sc)


# ---- shared synthetic data: one 2-state and one 3-state model, references computed once -------------------------------------------------
_DT, _CELL, _PBL, _MINLEN = 0.02, [1.0], 0.08, 3
_MODELS = {2: (np.array([0.004, 0.25]), np.array([[0.9, 0.1], [0.15, 0.85]]), np.array([0.6, 0.4])),
           3: (np.array([0.004, 0.06, 0.3]), np.array([[0.88, 0.07, 0.05], [0.06, 0.9, 0.04], [0.05, 0.08, 0.87]]), np.array([0.3, 0.3, 0.4]))}
_LE = np.array([0.02])
_POOL = {}


def _dirs(S, ns=1):
    Ds, Tm, Fs = _MODELS[S]
    return model_directions(S, 1, ns, 2 * Ds * _DT, Tm, _LE, _CELL)


def _pool(S, L, N, F, isBL):
    """(tracks [N, L, 2], oracle scores [N, n_dir]) of the shared model, computed once per shape."""
    key = (S, L, N, F, isBL)
    if key not in _POOL:
        from extrack_amd import synth
        Ds, Tm, Fs = _MODELS[S]
        Cs = synth.brownian_tracks(N, L, Ds, Tm, Fs, seed=100 * S + L, dims=2)
        fd = oracle_fd_scores(Cs, lambda xx, d: (_LE + xx * d.get("le", 0.0))[None, None], 2 * Ds * _DT, Fs, Tm, _PBL, isBL, _CELL, 1, F, _MINLEN,
                              _dirs(S))
        fd.setflags(write=False)
        Cs.setflags(write=False)
        _POOL[key] = (Cs, fd)
    return _POOL[key]


def _model_of(ts, S, F):
    Ds, Tm, Fs = _MODELS[S]
    return ts.make_model(_LE[None, None], np.sqrt(2 * Ds * _DT), Fs, Tm, _PBL, _CELL, 1, F)


_FAMILIES = [("reg2", 2), ("gradr", 3), ("lds", 2)]  # (EXTRACK_GRAD_PATH, states): xt_reg2.h, xt_gradr.h, xt_grad.h


# the 2-state model for every family here (EXTRACK_GRAD_PATH=gradr puts xt_gradr.h before xt_reg2.h): one oracle reference of 3073 tracks
@pytest.mark.parametrize("path,S", [("reg2", 2), ("gradr", 2), ("lds", 2)])
def test_scores_at_the_block_and_tile_edges(path, S, monkeypatch):
    """N = 1, one less than / equal to / one more than the tracks per workgroup of the family (read from extrack_last_launch_info), and
    three OPG reduction tiles plus one row: every row against the oracle, column sums and outer products against grad and opg."""
    from extrack_amd import tracking as T
    monkeypatch.setenv("EXTRACK_GRAD_PATH", path)
    L, F = 5, 4
    Cs, fd = _pool(S, L, 3 * OPG_TILE + 1, F, 1)
    dirs = [d[1] for d in _dirs(S)]
    ts = T.TrackSet([Cs[:1]], None, min_len=_MINLEN, max_len=L + 1)
    try:
        ts.ctx.loglik_scores(_model_of(ts, S, F), dirs)
        tpb = ts.ctx.last_launch_info()["tracks_per_block"]
    finally:
        ts.close()
    assert 1 <= tpb < OPG_TILE
    for N in sorted({1, max(tpb - 1, 1), tpb, tpb + 1, 3 * OPG_TILE + 1}):
        ts = T.TrackSet([Cs[:N]], None, min_len=_MINLEN, max_len=L + 1)
        try:
            model = _model_of(ts, S, F)
            ll, g, B, sc = ts.ctx.loglik_scores(model, dirs, scores=True)
            ll2, g2 = ts.ctx.loglik_grad(model, dirs)
            assert ts.ctx.last_launch_info()["tracks_per_block"] == tpb
        finally:
            ts.close()
        assert sc.shape == (N, len(dirs))
        assert_scores_match(sc, fd[:N], "%s N=%d:" % (path, N))
        assert_consistent(ll, g, B, sc, (path, N))
        assert abs(ll - ll2) <= 1e-12 * abs(ll) and np.all(np.abs(sc.sum(0) - g2) <= 4 * N * EPS * np.abs(sc).sum(0))


@pytest.mark.parametrize("path,S", _FAMILIES)
def test_scores_rows_of_several_buckets_and_shortest_tracks(path, S, monkeypatch):
    """Buckets are launched longest first but their rows are those of the upload order: L = 3 (5 tracks) uploaded before L = 9 (70 tracks).
    Then L = 2, 3 and 4 with frame_len 6: no recursion step (the score comes from the first and last position terms only) and tracks
    shorter than the window."""
    from extrack_amd import tracking as T
    monkeypatch.setenv("EXTRACK_GRAD_PATH", path)
    dirs = [d[1] for d in _dirs(S)]
    for shapes, F in ((((3, 5), (9, 70)), 4), (((2, 6), (3, 7), (4, 9)), 6)):
        Lmax = max(L for L, _ in shapes)
        parts = [_pool(S, L, N, F, int(L != Lmax)) for L, N in shapes]
        ts = T.TrackSet([p[0] for p in parts], None, min_len=_MINLEN, max_len=Lmax)
        try:
            model = _model_of(ts, S, F)
            ll, g, B, sc = ts.ctx.loglik_scores(model, dirs, scores=True)
            ll_pt = ts.loglik(model, per_track=True)[1]
        finally:
            ts.close()
        fd = np.concatenate([p[1] for p in parts])
        assert sc.shape == fd.shape and len(ll_pt) == len(fd)
        assert_scores_match(sc, fd, "%s buckets %s:" % (path, shapes))
        assert_consistent(ll, g, B, sc, (path, shapes))


@pytest.mark.parametrize("path,S", _FAMILIES)
def test_nan_position_poisons_its_row_only(path, S, monkeypatch):
    from extrack_amd import tracking as T
    monkeypatch.setenv("EXTRACK_GRAD_PATH", path)
    L, F, N = 9, 4, 70
    Cs = np.array(_pool(S, L, N, F, 0)[0])
    dirs = [d[1] for d in _dirs(S)]
    out = []
    for poison in (False, True):
        if poison:
            Cs[17, 2, 0] = np.nan
        ts = T.TrackSet([Cs], None, min_len=_MINLEN, max_len=L)
        try:
            out.append(ts.ctx.loglik_scores(_model_of(ts, S, F), dirs, scores=True))
        finally:
            ts.close()
    (ll0, g0, B0, s0), (ll1, g1, B1, s1) = out
    assert np.all(np.isfinite(s0)) and np.all(np.isfinite(B0))
    assert np.all(np.isnan(s1[17])) and np.isnan(ll1) and np.all(np.isnan(g1))
    keep = np.arange(N) != 17
    assert np.array_equal(s1[keep], s0[keep])
    assert not np.all(np.isfinite(B1))


# ---- 4. + 6. self-consistency, reproducibility, the existing entry point before and after -----------------------------------------------
def _c1(rows=300):
    info = json.load(open(os.path.join(GOLDEN, "c1_simfov_10k.json")))
    data = np.load(os.path.join(GOLDEN, "c1_simfov_10k.npz"))
    return info, {k: data["tr_" + k][:rows] for k in info["keys"]}


@pytest.mark.parametrize("path", [None, "gradr", "lds"])
def test_scores_grad_and_opg_are_consistent_and_reproducible(path, monkeypatch):
    """16 length buckets of the configs[0] fixture, the 7 free parameters of a 2-state fit as directions (parameter-level tangents).
    loglik_grad on the same context gives bit-identical (ll, g) before and after a scores call; two scores calls are bit-identical."""
    from extrack_amd import gradient, tracking as T
    if path:
        monkeypatch.setenv("EXTRACK_GRAD_PATH", path)
    info, tr = _c1()
    p = T.generate_params(nb_states=2, LocErr_type=1, LocErr_bounds=[0.005, 0.1], D_max=3, estimated_Ds=[0.002, 0.2], estimated_Fs=[0.55],
                          estimated_transition_rates=[0.08, 0.12])
    p["pBL"].value = 0.07
    names = gradient.free_names(p)
    _, lst, _ = T.engine.sort_buckets(tr)
    ts = T.TrackSet(lst)
    try:
        model = T._objective_model(p, ts, info["dt"], info["cell_dims"], None, 2, 1, 6, 1)
        tang = gradient.model_tangents(p, info["dt"], 1, 1, info["cell_dims"], names)
        before = ts.ctx.loglik_grad(model, tang)
        a = ts.ctx.loglik_scores(model, tang, scores=True)
        after = ts.ctx.loglik_grad(model, tang)
        b = ts.ctx.loglik_scores(model, tang, scores=True)
        c = ts.ctx.loglik_scores(model, tang)
    finally:
        ts.close()
    assert before[0] == after[0] and np.array_equal(before[1], after[1])
    ll, g, B, sc = a
    N = ts.n_tracks
    assert sc.shape == (N, len(names)) and B.shape == (len(names),) * 2
    assert_consistent(ll, g, B, sc, path)
    assert abs(ll - before[0]) <= 1e-12 * abs(ll)
    assert np.all(np.abs(sc.sum(0) - before[1]) <= 4 * N * EPS * np.abs(sc).sum(0))
    assert a[0] == b[0] == c[0]
    for u, v in zip(a[1:], b[1:]):
        assert np.array_equal(u, v)
    assert np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2])


def test_scores_argument_checks():
    from extrack_amd import _lib, tracking as T
    Cs = _pool(2, 5, 8, 4, 1)[0]
    ts = T.TrackSet([Cs], None, min_len=_MINLEN, max_len=6)
    try:
        model = _model_of(ts, 2, 4)
        with pytest.raises(_lib.ExtrackError) as e:
            ts.ctx.loglik_scores(model, [])
        assert e.value.code == _lib.E_INVALID
        with pytest.raises(_lib.ExtrackError) as e:
            ts.ctx.loglik_scores(model, [dict(pBL=1.0)] * 33)
        assert e.value.code == _lib.E_UNSUPPORTED
    finally:
        ts.close()


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------------
def test_param_fitting_with_uncertainties_end_to_end(capsys):
    """configs[0] fixture, first 300 rows per key.  fit.covar must be the inverse of the numpy OPG of track_scores at the fitted
    parameters: 1e-9 relative to sqrt(C_ii C_jj), the natural scale of a covariance entry (both inversions work on a matrix that is
    well conditioned once the parameters' units are scaled out).  Hessian and sandwich covariances on the same fit: finite, symmetric,
    positive definite - and the ratio of their standard errors to the OPG ones is printed, not bounded (it tends to 1 only
    asymptotically and under correct specification)."""
    from extrack_amd import gradient, tracking as T, uncertainty as U
    info, tr = _c1()
    dt, cell = info["dt"], info["cell_dims"]
    p0 = T.generate_params(nb_states=2, LocErr_type=1, LocErr_bounds=[0.005, 0.1], D_max=3, estimated_Ds=[0.002, 0.2], estimated_Fs=[0.55],
                           estimated_transition_rates=[0.08, 0.12])
    kw = dict(params=p0, nb_states=2, frame_len=6, verbose=0, method="bfgs", cell_dims=cell, gradient="analytic")
    fit = T.param_fitting(tr, dt, uncertainties="opg", **kw)
    plain = T.param_fitting(tr, dt, uncertainties=None, **kw)
    with pytest.raises(NotImplementedError):
        T.param_fitting(tr, dt, fusion="threshold", uncertainties=True, **kw)
    capsys.readouterr()
    assert plain.errorbars is False and all(q.stderr is None for q in plain.params.values()) and not hasattr(plain, "covar")
    for k in plain.params:
        assert plain.params[k].value == fit.params[k].value  # the fit itself is untouched
    print("uncertainties:", fit.uncertainty_message)
    assert fit.errorbars is True and fit.uncertainty_method == "opg"
    kept = fit.uncertainty_var_names
    free = gradient.free_names(fit.params)
    assert set(kept) <= set(free) and len(kept) >= 5
    sc = U.track_scores(tr, dt, fit.params, nb_states=2, frame_len=6, cell_dims=cell)
    assert sorted(sc, key=int) == sorted(tr, key=int) and all(sc[k].shape == (len(tr[k]), len(free)) for k in tr)
    Sm = np.concatenate([sc[k] for k in sorted(sc, key=int)])[:, [free.index(k) for k in kept]]
    C = np.linalg.inv(Sm.T @ Sm)
    sd = np.sqrt(np.diag(C))
    rel = np.abs(fit.covar - C) / np.outer(sd, sd)
    print("covar vs inv(numpy OPG): worst relative difference %.3g" % rel.max())
    assert rel.max() <= 1e-9
    for i, k in enumerate(kept):
        assert fit.params[k].stderr == np.sqrt(fit.covar[i, i]) and fit.params[k].stderr > 0
        assert set(fit.params[k].correl) == set(kept) - {k}
    for k in free:
        if k not in kept:
            assert fit.params[k].stderr is None and k in fit.uncertainty_message
    if "F0" in kept:
        assert abs(fit.params["F1"].stderr - fit.params["F0"].stderr) <= 1e-12 * fit.params["F0"].stderr
    res = {m: U.parameter_uncertainties(tr, dt, fit.params, nb_states=2, frame_len=6, cell_dims=cell, method=m) for m in ("hessian", "sandwich")}
    for m, r in res.items():
        assert r["covar"] is not None, r["message"]
        assert r["var_names"] == kept and np.all(np.isfinite(r["covar"])) and np.array_equal(r["covar"], r["covar"].T)
        assert np.linalg.eigvalsh(r["covar"])[0] > 0
    assert np.all(np.abs(res["sandwich"]["opg"] - Sm.T @ Sm) <= 4 * len(Sm) * EPS * (np.abs(Sm).T @ np.abs(Sm)))
    print("parameter : value, stderr opg, stderr hessian / opg, stderr sandwich / opg")
    for i, k in enumerate(kept):
        print("%-8s %.6g %.3g %.3f %.3f" % (k, fit.params[k].value, fit.params[k].stderr, res["hessian"]["stderr"][k] / fit.params[k].stderr,
                                            res["sandwich"]["stderr"][k] / fit.params[k].stderr))
