"""GPU tests of the gap-aware gradient, per-track scores and standard errors (extrack_loglik_grad_gaps / extrack_loglik_scores_gaps, DESIGN.md
section 21) against Richardson differences of the reference built from the unchanged oracle: tests/grad_gap_reference.py, read from
tests/golden/grad_gap_reference.npz (the CPU test test_emul_grad_gaps.py recomputes it and checks that the file is current).
Metric of gradient and scores: ``test_grad_edges_cpu.check_gradient`` with the reference's own condition asserted first; LL tolerances are
those of tests/test_hip_gaps.py (per track rtol 1e-13 / atol 1e-10, totals 1e-12 relative)."""
import numpy as np
import pytest

import gap_reference as R
import grad_gap_reference as GR
from oracle import oracle_np as O
from test_emul_grad_gaps import assert_bodies_agree, check_against_reference
from test_grad_edges_cpu import check_gradient
from test_hip_gaps import _case_model, _model, _upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from extrack_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _evaluate(ctx, case, dirs, gaps=True):
    """(LL [sum N], sum LL, gradient, scores, opg) of the uploaded case: per-track LL from the likelihood call, the rest from ONE scores call."""
    model = _case_model(case)
    tang = [d[1] for d in dirs]
    tot, g, B, sc = ctx.loglik_scores(model, tang, scores=True, gaps=gaps)
    _, ll = ctx.loglik(model, per_track=True, gaps=gaps)
    return ll, tot, g, sc, B


@pytest.mark.parametrize("S,D,layout,F", GR.CASES)
def test_gap_gradient_and_scores_against_reference(ctx, S, D, layout, F):
    """All buckets of the case in one call each of loglik_grad and loglik_scores (2 and 3 states at frame_len 5, 4 states at frame_len 3:
    xt_gradr.h, passes of 3 or 4 directions)."""
    case = R.make_case(S, D, layout, F)
    ref = GR.reference(case, (S, D, layout, F), golden=True)
    _upload(ctx, case)
    model = _case_model(case)
    tang = [d[1] for d in ref["dirs"]]
    ll, tot, g, sc, B = _evaluate(ctx, case, ref["dirs"])
    assert ctx.last_launch_info()["threads"] <= 256
    check_against_reference("scores call", case, ref, ll, tot, g, sc)
    tot2, g2 = ctx.loglik_grad(model, tang, gaps=True)
    assert abs(tot2 - ll.sum()) <= 1e-12 * abs(ll.sum()) and abs(tot - ll.sum()) <= 1e-12 * abs(ll.sum())  # the value of ctx.loglik(gaps=True)
    GR.assert_condition("gradient call", ref["gfd"], ref["gest"])
    check_gradient("gradient call", ref["dirs"], g2, ref["gfd"], ref["gest"])
    # two calls give the same bits; the outer products are those of the returned scores
    again = ctx.loglik_scores(model, tang, scores=True, gaps=True)
    assert again[0] == tot and np.array_equal(again[1], g) and np.array_equal(again[2], B) and np.array_equal(again[3], sc)
    tot3, g3 = ctx.loglik_grad(model, tang, gaps=True)
    assert tot3 == tot2 and np.array_equal(g3, g2)
    assert np.all(np.abs(B - sc.T @ sc) <= 1e-12 * (np.abs(sc).T @ np.abs(sc)))
    assert ctx.last_grad_ms() > 0


def test_lds_fallback_beyond_256_groups(ctx):
    """2 states at frame_len 10: 512 groups of sequences per track, more than xt_gradr.h serves - the LDS-resident body, one track per
    workgroup of 512 threads, one direction per pass (xt_gradr.h never launches more than 256 threads).  The model the fallback was first
    meant to be shown on, 4 states at frame_len 6, fits neither kernel (two primal regions of 128 KiB) and is refused: test_host_decided_refusals."""
    case = GR.lds_case()
    ref = GR.reference(case, "lds", golden=True)
    _upload(ctx, case)
    ll, tot, g, sc, B = _evaluate(ctx, case, ref["dirs"])
    tot2, g2 = ctx.loglik_grad(_case_model(case), [d[1] for d in ref["dirs"]], gaps=True)
    info = ctx.last_launch_info()
    assert info["threads"] > 256 and info["tracks_per_block"] == 1, info
    check_against_reference("lds scores call", case, ref, ll, tot, g, sc)
    check_gradient("lds gradient call", ref["dirs"], g2, ref["gfd"], ref["gest"])
    assert abs(tot2 - ll.sum()) <= 1e-12 * abs(ll.sum())
    assert np.all(np.abs(B - sc.T @ sc) <= 1e-12 * (np.abs(sc).T @ np.abs(sc)))


@pytest.mark.parametrize("S,D,layout,F", [(3, 2, "global1", 5), (2, 2, "global1", 6), (4, 3, "peak", 3), (2, 1, "affine", 5)])
def test_gap_free_data_agree_with_the_plain_entry_points(ctx, S, D, layout, F):
    """No missed detection: the gap entry points return what the plain ones do, up to the rounding of another kernel family (two states with a
    global error: the plain call runs xt_reg2.h; three and four states: the plain gradient call runs xt_rev.h)."""
    from extrack_amd import synth
    case = R.make_case(S, D, layout, F)
    Ds, Tm, Fs = R.MODELS[S]
    full = [synth.brownian_tracks(len(b), b.shape[1], list(Ds), Tm.tolist(), list(Fs), dt=R.DT, dims=D, seed=3 + i) for i, b in enumerate(case["buckets"])]
    if case["sig"] is not None:
        case["sig"] = [np.where(np.isfinite(s) & (s < 100), s, 0.03) for s in case["sig"]]
    _upload(ctx, case, buckets=full)
    model = _case_model(case)
    tang = [d[1] for d in GR.directions(case)]
    a = ctx.loglik_scores(model, tang, scores=True, gaps=True)
    b = ctx.loglik_scores(model, tang, scores=True)
    assert np.all(np.isfinite(a[3]))
    assert_bodies_agree((a[0], a[1], a[3]), (b[0], b[1], b[3]))
    assert_bodies_agree(ctx.loglik_grad(model, tang, gaps=True), ctx.loglik_grad(model, tang))


def test_host_decided_refusals(ctx):
    from extrack_amd import _lib
    case = R.make_case(2, 2, "global1", 4)
    _upload(ctx, case)
    model = _case_model(case)
    tang = [d[1] for d in GR.directions(case)]
    ctx.loglik_grad(model, tang, gaps=True)
    info = ctx.last_launch_info()
    two = _model(2, 4, R.MIN_LEN, 40, le=[0.02], nb_substeps=2)
    Ds5 = np.array([0.001, 0.01, 0.05, 0.1, 0.4])
    T5 = np.full((5, 5), 0.03) + np.eye(5) * 0.85
    ds5 = np.sqrt(2 * Ds5 * R.DT)
    five = _lib.ModelHandle(ds5, np.full(5, 0.2), T5, O.p_stay_table(ds5, 5, 1, R.CELL), R.PBL, 1, 3, R.MIN_LEN, 40, locerr=[0.02])
    # 4 states at frame_len 6: 1024 groups are too many for xt_gradr.h, and two primal regions of 4^6 sequences too much LDS for xt_grad.h
    six = _model(4, 6, R.MIN_LEN, 40, le=[0.02])
    t2 = [dict(pBL=1.0)]
    for m in (two, five, six):
        for call in (lambda: ctx.loglik_grad(m, t2, gaps=True), lambda: ctx.loglik_scores(m, t2, gaps=True)):
            with pytest.raises(_lib.ExtrackError) as e:
                call()
            assert e.value.code == _lib.E_UNSUPPORTED and ctx.last_launch_info() == info
    ctx.set_bucket_dt(1, np.full(case["buckets"][1].shape[:2], R.DT))
    for call in (lambda: ctx.loglik_grad(model, tang, gaps=True), lambda: ctx.loglik_scores(model, tang, gaps=True)):
        with pytest.raises(_lib.ExtrackError) as e:
            call()
        assert e.value.code == _lib.E_UNSUPPORTED and ctx.last_launch_info() == info
    ctx.set_bucket_dt(1, None)
    ll, g = ctx.loglik_grad(model, tang, gaps=True)  # the context is usable afterwards
    assert np.isfinite(ll) and np.all(np.isfinite(g))
    assert ctx.loglik_grad(model, [], gaps=True)[0] == ctx.loglik(model, gaps=True)  # no direction: the gap-aware likelihood


# ---- parameter level: 300 tracks x 12, 2 states, 25 % of the interior rows missed

_VALS = dict(D0=1e-3, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1)


def _params(vals=_VALS):
    from extrack_amd.lmfit_compat import Parameters
    p = Parameters()
    for k, v in vals.items():
        if k != "F1":  # one bucket, the longest: no leaving term, the data do not see pBL (it stays fixed)
            p.add(k, value=v, min=0.0, max=3.0 if k.startswith("D") else 1.0, vary=k != "pBL")
    p.add("F1", expr="1 - F0")
    return p


@pytest.fixture(scope="module")
def gapped300():
    from extrack_amd import synth
    Tm = O.extract_params(_VALS, 0.02, 1, 1)[3]
    return {"12": synth.drop_positions(synth.brownian_tracks(300, 12, [1e-3, 0.25], Tm, [0.6, 0.4], seed=21), 0.25, seed=22)}


def test_objective_gradient_and_track_scores_of_a_gapped_trackset(gapped300):
    from test_grad_cpu import _richardson
    from extrack_amd import engine, gradient, uncertainty as U
    p = _params()
    names = gradient.free_names(p)
    ts = engine.TrackSet([gapped300["12"]], None, device=0, gaps=True)
    try:
        f, g = gradient.objective_and_gradient(p, ts, 0.02, [1], 2, 1, 6)
        sc = U.track_scores(ts, 0.02, p, nb_states=2, frame_len=6, cell_dims=[1])["12"]
    finally:
        ts.close()

    def obj(name, x):
        v = {k: q.value for k, q in p.items()}
        v[name] += x
        v["F1"] = 1 - v["F0"]
        return R.objective(v, gapped300, 0.02, (1,), 6)
    lv = [np.array([_richardson(lambda x: obj(n, x), 1e-4 * p[n].value * hs) for n in names]) for hs in (1.0, 0.5)]
    fd, est = lv[1], np.abs(lv[1] - lv[0])
    ref0 = obj(names[0], 0.0)
    assert abs(f - ref0) <= 1e-9 * abs(ref0), (f, ref0)  # the bound of test_hip_gaps.py's fit on its objective
    dirs = [(n,) for n in names]
    GR.assert_condition("objective_and_gradient", fd, est)
    check_gradient("objective_and_gradient", dirs, g, fd, est)
    # scores are d LL_n / d theta, the objective is -sum LL: the rows sum to minus its gradient
    assert sc.shape == (300, len(names))
    assert np.all(np.abs(sc.sum(0) + g) <= 4 * 300 * 2.0 ** -52 * np.abs(sc).sum(0))
    assert U.track_scores(gapped300, 0.02, p, nb_states=2, frame_len=6, cell_dims=[1], gaps=True)["12"].tobytes() == sc.tobytes()


def test_parameter_uncertainties_of_gapped_tracks(gapped300):
    from extrack_amd import uncertainty as U
    p = _params()
    res = {m: U.parameter_uncertainties(gapped300, 0.02, p, nb_states=2, frame_len=6, cell_dims=[1], method=m, gaps=True) for m in U.METHODS}
    for m, r in res.items():
        assert r["covar"] is not None, (m, r["message"])
        assert np.all(np.isfinite(r["covar"])) and np.linalg.eigvalsh(r["covar"])[0] > 0, m
        print(m, {k: "%.3g" % r["stderr"][k] for k in r["var_names"]})
    for k in res["opg"]["var_names"]:
        ratio = res["hessian"]["stderr"][k] / res["opg"]["stderr"][k]
        assert 0.5 <= ratio <= 2.0, (k, ratio)


def test_forward_gradient_fit_of_gapped_tracks():
    """The 3000 x 12 dataset of test_hip_gaps.py's fit: the exact gap-aware gradient ends where the differenced objective does, in fewer
    objective calls."""
    from extrack_amd import synth, tracking as T
    from extrack_amd.lmfit_compat import Parameters
    Tm = O.extract_params(_VALS, 0.02, 1, 1)[3]
    tr = synth.brownian_tracks(3000, 12, [1e-3, 0.25], Tm, [0.6, 0.4], seed=5)
    mask = np.random.default_rng(11).random((3000, 12)) < 0.25
    mask[:, 0] = mask[:, -1] = False
    gapped = tr.copy()
    gapped[mask] = np.nan

    def start():
        p = Parameters()
        for k, v in _VALS.items():
            p.add(k, value=0.4 if k == "D1" else v, min=0.0 if k == "D1" else -np.inf, max=3.0 if k == "D1" else np.inf, vary=k == "D1")
        return p
    kw = dict(nb_states=2, frame_len=6, verbose=0, cell_dims=[1], gaps=True)
    fwd = T.param_fitting({"12": gapped}, 0.02, params=start(), gradient="forward", **kw)
    fdf = T.param_fitting({"12": gapped}, 0.02, params=start(), **kw)
    print("forward: D1 %.5f objective %.9f calls %d (%s); differenced: D1 %.5f objective %.9f calls %d" %
          (fwd.params["D1"].value, fwd.residual[0], fwd.nfev, fwd.message, fdf.params["D1"].value, fdf.residual[0], fdf.nfev))
    assert fwd.gradient_path == "analytic" and "gap-aware forward-mode" in fwd.gradient_why and fdf.gradient_path == "fd"
    assert fwd.success
    assert 0.22 <= fwd.params["D1"].value <= 0.29
    assert fwd.residual[0] <= fdf.residual[0] + 1e-9 * abs(fdf.residual[0])
    assert fwd.nfev < fdf.nfev, (fwd.nfev, fdf.nfev)
