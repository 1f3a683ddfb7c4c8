"""GPU tests of the gap-aware register-resident 2-state GRADIENT kernels (xt_reg2.h: xt_grad_r2_gap_kernel): a two-state
extrack_loglik_grad_gaps / extrack_loglik_scores_gaps launch with one global localisation error runs with the tangents in registers
(``last_grad_path() == "gaps_reg2"``) instead of the gap instantiation of xt_gradr.h ("gradr").  Frame_len 5, 6, 7 in a default context; frame_len 4
in a context created under EXTRACK_GAP_REG2_F=all (a default one keeps "gradr").  EXTRACK_GRAD_PATH=gradr gives the parent's kernels in the same build.
Reference: tests/golden/r2_grad_gap_reference.npz (tests/r2_grad_gap_cases.py; the CPU test recomputes it and checks that the file is current).
Metrics, unchanged: ``test_emul_grad_gaps.check_against_reference`` and ``assert_bodies_agree`` (1e-9 relative + 1e-12 between two kernel families)."""
import os

import numpy as np
import pytest

import gap_reference as R
import grad_gap_reference as GR
import r2_grad_gap_cases as RC
from oracle import oracle_np as O
from test_emul_grad_gaps import assert_bodies_agree, check_against_reference
from test_grad_edges_cpu import check_gradient
from test_hip_gaps import _case_model, _model, _upload

pytestmark = pytest.mark.gpu


def _context_under(name, value):
    """A context created with the environment variable set (the knobs bind when the context is created)."""
    from extrack_amd import _lib
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return _lib.Context(0)
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


@pytest.fixture(scope="module")
def ctx():
    from extrack_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def all_ctx():
    """EXTRACK_GAP_REG2_F=all: frame_len 4 is upgraded too."""
    c = _context_under("EXTRACK_GAP_REG2_F", "all")
    yield c
    c.close()


@pytest.fixture(scope="module")
def gradr_ctx():
    """EXTRACK_GRAD_PATH=gradr: the parent's path, the gap instantiation of xt_gradr.h."""
    c = _context_under("EXTRACK_GRAD_PATH", "gradr")
    yield c
    c.close()


def _scores(c, case, dirs, gaps=True):
    model = _case_model(case)
    tot, g, B, sc = c.loglik_scores(model, [d[1] for d in dirs], scores=True, gaps=gaps)
    return tot, g, sc, B


def _geometry(c, F):
    info = c.last_launch_info()
    assert info["threads"] == 256 and info["tracks_per_block"] == 4 * (64 >> (F - 1)), info


@pytest.mark.parametrize("D,F", RC.CASES)
def test_cases_against_reference(ctx, all_ctx, D, F):
    """All five buckets of a case in one call each of loglik_scores and loglik_grad: path, geometry, LL, sums and scores against the reference; repeat calls
    give identical bits; OPG = sum s_n s_n^T."""
    c = all_ctx if F == 4 else ctx
    case = RC.make(D, F)
    ref = RC.golden(case, RC.key(D, F))
    _upload(c, case)
    model = _case_model(case)
    tang = [d[1] for d in ref["dirs"]]
    tot, g, sc, B = _scores(c, case, ref["dirs"])
    assert c.last_grad_path() == "gaps_reg2"
    _geometry(c, F)
    _, ll = c.loglik(model, per_track=True, gaps=True)
    check_against_reference("scores call", case, ref, ll, tot, g, sc)
    tot2, g2 = c.loglik_grad(model, tang, gaps=True)
    assert c.last_grad_path() == "gaps_reg2"
    _geometry(c, F)
    assert abs(tot2 - ll.sum()) <= 1e-12 * abs(ll.sum()) and abs(tot - ll.sum()) <= 1e-12 * abs(ll.sum())
    GR.assert_condition("gradient call", ref["gfd"], ref["gest"])
    check_gradient("gradient call", ref["dirs"], g2, ref["gfd"], ref["gest"])
    again = c.loglik_scores(model, tang, scores=True, gaps=True)
    assert again[0] == tot and np.array_equal(again[1], g) and np.array_equal(again[2], B) and np.array_equal(again[3], sc)
    tot3, g3 = c.loglik_grad(model, tang, gaps=True)
    assert tot3 == tot2 and np.array_equal(g3, g2)
    assert np.all(np.abs(B - sc.T @ sc) <= 1e-12 * (np.abs(sc).T @ np.abs(sc)))
    assert c.last_grad_ms() > 0


def test_frame_len_4_in_a_default_context_keeps_the_general_gap_kernels(ctx, all_ctx):
    case = RC.make(1, 4)
    dirs = GR.directions(case)
    res = []
    for c, path in ((ctx, "gradr"), (all_ctx, "gaps_reg2")):
        _upload(c, case)
        tot, g, sc, _ = _scores(c, case, dirs)
        assert c.last_grad_path() == path
        res.append((tot, g, sc))
    assert_bodies_agree(res[0], res[1])


def _gapped(N, L, D, seed):
    from extrack_amd import synth
    Ds, Tm, Fs = R.MODELS[2]
    tr = synth.brownian_tracks(N, L, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=R.DT, dims=D, seed=seed)
    m = np.random.default_rng(seed + 1).random((N, L)) < 0.25
    m[:, 0] = m[:, -1] = False
    full = tr.copy()
    tr[m] = np.nan
    return tr, full


@pytest.mark.parametrize("F", [5, 6, 7])
def test_against_the_general_gap_kernels_in_the_same_build(ctx, gradr_ctx, F):
    """2000 x 12 and one 300 x 40 bucket (blocks walk several batches; two staging chunks), 25 % of the interior rows missed: total, gradient and scores
    against a context created under EXTRACK_GRAD_PATH=gradr."""
    case = RC.simple_case([_gapped(2000, 12, 2, 40 + F)[0], _gapped(300, 40, 2, 50 + F)[0]], 2, F)
    dirs = GR.directions(case)
    res = []
    for c, path in ((ctx, "gaps_reg2"), (gradr_ctx, "gradr")):
        _upload(c, case)
        tot, g, sc, _ = _scores(c, case, dirs)
        assert c.last_grad_path() == path
        assert np.isfinite(tot) and np.all(np.isfinite(sc))
        res.append((tot, g, sc))
    _geometry(ctx, F)
    assert_bodies_agree(res[0], res[1])


@pytest.mark.parametrize("D,F", [(2, 6), (3, 7)])
def test_gap_free_data_agree_with_the_plain_entry_points(ctx, D, F):
    case = RC.simple_case([_gapped(len(b), b.shape[1], D, 3 + i)[1] for i, b in enumerate(RC.make(D, F)["buckets"])], D, F)
    dirs = GR.directions(case)
    _upload(ctx, case)
    a = _scores(ctx, case, dirs)
    assert ctx.last_grad_path() == "gaps_reg2"
    b = _scores(ctx, case, dirs, gaps=False)
    assert ctx.last_grad_path() == "reg2"
    assert np.all(np.isfinite(a[2]))
    assert_bodies_agree(a[:3], b[:3])
    model, tang = _case_model(case), [d[1] for d in dirs]
    assert_bodies_agree(ctx.loglik_grad(model, tang, gaps=True), ctx.loglik_grad(model, tang))


def test_poison_rules(ctx):
    """A row with only some NaN coordinates (first steps, steady state, second chunk), a NaN first and a NaN last row: NaN LL-sum aside, that track's scores
    are NaN and every other row has the bits of the clean call."""
    tr = _gapped(11, 37, 2, 9)[0]
    case = RC.simple_case([tr], 2, 6)
    dirs = GR.directions(case)
    _upload(ctx, case)
    clean = _scores(ctx, case, dirs)
    dirty = tr.copy()
    for i, t, d in ((1, 2, 1), (3, 9, 0), (4, 33, 1)):
        dirty[i, t] = 0.3
        dirty[i, t, d] = np.nan
    dirty[6, 0] = np.nan
    dirty[9, -1] = np.nan
    _upload(ctx, case, buckets=[dirty])
    got = _scores(ctx, case, dirs)
    assert ctx.last_grad_path() == "gaps_reg2"
    _, ll = ctx.loglik(_case_model(case), per_track=True, gaps=True)
    bad = np.zeros(11, bool)
    bad[[1, 3, 4, 6, 9]] = True
    assert np.all(np.isfinite(clean[2])) and np.array_equal(np.isnan(ll), bad)
    assert np.all(np.isnan(got[2][bad])) and np.array_equal(got[2][~bad], clean[2][~bad])


def test_launches_that_are_not_upgraded_report_their_old_family(ctx):
    """Per-peak errors, one error per dimension and three states keep "gradr"; EXTRACK_GRAD_PATH=lds keeps "lds"; values as the reference has them."""
    for S, D, layout, F in ((2, 3, "peak", 5), (2, 2, "globalD", 5), (3, 2, "global1", 5)):
        case = R.make_case(S, D, layout, F)
        _upload(ctx, case)
        tot, g, sc, _ = _scores(ctx, case, GR.directions(case))
        assert ctx.last_grad_path() == "gradr" and np.isfinite(tot), (S, D, layout)
    case = RC.make(2, 6)
    dirs = GR.directions(case)
    _upload(ctx, case)
    up = _scores(ctx, case, dirs)
    assert ctx.last_grad_path() == "gaps_reg2"
    lds = _context_under("EXTRACK_GRAD_PATH", "lds")
    try:
        _upload(lds, case)
        old = _scores(lds, case, dirs)
        assert lds.last_grad_path() == "lds"
    finally:
        lds.close()
    assert_bodies_agree(up[:3], old[:3])


_VALS = dict(D0=1e-3, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1)


def test_forward_gradient_fit_ends_where_the_general_kernels_end():
    """The gradient="forward" fit of the 3000 x 12 dataset of test_hip_grad_gaps.test_forward_gradient_fit_of_gapped_tracks: the objective it reaches is
    within 1e-9 relative of the one the same fit reaches under EXTRACK_GRAD_PATH=gradr."""
    from extrack_amd import synth, tracking as T
    from extrack_amd.lmfit_compat import Parameters
    Tm = O.extract_params(_VALS, 0.02, 1, 1)[3]
    tr = synth.brownian_tracks(3000, 12, [1e-3, 0.25], Tm, [0.6, 0.4], seed=5)
    mask = np.random.default_rng(11).random((3000, 12)) < 0.25
    mask[:, 0] = mask[:, -1] = False
    tr[mask] = np.nan

    def fit():
        p = Parameters()
        for k, v in _VALS.items():
            p.add(k, value=0.4 if k == "D1" else v, min=0.0 if k == "D1" else -np.inf, max=3.0 if k == "D1" else np.inf, vary=k == "D1")
        return T.param_fitting({"12": tr}, 0.02, params=p, gradient="forward", nb_states=2, frame_len=6, verbose=0, cell_dims=[1], gaps=True)
    new = fit()
    old_env = os.environ.get("EXTRACK_GRAD_PATH")
    os.environ["EXTRACK_GRAD_PATH"] = "gradr"
    try:
        old = fit()
    finally:
        if old_env is None:
            del os.environ["EXTRACK_GRAD_PATH"]
        else:
            os.environ["EXTRACK_GRAD_PATH"] = old_env
    print("gaps_reg2: D1 %.6f objective %.9f calls %d; gradr: D1 %.6f objective %.9f calls %d" %
          (new.params["D1"].value, new.residual[0], new.nfev, old.params["D1"].value, old.residual[0], old.nfev))
    assert new.success and new.gradient_path == "analytic" and "gap-aware forward-mode" in new.gradient_why
    assert abs(new.residual[0] - old.residual[0]) <= 1e-9 * abs(old.residual[0])


def test_opg_standard_errors_equal_the_general_kernels():
    """parameter_uncertainties(..., gaps=True, method="opg") on the 300 x 12 set of test_hip_grad_gaps against the same call under EXTRACK_GRAD_PATH=gradr."""
    from extrack_amd import synth, uncertainty as U
    from extrack_amd.lmfit_compat import Parameters
    Tm = O.extract_params(_VALS, 0.02, 1, 1)[3]
    data = {"12": synth.drop_positions(synth.brownian_tracks(300, 12, [1e-3, 0.25], Tm, [0.6, 0.4], seed=21), 0.25, seed=22)}

    def run():
        p = Parameters()
        for k, v in _VALS.items():
            if k != "F1":
                p.add(k, value=v, min=0.0, max=3.0 if k.startswith("D") else 1.0, vary=k != "pBL")
        p.add("F1", expr="1 - F0")
        return U.parameter_uncertainties(data, 0.02, p, nb_states=2, frame_len=6, cell_dims=[1], method="opg", gaps=True)
    new = run()
    old_env = os.environ.get("EXTRACK_GRAD_PATH")
    os.environ["EXTRACK_GRAD_PATH"] = "gradr"
    try:
        old = run()
    finally:
        if old_env is None:
            del os.environ["EXTRACK_GRAD_PATH"]
        else:
            os.environ["EXTRACK_GRAD_PATH"] = old_env
    assert new["covar"] is not None and old["covar"] is not None and new["var_names"] == old["var_names"]
    assert_bodies_agree((new["covar"], [new["stderr"][k] for k in new["var_names"]]), (old["covar"], [old["stderr"][k] for k in old["var_names"]]))
