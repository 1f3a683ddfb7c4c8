"""GPU tests of the gap-aware reverse-mode gradient (xt_rev_gap_kernel behind extrack_loglik_grad_gaps) against Richardson
differences of the reference built from the unchanged oracle: tests/grad_gap_reference.py, read from tests/golden/grad_gap_reference.npz and
tests/golden/rev_gap_reference.npz (the CPU test test_emul_rev_gaps.py recomputes them and checks that the files are current), and against the
forward-mode gap kernels of a context created under EXTRACK_GRAD_PATH=gradr.
Metric of the gradient: ``test_grad_edges_cpu.check_gradient`` with the reference's own condition asserted first; totals 1e-12 relative; kernel
family against kernel family by ``test_emul_grad_gaps.assert_bodies_agree`` (1e-9 |y| + 1e-12)."""
import os

import numpy as np
import pytest

import gap_reference as R
import grad_gap_reference as GR
import rev_gap_reference as RG
from test_emul_grad_gaps import assert_bodies_agree
from test_grad_edges_cpu import check_gradient
from test_grad_gap_rev_cpu import NBUF1_MODEL, NBUF2_MODEL
from test_hip_gaps import _case_model, _model, _upload

pytestmark = pytest.mark.gpu


def _context_under(**env):
    """A context created with the environment variables set (the knobs bind when the context is created)."""
    from extrack_amd import _lib
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _lib.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx():
    from extrack_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_gradr():
    c = _context_under(EXTRACK_GRAD_PATH="gradr")
    yield c
    c.close()


@pytest.mark.parametrize("S,D,layout,F", RG.CASES)
def test_gap_gradient_on_reverse_mode_against_reference(ctx, ctx_gradr, S, D, layout, F):
    """All buckets of the case in one loglik_grad call of a default context: the new kernel family, the reference, the forward-mode kernels."""
    key = (S, D, layout, F)
    case = R.make_case(*key)
    ref = RG.golden(case, key)
    _upload(ctx, case)
    model = _case_model(case)
    tang = [d[1] for d in ref["dirs"]]
    tot, g = ctx.loglik_grad(model, tang, gaps=True)
    assert ctx.last_grad_path() == "gaps_rev"
    assert ctx.last_launch_info()["threads"] <= 256 and ctx.last_grad_ms() > 0
    lsum = ref["ll"].sum()
    assert np.all(np.isfinite(ref["ll"])) and abs(tot - lsum) <= 1e-12 * abs(lsum), (tot, lsum)
    assert abs(tot - ctx.loglik(model, gaps=True)) <= 1e-12 * abs(tot)
    GR.assert_condition("%s sum" % (key,), ref["gfd"], ref["gest"])
    check_gradient("%s sum" % (key,), ref["dirs"], g, ref["gfd"], ref["gest"])
    tot2, g2 = ctx.loglik_grad(model, tang, gaps=True)
    assert tot2 == tot and np.array_equal(g2, g)  # two calls give the same bits
    _upload(ctx_gradr, case)
    fwd = ctx_gradr.loglik_grad(model, tang, gaps=True)
    assert ctx_gradr.last_grad_path() == "gradr"
    assert_bodies_agree((tot, g), fwd)


@pytest.mark.parametrize("model,nbuf", [(NBUF1_MODEL, 1), (NBUF2_MODEL, 2)])
def test_one_and_two_exchange_buffers(ctx, ctx_gradr, model, nbuf):
    """The models tests/test_grad_gap_rev_cpu.py names for either buffer count: the launch has the LDS bytes the pure function gives that count."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))
    import run_emul_rev_gap as E
    case = R.make_case(model["S"], model["D"], "global1", model["F"])
    m = _case_model(case)
    tang = [d[1] for d in GR.directions(case)]
    pick = E.decide(n_dir=len(tang), Lmax=40, nbuckets=len(case["buckets"]), **model)[2]
    assert pick["path"] == "gaps_rev" and pick["nbuf"] == nbuf
    _upload(ctx, case)
    _upload(ctx_gradr, case)
    got = ctx.loglik_grad(m, tang, gaps=True)
    info = ctx.last_launch_info()
    assert ctx.last_grad_path() == "gaps_rev" and info["lds_bytes"] == pick["lds"] and info["tracks_per_block"] == pick["tpb"], (info, pick)
    assert_bodies_agree(got, ctx_gradr.loglik_grad(m, tang, gaps=True))
    assert ctx_gradr.last_grad_path() == "gradr"


@pytest.fixture(scope="module")
def batches():
    """2000 x 12 and 300 x 40, 3 states, 25 % of the interior rows missed: blocks that walk several batches and reuse their log region."""
    from extrack_amd import synth
    Ds, Tm, Fs = R.MODELS[3]
    bk = []
    for i, (N, L) in enumerate(((2000, 12), (300, 40))):
        tr = synth.brownian_tracks(N, L, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=R.DT, dims=2, seed=90 + i)
        m = np.random.default_rng(95 + i).random((N, L)) < 0.25
        m[:, 0] = m[:, -1] = False
        tr[m] = np.nan
        bk.append(tr)
    case = dict(S=3, D=2, F=5, layout="global1", buckets=bk, masks=[np.isnan(b).all(axis=2) for b in bk], sig=None, le=[0.02], slope_offset=None)
    return case, _case_model(case), [d[1] for d in GR.directions(case)]


def test_blocks_that_walk_several_batches(ctx, ctx_gradr, batches):
    case, model, tang = batches
    _upload(ctx_gradr, case)
    fwd = ctx_gradr.loglik_grad(model, tang, gaps=True)
    assert ctx_gradr.last_grad_path() == "gradr" and np.isfinite(fwd[0]) and np.all(np.isfinite(fwd[1]))
    _upload(ctx, case)
    got = ctx.loglik_grad(model, tang, gaps=True)
    info = ctx.last_launch_info()
    assert ctx.last_grad_path() == "gaps_rev"
    assert_bodies_agree(got, fwd)
    assert abs(got[0] - ctx.loglik(model, gaps=True)) <= 1e-12 * abs(got[0])
    # a log budget that cuts the block count: 3 tracks x 38 steps x 365 doubles = 332 880 bytes per block -> 201 blocks in 64 MiB, at least
    # max(n_cu / 2, 2 buckets) = 128, fewer than the 2300 / 3 batches: every block walks several batches on one log region
    small = _context_under(EXTRACK_REV_LOG_MB="64")
    try:
        _upload(small, case)
        cut = small.loglik_grad(model, tang, gaps=True)
        sinfo = small.last_launch_info()
        assert small.last_grad_path() == "gaps_rev"
        assert sinfo["blocks"] <= (64 << 20) // (3 * 38 * 365 * 8) and sinfo["blocks"] < info["blocks"], (sinfo, info)
        assert_bodies_agree(cut, fwd)
    finally:
        small.close()
    # a budget too small for max(n_cu / 2, nbuckets) blocks: the forward-mode kernels, the same value
    tiny = _context_under(EXTRACK_REV_LOG_MB="1")
    try:
        _upload(tiny, case)
        low = tiny.loglik_grad(model, tang, gaps=True)
        assert tiny.last_grad_path() == "gradr"
        assert_bodies_agree(low, fwd)
    finally:
        tiny.close()


def test_scores_call_after_a_reverse_mode_launch_stays_on_gradr(ctx):
    case = R.make_case(3, 2, "global1", 5)
    ref = RG.golden(case, (3, 2, "global1", 5))
    _upload(ctx, case)
    model = _case_model(case)
    tang = [d[1] for d in ref["dirs"]]
    tot, g = ctx.loglik_grad(model, tang, gaps=True)
    assert ctx.last_grad_path() == "gaps_rev"
    stot, sg, _, sc = ctx.loglik_scores(model, tang, scores=True, gaps=True)
    assert ctx.last_grad_path() == "gradr"
    assert sc.shape == (len(ref["ll"]), len(tang))
    assert_bodies_agree((tot, g), (stot, sg))
    ctx.loglik_grad(model, tang, gaps=True)
    assert ctx.last_grad_path() == "gaps_rev"


def test_a_poisoned_track_and_the_context_afterwards(ctx):
    case = R.make_case(3, 2, "global1", 5)
    _upload(ctx, case)
    model = _case_model(case)
    tang = [d[1] for d in GR.directions(case)]
    clean = ctx.loglik_grad(model, tang, gaps=True)
    assert np.isfinite(clean[0]) and np.all(np.isfinite(clean[1]))
    for bi, n, t, d in ((3, 6, 5, 1), (4, 2, 0, None)):  # a row with one NaN coordinate; a NaN first row
        dirty = [b.copy() for b in case["buckets"]]
        if d is None:
            dirty[bi][n, t] = np.nan
        else:
            dirty[bi][n, t] = 0.1
            dirty[bi][n, t, d] = np.nan
        _upload(ctx, case, buckets=dirty)
        tot, g = ctx.loglik_grad(model, tang, gaps=True)
        assert ctx.last_grad_path() == "gaps_rev" and np.isnan(tot) and np.all(np.isnan(g))
        _upload(ctx, case)
        again = ctx.loglik_grad(model, tang, gaps=True)
        assert again[0] == clean[0] and np.array_equal(again[1], clean[1])


def test_forward_gradient_fit_of_a_gapped_three_state_model():
    """3000 x 12, 3 states, 25 % of the interior rows missed, D2 free: the exact gradient on the reverse-mode kernels ends where the differenced
    objective does, in fewer objective calls."""
    from extrack_amd import synth, tracking as T
    from extrack_amd.lmfit_compat import Parameters
    Ds, Tm, Fs = R.MODELS[3]
    tr = synth.brownian_tracks(3000, 12, list(Ds), Tm.tolist(), list(Fs), seed=5)
    mask = np.random.default_rng(11).random((3000, 12)) < 0.25
    mask[:, 0] = mask[:, -1] = False
    gapped = tr.copy()
    gapped[mask] = np.nan
    vals = dict(LocErr=0.02, pBL=0.1)
    for i in range(3):
        vals["D%d" % i], vals["F%d" % i] = float(Ds[i]), float(Fs[i])
        for j in range(3):
            if i != j:
                vals["p%d%d" % (i, j)] = float(-np.log1p(-Tm[i, j]))  # Matrix_type 1: T_ij = 1 - exp(-p_ij)

    def start():
        p = Parameters()
        for k, v in vals.items():
            p.add(k, value=0.4 if k == "D2" else v, min=0.0 if k == "D2" else -np.inf, max=3.0 if k == "D2" else np.inf, vary=k == "D2")
        return p
    kw = dict(nb_states=3, frame_len=5, verbose=0, cell_dims=[1], gaps=True)
    fwd = T.param_fitting({"12": gapped}, 0.02, params=start(), gradient="forward", **kw)
    fdf = T.param_fitting({"12": gapped}, 0.02, params=start(), **kw)
    print("forward: D2 %.5f objective %.9f calls %d (%s, %s); differenced: D2 %.5f objective %.9f calls %d" %
          (fwd.params["D2"].value, fwd.residual[0], fwd.nfev, fwd.message, fwd.gradient_kernel, fdf.params["D2"].value, fdf.residual[0], fdf.nfev))
    assert fwd.gradient_kernel == "gaps_rev" and fdf.gradient_kernel == "none"
    assert fwd.gradient_path == "analytic" and "gap-aware forward-mode" in fwd.gradient_why and fwd.gradient_why.endswith("'gaps_rev'")
    assert fwd.success
    assert fwd.residual[0] <= fdf.residual[0] + 1e-9 * abs(fdf.residual[0])
    assert fwd.nfev < fdf.nfev, (fwd.nfev, fdf.nfev)
