"""GPU counterparts of tests/test_grad_edges_cpu.py: the same edge inputs (tiny / zero transition probabilities, jumps inside and beyond
the clamp of the table-driven exp, 300-position tracks, the smallest and ragged inputs, NaN) through the C ABI - ctx.loglik_grad
(extrack_loglik_grad) and ctx.loglik_th_grad (extrack_loglik_th_grad) - once per kernel family, forced as tests/test_hip_grad.py and
tests/test_hip_th_grad.py force them, and once with the launcher's own choice.  References, metric and tolerances are those of the CPU file
(per direction 1e-6 |fd_k| + the reference's own error estimate; LL rtol 1e-13 / atol 1e-10 at the edges, 1e-10 elsewhere - on the SUM over the
tracks, which is what the gradient entry points return).  Only oracle/ and tests/golden/ are read."""
import numpy as np
import pytest

from test_grad_cpu import model_directions
from test_grad_edges_cpu import (CELL, CHECKED, H_ONE_SIDED, MIN_LEN, PBL, SHAPES, TH, _one_sided, check_gradient, jump_data, jump_set_reference,
                                 pin_t01_across_families, reference, same_plan, shape_model, tiny_rate_data, with_t01)

pytestmark = pytest.mark.gpu

FORCE = {  # environment read when a context is created
    "auto": {},                                                           # the launcher's choice (2 states: xt_reg2.h; else xt_rev.h / xt_gradr.h / xt_grad.h)
    "rev": {"EXTRACK_GRAD_PATH": "rev"},
    "gradr3": {"EXTRACK_GRAD_PATH": "gradr", "EXTRACK_GRADR_NPC": "3"},
    "gradr4": {"EXTRACK_GRAD_PATH": "gradr", "EXTRACK_GRADR_NPC": "4"},
    "lds": {"EXTRACK_GRAD_PATH": "lds"},
    "th_auto": {},                                                        # extrack_loglik_th_grad, the launcher's choice of body
    "th1": {"EXTRACK_THG_KERNEL": "1"},
    "th2": {"EXTRACK_THG_KERNEL": "2"},
}
GPU_CASES = [(sh, f) for sh in SHAPES for f in FORCE]
_refs = {}


def _cached(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def run_gpu(force, Cs, m, T, dirs, monkeypatch, chunk=None, want_plan=False):
    """(sum LL, gradient[n_dir]) through the C ABI with the kernel family ``force``.  want_plan (threshold fusion): run_gpu.last_plan =
    the merge groups of every chunk and step, read back after a plain extrack_loglik_th evaluation of the same model."""
    from extrack_amd import tracking as TR
    for k in ("EXTRACK_GRAD_PATH", "EXTRACK_GRADR_NPC", "EXTRACK_THG_KERNEL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FORCE[force].items():
        monkeypatch.setenv(k, v)
    ts, le = TR._one_bucket(Cs, m["le"][None, None], m["isBL"], MIN_LEN, 0)
    try:
        model = ts.make_model(le, np.sqrt(m["ds2"]), m["Fs"], T, PBL, CELL, m["ns"], m["F"])
        tang = [d[1] for d in dirs]
        if force.startswith("th"):
            ch = chunk or len(Cs)
            if want_plan:
                ts.loglik_th(model, TH["thr"], TH["max_nb"], ch)
                run_gpu.last_plan = [{t: ts.ctx.th_plan_step(0, c, t)[1] for t in range(2, Cs.shape[1] - 1)} for c in range(-(-len(Cs) // ch))]
            return ts.ctx.loglik_th_grad(model, tang, TH["thr"], TH["max_nb"], ch)
        return ts.ctx.loglik_grad(model, tang)
    finally:
        ts.close()


def check_total(ll, ref, edge=True, extra=0.0):
    tol = np.sum(1e-13 * np.abs(ref) + 1e-10) if edge else 1e-10 * len(ref)
    assert abs(ll - ref.sum()) <= tol + extra, (ll, ref.sum(), tol + extra)


@pytest.mark.parametrize("t01", [1e-25, 1e-200, 1e-300, 0.0])
@pytest.mark.parametrize("shape,force", GPU_CASES)
def test_tiny_and_zero_transition_probability(shape, force, t01, monkeypatch):
    """T[0, 1] = 1e-25 / 1e-200 / 1e-300: sum LL and EVERY direction against the oracle (dLL/dT01 by one-sided differences).  T[0, 1] = 0:
    finite, and equal to the 1e-300 result in every direction but T01 (threshold fusion: finite - its plan differs there, DESIGN.md
    section 9)."""
    m = shape_model(shape)
    Cs = tiny_rate_data(m)
    Tm = with_t01(m["T"], t01 if t01 > 0 else 1e-300)
    dirs = model_directions(m["S"], m["K"], m["ns"], m["ds2"], Tm, m["le"], CELL)
    if t01 == 0.0:
        th = force.startswith("th")
        ll3, g3 = run_gpu(force, Cs, m, Tm, dirs, monkeypatch, want_plan=th)
        plan3 = run_gpu.last_plan if th else None
        ll0, g0 = run_gpu(force, Cs, m, with_t01(m["T"], 0.0), dirs, monkeypatch, want_plan=th)
        assert np.isfinite(ll0) and np.all(np.isfinite(g0)), (ll0, g0)
        if th and not same_plan(plan3, run_gpu.last_plan):  # as the CPU test: a group of weight exactly 0 has no moments to group by
            return
        rest = np.arange(len(dirs)) != [d[0] for d in dirs].index("T01")
        assert abs(ll0 - ll3) <= 1e-13 * abs(ll3)
        np.testing.assert_allclose(g0[rest], g3[rest], rtol=1e-12, atol=0)
        return
    ref, fd, est = _cached(("tiny", shape, force.startswith("th"), t01), lambda: reference(force, Cs, m, Tm, dirs, one_sided=("T01",)))
    ll, g = run_gpu(force, Cs, m, Tm, dirs, monkeypatch)
    print("tiny rate %s %s %g: dLL/dT01 kernel %.9g oracle %.9g" % (shape, force, t01, g[[d[0] for d in dirs].index("T01")], fd[[d[0] for d in dirs].index("T01")]))
    check_total(ll, ref)
    check_gradient("tiny rate %s %s %g" % (shape, force, t01), dirs, g, fd, est)
    pin_t01_across_families(("gpu", shape, t01, force.startswith("th")), g[[d[0] for d in dirs].index("T01")])


@pytest.mark.parametrize("F", [4, 5, 6, 7])
def test_small_rate_inside_the_well_scaled_bounds_reg2(F, monkeypatch):
    """T[0, 1] = 1e-18, inside the well-scaled bounds: the lazily normalised steps of xt_reg2.h (every frame_len it serves)."""
    m = shape_model("s2_bl")
    m["F"] = F
    Cs = tiny_rate_data(m)
    Tm = with_t01(m["T"], 1e-18)
    dirs = model_directions(m["S"], m["K"], m["ns"], m["ds2"], Tm, m["le"], CELL)
    ref, fd, est = reference("auto", Cs, m, Tm, dirs, one_sided=("T01",))
    ll, g = run_gpu("auto", Cs, m, Tm, dirs, monkeypatch)
    check_total(ll, ref)
    check_gradient("1e-18 reg2 F=%d" % F, dirs, g, fd, est)


@pytest.mark.parametrize("shape,force", GPU_CASES)
def test_jumps_inside_the_clamp(shape, force, monkeypatch):
    """40 um jumps: the jump tracks alone and the ordinary tracks alone against oracle differences of that set; joint - jump-only =
    ordinary-only."""
    m = shape_model(shape)
    Cs, ij, io = jump_data(m, 40.0)
    dirs = model_directions(m["S"], m["K"], m["ns"], m["ds2"], m["T"], m["le"], CELL)
    th = force.startswith("th")
    refj, fdj, estj = _cached(("jump", shape, th), lambda: jump_set_reference(force, Cs[ij], m, dirs, len(ij)))
    refo, fdo, esto = _cached(("ordinary", shape, th), lambda: reference(force, Cs[io], m, m["T"], dirs, chunk=len(ij)))
    chk = np.array([d[0].startswith(CHECKED) for d in dirs])
    assert np.all(estj[chk] < 1e-7 * np.abs(fdj[chk])) and np.all(esto[chk] < 1e-7 * np.abs(fdo[chk]))
    llj, gj = run_gpu(force, Cs[ij], m, m["T"], dirs, monkeypatch, chunk=len(ij))
    llo, go = run_gpu(force, Cs[io], m, m["T"], dirs, monkeypatch, chunk=len(ij))
    lla, ga = run_gpu(force, Cs[np.concatenate([ij, io])], m, m["T"], dirs, monkeypatch, chunk=len(ij))
    check_total(llj, refj)
    check_total(llo, refo)
    check_total(lla, np.concatenate([refj, refo]))
    check_gradient("jump set %s %s" % (shape, force), dirs, gj, fdj, estj)
    check_gradient("ordinary set %s %s" % (shape, force), dirs, go, fdo, esto)
    check_gradient("joint - jump %s %s" % (shape, force), dirs, ga - gj, fdo, esto, extra=1e-13 * np.abs(gj))


@pytest.mark.parametrize("shape,force", GPU_CASES)
def test_jump_beyond_the_clamp(shape, force, monkeypatch):
    """A 3000 um jump in one track: finite gradient; joint - that track alone = the gradient of the other tracks."""
    from extrack_amd import synth
    m = shape_model(shape)
    Cs = synth.brownian_tracks(12, 15, m["Ds"], m["T"], m["Fs"], seed=6, dims=m["D"])
    Cs[3, 7:] += 3000.0
    io = np.flatnonzero(np.arange(12) != 3)
    dirs = model_directions(m["S"], m["K"], m["ns"], m["ds2"], m["T"], m["le"], CELL)
    refo, fdo, esto = _cached(("beyond", shape, force.startswith("th")), lambda: reference(force, Cs[io], m, m["T"], dirs, chunk=1))
    llc, gc = run_gpu(force, Cs[[3]], m, m["T"], dirs, monkeypatch, chunk=1)
    lla, ga = run_gpu(force, Cs[np.concatenate([[3], io])], m, m["T"], dirs, monkeypatch, chunk=1)
    print("clamped track %s %s: LL %.6g, gradient %s" % (shape, force, llc, dict(zip([d[0] for d in dirs], gc))))
    assert np.all(np.isfinite(gc)) and np.all(np.isfinite(ga)) and np.isfinite(llc) and llc < -7e6
    check_total(lla - llc, refo, extra=2e-16 * abs(llc))
    check_gradient("joint - clamped %s %s" % (shape, force), dirs, ga - gc, fdo, esto, extra=1e-13 * np.abs(gc))


@pytest.mark.parametrize("shape,force", [c for c in GPU_CASES if c[0] in ("s2_bl", "s3_nobl")])
def test_long_tracks(shape, force, monkeypatch):
    """L = 300, 5 tracks, at the ordinary 1e-6."""
    from extrack_amd import synth
    m = shape_model(shape)
    Cs = synth.brownian_tracks(5, 300, m["Ds"], m["T"], m["Fs"], seed=11, dims=m["D"])
    dirs = model_directions(m["S"], m["K"], m["ns"], m["ds2"], m["T"], m["le"], CELL)
    ref, fd, est = _cached(("long", shape, force.startswith("th")), lambda: reference(force, Cs, m, m["T"], dirs))
    ll, g = run_gpu(force, Cs, m, m["T"], dirs, monkeypatch)
    check_total(ll, ref, edge=False)
    check_gradient("L=300 %s %s" % (shape, force), dirs, g, fd, est)


@pytest.mark.parametrize("N,L", [(1, 9), (1, 2), (5, 2), (7, 3), (67, 5)])
@pytest.mark.parametrize("shape,force", GPU_CASES)
def test_smallest_and_ragged_inputs(shape, force, N, L, monkeypatch):
    """One track; 2 and 3 positions; track counts that are no multiple of the tracks per workgroup / wave / tile."""
    from extrack_amd import synth
    m = shape_model(shape)
    Cs = synth.brownian_tracks(N, L, m["Ds"], m["T"], m["Fs"], seed=N + L, dims=m["D"])
    dirs = model_directions(m["S"], m["K"], m["ns"], m["ds2"], m["T"], m["le"], CELL)
    chunk = 32 if N > 32 else N
    ref, fd, est = _cached(("ragged", shape, force.startswith("th"), N, L), lambda: reference(force, Cs, m, m["T"], dirs, chunk=chunk))
    ll, g = run_gpu(force, Cs, m, m["T"], dirs, monkeypatch, chunk=chunk)
    check_total(ll, ref, edge=False)
    check_gradient("N=%d L=%d %s %s" % (N, L, shape, force), dirs, g, fd, est)


@pytest.mark.parametrize("shape,force", GPU_CASES)
def test_nan_position_gives_nan_sum(shape, force, monkeypatch):
    """A NaN position poisons its track: the sum over the launch is NaN (never a finite number that silently drops the track)."""
    from extrack_amd import synth
    m = shape_model(shape)
    Cs = synth.brownian_tracks(9, 8, m["Ds"], m["T"], m["Fs"], seed=3, dims=m["D"])
    Cs[4, 5, 0] = np.nan
    dirs = model_directions(m["S"], m["K"], m["ns"], m["ds2"], m["T"], m["le"], CELL)
    ll, g = run_gpu(force, Cs, m, m["T"], dirs, monkeypatch, chunk=3)
    assert np.isnan(ll), (ll, g)


def _edge_dataset():
    """2 states, two length buckets, simulated without the 0 -> 1 transition; two of the longer tracks jump by 40 um."""
    from extrack_amd import synth
    Ds, Tm, Fs = [0.001, 0.25], np.array([[1.0, 0.0], [0.1, 0.9]]), [0.6, 0.4]
    tr = {"8": synth.brownian_tracks(30, 8, Ds, Tm, Fs, seed=21), "12": synth.brownian_tracks(24, 12, Ds, Tm, Fs, seed=22)}
    tr["12"][::12, 6:] += 40.0
    return tr


def test_parameter_level_gradient_with_a_rate_of_1e_25_and_jump_tracks():
    """gradient.objective_and_gradient (host chain rule + the launcher's own kernel, xt_reg2.h) on a 2-state dataset with p01 = 1e-25
    (Matrix_type 0: the rate IS the probability) and two 40 um jump tracks, against differences of the oracle's cum_proba_cs: central
    Richardson for every parameter but p01, one-sided for p01; value to 1e-12 relative."""
    from extrack_amd import gradient, tracking as TR
    from oracle import oracle_np as O
    tr = _edge_dataset()
    p = TR.generate_params(nb_states=2, LocErr_type=1, estimated_Ds=[0.001, 0.25], estimated_LocErr=[0.02], estimated_Fs=[0.6], estimated_transition_rates=[0.1, 0.1])
    p["p01"].value = 1e-25
    p["pBL"].value = 0.07
    p.update_constraints()
    names = gradient.free_names(p)
    vals = {k: p[k].value for k in p}
    _, lst, _ = TR.engine.sort_buckets(tr)
    ts = TR.TrackSet(lst)
    try:
        v, g = gradient.objective_and_gradient(p, ts, 0.02, [1.0], 2, 1, 6, Matrix_type=0, names=names)
    finally:
        ts.close()
    assert np.isfinite(v) and np.all(np.isfinite(g))

    def f(n, x):
        q = dict(vals)
        q[n] = vals[n] + x
        q["F1"] = 1 - q["F0"]
        return O.cum_proba_cs(q, tr, 0.02, [1.0], None, 1, 6, Matrix_type=0)

    assert abs(v - f(names[0], 0.0)) < 1e-12 * abs(v)
    from test_grad_cpu import _richardson
    for n, gi in zip(names, g):
        if n == "p01":
            lv = [_one_sided(lambda x: f(n, x), H_ONE_SIDED * s) for s in (1.0, 0.5)]
        else:
            h = 1e-2 * max(abs(vals[n]), 1e-3)  # the jump tracks' LL of -1e6 rounds at 1e-9: large steps, O(h^4) after extrapolation
            lv = [_richardson(lambda x: f(n, x), h * s) for s in (1.0, 0.5)]
        fd, est = lv[1], abs(lv[1] - lv[0])
        print("parameter %s: kernel %.12g oracle %.12g est %.3g" % (n, gi, fd, est))
        assert abs(gi - fd) <= 1e-6 * abs(fd) + est, (n, gi, fd, est)


def test_objective_and_gradient_nan_input_is_inf_and_zeros():
    """Host level on the device path: a NaN position in the dataset -> (+inf, zeros), for the window and the threshold objective."""
    from extrack_amd import gradient, tracking as TR
    tr = _edge_dataset()
    tr["8"][3, 2, 1] = np.nan
    p = TR.generate_params(nb_states=2, LocErr_type=1, estimated_Ds=[0.001, 0.25], estimated_LocErr=[0.02], estimated_Fs=[0.6], estimated_transition_rates=[0.1, 0.1])
    names = gradient.free_names(p)
    _, lst, _ = TR.engine.sort_buckets(tr)
    ts = TR.TrackSet(lst)
    try:
        for fusion in (None, (0.2, 120, 2000)):
            v, g = gradient.objective_and_gradient(p, ts, 0.02, [1.0], 2, 1, 6, names=names, threshold_fusion=fusion)
            assert v == np.inf and g.shape == (len(names),) and np.all(g == 0.0), (fusion, v, g)
    finally:
        ts.close()
