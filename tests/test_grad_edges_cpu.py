"""Edge inputs for the GRADIENT kernel bodies on CPU threads (tests/emul): what tests/test_hip_parity.py asks of the likelihood kernels -
transition probabilities of 1e-25 / 1e-200 / 1e-300 / 0, 40 um jumps inside the clamp of the table-driven exp, a jump beyond it, tracks of
hundreds of positions, the smallest and ragged inputs, NaN - asked of every gradient family: xt_grad.h ("lds"), xt_reg2.h with NP > 0 ("reg2"),
xt_gradr.h ("gradr3" / "gradr4": 3 / 4 directions per pass), xt_rev.h ("rev") and the frozen-plan threshold-fusion bodies xt_thgrad.h /
xt_thgrad2.h ("th1" / "th2").

Reference: differences of the pinned numpy oracle (oracle_np / oracle_th at the frozen plan) in two Richardson levels (steps h and h / 2); the
finer level is the reference value and |finer - coarser| its error estimate.  Metric: PER DIRECTION |g_k - fd_k| <= 1e-6 |fd_k| + estimate_k -
no floor taken from the largest direction, which on a dataset with outlier tracks (1e11 in the ds2 / LocErr directions) would hide every
other direction and every ordinary track.  Log-likelihoods: rtol 1e-13 / atol 1e-10 at the edges (as test_hip_parity), 1e-10 elsewhere.
The contracts asserted for a zero transition probability, a track beyond the clamp and NaN input are stated in DESIGN.md section 9."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))
from test_grad_cpu import _model, model_directions, oracle_fd_gradient  # noqa: E402

CELL, PBL, MIN_LEN, DT = [1.0], 0.1, 3, 0.02
WINDOW_FAMILIES = {"lds": dict(generic_g=0, PJ=2), "reg2": dict(generic_g=2), "gradr3": dict(generic_g=3), "gradr4": dict(generic_g=4), "rev": dict(generic_g=5)}
TH = dict(thr=0.2, max_nb=120)

# model shapes: name -> (S, ns, F, D, K, isBL, model seed, window families that serve it).  Every shape also runs th1 and th2.
SHAPES = {
    "s2_bl": (2, 1, 6, 2, 1, 1, 26, ("lds", "reg2", "gradr4", "rev")),
    "s2_nobl": (2, 1, 4, 3, 3, 0, 24, ("reg2", "gradr3")),
    "s3_nobl": (3, 1, 4, 2, 2, 0, 34, ("lds", "gradr3", "rev")),
    "s3_bl": (3, 1, 4, 1, 1, 1, 33, ("gradr4", "rev")),
}
CASES = [(sh, fam) for sh, v in SHAPES.items() for fam in v[7] + ("th1", "th2")]


def shape_model(shape):
    S, ns, F, D, K, isBL, seed, _ = SHAPES[shape]
    Ds, T, Fs = _model(S, seed)
    return dict(S=S, ns=ns, F=F, D=D, K=K, isBL=isBL, Ds=Ds, T=T, Fs=Fs, ds2=2 * Ds * DT, le=np.array([0.02, 0.025, 0.03][:K]))


def with_t01(T, v):
    """T with T[0, 1] = v, the row still summing to 1 (what a fit that drives a rate to its bound hands over)."""
    T = np.array(T, float)
    T[0, 0] += T[0, 1] - v
    T[0, 1] = v
    return T


# ---- reference: two Richardson levels of oracle differences -> (value, error estimate) per direction

def _halved(dirs):
    return [(n, t, d, h / 2) for n, t, d, h in dirs]


H_ONE_SIDED = 1e-7


def _one_sided(f, h):
    """Second-order forward difference (-3 f(0) + 4 f(h) - f(2h)) / 2h at h and h / 2, extrapolated (error O(h^3)): for a parameter ON its
    lower bound (a transition probability of 0 or next to it), where a central difference would step across the bound.
    Step (checked against the oracle alone): a sequence that needs the 0 -> 1 transition weighs T01 * r against its merge partner, with r up to
    1e4 - 1e6 on these models (the product over the window of the per-step Gaussian ratios of the two states), so sum LL is only polynomial in
    T01 on a scale well below 1e-6: at h = 1e-4 .. 1e-5 the two levels agree to 2e-7 relative while both are off by 2.5e-6 (dLL/dT01 = 2.27756 /
    2.27756 / 2.277562 / 2.277566 / 2.2775657 at h = 1e-3 .. 1e-7 against 2.2775658 from three kernel families).  h = 1e-7 is inside the
    polynomial range; the rounding of the oracle's sum (1e-13) then shows in the error estimate (1e-6 absolute), which is what it is for."""
    d = lambda s: (-3 * f(0.0) + 4 * f(s) - f(2 * s)) / (2 * s)
    return (4 * d(h / 2) - d(h)) / 3


def _levels(total, dirs, one_sided=()):
    """total(x, perturbation dict) -> sum LL.  Central Richardson (test_grad_cpu._richardson) per direction at its step h and at h / 2;
    directions named in ``one_sided``: forward differences with h = H_ONE_SIDED and half of it."""
    from test_grad_cpu import _richardson
    lv = []
    for hs in (1.0, 0.5):
        lv.append(np.array([_one_sided(lambda x: total(x, d), H_ONE_SIDED * hs) if n in one_sided else _richardson(lambda x: total(x, d), h * hs)
                            for n, _, d, h in dirs]))
    return lv[1], np.abs(lv[1] - lv[0])


def window_reference(Cs, m, T, dirs, one_sided=()):
    """(per-track LL, fd[n_dir], est[n_dir]) of the fixed-window objective from oracle_np."""
    from oracle import oracle_np as O
    a = (m["isBL"], CELL, m["ns"], m["F"], MIN_LEN)
    ref = O.proba_cs(Cs, m["le"][None, None], np.sqrt(m["ds2"]), m["Fs"], T, PBL, *a)
    if not one_sided:  # all central: the two levels are two calls of the existing helper
        r1 = oracle_fd_gradient(Cs, m["le"], m["ds2"], m["Fs"], T, PBL, *a, dirs)
        r2 = oracle_fd_gradient(Cs, m["le"], m["ds2"], m["Fs"], T, PBL, *a, _halved(dirs))
        return ref, r2, np.abs(r2 - r1)

    def total(x, d):
        return O.proba_cs(Cs, (m["le"] + x * d.get("le", 0.0))[None, None], np.sqrt(m["ds2"] + x * d.get("ds2", 0.0)), m["Fs"] + x * d.get("Fs", 0.0),
                          T + x * d.get("T", 0.0), PBL + x * d.get("pBL", 0.0), *a).sum()

    return (ref,) + _levels(total, dirs, one_sided)


def th_reference(Cs, m, T, dirs, chunk, one_sided=()):
    """(per-track LL, fd, est, plans) of the threshold-fusion objective from oracle_th, every chunk's plan frozen at the evaluation point."""
    from oracle import oracle_th as OT
    a = (m["isBL"], CELL, m["ns"], m["F"], MIN_LEN, TH["thr"], TH["max_nb"])
    plans, base = [], []
    for a0 in range(0, len(Cs), chunk):
        tr = []
        base.append(OT.proba_cs_th(Cs[a0:a0 + chunk], m["le"][None, None], np.sqrt(m["ds2"]), m["Fs"], T, PBL, *a, trace=tr))
        plans.append(tr)

    def total(x, d):
        return sum(OT.proba_cs_th(Cs[a0:a0 + chunk], (m["le"] + x * d.get("le", 0.0))[None, None], np.sqrt(m["ds2"] + x * d.get("ds2", 0.0)),
                                  m["Fs"] + x * d.get("Fs", 0.0), T + x * d.get("T", 0.0), PBL + x * d.get("pBL", 0.0), *a, plan=plans[ci]).sum()
                   for ci, a0 in enumerate(range(0, len(Cs), chunk)))

    return (np.concatenate(base),) + _levels(total, dirs, one_sided) + (plans,)


_ref_cache = {}


def cached_reference(key, fam, *a, **k):
    """One reference per (input, shape, objective): the families of a shape share it."""
    key = key + (fam.startswith("th"),)
    if key not in _ref_cache:
        _ref_cache[key] = reference(fam, *a, **k)
    return _ref_cache[key]


def reference(fam, Cs, m, T, dirs, chunk=None, one_sided=()):
    if fam.startswith("th"):
        return th_reference(Cs, m, T, dirs, chunk or len(Cs), one_sided)[:3]
    return window_reference(Cs, m, T, dirs, one_sided)


# ---- the emulated bodies

def run_family(fam, Cs, m, T, dirs, chunk=None, monkeypatch=None):
    """(per-track LL, gradient[n_dir]) from the emulated body of family ``fam``."""
    import run_emul as E
    from oracle import oracle_np as O
    ps = O.p_stay_table(np.sqrt(m["ds2"]), m["S"], m["ns"], CELL)
    tang = [d[1] for d in dirs]
    if fam.startswith("th"):
        if fam == "th2":
            monkeypatch.setenv("XT_EMUL_THG2", "4")
        else:
            monkeypatch.delenv("XT_EMUL_THG2", raising=False)
        ll, llg, totg, g, plan = E.run_th_grad(Cs, m["le"][None, None], np.sqrt(m["ds2"]), m["Fs"], T, PBL, m["isBL"], ps, m["ns"], m["F"], MIN_LEN,
                                               TH["thr"], TH["max_nb"], tang, chunk=chunk or len(Cs), capE=512, TT=8, threads=64, nblocks=2)
        assert np.array_equal(np.isnan(ll), np.isnan(llg)) and np.allclose(llg[~np.isnan(ll)], ll[~np.isnan(ll)], rtol=1e-13, atol=1e-11)  # gradient body's value = apply body's
        run_family.last_plan = plan
        return llg, g
    run_family.last_plan = None
    ll, tot, g = E.run_grad(Cs, m["le"][None, None], np.sqrt(m["ds2"]), m["Fs"], T, PBL, m["isBL"], ps, m["ns"], m["F"], MIN_LEN, tang, **WINDOW_FAMILIES[fam])
    return ll, g


def same_plan(a, b):
    return all(sorted(tuple(int(v) for v in g) for g in ca[t]) == sorted(tuple(int(v) for v in g) for g in cb[t]) for ca, cb in zip(a, b) for t in ca)


def check_gradient(tag, dirs, g, fd, est, extra=0.0):
    """|g - fd| <= 1e-6 |fd| + est (+ extra) per direction.  Prints the figures before asserting."""
    tol = 1e-6 * np.abs(fd) + est + extra
    err = np.abs(g - fd)
    den = np.where(fd != 0, np.abs(fd), 1.0)  # a direction the data cannot see (T with 2 positions and no leaving term): 0 = 0
    ke, kr = int(np.argmax(err / den)), int(np.argmax(est / den))
    print("%s: worst |g - fd| / |fd| = %.3g (%s), worst est / |fd| = %.3g (%s)" % (tag, (err / den)[ke], dirs[ke][0], (est / den)[kr], dirs[kr][0]))
    assert np.all(np.isfinite(g)) and np.all(err <= tol), (tag, [(d[0], a, b, e) for d, a, b, e, ok in zip(dirs, g, fd, est, err <= tol) if not ok])


# ---- tiny and zero transition probabilities

_t01_seen = {}


def pin_t01_across_families(key, value):
    """The one-sided reference of dLL/dT01 carries the oracle's rounding (its error estimate reaches 3e-5 relative where the derivative is
    small), so that direction is ALSO pinned between the kernel families of one objective: every family must return what the first
    family run on that input returned, to the ordinary 1e-6 (independent code paths: tangents in LDS / registers, reverse mode)."""
    first = _t01_seen.setdefault(key, value)
    assert abs(value - first) <= 1e-6 * abs(first), (key, value, first)


def tiny_rate_data(m, N=8, L=12):
    """Tracks simulated WITHOUT the 0 -> 1 transition: the model with a tiny T[0, 1] explains them, dLL/dT01 stays moderate and the
    objective is smooth in T01 on the scale of the one-sided step."""
    from extrack_amd import synth
    return synth.brownian_tracks(N, L, m["Ds"], with_t01(m["T"], 0.0), m["Fs"], seed=m["S"] + m["F"], dims=m["D"])


@pytest.mark.parametrize("t01", [1e-25, 1e-200, 1e-300, 0.0])
@pytest.mark.parametrize("shape,fam", CASES)
def test_tiny_and_zero_transition_probability(shape, fam, t01, monkeypatch):
    """T[0, 1] = 1e-25 / 1e-200 / 1e-300: LL and EVERY direction against the oracle (dLL/dT01 by one-sided differences: d log T = 1 / T is
    1e25 .. 1e300 there and multiplies weights of 1e-25 .. 1e-300 - the merge of the tangents must not round at the size of the larger).
    T[0, 1] = 0 (contract): LL and every direction but T01 equal the 1e-300 result, dLL/dT01 is finite."""
    m = shape_model(shape)
    Cs = tiny_rate_data(m)
    Tm = with_t01(m["T"], t01 if t01 > 0 else 1e-300)
    dirs = model_directions(m["S"], m["K"], m["ns"], m["ds2"], Tm, m["le"], CELL)
    names = [d[0] for d in dirs]
    if t01 == 0.0:
        ll3, g3 = run_family(fam, Cs, m, Tm, dirs, monkeypatch=monkeypatch)
        plan3 = run_family.last_plan
        ll0, g0 = run_family(fam, Cs, m, with_t01(m["T"], 0.0), dirs, monkeypatch=monkeypatch)
        assert np.all(np.isfinite(ll0)) and np.all(np.isfinite(g0)), (ll0, g0)
        if fam.startswith("th") and not same_plan(plan3, run_family.last_plan):
            # threshold fusion groups sequences by their moments, and a group of weight exactly 0 has none: the plan differs from the
            # one at 1e-300 on these data, and value and gradient are those of the plan of the evaluation
            return
        rest = np.arange(len(dirs)) != names.index("T01")
        np.testing.assert_allclose(ll0, ll3, rtol=1e-13, atol=1e-10)
        np.testing.assert_allclose(g0[rest], g3[rest], rtol=1e-12, atol=0)
        return
    ref, fd, est = cached_reference(("tiny", shape, t01), fam, Cs, m, Tm, dirs, one_sided=("T01",))
    ll, g = run_family(fam, Cs, m, Tm, dirs, monkeypatch=monkeypatch)
    np.testing.assert_allclose(ll, ref, rtol=1e-13, atol=1e-10)
    check_gradient("tiny rate %s %s %g" % (shape, fam, t01), dirs, g, fd, est)
    pin_t01_across_families(("cpu", shape, t01, fam.startswith("th")), g[names.index("T01")])


@pytest.mark.parametrize("F", [4, 6, 7])
def test_small_rate_inside_the_well_scaled_bounds_reg2(F):
    """T[0, 1] = 1e-18 is INSIDE the well-scaled bounds (>= 1e-20): xt_reg2.h then runs its lazily normalised steps, whose tangent merge is
    the same code - d log T = 1e18 against an fp64 ulp of 1e-16."""
    m = shape_model("s2_bl")
    m["F"] = F
    Cs = tiny_rate_data(m)
    Tm = with_t01(m["T"], 1e-18)
    dirs = model_directions(m["S"], m["K"], m["ns"], m["ds2"], Tm, m["le"], CELL)
    ref, fd, est = window_reference(Cs, m, Tm, dirs, one_sided=("T01",))
    ll, g = run_family("reg2", Cs, m, Tm, dirs)
    np.testing.assert_allclose(ll, ref, rtol=1e-13, atol=1e-10)
    check_gradient("1e-18 reg2 F=%d" % F, dirs, g, fd, est)


# ---- large jumps

def jump_data(m, jump, N=12, L=15):
    """The recipe of test_hip_parity.test_extreme_displacements_do_not_underflow / test_absurd_jump_clamps_instead_of_wrapping: every fourth
    track jumps by ``jump`` um at position 7.  Returns (tracks, index of the jump tracks, index of the ordinary ones)."""
    from extrack_amd import synth
    Cs = synth.brownian_tracks(N, L, m["Ds"], m["T"], m["Fs"], seed=5, dims=m["D"])
    Cs[::4, 7:] += jump
    isj = np.zeros(N, bool)
    isj[::4] = True
    return Cs, np.flatnonzero(isj), np.flatnonzero(~isj)


CHECKED = ("ds2", "le", "T", "pBL")  # directions whose reference error must stay below 1e-7 relative on the jump sets

_jump_ref_cache = {}


def jump_set_reference(fam, Cs, m, dirs, chunk):
    """Reference for the JUMP tracks alone.  Their LL is about -1e6 per track, so the oracle's sum rounds at 1e-9 absolute and the
    default steps of model_directions (1e-3 relative) leave 1e-6 relative noise in every direction that does not see the jump (T, pBL, the
    slow states' ds2).  Steps 10x larger bring the noise to ~3e-8 while the O(h^4) term stays below it; where one direction still misses
    1e-7 (the noise is erratic) the next candidate step is taken FOR THAT DIRECTION - chosen on the oracle's two levels alone, before any
    kernel result is looked at.  Fs (not subject to the 1e-7 condition) steps 3x larger."""
    best_fd = best_est = None
    for c in (10, 20, 5, 40):
        d2 = [(n, t, d, h * (c if n.startswith(CHECKED) and not n.startswith("le") else 3 if n.startswith("F") else 1)) for n, t, d, h in dirs]
        ref, fd, est = reference(fam, Cs, m, m["T"], d2, chunk=chunk)
        if best_fd is None:
            best_fd, best_est = fd.copy(), est.copy()
        else:
            better = est / np.abs(fd) < best_est / np.abs(best_fd)
            best_fd[better], best_est[better] = fd[better], est[better]
        chk = np.array([d[0].startswith(CHECKED) for d in dirs])
        if np.all(best_est[chk] < 1e-7 * np.abs(best_fd[chk])):
            break
    return ref, best_fd, best_est


def _jump_refs(shape, fam, m, Cs, ij, io, dirs):
    key = (shape, fam.startswith("th"))
    if key not in _jump_ref_cache:
        _jump_ref_cache[key] = [jump_set_reference(fam, Cs[ij], m, dirs, len(ij)), reference(fam, Cs[io], m, m["T"], dirs, chunk=len(ij))]
    return _jump_ref_cache[key]


@pytest.mark.parametrize("shape,fam", CASES)
def test_jumps_inside_the_clamp(shape, fam, monkeypatch):
    """40 um jumps (Gaussian exponents of about -1e6, inside the clamp of the table-driven exp at -1.1e7): the jump tracks alone and the
    ordinary tracks alone against oracle differences of that set, and joint - jump-only = ordinary-only: an error on the ordinary tracks
    cannot hide behind the 1e11 the jump tracks put into the ds2 / LocErr directions."""
    m = shape_model(shape)
    Cs, ij, io = jump_data(m, 40.0)
    dirs = model_directions(m["S"], m["K"], m["ns"], m["ds2"], m["T"], m["le"], CELL)
    order = np.concatenate([ij, io])  # jump tracks first: with chunk = len(ij) no threshold-fusion chunk mixes the two sets
    (refj, fdj, estj), (refo, fdo, esto) = _jump_refs(shape, fam, m, Cs, ij, io, dirs)
    chk = np.array([d[0].startswith(CHECKED) for d in dirs])
    for name, fd, est in (("jump", fdj, estj), ("ordinary", fdo, esto)):
        print("reference error estimate / |fd|, %s set: %s" % (name, dict(zip([d[0] for d in dirs], np.round(est / np.abs(fd), 12)))))
        assert np.all(est[chk] < 1e-7 * np.abs(fd[chk])), "the oracle differences are not good to 1e-7: fix the step, not the tolerance"
    llj, gj = run_family(fam, Cs[ij], m, m["T"], dirs, chunk=len(ij), monkeypatch=monkeypatch)
    llo, go = run_family(fam, Cs[io], m, m["T"], dirs, chunk=len(ij), monkeypatch=monkeypatch)
    lla, ga = run_family(fam, Cs[order], m, m["T"], dirs, chunk=len(ij), monkeypatch=monkeypatch)
    assert refj.max() < -1e4  # as test_extreme_displacements_do_not_underflow: exp() of it underflows in the linear domain
    np.testing.assert_allclose(llj, refj, rtol=1e-13, atol=1e-10)
    np.testing.assert_allclose(llo, refo, rtol=1e-13, atol=1e-10)
    np.testing.assert_allclose(lla, np.concatenate([refj, refo]), rtol=1e-13, atol=1e-10)
    check_gradient("jump set %s %s" % (shape, fam), dirs, gj, fdj, estj)
    check_gradient("ordinary set %s %s" % (shape, fam), dirs, go, fdo, esto)
    check_gradient("joint - jump %s %s" % (shape, fam), dirs, ga - gj, fdo, esto, extra=1e-13 * np.abs(gj))


@pytest.mark.parametrize("shape,fam", CASES)
def test_jump_beyond_the_clamp(shape, fam, monkeypatch):
    """A 3000 um jump in ONE track (exponent below the clamp): the gradient is finite, and joint - that track alone = the gradient of the
    other tracks (checked against their oracle differences).  On the clamped track itself the families return different finite numbers -
    DESIGN.md section 9 records what and why; its value is only bounded (LL < -7e6), as in the likelihood test."""
    from extrack_amd import synth
    m = shape_model(shape)
    Cs = synth.brownian_tracks(12, 15, m["Ds"], m["T"], m["Fs"], seed=6, dims=m["D"])
    Cs[3, 7:] += 3000.0
    io = np.flatnonzero(np.arange(12) != 3)
    dirs = model_directions(m["S"], m["K"], m["ns"], m["ds2"], m["T"], m["le"], CELL)
    refo, fdo, esto = cached_reference(("beyond", shape), fam, Cs[io], m, m["T"], dirs, chunk=1)
    order = np.concatenate([[3], io])
    llc, gc = run_family(fam, Cs[[3]], m, m["T"], dirs, chunk=1, monkeypatch=monkeypatch)
    lla, ga = run_family(fam, Cs[order], m, m["T"], dirs, chunk=1, monkeypatch=monkeypatch)
    print("clamped track %s %s: LL %.6g, gradient %s" % (shape, fam, llc[0], dict(zip([d[0] for d in dirs], gc))))
    assert np.all(np.isfinite(gc)) and np.all(np.isfinite(ga)) and np.isfinite(llc[0]) and llc[0] < -7e6
    np.testing.assert_allclose(lla[1:], refo, rtol=1e-13, atol=1e-10)
    assert lla[0] == llc[0]
    check_gradient("joint - clamped %s %s" % (shape, fam), dirs, ga - gc, fdo, esto, extra=1e-13 * np.abs(gc))
    if not fam.startswith("th"):
        # the window families return the same thing on the clamped track: pinned against xt_grad.h.  The directions
        # of ONE track share their intermediate tangents (d m_bar, d u_bar), which round at the size of the largest direction (1e13 here,
        # amplified by the jump over ~10 steps): 1e-13 of it on top of the relative term
        _, gl = run_family("lds", Cs[[3]], m, m["T"], dirs)
        assert np.all(np.abs(gc - gl) <= 1e-6 * np.abs(gl) + 1e-13 * np.abs(gl).max()), (gc, gl)


# ---- long tracks

# every family at one shape at least (the emulated threshold-fusion bodies take a minute per shape at this length)
LONG_CASES = [("s2_bl", f) for f in ("lds", "reg2", "gradr4", "rev", "th1", "th2")] + [("s3_nobl", "gradr3"), ("s3_nobl", "rev")]


@pytest.mark.parametrize("shape,fam", LONG_CASES)
def test_long_tracks(shape, fam, monkeypatch):
    """L = 300 (hundreds of renormalisations of the weights and as many steps of tangent / adjoint propagation), 5 tracks, against the
    oracle at the ordinary 1e-6."""
    from extrack_amd import synth
    m = shape_model(shape)
    Cs = synth.brownian_tracks(5, 300, m["Ds"], m["T"], m["Fs"], seed=11, dims=m["D"])
    dirs = model_directions(m["S"], m["K"], m["ns"], m["ds2"], m["T"], m["le"], CELL)
    ref, fd, est = cached_reference(("long", shape), fam, Cs, m, m["T"], dirs)
    ll, g = run_family(fam, Cs, m, m["T"], dirs, monkeypatch=monkeypatch)
    assert np.abs(ll - ref).max() < 1e-10
    check_gradient("L=300 %s %s" % (shape, fam), dirs, g, fd, est)


# ---- smallest and ragged inputs

@pytest.mark.parametrize("N,L", [(1, 9), (1, 2), (5, 2), (7, 3), (67, 5)])
@pytest.mark.parametrize("shape,fam", CASES)
def test_smallest_and_ragged_inputs(shape, fam, N, L, monkeypatch):
    """One track; 2 and 3 positions (shorter than every window here); track counts that are not a multiple of the tracks per workgroup /
    wave / tile (1, 5, 7, 67)."""
    from extrack_amd import synth
    m = shape_model(shape)
    Cs = synth.brownian_tracks(N, L, m["Ds"], m["T"], m["Fs"], seed=N + L, dims=m["D"])
    dirs = model_directions(m["S"], m["K"], m["ns"], m["ds2"], m["T"], m["le"], CELL)
    chunk = 32 if N > 32 else N
    ref, fd, est = cached_reference(("ragged", shape, N, L), fam, Cs, m, m["T"], dirs, chunk=chunk)
    ll, g = run_family(fam, Cs, m, m["T"], dirs, chunk=chunk, monkeypatch=monkeypatch)
    assert np.abs(ll - ref).max() < 1e-10
    check_gradient("N=%d L=%d %s %s" % (N, L, shape, fam), dirs, g, fd, est)


@pytest.mark.parametrize("shape,fam", CASES)
def test_nan_position_poisons_its_track_only(shape, fam, monkeypatch):
    """A NaN position: the body returns NaN for that track's LL (as the reference does) and the other tracks' values are untouched (threshold
    fusion: those of the other chunks).  The
    sums over the launch (objective and gradient) are NaN then; gradient.objective_and_gradient maps that to (+inf, zeros)."""
    from extrack_amd import synth
    m = shape_model(shape)
    Cs = synth.brownian_tracks(9, 8, m["Ds"], m["T"], m["Fs"], seed=3, dims=m["D"])
    dirs = model_directions(m["S"], m["K"], m["ns"], m["ds2"], m["T"], m["le"], CELL)
    ll0, g0 = run_family(fam, Cs, m, m["T"], dirs, chunk=3, monkeypatch=monkeypatch)
    Cs[4, 5, 0] = np.nan
    ll, g = run_family(fam, Cs, m, m["T"], dirs, chunk=3, monkeypatch=monkeypatch)
    ok = np.arange(9) != 4
    if fam.startswith("th"):  # the chunk's plan is decided on its (pilot) tracks, the NaN one included: only the OTHER chunks keep their values bit for bit
        assert np.all(np.isfinite(ll[ok]))
        ok = np.arange(9) // 3 != 1
    assert np.isnan(ll[4]) and np.array_equal(ll[ok], ll0[ok])
    assert np.all(np.isnan(g) | (g == g0)), (g, g0)  # no finite number that is not the clean one


def test_objective_and_gradient_maps_nan_to_inf_and_zeros():
    """Host level: a NaN objective (NaN input poisons a track's LL in every kernel) comes back as (+inf, zeros), as cum_Proba_Cs returns
    +inf for it - never as a NaN value with a half-NaN gradient the optimiser would step along."""
    from extrack_amd import gradient, tracking as T

    class Ctx:
        def loglik_grad(self, model, tang):
            return float("nan"), np.array([1.0, np.nan] + [2.0] * (len(tang["pBL"]) - 2))

        def loglik_th_grad(self, model, tang, *a):
            return float("nan"), np.full(len(tang["pBL"]), np.nan)

    class TS:
        has_dt, has_sigma, n_tracks, ctx = False, False, 3, Ctx()

        def make_model(self, *a, **k):
            return object()

    p = T.generate_params(nb_states=2, LocErr_type=1, estimated_Ds=[1e-3, 0.25], estimated_LocErr=[0.02], estimated_Fs=[0.6], estimated_transition_rates=0.1)
    names = gradient.free_names(p)
    for tf in (None, (0.2, 120, 2000)):
        v, g = gradient.objective_and_gradient(p, TS(), 0.02, [1.0], 2, 1, 6, names=names, threshold_fusion=tf)
        assert v == np.inf and g.shape == (len(names),) and np.all(g == 0.0)
