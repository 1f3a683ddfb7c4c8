"""g-form steps of the register-resident 2-state body (extrack_amd/csrc/xt_reg2.h: xt_r2_step_g, likelihood only): launches with one global
localisation variance l2 >= 1e-12 in a well-scaled model run every full-window step on the ratio g = l2 / den, with the transition weight
and l2^(-D/2) folded into the exponential's argument (which is then positive for small l2).  Run on CPU threads
(tests/emul/emul_gform.cpp: the body under the product's own scaling decision) against the numpy oracle; the fully guarded steps (the
general algebra) on the same input are the second opinion.  Which steps a launch took is read back from that launcher
(XtKernelArgs::well_scaled: 0 guarded, 1 well scaled, 2 g-form)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle_np as O

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

DS, FS, TM = np.array([0.004, 0.1]), np.array([.35, .65]), np.array([[.92, .08], [.15, .85]])
GUARDED, WELL_SCALED, GFORM = 0, 1, 2


HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul")
CSRC = os.path.join(HERE, "..", "..", "extrack_amd", "csrc")
_lib = None


def _gform_lib():
    """tests/emul/emul_gform.cpp -> tests/emul/libxt_emul_gform.so (rebuilt when a source it includes is newer)."""
    global _lib
    if _lib is None:
        so, src = os.path.join(HERE, "libxt_emul_gform.so"), os.path.join(HERE, "emul_gform.cpp")
        deps = [src, os.path.join(HERE, "emul_ctx.h")] + [os.path.join(CSRC, h) for h in ("xt_kernel.h", "xt_math.h", "xt_tables.h", "xt_fast2.h", "xt_grad.h", "xt_reg2.h")]
        if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-pthread", "-shared", src, "-o", so])
        _lib = C.CDLL(so)
    return _lib


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _run(Cs, LE, T, isBL, F, min_len, path, nblocks=2, ds=DS, guarded=False):
    """(emulated per-track LL, total, oracle per-track LL) of one launch that must have taken `path`."""
    ps = np.ascontiguousarray(O.p_stay_table(ds, 2, 1, [1.0]), float)
    ref = O.proba_cs(Cs, LE, ds, FS, T, 0.1, isBL, [1.0], 1, F, min_len)
    Cs = np.ascontiguousarray(Cs, float)
    N, L, D = Cs.shape
    LE = np.ascontiguousarray(LE, float)
    if LE.shape[1] == 1:
        mode, K, KS, sigma, locerr = 0, LE.shape[2], 1, None, np.zeros(3)
        locerr[:K] = LE[0, 0]
    else:
        mode, K, KS, sigma, locerr = 1, LE.shape[2], LE.shape[2], LE, np.zeros(3)
    ll, tot, scaling = np.zeros(N), C.c_double(0), C.c_int(-1)
    dsc, Fsc, Tc = [np.ascontiguousarray(x, float) for x in (ds, FS, T)]
    rc = _gform_lib().xt_emul_gform_run(_dp(Cs), _dp(sigma), C.c_longlong(N), L, D, KS, F, int(isBL), int(min_len), mode, K, _dp(locerr),
                                        C.c_double(0.1), _dp(dsc), _dp(Fsc), _dp(Tc), _dp(ps), nblocks, int(guarded), _dp(ll), C.byref(tot),
                                        C.byref(scaling))
    assert rc == 0, rc
    assert scaling.value == path, (scaling.value, path)
    return ll, tot.value, ref


def _check(Cs, LE, T, isBL, F, min_len, path, ok=None, **kw):
    ll, tot, ref = _run(Cs, LE, T, isBL, F, min_len, path, **kw)
    ok = np.isfinite(ref) if ok is None else ok
    err = np.abs(ll[ok] - ref[ok]).max()
    print("F=%d shape=%s min_len=%d isBL=%d path=%d: max |dLL| %.3e, total %.3e" % (F, Cs.shape, min_len, isBL, path, err, abs(tot - ref.sum())))
    assert err < 1e-10, (F, Cs.shape, err)
    assert np.array_equal(np.isnan(ll), np.isnan(ref))
    if ok.all():
        assert abs(tot - ref.sum()) < 1e-9
    return ll


@pytest.mark.parametrize("F", [4, 5, 6, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("isBL", [0, 1])
def test_gform_lengths_dims_and_tables(F, D, isBL):
    """Lengths F - 1 .. F + 3 (F - 1 and F end inside the warm-up: no g-form step runs; F + 1 runs the merge-free first step only), 33
    (two staging chunks) and 65 (three); min_len 2 and 3 move the switch to the stay-in-FOV table.  N = 2 * 64 / 2^(F-1) + 1 tracks in
    two blocks: a partial last batch."""
    rng = np.random.default_rng(F * 100 + D * 10 + isBL)
    N = 2 * (64 >> (F - 1)) + 1
    for min_len in (2, 3):
        for L in list(range(F - 1, F + 4)) + [33, 65]:
            Cs = np.cumsum(rng.normal(0, 0.08, (N, L, D)), 1)
            _check(Cs, np.array([[[0.02]]]), TM, isBL, F, min_len, GFORM)


@pytest.mark.parametrize("F", [4, 6, 7])
@pytest.mark.parametrize("le,path", [(0.0, WELL_SCALED), (1e-7, WELL_SCALED), (1e-5, GFORM)])
def test_gform_eligibility(F, le, path):
    """g = l2 / den needs l2 > 0: the launcher asks for l2 >= 1e-12.  Localisation errors 0 and 1e-7 (l2 = 1e-14) keep the general
    steps, 1e-5 (l2 = 1e-10) takes the g-form; all agree with the oracle."""
    rng = np.random.default_rng(int(F * 10 + path))
    N = 2 * (64 >> (F - 1)) + 1
    for L in (F + 1, F + 3, 33):
        Cs = np.cumsum(rng.normal(0, 0.08, (N, L, 2)), 1)
        _check(Cs, np.array([[[le]]]), TM, 1, F, 3, path)


@pytest.mark.parametrize("F,D,le", [(4, 3, 1e-5), (6, 3, 1e-5), (7, 3, 2e-6), (6, 2, 1e-5), (5, 1, 1e-5), (6, 3, 1e-3)])
def test_gform_positive_exp_arguments(F, D, le):
    """T / l2^(D/2) far above 1 (1e15 at D = 3, l2 = 1e-10; 2e17 at l2 = 4e-12): the exponential is evaluated at arguments up to + 40,
    i.e. with a positive integer part n, whose table index and exponent come out of the same bit extraction as for n < 0."""
    rng = np.random.default_rng(F * 10 + D)
    N = 2 * (64 >> (F - 1)) + 1
    assert np.log(TM.min()) - 0.5 * D * np.log(le * le) > 5.0
    for L in (F + 1, F + 2, 33, 65):
        Cs = np.cumsum(rng.normal(0, 0.08, (N, L, D)), 1)
        _check(Cs, np.array([[[le]]]), TM, 0, F, 2, GFORM)


@pytest.mark.parametrize("F,D", [(4, 2), (6, 2), (7, 1), (5, 3)])
def test_gform_coordinate_offset(F, D):
    """Tracks offset by + 100 in every coordinate: the oracle itself loses digits there (c - m at |c| = 100), so the yardstick is the
    guarded path (general algebra) on the same input - the g-form's largest error against the oracle may be at most twice its, + 1e-12."""
    rng = np.random.default_rng(F * 10 + D)
    N = 2 * (64 >> (F - 1)) + 1
    for L in (F + 2, 33):
        Cs = np.cumsum(rng.normal(0, 0.08, (N, L, D)), 1) + 100.0
        LE = np.array([[[0.02]]])
        ll, _, ref = _run(Cs, LE, TM, 1, F, 3, GFORM)
        llg, _, _ = _run(Cs, LE, TM, 1, F, 3, GUARDED, guarded=True)
        err, errg = np.abs(ll - ref).max(), np.abs(llg - ref).max()
        print("F=%d D=%d L=%d offset 100: g-form %.3e guarded %.3e" % (F, D, L, err, errg))
        assert err <= 2.0 * errg + 1e-12, (F, D, L, err, errg)


@pytest.mark.parametrize("F", [4, 6, 7])
def test_gform_nan_track(F):
    """A NaN position inside the warm-up and one in a g-form step: those tracks' likelihoods are NaN, the others exact."""
    rng = np.random.default_rng(F)
    N, L = 9, F + 5
    Cs = np.cumsum(rng.normal(0, 0.08, (N, L, 2)), 1)
    Cs[2, 1, 0] = np.nan
    Cs[5, F + 2, 1] = np.nan
    ll = _check(Cs, np.array([[[0.02]]]), TM, 1, F, 3, GFORM, nblocks=1, ok=np.array([i not in (2, 5) for i in range(N)]))
    assert np.isnan(ll[2]) and np.isnan(ll[5])


@pytest.mark.parametrize("F,D,K,per_peak", [(6, 2, 1, True), (4, 2, 2, True), (6, 2, 2, False), (5, 3, 3, False)])
def test_per_peak_and_per_dimension_errors_keep_the_general_steps(F, D, K, per_peak):
    """Per-peak errors (no constant l2) and one error per dimension (K == D) are not g-form launches: unchanged steps, same agreement."""
    rng = np.random.default_rng(F * 100 + D * 10 + K)
    N = 13
    for L in (F + 1, F + 2, 33):
        Cs = np.cumsum(rng.normal(0, 0.08, (N, L, D)), 1)
        LE = rng.uniform(0.01, 0.04, (N, L, K)) if per_peak else np.array([[[0.02, 0.03, 0.025][:K]]])
        _check(Cs, LE, TM, 1, F, 3, WELL_SCALED, nblocks=1)
