"""Log-carried read-out of the last position of a g-form launch (extrack_amd/csrc/xt_reg2.h: xt_r2_body): one more
re-centring through the track's LDS cell, the four terms of a lane added as plain doubles, the shift given back with the steps' shifts.  Run on
CPU threads through the existing harnesses (tests/emul/emul_gform.cpp; tests/emul/emul_r2_gap.cpp for the GAPS instantiation) on the inputs of
tests/r2_readout_cases.py, per-track LL against oracle.oracle_np.proba_cs (the gap reference of tests/gap_reference.py for GAPS) at 1e-10.
Every launch is run twice, with and without per-track output: the summed log-likelihood equals the sum of the per-track values to 1e-12
relative.

Outlier cases (|LL| ~ 3.7e4 and 2.5e7): the bound comes from the parent commit - 4 x its library's largest |LL - oracle| / |LL| on the same
inputs, not less than 4 ulp of |LL| - applied per population (r2_readout_cases.check_outlier).  Measured on MI355X with the parent's library
(EXTRACK_HIP_LIB): 0.562 on the track shifted by 520 in every case (its exponential clamps at -1.1e7 where the argument is -2.5e7), so that
track's bound, 2.25 |LL|, checks nothing but finiteness; 5.94e-16 (3.00 ulp) on the tracks shifted by 20, whose bound is 2.4e-15 |LL|.  This
build: at most 4.00 ulp (7.9e-16 relative) over all tracks on MI355X; in the emulation 4 ulp on the tracks shifted by 20, 3 ulp on the 520 one."""
import ctypes as C

import numpy as np
import pytest

import r2_readout_cases as RC
from oracle import oracle_np as O
from test_emul_r2_gform import GFORM, _dp, _gform_lib, pytestmark  # noqa: F401


def _launch(Cs, le, F, per_track, isBL=1, min_len=3, nblocks=2):
    """(per-track LL or None, total) of one emulated launch, which must have taken the g-form."""
    Cs = np.ascontiguousarray(Cs, float)
    N, L, D = Cs.shape
    ps = np.ascontiguousarray(O.p_stay_table(RC.DS, 2, 1, [1.0]), float)
    locerr = np.array([le, 0.0, 0.0])
    ll, tot, scaling = (np.zeros(N) if per_track else None), C.c_double(0), C.c_int(-1)
    dsc, Fsc, Tc = [np.ascontiguousarray(x, float) for x in (RC.DS, RC.FS, RC.TM)]
    rc = _gform_lib().xt_emul_gform_run(_dp(Cs), None, C.c_longlong(N), L, D, 1, F, int(isBL), int(min_len), 0, 1, _dp(locerr), C.c_double(0.1),
                                        _dp(dsc), _dp(Fsc), _dp(Tc), _dp(ps), nblocks, 0, _dp(ll), C.byref(tot), C.byref(scaling))
    assert rc == 0 and scaling.value == GFORM, (rc, scaling.value)
    return ll, tot.value


def _run(Cs, le, F, **kw):
    """Per-track LL, oracle; asserts the sum of a launch without per-track output against the per-track values."""
    ref = O.proba_cs(Cs, np.array([[[le]]]), RC.DS, RC.FS, RC.TM, 0.1, kw.get("isBL", 1), [1.0], 1, F, kw.get("min_len", 3))
    ll, tot = _launch(Cs, le, F, True, **kw)
    _, tot0 = _launch(Cs, le, F, False, **kw)
    if np.all(np.isfinite(ll)):
        assert abs(tot0 - ll.sum()) <= 1e-12 * abs(ll.sum()), (tot0, ll.sum())
        assert abs(tot - ll.sum()) <= 1e-12 * abs(ll.sum()), (tot, ll.sum())
    else:
        assert np.isnan(tot0) == np.isnan(ll).any()
    return ll, ref


def _exact(Cs, le, F, what, ok=None, **kw):
    ll, ref = _run(Cs, le, F, **kw)
    ok = np.isfinite(ref) if ok is None else ok
    err = np.abs(ll[ok] - ref[ok]).max()
    print("%s F=%d shape=%s le=%g: max |dLL| %.3e (|LL| up to %.0f)" % (what, F, Cs.shape, le, err, np.abs(ref[ok]).max()))
    assert np.abs(ref[ok]).max() <= 1e4
    assert err < RC.TOL_LL, (what, F, Cs.shape, err)
    return ll, ref


@pytest.mark.parametrize("F", RC.FS_ALL)
@pytest.mark.parametrize("D", RC.DS_ALL)
def test_readout_lengths(F, D):
    """L = 3, F, F + 1 (no steady step before the read-out; 3: no step at all, the chain's dead lanes and the dead member take part), every
    L from F + 2 to 2 F (each exchange phase, so each `prev` lane bit; the re-centring phase leaves the cell in use), 32, 33, 34 (staging
    chunk boundary) and 65."""
    for what, Cs in RC.length_cases(F, D):
        _exact(Cs, RC.LE, F, what, isBL=D % 2, min_len=2 + D % 2)


@pytest.mark.parametrize("F", RC.FS_ALL)
@pytest.mark.parametrize("last_only", [True, False])
def test_readout_last_row_outlier(F, last_only):
    """The last position (or every position from L - 2 on) shifted by 20, one track's by 520: every a_Qq far beyond the exponential's range, the
    read-out's shift 1e5 .. 1e8 (carried as a double, not in the 32-bit cell).  Finite, and within the bound derived from the parent."""
    for what, Cs in RC.outlier_cases(F, 2, last_only):
        ll, ref = _run(Cs, RC.LE, F)
        RC.check_outlier(ll, ref, "F=%d %s %s" % (F, "last row" if last_only else "from L-2", what))


@pytest.mark.parametrize("F,D,le", RC.SMALL_L2)
def test_readout_small_l2(F, D, le):
    for what, Cs in RC.small_l2_cases(F, D):
        _exact(Cs, le, F, "small l2 " + what)


@pytest.mark.parametrize("F", RC.FS_ALL)
def test_readout_single_tracks(F):
    """N = 1 and N = tracks-per-wave + 1: one block, the other slots of the wave mirror the last track."""
    for what, Cs in RC.single_track_cases(F, 2):
        _exact(Cs, RC.LE, F, what, nblocks=1)


@pytest.mark.parametrize("F", RC.FS_ALL)
@pytest.mark.parametrize("L", [3, 12, 33])
def test_readout_nan_poisons_its_track_only(F, L):
    """A NaN coordinate in the last row of one track and in a steady step of another: those are NaN, their neighbours in the same wave equal
    the clean launch bit for bit."""
    Cs, bad = RC.nan_case(F, 2, L)
    ll, ref = _exact(Cs, RC.LE, F, "NaN L=%d" % L, ok=~bad)
    assert np.all(np.isnan(ll[bad])) and np.all(np.isnan(ref[bad])) and not np.isnan(ll[~bad]).any()
    clean = Cs.copy()
    clean[np.isnan(clean)] = 0.1
    llc, _ = _launch(clean, RC.LE, F, True)
    assert np.array_equal(llc[~bad], ll[~bad])


@pytest.mark.parametrize("F,D", [(4, 2), (6, 1), (6, 2), (6, 3), (7, 2)])
def test_readout_gaps(F, D):
    """The GAPS instantiation as tests/test_emul_r2_gaps.py reaches it: 25 % of the interior rows missed, a missed row at L - 2, against the gap
    reference; the sum without per-track output against the per-track values."""
    import gap_reference as R
    import test_emul_r2_gaps as G
    ps = np.ascontiguousarray(O.p_stay_table(G.DS, 2, 1, R.CELL), float)
    dsc, Fsc, Tc = [np.ascontiguousarray(x, float) for x in (G.DS, G.FS, G.TM)]
    fmask = G.F_DEFAULT if (G.F_DEFAULT >> F) & 1 else G.F_ALL
    for what, Cs in RC.gap_cases(F, D):
        ll = G.served(Cs, F, 1, 3)
        Cs = np.ascontiguousarray(Cs, float)
        tot0, info = C.c_double(0), (C.c_int * 4)()
        rc = G.gap_lib().xt_emul_r2_gap_run(_dp(Cs), C.c_longlong(len(Cs)), Cs.shape[1], D, F, 1, 3, C.c_double(G.LE), C.c_double(R.PBL), _dp(dsc),
                                            _dp(Fsc), _dp(Tc), _dp(ps), 2, 1, 1, int(fmask), None, C.byref(tot0), info)
        assert rc == 0 and info[0] == G.GAPS_REG2, (rc, list(info))
        assert np.all(np.isfinite(ll)) and abs(tot0.value - ll.sum()) <= 1e-12 * abs(ll.sum()), (what, tot0.value, ll.sum())
