"""GPU twin of tests/test_emul_r2_readout.py: the log-carried read-out of the last position of a g-form launch (csrc/xt_reg2.h: xt_r2_body,
DESIGN.md section 26) through tracking.Proba_Cs on the inputs of tests/r2_readout_cases.py, per-track LL against the numpy oracle at 1e-10;
the GAPS instantiation as tests/test_hip_reg2_gaps.py reaches it, against the gap reference.  For every case the launch's summed
log-likelihood without per-track output equals the sum of the per-track values to 1e-12 relative.

Outlier cases (|LL| ~ 3.7e4 and 2.5e7): the bound comes from the parent commit - 4 x its library's largest |LL - oracle| / |LL| on the same
inputs, not less than 4 ulp of |LL| - applied per population (r2_readout_cases.check_outlier).  Measured on MI355X with the parent's library
(EXTRACK_HIP_LIB): 0.562 on the track shifted by 520 in every case (its exponential clamps at -1.1e7 where the argument is -2.5e7), so that
track's bound, 2.25 |LL|, checks nothing but finiteness; 5.94e-16 (3.00 ulp) on the tracks shifted by 20, whose bound is 2.4e-15 |LL|.  This
build: at most 4.00 ulp (7.9e-16 relative) over all tracks on MI355X; in the emulation 4 ulp on the tracks shifted by 20, 3 ulp on the 520 one."""
import numpy as np
import pytest

import r2_readout_cases as RC

pytestmark = pytest.mark.gpu


def _run(Cs, le, F, isBL=1, min_len=3):
    """Per-track LL (tracking.Proba_Cs), oracle; asserts the sum of a launch without per-track output against the per-track values."""
    from extrack_amd import tracking as TR
    from oracle import oracle_np as O
    LE = np.array([[[le]]])
    ref = O.proba_cs(Cs, LE, RC.DS, RC.FS, RC.TM, 0.1, isBL, [1.0], 1, F, min_len)
    ll = TR.Proba_Cs(Cs, LE, RC.DS, RC.FS, RC.TM, 0.1, isBL, [1.0], 1, F, min_len)
    ts, lev = TR._one_bucket(Cs, LE, isBL, min_len, 0)
    try:
        model = ts.make_model(lev, RC.DS, RC.FS, RC.TM, 0.1, [1.0], 1, F)
        tot0 = ts.loglik(model)
        # no quiet fall-back to another kernel family; that the scaling decision of these very inputs is the g-form is asserted by the emulation
        # twin, which runs the product's own xt_launch_scaling
        assert ts.ctx.last_ll_path() == "reg2", ts.ctx.last_ll_path()
        tot1, ll1 = ts.loglik(model, per_track=True)
        assert ts.ctx.last_ll_path() == "reg2" and np.array_equal(ll1, ll, equal_nan=True)
    finally:
        ts.close()
    if np.all(np.isfinite(ll)):
        assert abs(tot0 - ll.sum()) <= 1e-12 * abs(ll.sum()), (tot0, ll.sum())
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
    """L = 3, F, F + 1, every L from F + 2 to 2 F, 32, 33, 34 and 65 (r2_readout_cases.lengths)."""
    for what, Cs in RC.length_cases(F, D):
        _exact(Cs, RC.LE, F, what, isBL=D % 2, min_len=2 + D % 2)


@pytest.mark.parametrize("F", RC.FS_ALL)
@pytest.mark.parametrize("last_only", [True, False])
def test_readout_last_row_outlier(F, last_only):
    """The last position (or every position from L - 2 on) shifted by 20, one track's by 520: finite, within the bound derived from the parent."""
    for what, Cs in RC.outlier_cases(F, 2, last_only):
        ll, ref = _run(Cs, RC.LE, F)
        RC.check_outlier(ll, ref, "F=%d %s %s" % (F, "last row" if last_only else "from L-2", what))


@pytest.mark.parametrize("F,D,le", RC.SMALL_L2)
def test_readout_small_l2(F, D, le):
    for what, Cs in RC.small_l2_cases(F, D):
        _exact(Cs, le, F, "small l2 " + what)


@pytest.mark.parametrize("F", RC.FS_ALL)
def test_readout_single_tracks(F):
    for what, Cs in RC.single_track_cases(F, 2):
        _exact(Cs, RC.LE, F, what)


@pytest.mark.parametrize("F", RC.FS_ALL)
@pytest.mark.parametrize("L", [3, 12, 33])
def test_readout_nan_poisons_its_track_only(F, L):
    """A NaN coordinate in one track gives NaN for that track only; its neighbours in the same wave equal the clean launch bit for bit."""
    from extrack_amd import tracking as TR
    Cs, bad = RC.nan_case(F, 2, L)
    ll, ref = _exact(Cs, RC.LE, F, "NaN L=%d" % L, ok=~bad)
    assert np.all(np.isnan(ll[bad])) and np.all(np.isnan(ref[bad])) and not np.isnan(ll[~bad]).any()
    clean = Cs.copy()
    clean[np.isnan(clean)] = 0.1
    llc = TR.Proba_Cs(clean, np.array([[[RC.LE]]]), RC.DS, RC.FS, RC.TM, 0.1, 1, [1.0], 1, F, 3)
    assert np.array_equal(llc[~bad], ll[~bad])


@pytest.mark.parametrize("F,D", [(4, 2), (6, 1), (6, 2), (6, 3), (7, 2)])
def test_readout_gaps(F, D):
    """25 % of the interior rows missed at L = F + 2, 12, 33 and a missed row at L - 2, on the upgraded gap launch, against the gap reference."""
    import test_hip_reg2_gaps as G
    from extrack_amd import _lib
    c = G._context_under("EXTRACK_GAP_REG2_F", "all") if F == 4 else _lib.Context(0)
    try:
        for what, Cs in RC.gap_cases(F, D):
            L = Cs.shape[1]
            model = G._model(F, 3, L)
            tot, got = G._loglik(c, model, [Cs])
            assert c.last_ll_path() == "gaps_reg2"
            G._compare(tot, got, G._reference([Cs], F, 3), "gaps F=%d D=%d %s" % (F, D, what))
            tot0 = c.loglik(model, gaps=True)
            assert c.last_ll_path() == "gaps_reg2" and abs(tot0 - got[0].sum()) <= 1e-12 * abs(got[0].sum()), (what, tot0, got[0].sum())
    finally:
        c.close()
