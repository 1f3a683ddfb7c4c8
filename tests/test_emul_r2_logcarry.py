"""Log-carried weights of the g-form step (extrack_amd/csrc/xt_reg2.h: xt_r2_step_g): a member's weight is y exp(lx), the merge takes ONE
exponential of lx1 - lx0, the merged log part is re-centred by an integer shift once per F - 1 steps and the shifts are added back at the
read-out.  Run on CPU threads (tests/emul/emul_gform.cpp) against the numpy oracle; the fully guarded steps (general algebra, linear
weights with integer exponents) on the same input are the second opinion.  Every case asserts that the launch took the g-form,
err < 1e-10 and err <= 2 err_guarded + 1e-12."""
import numpy as np
import pytest

from test_emul_r2_gform import GFORM, GUARDED, TM, _run, pytestmark  # noqa: F401

TOL_LL = 1e-10


def _tracks(rng, N, L, D):
    return np.cumsum(rng.normal(0, 0.08, (N, L, D)), 1)


def _both(Cs, le, F, isBL=1, min_len=3, ok=None, nblocks=2, what=""):
    LE = np.array([[[le]]])
    ll, _, ref = _run(Cs, LE, TM, isBL, F, min_len, GFORM, nblocks=nblocks)
    llg, _, _ = _run(Cs, LE, TM, isBL, F, min_len, GUARDED, nblocks=nblocks, guarded=True)
    ok = np.isfinite(ref) if ok is None else ok
    err, errg = np.abs(ll[ok] - ref[ok]).max(), np.abs(llg[ok] - ref[ok]).max()
    print("%s F=%d shape=%s le=%g: log-carried %.3e guarded %.3e (|LL| up to %.0f)" % (what, F, Cs.shape, le, err, errg, np.abs(ref[ok]).max()))
    assert err < TOL_LL, (F, Cs.shape, err)
    assert err <= 2.0 * errg + 1e-12, (F, Cs.shape, err, errg)
    return ll, ref


@pytest.mark.parametrize("F", [4, 5, 6, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_logcarry_windows_and_lengths(F, D):
    """L = F + 1: the merge-free first step only; F + 2: one merge; F + 4: crosses a re-normalisation; 2 F + 1: crosses a re-centring; 33 and
    65: staging-chunk boundaries.  Two blocks, a partial last batch."""
    rng = np.random.default_rng(1000 + F * 10 + D)
    N = 2 * (64 >> (F - 1)) + 1
    for L in (F + 1, F + 2, F + 4, 2 * F + 1, 33, 65):
        _both(_tracks(rng, N, L, D), 0.02, F, what="lengths")


@pytest.mark.parametrize("F,L,N", [(6, 513, 5), (4, 513, 17)])
def test_logcarry_long_tracks(F, L, N):
    """|LL| ~ 1000: the error must not grow with the accumulated log-likelihood faster than the guarded path's (both sit at the oracle's own
    log-domain rounding, ~ 7e-12 on this input) - what the re-centring is for."""
    rng = np.random.default_rng(F)
    _both(_tracks(rng, N, L, 2), 0.02, F, what="long")


@pytest.mark.parametrize("shift", [0.5, 2.0, 5.0, 20.0])
def test_logcarry_negligible_member(shift):
    """Every coordinate from position 12 on shifted: one member of the merges around the jump is negligible, |lx1 - lx0| runs far beyond the
    exponential's range (the scaled member's factor saturates to 0)."""
    rng = np.random.default_rng(int(shift * 10))
    Cs = _tracks(rng, 9, 20, 2)
    Cs[:, 12:] += shift
    _both(Cs, 0.02, 6, what="jump %g" % shift)


@pytest.mark.parametrize("F,D,le", [(6, 3, 1e-5), (7, 3, 2e-6), (4, 2, 1e-5)])
def test_logcarry_small_l2(F, D, le):
    """lnT' = ln T - D/2 ln l2 > 0 (up to + 39 per step): the large-base regime, lx grows by tens per step between the lazy re-normalisations."""
    rng = np.random.default_rng(F * 10 + D)
    N = 2 * (64 >> (F - 1)) + 1
    assert np.log(TM.min()) - 0.5 * D * np.log(le * le) > 5.0
    for L in (F + 2, 33):
        _both(_tracks(rng, N, L, D), le, F, what="small l2")


def test_logcarry_nan_in_a_steady_step():
    """A NaN position in a steady step: that track's likelihood is NaN, the others stay exact."""
    F, N = 6, 9
    rng = np.random.default_rng(7)
    Cs = _tracks(rng, N, F + 5, 2)
    Cs[5, F + 2, 1] = np.nan
    ok = np.array([i != 5 for i in range(N)])
    ll, ref = _both(Cs, 0.02, F, ok=ok, nblocks=1, what="NaN")
    assert np.isnan(ll[5]) and np.isnan(ref[5])
    assert not np.isnan(ll[ok]).any()
