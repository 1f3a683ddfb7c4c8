"""GPU counterpart of tests/test_emul_r2_logcarry.py: the log-carried g-form step of the register-resident 2-state likelihood kernel
(csrc/xt_reg2.h: xt_r2_step_g - weights y exp(lx), one exponential per merge, integer re-centring of the log part) through the C ABI,
per-track LL against the numpy oracle at 1e-10.  N = 2 * (64 / 2^(F-1)) * 4 + 1 tracks: two workgroups of four waves and a partial batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DS, FS, TM = np.array([0.004, 0.1]), np.array([.35, .65]), np.array([[.92, .08], [.15, .85]])
TOL_LL = 1e-10


def _check(Cs, le, F, what, ok=None):
    from extrack_amd import tracking as TR
    from oracle import oracle_np as O
    LE = np.array([[[le]]])
    ref = O.proba_cs(Cs, LE, DS, FS, TM, 0.1, 1, [1.0], 1, F, 3)
    ll = TR.Proba_Cs(Cs, LE, DS, FS, TM, 0.1, 1, [1.0], 1, F, 3)
    ok = np.isfinite(ref) if ok is None else ok
    err = np.abs(ll[ok] - ref[ok]).max()
    print("%s F=%d shape=%s le=%g: max |dLL| %.3e (|LL| up to %.0f)" % (what, F, Cs.shape, le, err, np.abs(ref[ok]).max()))
    assert err < TOL_LL, (what, F, Cs.shape, le, err)
    return ll, ref


def _tracks(rng, N, L, D):
    return np.cumsum(rng.normal(0, 0.08, (N, L, D)), 1)


@pytest.mark.parametrize("F", [4, 6, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_logcarry_windows_and_lengths(F, D):
    """F + 1: the merge-free first step only; F + 2: one merge; 2 F + 1: crosses a re-centring; 33 and 65: staging-chunk boundaries."""
    rng = np.random.default_rng(2000 + F * 10 + D)
    N = 2 * (64 >> (F - 1)) * 4 + 1
    for L in (F + 1, F + 2, 2 * F + 1, 33, 65):
        _check(_tracks(rng, N, L, D), 0.02, F, "lengths")


def test_logcarry_long_tracks():
    """|LL| ~ 1000 over 513 positions: the re-centred log part does not lose digits to the accumulated log-likelihood."""
    _check(_tracks(np.random.default_rng(6), 9, 513, 2), 0.02, 6, "long")


@pytest.mark.parametrize("shift", [0.5, 2.0, 5.0, 20.0])
def test_logcarry_negligible_member(shift):
    """Every coordinate from position 12 on shifted: |lx1 - lx0| far beyond the exponential's range around the jump."""
    Cs = _tracks(np.random.default_rng(int(shift * 10)), 9, 20, 2)
    Cs[:, 12:] += shift
    _check(Cs, 0.02, 6, "jump %g" % shift)


@pytest.mark.parametrize("F,D,le", [(6, 3, 1e-5), (7, 3, 2e-6), (4, 2, 1e-5)])
def test_logcarry_small_l2(F, D, le):
    """lnT' = ln T - D/2 ln l2 > 0: the log part grows by tens per step between the lazy re-normalisations."""
    rng = np.random.default_rng(F * 10 + D)
    N = 2 * (64 >> (F - 1)) * 4 + 1
    for L in (F + 2, 33):
        _check(_tracks(rng, N, L, D), le, F, "small l2")
