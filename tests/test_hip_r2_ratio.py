"""GPU counterpart of tests/test_emul_r2_ratio.py: the ratio form of the log-carried g-form step of the register-resident 2-state likelihood
kernel (csrc/xt_reg2.h: xt_r2_step_g - children from h_q = 1 / (Ws Dq_q), table offsets from the per-lane packed word, three-FMA reciprocal)
through tracking.Proba_Cs, per-track LL against the numpy oracle at 1e-10 (TOL_LL of tests/test_hip_r2_logcarry.py).
N = 2 * (64 / 2^(F-1)) * 4 + 1 tracks: two workgroups of four waves and a partial batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DS, FS, TM = np.array([0.004, 0.1]), np.array([.35, .65]), np.array([[.92, .08], [.15, .85]])
TOL_LL = 1e-10


def _check(Cs, le, F, what, min_len=3, ok=None):
    from extrack_amd import tracking as TR
    from oracle import oracle_np as O
    LE = np.array([[[le]]])
    ref = O.proba_cs(Cs, LE, DS, FS, TM, 0.1, 1, [1.0], 1, F, min_len)
    ll = TR.Proba_Cs(Cs, LE, DS, FS, TM, 0.1, 1, [1.0], 1, F, min_len)
    ok = np.isfinite(ref) if ok is None else ok
    err = np.abs(ll[ok] - ref[ok]).max()
    print("%s F=%d shape=%s le=%g min_len=%d: max |dLL| %.3e (|LL| up to %.0f)" % (what, F, Cs.shape, le, min_len, err, np.abs(ref[ok]).max()))
    assert err < TOL_LL, (what, F, Cs.shape, le, err)
    return ll, ref


def _tracks(rng, N, L, D):
    return np.cumsum(rng.normal(0, 0.08, (N, L, D)), 1)


@pytest.mark.parametrize("le", [0.02, 1e-5])
@pytest.mark.parametrize("F", [4, 5, 6, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_ratio_windows_dims_and_lengths(F, D, le):
    """F + 1: the merge-free first step only; F + 2: one merge; 2 F + 1: every phase and one re-centring; 33: a staging-chunk boundary."""
    rng = np.random.default_rng(4000 + F * 10 + D)
    N = 2 * (64 >> (F - 1)) * 4 + 1
    for L in (F + 1, F + 2, 2 * F + 1, 33):
        _check(_tracks(rng, N, L, D), le, F, "ratio")


@pytest.mark.parametrize("le", [0.02, 1e-5])
@pytest.mark.parametrize("F", [4, 5, 6, 7])
def test_ratio_steady_steps_without_the_stay_factor(F, le):
    """min_len = F + 4 at L = 2 F + 5: steady steps on the plain transition table before the switch to T * stay."""
    rng = np.random.default_rng(4100 + F)
    N = 2 * (64 >> (F - 1)) * 4 + 1
    _check(_tracks(rng, N, 2 * F + 5, 2), le, F, "late stay", min_len=F + 4)


def test_ratio_long_tracks():
    """513 positions, |LL| ~ 1000: 102 passes over the five phases of F = 6 and as many re-centrings."""
    _check(_tracks(np.random.default_rng(8), 9, 513, 2), 0.02, 6, "long")


def test_ratio_nan_track():
    """A NaN coordinate in a steady step: that track's LL is NaN, its neighbours are finite and within tolerance."""
    F, N = 6, 9
    Cs = _tracks(np.random.default_rng(9), N, F + 5, 2)
    Cs[5, F + 2, 1] = np.nan
    ok = np.array([i != 5 for i in range(N)])
    ll, ref = _check(Cs, 0.02, F, "NaN", ok=ok)
    assert np.isnan(ll[5]) and np.isnan(ref[5])
    assert np.isfinite(ll[ok]).all()
