"""GPU counterpart of tests/test_emul_r2_resid.py: residual-carried means, doubled log units and the log-carried warm-up chain of the
g-form launches of the register-resident 2-state likelihood kernel (csrc/xt_reg2.h: xt_r2_step_g, xt_r2_chain_g) through
tracking.Proba_Cs, per-track LL against the numpy oracle at 1e-10 (TOL_LL of tests/test_hip_r2_ratio.py).
N = 2 * (64 / 2^(F-1)) * 4 + 1 tracks: two workgroups of four waves and a partial batch."""
import numpy as np
import pytest

from test_hip_r2_ratio import _check, _tracks

pytestmark = pytest.mark.gpu


def _n(F):
    return 2 * (64 >> (F - 1)) * 4 + 1


@pytest.mark.parametrize("le", [0.02, 1e-5])
@pytest.mark.parametrize("F", [4, 5, 6, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_resid_windows_dims_and_lengths(F, D, le):
    """2, 3, F - 1, F: the chain alone goes into the read-out, with dummy digits; F + 1: the merge-free first step; F + 2: one merge;
    2 F + 1: every phase and one re-centring; 33, 34, 65: the delta across a staging boundary."""
    rng = np.random.default_rng(6000 + F * 10 + D)
    for L in sorted({2, 3, F - 1, F, F + 1, F + 2, 2 * F + 1, 33, 34, 65}):
        _check(_tracks(rng, _n(F), L, D), le, F, "resid")


@pytest.mark.parametrize("le", [0.02, 1e-5])
@pytest.mark.parametrize("F", [4, 5, 6, 7])
def test_resid_late_stay_factor(F, le):
    """min_len = F + 4 at L = 2 F + 5: chain and first steady steps on the table without the stay factor; min_len = 3: the switch inside
    the chain."""
    rng = np.random.default_rng(6100 + F)
    Cs = _tracks(rng, _n(F), 2 * F + 5, 2)
    _check(Cs, le, F, "late stay", min_len=F + 4)
    _check(Cs, le, F, "chain switch", min_len=3)


@pytest.mark.parametrize("le", [0.02, 1e-5])
@pytest.mark.parametrize("F", [4, 6])
def test_resid_coordinate_offset(F, le):
    """Every coordinate shifted by + 200, against the oracle on the same shifted input (which alone moves by at most 2.2e-11 under the
    shift at these settings)."""
    rng = np.random.default_rng(6200 + F)
    for L in (F, F + 2, 2 * F + 1, 34):
        _check(_tracks(rng, _n(F), L, 2) + 200.0, le, F, "offset 200")


def test_resid_long_tracks():
    """513 positions, |LL| ~ 1000: a hundred re-centrings in lambda units, sixteen staging boundaries."""
    _check(_tracks(np.random.default_rng(8), 9, 513, 2), 0.02, 6, "long")


@pytest.mark.parametrize("F", [4, 6])
@pytest.mark.parametrize("where", ["chain", "steady"])
def test_resid_nan_track(F, where):
    """A NaN coordinate at position 2 (inside the chain) or F + 2 (a steady step): that track's LL is NaN, its neighbours are finite and
    within tolerance."""
    N = 9
    Cs = _tracks(np.random.default_rng(6300 + F), N, F + 5, 2)
    Cs[5, 2 if where == "chain" else F + 2, 1] = np.nan
    ok = np.array([i != 5 for i in range(N)])
    ll, ref = _check(Cs, 0.02, F, "NaN " + where, ok=ok)
    assert np.isnan(ll[5]) and np.isnan(ref[5])
    assert np.isfinite(ll[ok]).all()
