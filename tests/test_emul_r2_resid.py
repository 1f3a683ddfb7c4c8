"""Residual-carried means, doubled log units and the log-carried warm-up chain of the g-form launches of the register-resident 2-state
likelihood kernel (extrack_amd/csrc/xt_reg2.h: xt_r2_step_g, xt_r2_chain_g): the members carry r = c_next - m instead of m (the staged
array holds the position deltas, a chunk's last one reaching into the next chunk), lambda = -2 x the log weight (the merge takes
exp(-|lambda1 - lambda0| / 2), the re-centring integers are in lambda units), and the warm-up hands (y, lambda, r, v = l2 + u) over without an
exponential - to the merge-free first step, or straight to the read-out when the bucket is too short to fill the window.  Run on CPU
threads (tests/emul/emul_gform.cpp) against the numpy oracle and the fully guarded steps, by the rule of tests/test_emul_r2_logcarry.py:
err < 1e-10, err <= 2 err_guarded + 1e-12, and every launch must have taken the g-form.  N = 2 * (64 / 2^(F-1)) * 4 + 1 tracks: two
workgroups of four waves and a partial batch."""
import numpy as np
import pytest

from test_emul_r2_gform import pytestmark  # noqa: F401
from test_emul_r2_logcarry import _both, _tracks


def _n(F):
    return 2 * (64 >> (F - 1)) * 4 + 1


@pytest.mark.parametrize("le", [0.02, 1e-5])
@pytest.mark.parametrize("F", [4, 5, 6, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_resid_windows_dims_and_lengths(F, D, le):
    """2, 3, F - 1, F: the chain alone goes into the read-out, with dummy digits; F + 1: the merge-free first step; F + 2: one merge;
    2 F + 1: every phase and one re-centring; 33, 34, 65: the delta across a staging boundary (the last position of the track in the next
    chunk, one step in the next chunk, two boundaries)."""
    rng = np.random.default_rng(5000 + F * 10 + D)
    for L in sorted({2, 3, F - 1, F, F + 1, F + 2, 2 * F + 1, 33, 34, 65}):
        _both(_tracks(rng, _n(F), L, D), le, F, what="resid")


@pytest.mark.parametrize("le", [0.02, 1e-5])
@pytest.mark.parametrize("F", [4, 5, 6, 7])
def test_resid_late_stay_factor(F, le):
    """min_len = F + 4 at L = 2 F + 5: the whole chain and the first steady steps run on the table without the stay factor; min_len = 3 at
    the same length switches tables inside the chain."""
    rng = np.random.default_rng(5100 + F)
    Cs = _tracks(rng, _n(F), 2 * F + 5, 2)
    _both(Cs, le, F, min_len=F + 4, what="late stay")
    _both(Cs, le, F, min_len=3, what="chain switch")


@pytest.mark.parametrize("le", [0.02, 1e-5])
@pytest.mark.parametrize("F", [4, 6])
def test_resid_coordinate_offset(F, le):
    """Every coordinate shifted by + 200, against the oracle on the same shifted input (the oracle alone moves by at most 2.2e-11 under this
    shift at these settings, so the rule's 1e-10 holds for the reference): the deltas are rounded at ulp(200), the absolute coordinates
    are never read."""
    rng = np.random.default_rng(5200 + F)
    for L in (F, F + 2, 2 * F + 1, 34):
        _both(_tracks(rng, _n(F), L, 2) + 200.0, le, F, what="offset 200")


def test_resid_long_tracks():
    """513 positions, |LL| ~ 1000: a hundred re-centrings in lambda units, sixteen staging boundaries."""
    _both(_tracks(np.random.default_rng(8), 9, 513, 2), 0.02, 6, what="long")


@pytest.mark.parametrize("F", [4, 6])
@pytest.mark.parametrize("where", ["chain", "steady"])
def test_resid_nan_track(F, where):
    """A NaN coordinate at position 2 (inside the chain; it enters two deltas) or F + 2 (a steady step): that track's LL is NaN, its
    neighbours are finite and within tolerance."""
    N = 9
    Cs = _tracks(np.random.default_rng(5300 + F), N, F + 5, 2)
    Cs[5, 2 if where == "chain" else F + 2, 1] = np.nan
    ok = np.array([i != 5 for i in range(N)])
    ll, ref = _both(Cs, 0.02, F, ok=ok, nblocks=1, what="NaN " + where)
    assert np.isnan(ll[5]) and np.isnan(ref[5])
    assert np.isfinite(ll[ok]).all()
