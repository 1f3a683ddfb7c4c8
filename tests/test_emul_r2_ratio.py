"""Ratio form of the log-carried g-form step (extrack_amd/csrc/xt_reg2.h: xt_r2_step_g): the children are formed from h_q = 1 / (Ws Dq_q)
and k_q = l2 Ws h_q instead of 1 / W, G and g_q, and the step reads its [prev][q] table offsets from a per-lane word packed once per kernel
(xt_r2_pack_io, built from the context's own pair_natural predicate) instead of deriving them from the lane id.  Run on CPU threads
(tests/emul/emul_gform.cpp) against the numpy oracle and the fully guarded steps, at the tolerances of tests/test_emul_r2_logcarry.py:
err < 1e-10 and err <= 2 err_guarded + 1e-12, and every launch must have taken the g-form.  What the change can newly break: a phase's
field of the packed word (every F, F = 5 and the lane bit 2 of F = 7 included; every phase is run from F + 2 positions on, all of them and
one re-centring by 2 F + 1), the D = 2 branch of y_q against the general one (D = 1, 3), the merge-free first step (F + 1), the staging
boundary (33), and steady steps on the table WITHOUT the stay factor (min_len beyond the warm-up)."""
import numpy as np
import pytest

from test_emul_r2_gform import pytestmark  # noqa: F401
from test_emul_r2_logcarry import _both, _tracks


@pytest.mark.parametrize("le", [0.02, 1e-5])
@pytest.mark.parametrize("F", [4, 5, 6, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_ratio_windows_dims_and_lengths(F, D, le):
    """N = 2 * (64 / 2^(F-1)) * 4 + 1 tracks: two blocks of four waves and a partial last batch."""
    rng = np.random.default_rng(3000 + F * 10 + D)
    N = 2 * (64 >> (F - 1)) * 4 + 1
    for L in (F + 1, F + 2, 2 * F + 1, 33):
        _both(_tracks(rng, N, L, D), le, F, what="ratio")


@pytest.mark.parametrize("le", [0.02, 1e-5])
@pytest.mark.parametrize("F", [4, 5, 6, 7])
def test_ratio_steady_steps_without_the_stay_factor(F, le):
    """min_len = F + 4 at L = 2 F + 5: positions F .. F + 3 are steady steps on the plain transition table, the later ones on T * stay (with
    min_len = 3 the switch happens during the warm-up and no steady step ever reads the first table)."""
    rng = np.random.default_rng(3100 + F)
    N = 2 * (64 >> (F - 1)) * 4 + 1
    _both(_tracks(rng, N, 2 * F + 5, 2), le, F, min_len=F + 4, what="late stay")
