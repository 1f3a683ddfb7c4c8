"""Warm-up of the register-resident 2-state body (extrack_amd/csrc/xt_reg2.h, likelihood only): well-scaled launches compute positions
1 .. F - 2 as one Kalman chain per lane (xt_r2_chain) and step F - 1 without the merge of the dead member; buckets too short to fill the
window end the chain with the lanes of still-dummy digits at zero weight.  Run on CPU threads (tests/emul, XT_EMUL_REG2=1) against the
numpy oracle: every length around the window size, the stay-in-FOV table switching inside the warm-up, per-peak errors, NaN tracks and
a model outside the well-scaled bounds (which keeps the fully guarded steps)."""
import os
import shutil
import sys

import numpy as np
import pytest

from oracle import oracle_np as O

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

DS, FS, TM = np.array([0.004, 0.1]), np.array([.35, .65]), np.array([[.92, .08], [.15, .85]])


def _emul(monkeypatch):
    monkeypatch.delenv("XT_EMUL_GENERIC", raising=False)
    monkeypatch.delenv("XT_EMUL_GUARDED", raising=False)
    monkeypatch.setenv("XT_EMUL_REG2", "1")
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emul"))
    import run_emul as E
    return E


def _check(E, Cs, LE, T, isBL, F, min_len, nblocks=1, ok=None):
    ps = O.p_stay_table(DS, 2, 1, [1.0])
    ref = O.proba_cs(Cs, LE, DS, FS, T, 0.1, isBL, [1.0], 1, F, min_len)
    ll, _, tot, info = E.run(Cs, LE, DS, FS, T, 0.1, isBL, ps, 1, F, min_len, nblocks=nblocks)
    assert info[1] == 256
    ok = np.isfinite(ref) if ok is None else ok
    assert (np.abs(ll[ok] - ref[ok]) < 1e-10).all(), (F, Cs.shape, np.abs(ll - ref).max())
    assert np.array_equal(np.isnan(ll), np.isnan(ref))
    if ok.all():
        assert abs(tot - ref.sum()) < 1e-9
    return ll


@pytest.mark.parametrize("F", [4, 5, 6, 7])
@pytest.mark.parametrize("isBL", [0, 1])
def test_warmup_every_length_around_the_window(F, isBL, monkeypatch):
    """Lengths 2 .. F + 3 (the window fills at L = F + 1) and 33 (two staging chunks); min_len 2 puts the stay-in-FOV table at step 2,
    inside the warm-up, min_len 3 one step later.  N = 64 / 2^(F-1) * 2 + 1: a partial last batch."""
    E = _emul(monkeypatch)
    rng = np.random.default_rng(F * 10 + isBL)
    N = (64 >> (F - 1)) * 2 + 1
    for min_len in (2, 3):
        for L in list(range(2, F + 4)) + [33]:
            Cs = np.cumsum(rng.normal(0, 0.08, (N, L, 2)), 1)
            _check(E, Cs, np.array([[[0.02]]]), TM, isBL, F, min_len, nblocks=2)


@pytest.mark.parametrize("F,D,K", [(4, 2, 1), (6, 2, 1), (6, 2, 2), (7, 1, 1), (5, 3, 3)])
def test_warmup_per_peak_errors(F, D, K, monkeypatch):
    """Per-peak localisation errors (one or per-dimension sigmas per position) through the chain and the merge-free first step."""
    E = _emul(monkeypatch)
    rng = np.random.default_rng(F * 100 + D * 10 + K)
    N = 13
    for L in (3, F, F + 1, F + 2, 33):
        Cs = np.cumsum(rng.normal(0, 0.08, (N, L, D)), 1)
        LE = rng.uniform(0.01, 0.04, (N, L, K))
        _check(E, Cs, LE, TM, 1, F, 3)


@pytest.mark.parametrize("F", [4, 6, 7])
def test_warmup_nan_track(F, monkeypatch):
    """A NaN position inside the warm-up and one after it: those tracks' likelihoods are NaN, the others exact."""
    E = _emul(monkeypatch)
    rng = np.random.default_rng(F)
    N, L = 9, F + 4
    Cs = np.cumsum(rng.normal(0, 0.08, (N, L, 2)), 1)
    Cs[2, 1, 0] = np.nan
    Cs[5, F + 1, 1] = np.nan
    ll = _check(E, Cs, np.array([[[0.02]]]), TM, 1, F, 3, ok=np.array([i not in (2, 5) for i in range(N)]))
    assert np.isnan(ll[2]) and np.isnan(ll[5])


@pytest.mark.parametrize("F", [4, 6, 7])
def test_not_well_scaled_model_takes_the_guarded_path(F, monkeypatch):
    """A transition probability of 1e-30 is outside the well-scaled bounds (>= 1e-20): the launch keeps the fully guarded steps, which
    must agree with the oracle at every length the warm-up covers."""
    E = _emul(monkeypatch)
    rng = np.random.default_rng(40 + F)
    T = np.array([[1.0 - 1e-30, 1e-30], [0.15, 0.85]])
    for L in (2, F - 1, F, F + 1, F + 3):
        Cs = np.cumsum(rng.normal(0, 0.08, (7, L, 2)), 1)
        _check(E, Cs, np.array([[[0.02]]]), T, 1, F, 2)
