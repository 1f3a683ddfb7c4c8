"""The batch edges of the likelihood-only register-resident 2-state body (extrack_amd/csrc/xt_reg2.h: xt_r2_body, NP == 0): a chunk of a
complete batch is staged from one wave-uniform base with all its loads in flight together (stage_ld / stage_st), the last batch of a bucket
by the loop with the track clamp; what a wave carries from one batch to the next (NaN flags, staged positions, accumulators); and the
read-out's sum of four terms of very different size.  Run on CPU threads against the numpy oracle with the rule of test_emul_r2_logcarry.py (_both): err < 1e-10, err <= 2 err_guarded + 1e-12,
and the launch took the g-form.  One block (nblocks=1), so that its four waves walk the batches 0 .. 3, 4 .. 7, ...: with TPW = 64 >> (F - 1)
tracks per wave-batch a block-batch is B = 4 TPW tracks."""
import os
import sys

import numpy as np
import pytest

import test_emul_r2_gform as G
from test_emul_r2_gform import GFORM, TM, _run, pytestmark  # noqa: F401
from test_emul_r2_logcarry import _both, _tracks

from oracle import oracle_np as O


def _tpw(F):
    return 64 >> (F - 1)


@pytest.mark.parametrize("F", [4, 6, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_batch_walk(F, D):
    """3 B + 1: every wave walks three complete batches, wave 0 a fourth that is partial (staged with the clamp);
    B - 1: one batch, partial in the last wave; TPW: one wave has work; 2 B + TPW + 1: waves with 3, 3, 2, 2 batches."""
    rng = np.random.default_rng(4000 + F * 10 + D)
    T, B = _tpw(F), 4 * _tpw(F)
    for le in (0.02, 1e-5):
        for N in (3 * B + 1, B - 1, T, 2 * B + T + 1):
            _both(_tracks(rng, N, F + 2, D), le, F, nblocks=1, what="walk N=%d" % N)


@pytest.mark.parametrize("L", [2, 3, 30, 32, 33, 34, 65])
def test_chunks_and_batches(L):
    """Tracks shorter than the window, one chunk exactly (its last delta is 0), and two and three chunks (a chunk's last delta reaches into
    the next chunk), over batches 0 .. 2 of wave 0."""
    F = 6
    rng = np.random.default_rng(5000 + L)
    _both(_tracks(rng, 2 * 4 * _tpw(F) + 1, L, 2), 0.02, F, nblocks=1, what="chunks L=%d" % L)


def test_batches_stay_in_their_bucket(monkeypatch):
    """Two buckets (L = 8 and L = 34) in ONE launch, one block each: the uniform base of a batch is formed from its own bucket's track array and
    length, and a wave's walk ends with its bucket.  The emulator's multi-bucket launcher (tests/emul/emul.cpp) runs the well-scaled steps, not
    the g-form: the staging is the same code, the staged values are positions instead of deltas.  Against the oracle, 1e-10 per track."""
    monkeypatch.setenv("XT_EMUL_REG2", "1")
    monkeypatch.delenv("XT_EMUL_GENERIC", raising=False)
    monkeypatch.delenv("XT_EMUL_GUARDED", raising=False)
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emul"))
    import run_emul as E
    F, N = 6, 2 * 4 * _tpw(6) + 1
    rng = np.random.default_rng(6000)
    buckets = [_tracks(rng, N, L, 2) for L in (8, 34)]
    ps = O.p_stay_table(G.DS, 2, 1, [1.0])
    ref = [O.proba_cs(b, np.array([[[0.02]]]), G.DS, G.FS, TM, 0.1, 0 if b.shape[1] == 34 else 1, [1.0], 1, F, 2) for b in buckets]
    outs, tot = E.run_multi(buckets, [0.02], G.DS, G.FS, TM, 0.1, ps, 1, F, 2, 34, [1, 1])
    for o, r in zip(outs, ref):
        err = np.abs(o - r).max()
        print("two buckets, L=%d: %.3e" % (34 if r is ref[1] else 8, err))
        assert err < 1e-10
    assert abs(tot - sum(r.sum() for r in ref)) < 1e-9


@pytest.mark.parametrize("F", [4, 6])
@pytest.mark.parametrize("where", ["first", "steady"])
def test_nan_in_a_later_batch(F, where):
    """A NaN in a track of wave 0's second batch, at position 0 and at position F + 2.  Exactly that track is NaN; the tracks of the same slot
    in wave 0's first and third batch are finite and within tolerance: the flag is set after the first batch has read its own, and is cleared
    for the third."""
    T = _tpw(F)
    N, L = 3 * 4 * T + 1, F + 5
    rng = np.random.default_rng(7000 + F)
    Cs = _tracks(rng, N, L, 2)
    slot = 1 if T > 1 else 0
    bad = 4 * T + slot  # wave 0 walks the batches 0, 4, 8, 12
    Cs[bad, 0 if where == "first" else F + 2, 1] = np.nan
    ok = np.arange(N) != bad
    ll, ref = _both(Cs, 0.02, F, ok=ok, nblocks=1, what="NaN %s" % where)
    assert np.isnan(ll[bad]) and np.isnan(ref[bad])
    assert np.isfinite(ll[ok]).all()
    for same_slot in (slot, 8 * T + slot):
        assert abs(ll[same_slot] - ref[same_slot]) < 1e-10


# Jumps of the last position by 2, 5 and 20: 100, 250 and 1e3 localisation errors (0.02), the shifts of test_logcarry_negligible_member.  The
# oracle's LL is finite for all of them (asserted below) and |LL| reaches 3.7e4.  Larger jumps leave the reach of the rule's absolute 1e-10: at
# 100 (|LL| 9.3e5, ulp 1.2e-10) the guarded steps and the g-form both sit 3.5e-10 from the oracle.
@pytest.mark.parametrize("jump", [2.0, 5.0, 20.0])
def test_readout_terms_of_very_different_size(jump):
    """The last position far from the track: the four (member, new state) terms of the read-out differ by hundreds to hundreds of thousands
    of binary orders, so the running sum is re-scaled to a new largest exponent (XtAcc::add) or a term vanishes against it."""
    le = 0.02
    rng = np.random.default_rng(8000 + int(jump))
    Cs = _tracks(rng, 9, 12, 2)
    Cs[:, -1] += jump
    ref = O.proba_cs(Cs, np.array([[[le]]]), G.DS, G.FS, TM, 0.1, 1, [1.0], 1, 6, 3)
    assert np.isfinite(ref).all(), ref
    _both(Cs, le, 6, nblocks=1, what="last jump %g" % jump)


def test_readout_with_a_zero_initial_fraction(monkeypatch):
    """One initial fraction is 0: on a track shorter than the window the sequences that start in that state reach the read-out with weight
    zero (terms that count for nothing in the sum's exponent).  Such a model is not well scaled, so the launch runs the guarded steps - the
    same read-out; against the oracle, 1e-10 per track."""
    monkeypatch.setattr(G, "FS", np.array([0.0, 1.0]))
    rng = np.random.default_rng(9000)
    for L in (3, 5, 12):
        Cs = _tracks(rng, 9, L, 2)
        ll, _, ref = _run(Cs, np.array([[[0.02]]]), TM, 1, 6, 3, G.GUARDED, nblocks=1)
        assert np.isfinite(ref).all()
        err = np.abs(ll - ref).max()
        print("F0 = 0, L=%d: %.3e" % (L, err))
        assert err < 1e-10
