"""GPU counterpart of tests/test_emul_r2_batch.py: the batch edges of the likelihood-only register-resident 2-state kernel (csrc/xt_reg2.h:
xt_r2_body, NP == 0) - complete batches staged from one wave-uniform base, the last batch of a bucket with the clamp, several batches per
wave - through tracking.Proba_Cs with _check of tests/test_hip_r2_ratio.py: per-track LL against the numpy oracle at 1e-10.  With
TPW = 64 >> (F - 1) tracks per wave-batch a workgroup takes B = 4 TPW tracks at a time.  The grid is the launcher's: the cases with 40 001
tracks assert from last_launch_info() that some wave walked three batches; their reference is the C oracle (the numpy one takes 4 - 27 s
on them; the two agree to 5e-14 per track)."""
import numpy as np
import pytest

from test_hip_r2_ratio import DS, FS, TM, TOL_LL, _check, _tracks

pytestmark = pytest.mark.gpu


def _tpw(F):
    return 64 >> (F - 1)


def _oracle_c(Cs, le, F, min_len=3):
    from oracle import oracle_c, oracle_np as O
    return oracle_c.run(Cs, np.array([[[le]]]), DS, FS, TM, 0.1, 1, O.p_stay_table(DS, 2, 1, [1.0]), 1, F, min_len, nthreads=8)[0]


def _trackset(Cs, le, F, min_len=3):
    from extrack_amd import tracking as TR
    ts, le_ = TR._one_bucket(Cs, np.array([[[le]]]), 1, min_len, 0)
    return ts, ts.make_model(le_, DS, FS, TM, 0.1, [1.0], 1, F)


@pytest.mark.parametrize("le", [0.02, 1e-5])
@pytest.mark.parametrize("F", [4, 6, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_batch_walk(F, D, le):
    """3 B + 1, B - 1, TPW and 2 B + TPW + 1 tracks of F + 2 positions: complete batches and a partial last one, waves without work."""
    rng = np.random.default_rng(4000 + F * 10 + D)
    T, B = _tpw(F), 4 * _tpw(F)
    for N in (3 * B + 1, B - 1, T, 2 * B + T + 1):
        _check(_tracks(rng, N, F + 2, D), le, F, "walk N=%d" % N)


@pytest.mark.parametrize("F", [6, 7])
def test_three_batches_per_wave(F):
    """40 001 tracks of F + 2 positions: more than three block-batches per workgroup of the launcher's grid, and a partial last batch."""
    N = 40001
    Cs = _tracks(np.random.default_rng(4200 + F), N, F + 2, 2)
    ref = _oracle_c(Cs, 0.02, F)
    ts, model = _trackset(Cs, 0.02, F)
    try:
        ll = ts.loglik(model, per_track=True)[1]
        info = ts.ctx.last_launch_info()
    finally:
        ts.close()
    print("F=%d: %d blocks of %d tracks at a time for %d tracks" % (F, info["blocks"], info["tracks_per_block"], N))
    assert -(-N // info["tracks_per_block"]) >= 3 * info["blocks"], info  # if not on this device: raise N
    err = np.abs(ll - ref).max()
    print("F=%d shape=%s: max |dLL| %.3e" % (F, Cs.shape, err))
    assert err < TOL_LL, (F, err)


def test_sum_only_launch():
    """TrackSet.loglik without per-track output - the launch of the headline benchmark, which Proba_Cs does not take - on 40 001 tracks of 30
    positions, frame_len 6: against the sum of the oracle's per-track values, relative 1e-12."""
    F, N = 6, 40001
    Cs = _tracks(np.random.default_rng(4300), N, 30, 2)
    ref = _oracle_c(Cs, 0.02, F).sum()
    ts, model = _trackset(Cs, 0.02, F)
    try:
        tot = ts.loglik(model)
    finally:
        ts.close()
    print("sum only: %.12f oracle %.12f rel %.3e" % (tot, ref, abs(tot - ref) / abs(ref)))
    assert abs(tot - ref) <= 1e-12 * abs(ref), (tot, ref)


@pytest.mark.parametrize("L", [33, 65])
def test_chunks_and_batches(L):
    """Two and three staging chunks per track over 2 B + 1 tracks."""
    F = 6
    _check(_tracks(np.random.default_rng(4400 + L), 2 * 4 * _tpw(F) + 1, L, 2), 0.02, F, "chunks")


@pytest.mark.parametrize("F", [4, 6])
@pytest.mark.parametrize("where", ["first", "steady"])
def test_nan_in_a_later_batch(F, where):
    """A NaN at position 0 or F + 2 of one track among 3 B + 1: exactly that track is NaN, the tracks one and two block-batches before and after
    it at the same place in the batch are finite and within tolerance."""
    T = _tpw(F)
    N, L = 3 * 4 * T + 1, F + 5
    Cs = _tracks(np.random.default_rng(4500 + F), N, L, 2)
    slot = 1 if T > 1 else 0
    bad = 4 * T + slot
    Cs[bad, 0 if where == "first" else F + 2, 1] = np.nan
    ok = np.arange(N) != bad
    ll, ref = _check(Cs, 0.02, F, "NaN %s" % where, ok=ok)
    assert np.isnan(ll[bad]) and np.isnan(ref[bad])
    assert np.isfinite(ll[ok]).all()
