"""GPU counterpart of tests/test_emul_r2_gform.py: the g-form steps of the register-resident 2-state likelihood kernel (csrc/xt_reg2.h,
launches with one global localisation variance l2 >= 1e-12 in a well-scaled model) through the C ABI, per-track LL against the numpy
oracle at 1e-10 - window sizes 4 / 6 / 7, 1 to 3 dimensions, both end terms, both positions of the stay-in-FOV switch, lengths F + 1 (the
merge-free first step only), F + 2 and 33 (two staging chunks) - plus localisation errors on either side of the eligibility bound and a
2000-track bucket of the benchmark's model against the C oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DS, FS, TM = np.array([0.004, 0.1]), np.array([.35, .65]), np.array([[.92, .08], [.15, .85]])


def _gpu_ll(Cs, le, ds, Fs, T, pBL, isBL, F, min_len):
    from extrack_amd import tracking as TR
    return TR.Proba_Cs(Cs, np.array([[[le]]]), ds, Fs, T, pBL, isBL, [1.0], 1, F, min_len)


@pytest.mark.parametrize("F", [4, 6, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("isBL", [0, 1])
def test_gform_against_the_oracle(F, D, isBL):
    from oracle import oracle_np as O
    rng = np.random.default_rng(F * 100 + D * 10 + isBL)
    N = 2 * (64 >> (F - 1)) * 4 + 1  # two workgroups of four waves and a partial batch
    for min_len in (2, 3):
        for L in (F + 1, F + 2, 33):
            Cs = np.cumsum(rng.normal(0, 0.08, (N, L, D)), 1)
            ref = O.proba_cs(Cs, np.array([[[0.02]]]), DS, FS, TM, 0.1, isBL, [1.0], 1, F, min_len)
            ll = _gpu_ll(Cs, 0.02, DS, FS, TM, 0.1, isBL, F, min_len)
            err = np.abs(ll - ref).max()
            print("F=%d D=%d isBL=%d min_len=%d L=%d: max |dLL| %.3e" % (F, D, isBL, min_len, L, err))
            assert err < 1e-10, (F, D, isBL, min_len, L, err)


@pytest.mark.parametrize("F,D", [(4, 2), (6, 3), (7, 1)])
@pytest.mark.parametrize("le", [0.0, 1e-7, 1e-5])
def test_gform_eligibility_bound(F, D, le):
    """Localisation errors 0 and 1e-7 (l2 < 1e-12: the general steps) and 1e-5 (g-form, with the exponential evaluated at positive
    arguments: T / l2^(D/2) up to 1e15) agree with the oracle alike."""
    from oracle import oracle_np as O
    rng = np.random.default_rng(F * 10 + D)
    N = 2 * (64 >> (F - 1)) * 4 + 1
    for L in (F + 2, 33):
        Cs = np.cumsum(rng.normal(0, 0.08, (N, L, D)), 1)
        ref = O.proba_cs(Cs, np.array([[[le]]]), DS, FS, TM, 0.1, 1, [1.0], 1, F, 3)
        ll = _gpu_ll(Cs, le, DS, FS, TM, 0.1, 1, F, 3)
        err = np.abs(ll - ref).max()
        print("F=%d D=%d le=%g L=%d: max |dLL| %.3e" % (F, D, le, L, err))
        assert err < 1e-10, (F, D, le, L, err)


def test_gform_bench_model_bucket():
    """2000 tracks x 30 positions of the benchmark's model (D = 0 / 0.25, dt = 0.02, localisation error 0.02, frame_len 6) against the C oracle."""
    from extrack_amd import synth
    from oracle import oracle_c, oracle_np as O
    Tm, Fs, ds = np.array([[.9, .1], [.1, .9]]), np.array([.6, .4]), np.sqrt(2 * np.array([0.0, 0.25]) * 0.02)
    Cs = synth.brownian_tracks(2000, 30, [0.0, 0.25], Tm, Fs, seed=5)
    ref, _ = oracle_c.run(Cs, np.array([[[0.02]]]), ds, Fs, Tm, 0.1, 0, O.p_stay_table(ds, 2, 1, [1.0]), 1, 6, 30)
    ll = _gpu_ll(Cs, 0.02, ds, Fs, Tm, 0.1, 0, 6, 30)
    err = np.abs(ll - ref).max()
    print("bench model 2000 x 30: max |dLL| %.3e, |sum| %.3e" % (err, abs(ll.sum() - ref.sum())))
    assert err < 1e-10, err
