"""CPU checks of the fixed-state position refinement with missed detections (no GPU): a hand-worked regression of the dense oracle
(tests/cond_gap_reference.py), the rule of csrc/xt_cond.h restated in numpy against that oracle on every gap mask of the shared cases, the
oracle's tie to the decoder's restatement (score - prior = logdens on its own paths), and the argument contract of
``refine_along_states(gaps=True)``."""
import numpy as np
import pytest

import cond_gap_reference as CG
import cond_reference as R
import gap_reference as G
import map_gap_reference as MG


def test_oracle_hand_worked_track_with_a_missed_detection():
    """L = 3, D = 1, c = (0, -, 3) with the middle row missing, error variance 1, ds = (1, 3), path (0, 0, 1): q = (1, 5).
    The recursion: f0 = 0, a0 = 1; gap: p = 1 + 1 = 2, f1 = 0, a1 = 2; t = 2: p = 2 + 5 = 7, w = 8, g = 7/8, r = 3: f2 = 21/8, a2 = 7/8,
    logdens = -log(2 pi 8) / 2 - 9/16.  Backward: mu2 = 21/8, v2 = 7/8; J1 = 2/7: mu1 = (2/7)(21/8) = 3/4, v1 = 2 + (4/49)(7/8 - 7) = 3/2;
    J0 = 1/2: mu0 = 3/8, v0 = 1 + (3/2 - 2) / 4 = 7/8.
    The same without the recursion: r0 ~ N(0, 1) from c0, c2 = r0 + N(0, 6 + 1): the posterior precision of r0 is 1 + 1/7 = 8/7 and its
    mean (3/7) / (8/7) = 3/8; by symmetry r2 has variance 7/8 and mean 3 - 3/8 = 21/8; the one observed displacement 3 has variance
    1 + 6 + 1 = 8.  The gap's sigma^2 = 3/2 exceeds both neighbours' 7/8 and its mean lies between theirs."""
    Cs = np.array([[[0.0], [np.nan], [3.0]]])
    st = np.array([[0, 0, 1]], dtype=np.int8)
    ds = np.array([1.0, 3.0])
    mu, sg, ld = CG.refine(Cs, st, ds, le=[1.0])
    assert np.abs(mu[0, :, 0] - np.array([3, 6, 21]) / 8).max() < 4e-15
    assert np.abs(sg[0, :, 0] ** 2 - np.array([7, 12, 7]) / 8).max() < 4e-15
    assert abs(ld[0] - (-0.5 * np.log(2 * np.pi * 8) - 9 / 16)) < 1e-14
    # the error of the gap row is never looked at; a gap-free track is the plain oracle's
    mu2, sg2, ld2 = CG.refine(Cs, st, ds, sigma=np.array([[[1.0], [np.nan], [1.0]]]))
    assert np.array_equal(mu2, mu) and np.array_equal(sg2, sg) and ld2[0] == ld[0]
    full = np.array([[[0.0], [1.0], [3.0]]])
    a, b = CG.refine(full, st, ds, le=[1.0]), R.refine(full, st, ds, le=[1.0])
    assert np.abs(a[0] - b[0]).max() < 4e-15 and np.abs(a[1] - b[1]).max() < 4e-15 and abs(a[2][0] - b[2][0]) < 1e-14
    # special rows: a negative state at the gap row, a missing last row, a partly missing row (two dimensions)
    mu3, sg3, ld3 = CG.refine(np.repeat(Cs, 2, axis=0), np.array([[0, -1, 1], [0, 0, 1]], dtype=np.int8), ds, le=[1.0])
    assert np.isnan(mu3[0]).all() and np.isnan(sg3[0]).all() and np.isnan(ld3[0]) and np.array_equal(mu3[1], mu[0]) and ld3[1] == ld[0]
    assert np.isnan(CG.refine(np.array([[[0.0], [1.0], [np.nan]]]), st, ds, le=[1.0])[2][0])
    assert np.isnan(CG.refine(np.array([[[0.0, 0.0], [1.0, np.nan], [3.0, 1.0]]]), st, ds, le=[1.0])[2][0])


@pytest.mark.parametrize("S", [2, 3, 4])
def test_recursion_against_the_dense_oracle_on_every_mask(S):
    """The rule of the kernel (predict through a gap row, add nothing to the density) restated in numpy, against the dense solve, on the
    buckets of ``gap_reference.make_case(., ., ., 5)`` with random paths: D 1..3, the four error layouts (K = 1 and K = D)."""
    Ds = G.MODELS[S][0]
    ds = np.sqrt(2 * Ds * G.DT)
    rng = np.random.default_rng(5)
    worst = np.zeros(3)
    for D in (1, 2, 3):
        for lay in G.LAYOUTS:
            case = G.make_case(S, D, lay, 5)
            for b, eff, m in zip(case["buckets"], case["eff"], case["masks"]):
                st = rng.integers(0, S, b.shape[:2]).astype(np.int8)
                l2 = np.array(np.broadcast_to(eff, b.shape[:2] + (eff.shape[2],)), dtype=float) ** 2
                q = R.step_variances(st, ds)
                rmu, rsg, rld = CG.smooth(b, l2, q, m)
                mu, sg, ld = CG.recursion(b, l2, q, m)
                worst = np.maximum(worst, [np.abs(mu - rmu).max(), (np.abs(sg - rsg) / rsg).max(), np.abs(ld - rld).max()])
    print("[cond gaps] S=%d: recursion - dense oracle: mu %.2e, sigma rel. %.2e, logdens %.2e" % ((S,) + tuple(worst)))
    assert worst[0] <= CG.MU_ATOL and worst[1] <= CG.SIGMA_RTOL and worst[2] <= CG.LOGDENS_ATOL


@pytest.mark.parametrize("S,F", [(2, 3), (3, 5), (4, 3)])
def test_oracle_ties_to_the_decoder_restatement(S, F):
    """On the restatement's own paths: score - prior (initial fraction, transitions, stay and end terms) = the dense gap-aware logdens."""
    Ds, Tm, Fs = G.MODELS[S]
    ds = np.sqrt(2 * Ds * G.DT)
    worst, n = 0.0, 0
    for D in (1, 2, 3):
        for lay in G.LAYOUTS:
            case = G.make_case(S, D, lay, F)
            Lmax = max(b.shape[1] for b in case["buckets"])
            for b, eff in zip(case["buckets"], case["eff"]):
                isBL = int(b.shape[1] != Lmax)
                st, sc, _ = MG.map_path(b, eff, ds, Fs, Tm, G.PBL, isBL, G.CELL, F, G.MIN_LEN)
                ps = MG.path_score(st, b, eff, ds, Fs, Tm, G.PBL, isBL, G.CELL, G.MIN_LEN)
                worst = max(worst, np.abs(sc - ps).max())
                n += len(b)
    print("[cond gaps] S=%d F=%d, %d tracks: |score - prior - logdens| <= %.2e" % (S, F, n, worst))
    assert worst <= CG.LOGDENS_ATOL


def test_refine_along_states_gaps_argument_errors():
    """Raised on the host before a context exists (this test runs without a GPU)."""
    from extrack_amd import refined_localization as RL
    from extrack_amd.lmfit_compat import Parameters
    p = Parameters()
    for k, v in dict(D0=1e-3, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1).items():
        p.add(k, value=v)
    rng = np.random.default_rng(0)
    tracks = {"5": rng.normal(size=(3, 5, 2)), "7": rng.normal(size=(2, 7, 2))}
    st = {"5": np.zeros((3, 5), np.int8), "7": np.ones((2, 7), np.int8)}
    bad = {k: v.copy() for k, v in tracks.items()}
    bad["7"][1, -1] = np.nan  # a NaN last row
    with pytest.raises(ValueError, match=r"bucket 1 \(length 7\), track 1"):
        RL.refine_along_states(bad, 0.02, p, states=st, gaps=True)
    with pytest.raises(ValueError, match=r"bucket 1 \(length 7\), track 1"):
        RL.refine_along_states(bad, 0.02, p, gaps=True)  # ... also when the states are to be decoded first
    bad = {k: v.copy() for k, v in tracks.items()}
    bad["5"][0, 2, 0] = np.nan  # a partly-NaN row
    with pytest.raises(ValueError, match=r"bucket 0 \(length 5\), track 0"):
        RL.refine_along_states(bad, 0.02, p, states=st, gaps=True)
    with pytest.raises(NotImplementedError):
        RL.refine_along_states(tracks, {"5": np.full((3, 5), 0.02), "7": np.full((2, 7), 0.02)}, p, states=st, gaps=True)
