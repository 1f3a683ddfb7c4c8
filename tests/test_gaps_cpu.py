"""CPU checks of the gap feature that need no GPU:
  * the reference construction (tests/gap_reference.py: the unchanged oracle with an error of 1e7 at the gap rows) against a brute-force sum
    over all S^L state paths - the dense Gaussian of the observed displacements with the missing rows deleted, times the path prior of
    tests/map_reference.py - for tracks of at most frame_len + 1 positions (no fusion: the recursion is exact there);
  * insert_gaps / drop_positions round trips and error cases;
  * the TrackSet(gaps=True) validation errors, which are raised before any device call."""
import itertools

import numpy as np
import pytest

import gap_reference as R
from extrack_amd import engine, gaps, synth
from oracle import oracle_np as O


def _brute_force(Cs, le, ds, Fs, T, pBL, isBL, cell_dims, min_len):
    """LL [N]: log sum over every state path of prior(path) * N(observed displacements | path).  Per dimension the observed rows y_t = c_t - c_0
    (t >= 1, observed) are jointly Gaussian with Cov(y_t, y_u) = sum_{j <= min(t, u)} d2_j + l2_0 + [t == u] l2_t, d2_j = (ds[b_{j-1}]^2 +
    ds[b_j]^2) / 2: the flat prior on the first real position leaves the density of the displacements.  le: [N, L, k] effective errors."""
    N, L, D = Cs.shape
    S = len(ds)
    pst = O.p_stay_table(ds, S, 1, cell_dims)
    lstay = np.log(pst * (1 - pBL))
    lend = np.log(T @ (pBL + (1 - pst) - pBL * (1 - pst)))
    out = np.full(N, -np.inf)
    gap, _ = R.gap_rows(Cs)
    for n in range(N):
        obs = np.nonzero(~gap[n])[0]
        assert obs[0] == 0 and obs[-1] == L - 1
        rows = obs[1:]
        terms = []
        for b in itertools.product(range(S), repeat=L):
            lp = np.log(Fs[b[0]]) + sum(np.log(T[b[t - 1], b[t]]) for t in range(1, L))
            lp += sum(lstay[b[t]] for t in range(max(min_len, 2), L))
            if isBL:
                lp += lend[b[-1]]
            cum = np.concatenate([[0.0], np.cumsum([(ds[b[t - 1]] ** 2 + ds[b[t]] ** 2) / 2 for t in range(1, L)])])
            for d in range(D):
                l2 = le[n, :, d if le.shape[2] > 1 else 0] ** 2
                cov = np.minimum.outer(cum[rows], cum[rows]) + l2[0] + np.diag(l2[rows])
                y = Cs[n, rows, d] - Cs[n, 0, d]
                sign, logdet = np.linalg.slogdet(cov)
                lp += -0.5 * (len(rows) * O.LOG2PI + logdet + y @ np.linalg.solve(cov, y))
            terms.append(lp)
        terms = np.array(terms)
        out[n] = np.log(np.exp(terms - terms.max()).sum()) + terms.max()
    return out


@pytest.mark.parametrize("S,L,D,k,isBL,min_len", [(2, 5, 2, 1, 1, 3), (2, 7, 1, 1, 0, 2), (3, 5, 2, 2, 1, 3), (3, 4, 3, 1, 0, 3), (2, 3, 2, 1, 1, 3),
                                                  (2, 2, 2, 1, 1, 3)])
def test_reference_equals_brute_force(S, L, D, k, isBL, min_len):
    Ds, Tm, Fs = R.MODELS[S]
    ds = np.sqrt(2 * Ds * R.DT)
    N = 6
    Cs = synth.brownian_tracks(N, L, list(Ds), Tm.tolist(), list(Fs), dt=R.DT, dims=D, seed=S * 10 + L)
    m = np.random.default_rng(L).random((N, L)) < 0.35
    m[0] = False          # a complete track
    m[1, 1:-1] = True     # every interior position missing
    m[:, 0] = m[:, -1] = False
    Cs[m] = np.nan
    le = np.random.default_rng(S).uniform(0.01, 0.05, (N, L, k))
    le[m] = np.nan        # never read
    ref, _ = R.loglik_and_preds(Cs, le, ds, Fs, Tm, R.PBL, isBL, R.CELL, L - 1 if L > 2 else 2, min_len)
    bf = _brute_force(Cs, le, ds, Fs, Tm, R.PBL, isBL, R.CELL, min_len)
    # the bias of the construction is ~1e-13 here (it falls as 1 / LAMBDA^2); the dense solve is good to ~1e-12 on these 1..6 x 1..6 systems
    np.testing.assert_allclose(ref, bf, rtol=0, atol=1e-10)
    # a gap-free track is the plain oracle
    plain = O.proba_cs(Cs[:1], le[:1], ds, Fs, Tm, R.PBL, isBL, R.CELL, 1, L - 1 if L > 2 else 2, min_len)
    assert abs(plain[0] - ref[0]) < 1e-12


def test_reference_poison_rules():
    Ds, Tm, Fs = R.MODELS[2]
    ds = np.sqrt(2 * Ds * R.DT)
    Cs = synth.brownian_tracks(5, 6, list(Ds), Tm.tolist(), list(Fs), dt=R.DT, dims=2, seed=1)
    Cs[0, 2] = np.nan
    Cs[1, 2, 0] = np.nan
    Cs[2, 0] = np.nan
    Cs[3, -1] = np.nan
    ll, pr = R.loglik_and_preds(Cs, np.array([[[0.02]]]), ds, Fs, Tm, R.PBL, 1, R.CELL, 4, 3, do_preds=True)
    assert np.array_equal(np.isnan(ll), [False, True, True, True, False])
    assert np.all(np.isfinite(pr[0])) and np.all(np.isnan(pr[1:4])) and np.all(np.isfinite(pr[4]))
    np.testing.assert_allclose(pr[0].sum(axis=1), 1.0, atol=1e-12)


def test_drop_positions():
    tr = synth.brownian_tracks(200, 9, [0.001, 0.25], [[.9, .1], [.1, .9]], [.6, .4], seed=2)
    dr = synth.drop_positions(tr, 0.25, seed=3)
    assert dr is not tr and not np.isnan(tr).any()
    gap, bad = R.gap_rows(dr)
    assert not bad.any() and not gap[:, 0].any() and not gap[:, -1].any()
    assert 0.15 < gap[:, 1:-1].mean() < 0.35
    assert np.array_equal(dr[~gap], tr[~gap])
    assert np.array_equal(synth.drop_positions(tr, 0.25, seed=3), dr, equal_nan=True)
    assert not np.isnan(synth.drop_positions(tr, 0.0, seed=3)).any()
    engine.check_gap_rows([dr])


def _compress(tracks):
    """Gapped buckets -> the readers' two dicts: rows of missed detections deleted, bucketed by the number of detections."""
    pos, fr = {}, {}
    for k, b in tracks.items():
        for n, tr in enumerate(b):
            keep = ~np.isnan(tr).all(axis=1)
            key = str(int(keep.sum()))
            pos.setdefault(key, []).append(tr[keep])
            fr.setdefault(key, []).append(np.nonzero(keep)[0] + 10 * n)
    return {k: np.array(v) for k, v in pos.items()}, {k: np.array(v) for k, v in fr.items()}


def test_insert_gaps_round_trip():
    full = {"9": synth.brownian_tracks(40, 9, [0.001, 0.25], [[.9, .1], [.1, .9]], [.6, .4], seed=4),
            "5": synth.brownian_tracks(30, 5, [0.001, 0.25], [[.9, .1], [.1, .9]], [.6, .4], seed=5)}
    gapped = {k: synth.drop_positions(v, 0.3, seed=int(k)) for k, v in full.items()}
    pos, fr = _compress(gapped)
    sig = {k: np.arange(v.shape[0] * v.shape[1], dtype=float).reshape(v.shape[0], v.shape[1], 1) + 1 for k, v in pos.items()}
    tracks, frames, errs, origin = gaps.insert_gaps(pos, fr, sig)
    assert sorted(tracks, key=int) == ["5", "9"] and errs is not None
    for k in tracks:
        assert tracks[k].shape == frames[k].shape + (2,) == errs[k].shape[:2] + (2,) and origin[k].shape == (len(tracks[k]), 2)
        engine.check_gap_rows([tracks[k]])
        assert np.all(np.diff(frames[k], axis=1) == 1)
        for row, (src_len, src_row) in zip(range(len(tracks[k])), origin[k]):
            src = pos[str(src_len)][src_row]
            got = tracks[k][row]
            obs = ~np.isnan(got).all(axis=1)
            assert np.array_equal(got[obs], src) and np.array_equal(frames[k][row][obs], fr[str(src_len)][src_row])
            assert np.array_equal(errs[k][row][obs], sig[str(src_len)][src_row]) and np.isnan(errs[k][row][~obs]).all()
        # the same set of tracks as before the compression (the order inside a bucket follows the source buckets)
        a = np.sort(np.nan_to_num(tracks[k], nan=-7.0).reshape(len(tracks[k]), -1), axis=0)
        b = np.sort(np.nan_to_num(gapped[k], nan=-7.0).reshape(len(gapped[k]), -1), axis=0)
        assert np.array_equal(a, b)
    assert gaps.insert_gaps(pos, fr)[2] is None
    # frames given as [n, len, 1]
    t2 = gaps.insert_gaps(pos, {k: v[:, :, None] for k, v in fr.items()})[0]
    assert all(np.array_equal(t2[k], tracks[k], equal_nan=True) for k in tracks)


def test_insert_gaps_max_gap_splits_and_drops():
    pos = {"6": np.arange(12, dtype=float).reshape(1, 6, 2)}
    fr = {"6": np.array([[3, 4, 8, 9, 10, 20]])}
    t, f, _, o = gaps.insert_gaps(pos, fr, max_gap=2)   # cuts after frame 4 (3 missing) and before frame 20; the single last row is dropped
    assert sorted(t) == ["2", "3"] and np.array_equal(f["2"], [[3, 4]]) and np.array_equal(f["3"], [[8, 9, 10]])
    assert np.array_equal(t["3"][0], pos["6"][0, 2:5]) and np.array_equal(o["3"], [[6, 0]]) and np.array_equal(o["2"], [[6, 0]])
    t, f, _, _ = gaps.insert_gaps(pos, fr, max_gap=3)
    assert sorted(t, key=int) == ["8"] and np.isnan(t["8"][0, 2:5]).all() and np.array_equal(t["8"][0, 5:], pos["6"][0, 2:5])
    t, f, _, _ = gaps.insert_gaps(pos, fr)
    assert list(t) == ["18"] and int(np.isnan(t["18"][0, :, 0]).sum()) == 12
    t, _, _, _ = gaps.insert_gaps(pos, fr, max_gap=0)
    assert sorted(t) == ["2", "3"]


@pytest.mark.parametrize("frames,word", [([[0, 1, 1, 2]], "repeated"), ([[0, 2, 1, 3]], "increase"), ([[0, 1.5, 2, 3]], "integers"),
                                         ([[0, np.nan, 2, 3]], "integers")])
def test_insert_gaps_rejects_bad_frames(frames, word):
    with pytest.raises(ValueError, match=word):
        gaps.insert_gaps({"4": np.zeros((1, 4, 2))}, {"4": np.array(frames, dtype=float)})


def test_insert_gaps_rejects_mismatched_inputs():
    with pytest.raises(ValueError):
        gaps.insert_gaps({"4": np.zeros((2, 4, 2))}, {"4": np.zeros((1, 4))})
    with pytest.raises(ValueError):
        gaps.insert_gaps({"4": np.zeros((1, 4, 2))}, {})
    with pytest.raises(ValueError):
        gaps.insert_gaps({"4": np.zeros((1, 4, 2))}, {"4": np.arange(4.0)[None]}, max_gap=-1)


@pytest.mark.parametrize("where,word", [((1, 0), "first and last"), ((2, -1), "first and last"), ((3, 2, 1), "all its coordinates")])
def test_trackset_gap_validation_raises_before_any_device_call(where, word, monkeypatch):
    from extrack_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the validation")
    monkeypatch.setattr(_lib, "Context", no_device)
    ok = synth.drop_positions(synth.brownian_tracks(5, 6, [0.001, 0.25], [[.9, .1], [.1, .9]], [.6, .4], seed=6), 0.3, seed=1)
    bad = ok.copy()
    bad[where] = np.nan
    with pytest.raises(ValueError, match=word) as e:
        engine.TrackSet([np.ones((3, 4, 2)), bad], gaps=True)
    assert "bucket 1" in str(e.value) and "track %d" % where[0] in str(e.value)
    with pytest.raises(AssertionError, match="device was touched"):  # valid data go on to the device
        engine.TrackSet([ok], gaps=True)


def test_gap_fits_refuse_what_is_not_built():
    from extrack_amd import tracking as T
    tr = {"6": synth.drop_positions(synth.brownian_tracks(5, 6, [0.001, 0.25], [[.9, .1], [.1, .9]], [.6, .4], seed=6), 0.3, seed=1)}
    for kw in (dict(gradient="analytic"), dict(uncertainties=True), dict(fusion="threshold"), dict(comm=object())):
        with pytest.raises(NotImplementedError):
            T.param_fitting(tr, 0.02, gaps=True, **kw)
