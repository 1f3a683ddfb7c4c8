"""CPU checks of the state-path decoder with missed detections (no GPU): the numpy restatement of the gap rule (tests/map_gap_reference.py)
against the UNCHANGED restatement ``map_reference.map_path`` on the infinite-error construction of tests/gap_reference.py (gap rows filled,
their error LAMBDA, the factor (2 pi LAMBDA^2)^(-D/2) per gap row taken out again), against brute force on the short buckets, and the
argument contract of ``predict_states(gaps=True)`` (everything raised on the host before the library is touched).

Inputs: ``gap_reference.make_case`` at its default seed 0 (seed 1 has a genuine near-tie on a gap-free track: do not use it)."""
import numpy as np
import pytest

import gap_reference as G
import map_gap_reference as MG
import map_reference as M
from oracle import oracle_np as O

SCORE_TOL = 1e-10  # the tolerance of tests/test_hip_map.py
_SF = [(S, F) for S in (2, 3, 4) for F in (3, 5)]
_DL = [(D, lay) for D in (1, 2, 3) for lay in G.LAYOUTS]


def _model(S):
    Ds, Tm, Fs = G.MODELS[S]
    return np.sqrt(2 * Ds * G.DT), Fs, Tm


def _construction(b, eff, lam):
    """(filled positions, errors [N, L, k] with ``lam`` at the gap rows, the per-track constant to add back)."""
    gap, bad = G.gap_rows(b)
    assert not bad.any()
    N, L, D = b.shape
    LE = np.array(np.broadcast_to(eff, (N, L, eff.shape[2])), dtype=float)
    LE[gap] = lam
    return G.fill_gaps(b, gap), LE, gap.sum(axis=1) * D * (0.5 * O.LOG2PI + np.log(lam))


def _buckets(case):
    Lmax = max(b.shape[1] for b in case["buckets"])
    for i, (b, eff, m) in enumerate(zip(case["buckets"], case["eff"], case["masks"])):
        yield i, b, eff, m, int(b.shape[1] != Lmax)


@pytest.mark.parametrize("S,F", _SF)
def test_restatement_against_the_infinite_error_construction(S, F):
    ds, Fs, Tm = _model(S)
    worst, worst_shift, most = 0.0, 0.0, 0
    for D, lay in _DL:
        case = G.make_case(S, D, lay, F)
        left = []
        for i, b, eff, m, isBL in _buckets(case):
            st, sc, mg = MG.map_path(b, eff, ds, Fs, Tm, G.PBL, isBL, G.CELL, F, G.MIN_LEN)
            assert np.all(np.isfinite(sc)) and not np.any(st < 0)
            filled, LE, const = _construction(b, eff, G.LAMBDA)
            rst, rsc, _ = M.map_path(filled, LE, ds, Fs, Tm, G.PBL, isBL, G.CELL, F, G.MIN_LEN)
            worst = max(worst, np.abs(sc - (rsc + const)).max())
            keep = mg >= M.TIE_MARGIN
            assert np.array_equal(st[keep], rst[keep]), (D, lay, i)
            left.append(~keep)
            f6, L6, c6 = _construction(b, eff, 1e6)
            _, rsc6, _ = M.map_path(f6, L6, ds, Fs, Tm, G.PBL, isBL, G.CELL, F, G.MIN_LEN)
            worst_shift = max(worst_shift, np.abs((rsc6 + c6) - (rsc + const)).max())
        MG.check_exclusions(left, case["masks"], what="S=%d F=%d D=%d %s" % (S, F, D, lay))
        most = max(most, sum(int(o.sum()) for o in left))
    print("[map gaps] S=%d F=%d: |restatement - construction| %.2e, LAMBDA 1e6 -> 1e7 moves the construction by %.2e, at most %d of 64 "
          "tracks left out" % (S, F, worst, worst_shift, most))
    assert worst <= SCORE_TOL
    assert worst_shift <= 1.2e-11


@pytest.mark.parametrize("S,F", [(2, 3), (3, 3), (4, 3), (2, 5), (3, 5)])
def test_restatement_against_brute_force_on_short_tracks(S, F):
    """L <= frame_len + 1: nothing is merged and the path is the exact maximiser over all S^L sequences (``exact_map`` on the construction)."""
    ds, Fs, Tm = _model(S)
    worst = 0.0
    for D, lay in _DL:
        case = G.make_case(S, D, lay, F)
        for i, b, eff, m, isBL in _buckets(case):
            if b.shape[1] > F + 1:
                continue
            st, sc, mg = MG.map_path(b, eff, ds, Fs, Tm, G.PBL, isBL, G.CELL, F, G.MIN_LEN)
            filled, LE, const = _construction(b, eff, G.LAMBDA)
            est, esc, emg = M.exact_map(filled, LE, ds, Fs, Tm, G.PBL, isBL, G.CELL, G.MIN_LEN)
            worst = max(worst, np.abs(sc - (esc + const)).max())
            keep = (mg >= M.TIE_MARGIN) & (emg >= M.TIE_MARGIN)
            assert np.array_equal(st[keep], est[keep]), (D, lay, i)
            assert np.all(MG.has_gap_run(m)[~keep])
    print("[map gaps] S=%d F=%d: |restatement - brute force| %.2e" % (S, F, worst))
    assert worst <= SCORE_TOL


@pytest.mark.parametrize("S,D,lay", [(2, 1, "global1"), (3, 2, "globalD"), (4, 3, "peak"), (2, 2, "affine")])
def test_gap_free_tracks_equal_the_plain_restatement(S, D, lay):
    from extrack_amd import synth
    ds, Fs, Tm = _model(S)
    Ds = G.MODELS[S][0]
    case = G.make_case(S, D, lay, 3)
    for i, b, eff, m, isBL in _buckets(case):
        full = synth.brownian_tracks(len(b), b.shape[1], list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=G.DT, dims=D, seed=90 + i)
        eff = np.where(np.isnan(eff) | (eff > 100), 0.03, eff)
        a = MG.map_path(full, eff, ds, Fs, Tm, G.PBL, isBL, G.CELL, 3, G.MIN_LEN)
        r = M.map_path(full, eff, ds, Fs, Tm, G.PBL, isBL, G.CELL, 3, G.MIN_LEN)
        assert all(np.array_equal(x, y) for x, y in zip(a, r))


def test_poison_rules_of_the_restatement():
    ds, Fs, Tm = _model(2)
    case = G.make_case(2, 2, "peak", 3)
    b, sg = case["buckets"][3].copy(), case["sig"][3].copy()
    clean = MG.map_path(b, sg, ds, Fs, Tm, G.PBL, 1, G.CELL, 3, G.MIN_LEN)
    b[6, 5, 1] = np.nan
    b[9, 0] = np.nan
    b[11, -1] = np.nan
    obs = np.nonzero(~case["masks"][3][12])[0]
    sg[12, obs[1], 0] = np.nan
    st, sc, _ = MG.map_path(b, sg, ds, Fs, Tm, G.PBL, 1, G.CELL, 3, G.MIN_LEN)
    bad = np.zeros(len(b), bool)
    bad[[6, 9, 11, 12]] = True
    assert np.all(st[bad] == -1) and np.all(np.isnan(sc[bad]))
    assert np.array_equal(st[~bad], clean[0][~bad]) and np.array_equal(sc[~bad], clean[1][~bad])


def _params():
    from extrack_amd.lmfit_compat import Parameters
    p = Parameters()
    for k, v in dict(D0=1e-3, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1).items():
        p.add(k, value=v)
    return p


def test_predict_states_gaps_argument_errors():
    """Raised on the host: the rules of ``TrackSet(gaps=True)`` name bucket and track before a context exists (this test runs without a GPU)."""
    from extrack_amd import tracking
    rng = np.random.default_rng(0)
    tracks = {"5": rng.normal(size=(3, 5, 2)), "7": rng.normal(size=(4, 7, 2))}
    p = _params()
    bad = {k: v.copy() for k, v in tracks.items()}
    bad["7"][2, 3, 1] = np.nan  # a partly-NaN row
    with pytest.raises(ValueError, match=r"bucket 1 \(length 7\), track 2"):
        tracking.predict_states(bad, 0.02, p, gaps=True)
    bad = {k: v.copy() for k, v in tracks.items()}
    bad["5"][1, 0] = np.nan  # a NaN first row
    with pytest.raises(ValueError, match=r"bucket 0 \(length 5\), track 1"):
        tracking.predict_states(bad, 0.02, p, gaps=True)
    ok = {k: v.copy() for k, v in tracks.items()}
    ok["7"][0, 2] = np.nan
    with pytest.raises(NotImplementedError):
        tracking.predict_states(ok, 0.02, p, gaps=True, fusion="threshold")
    with pytest.raises(NotImplementedError):
        tracking.predict_states(ok, {"5": np.full((3, 5), 0.02), "7": np.full((4, 7), 0.02)}, p, gaps=True)
