"""CPU checks behind the pairwise state posteriors, no GPU: the numpy restatement of tests/pair_reference.py against the
UNCHANGED oracle (first marginal at every t, second marginal inside the last window only, both at 1e-12) and against the exact pair posterior of
the unfused recursion for tracks of at most frame_len + 1 positions (1e-12); the same with missed detections against
gap_reference.loglik_and_preds; the pair launch's geometry function (csrc/xt_pair_geom.h, compiled for the host through tests/emul); and the
argument contract of predict_transitions."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))

import gap_reference as R
import pair_reference as PR
from oracle import oracle_np as O

TOL = 1e-12
_GRID = [(S, F, L, isBL) for S in (2, 3, 4) for F in (2, 3, 4, 6) for L in (2, 3, 4, 5, 7, 9, 14) for isBL in (0, 1)]


def _tracks(S, L, D=2, N=6, seed=0):
    from extrack_amd import synth
    Ds, Tm, Fs = R.MODELS[S]
    return synth.brownian_tracks(N, L, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=R.DT, dims=D, seed=seed + 31 * S + L)


def _model(S):
    Ds, Tm, Fs = R.MODELS[S]
    return np.sqrt(2 * Ds * R.DT), Fs, Tm


@pytest.mark.parametrize("S", (2, 3, 4))
def test_restatement_marginals_against_the_unchanged_oracle(S):
    ds, Fs, Tm = _model(S)
    le = np.array([[[0.02]]])
    worst1 = worst2 = 0.0
    for _, F, L, isBL in (g for g in _GRID if g[0] == S):
        Cs = _tracks(S, L)
        _, ref = O.p_cs_inter_bound_stats(Cs, le, ds, Fs, Tm, R.PBL, isBL, R.CELL, 1, F, 1, R.MIN_LEN)
        preds, trans = PR.windowed(Cs, le, ds, Fs, Tm, R.PBL, isBL, R.CELL, F, R.MIN_LEN)
        assert trans.shape == (len(Cs), L - 1, S, S) and np.all(trans >= 0)
        assert np.abs(preds - ref).max() <= TOL, (S, F, L, isBL)
        worst1 = max(worst1, np.abs(trans.sum(axis=3) - ref[:, :-1]).max())  # first marginal: every t
        t0 = max(L - 1 - F, 0)
        worst2 = max(worst2, np.abs(trans[:, t0:].sum(axis=2) - ref[:, t0 + 1:]).max())  # second marginal: the last window only
        assert np.abs(trans.sum(axis=(2, 3)) - 1).max() <= TOL
    assert worst1 <= TOL and worst2 <= TOL, (worst1, worst2)


def test_second_marginal_outside_the_last_window_is_a_different_lag():
    """Not a bug and not asserted elsewhere: before the last window the second marginal and the next position's posterior differ visibly."""
    ds, Fs, Tm = _model(2)
    le = np.array([[[0.02]]])
    Cs = _tracks(2, 14, N=40)
    preds, trans = PR.windowed(Cs, le, ds, Fs, Tm, R.PBL, 0, R.CELL, 2, R.MIN_LEN)
    assert np.abs(trans[:, :10].sum(axis=2) - preds[:, 1:11]).max() > 1e-3


@pytest.mark.parametrize("S", (2, 3, 4))
def test_restatement_is_exact_for_short_tracks(S):
    ds, Fs, Tm = _model(S)
    le = np.array([[[0.02, 0.03]]])
    n = 0
    for _, F, L, isBL in (g for g in _GRID if g[0] == S):
        if L > F + 1 or S ** (L + 1) > 3e5:
            continue
        Cs = _tracks(S, L, seed=5)
        _, trans = PR.windowed(Cs, le, ds, Fs, Tm, R.PBL, isBL, R.CELL, F, R.MIN_LEN)
        ex = PR.exact(Cs, le, ds, Fs, Tm, R.PBL, isBL, R.CELL, R.MIN_LEN)
        assert np.abs(trans - ex).max() <= TOL, (S, F, L, isBL)
        n += 1
    assert n >= 6


@pytest.mark.parametrize("S,F", [(2, 2), (2, 6), (3, 3), (4, 3)])
def test_restatement_with_gaps(S, F):
    """25 % missed rows: marginals against gap_reference.loglik_and_preds, and the exact pairs for the short buckets."""
    case = PR.make_case(S, 2, "peak", F)
    ds, Fs, Tm = _model(S)
    Lmax = max(b.shape[1] for b in case["buckets"])
    ref = PR.case_reference(case, gaps=True)
    assert any(m.any() for m in case["masks"])
    for b, eff, (preds, trans) in zip(case["buckets"], case["eff"], ref):
        L, isBL = b.shape[1], int(b.shape[1] != Lmax)
        _, pr = R.loglik_and_preds(b, eff, ds, Fs, Tm, R.PBL, isBL, R.CELL, F, R.MIN_LEN, do_preds=True)
        assert np.abs(preds - pr).max() <= TOL
        assert np.abs(trans.sum(axis=3) - pr[:, :-1]).max() <= TOL
        t0 = max(L - 1 - F, 0)
        assert np.abs(trans[:, t0:].sum(axis=2) - pr[:, t0 + 1:]).max() <= TOL
        if L <= F + 1 and S ** (L + 1) <= 3e5:
            assert np.abs(trans - PR.exact_gaps(b, eff, ds, Fs, Tm, R.PBL, isBL, R.CELL, R.MIN_LEN)).max() <= TOL


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
_DK = [(1, 1), (2, 1), (2, 2), (3, 1), (3, 3)]
GENERAL, GAPS, BIG = 4, 5, 6  # XtLlPath


@needs_gxx
def test_pair_geometry():
    import run_emul_pairs as E
    served = refused = wide = 0
    for S in range(2, 7):
        for NS in (1, 2):
            for F in range(NS + 1, 16):
                for D, K in _DK:
                    p = E.pair_pick(S, NS, F, D, K)
                    if p is None:
                        continue
                    NG = S ** (F - NS)
                    if NS != 1 or S > 4 or NG > 1024:
                        assert p["refusal"] in (1, 2, 3) and p["threads"] == 0, (S, NS, F, p)
                        refused += 1
                        continue
                    if p["refusal"]:
                        # the only refusal left: the state of one track with its pair accumulators exceeds the LDS of a CU
                        assert p["refusal"] == 4 and "LDS" in E.refusal_text(4), (S, F, D, K, p)
                        refused += 1
                        continue
                    served += 1
                    wide += p["wide"]
                    assert p["sel"] == S and p["tpb"] >= 1 and p["tpb"] * NG <= p["threads"] <= 1024 and p["threads"] % 64 == 0
                    assert p["lds"] <= 160 * 1024 and p["wide"] == (p["threads"] > 256)
                    assert p["tpb"] == 1 or (p["lds"] <= 64 * 1024 and p["tpb"] * NG <= 256)
                    # never less LDS than the posterior launch of the same body: at the same tracks per block exactly the larger
                    # accumulators more, and never more tracks per block than the posterior launch (with gaps: always this body) takes
                    grow = (2 + (F + 3) * S * S) - (2 * (S + 1) + (F + 1) * S + 2)
                    assert grow > 0 and p["lds"] - p["pred_lds_same_tpb"] == p["tpb"] * 8 * grow, (S, F, D, K, p)
                    if p["gap_path"] == GAPS:
                        assert p["tpb"] <= p["gap_tpb"] and p["threads"] <= p["gap_threads"], (S, F, D, K, p)
                        assert p["tpb"] < p["gap_tpb"] or p["lds"] > p["gap_lds"], (S, F, D, K, p)
    assert served >= 60 and refused >= 40 and wide >= 5
    # the 1024-thread case of the GPU test, and a refusal by LDS alone (4 states, frame_len 6, D 3: 1024 groups fit, the state does not)
    assert E.pair_pick(4, 1, 6, 2, 1)["threads"] == 1024
    assert E.pair_pick(3, 1, 8, 1, 1)["refusal"] == 3 and E.pair_pick(5, 1, 3, 2, 1)["refusal"] == 2 and E.pair_pick(2, 2, 4, 2, 1)["refusal"] == 1
    assert [bool(E.refusal_text(r)) for r in range(1, 6)] == [True] * 5


@needs_gxx
def test_ll_pick_is_not_consulted_differently():
    """xt_ll_pick keeps every result (tests/test_ll_geom_cpu.py runs unchanged against its recording) and knows nothing of pairs: wherever a
    pair launch is served, the posterior launch of the same point is served by the same workgroup body - "general", "gaps" with missed
    detections, never the global-state kernel or a refusal, since it needs less LDS - and where the pair launch is refused for its LDS alone
    the posterior launch may still fit."""
    import run_emul_pairs as E
    n = lds_only = 0
    for S in (2, 3, 4):
        for F in range(2, 11):
            for D, K in _DK:
                p = E.pair_pick(S, 1, F, D, K)
                if p is None:
                    continue
                if p["refusal"] == 0:
                    assert p["pred_path"] == GENERAL and p["gap_path"] == GAPS, (S, F, D, K, p)
                    n += 1
                elif p["refusal"] == 4:
                    lds_only += p["pred_path"] == GENERAL
    assert n >= 60 and lds_only >= 0


# ---- argument contract ------------------------------------------------------------------------------------------------------------------
def _params():
    from extrack_amd.lmfit_compat import Parameters
    p = Parameters()
    for k, v in dict(D0=1e-3, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1).items():
        p.add(k, value=v)
    return p


def test_predict_transitions_argument_contract():
    import extrack_amd
    from extrack_amd import tracking
    assert extrack_amd.predict_transitions is tracking.predict_transitions
    tr = {"5": _tracks(2, 5), "7": np.empty((0, 7, 2))}
    with pytest.raises(NotImplementedError, match="fusion='window'"):
        tracking.predict_transitions(tr, R.DT, _params(), fusion="threshold")
    with pytest.raises(NotImplementedError, match="fusion='window'"):
        tracking.predict_transitions(tr, R.DT, _params(), fusion="threshold", gaps=True)
    with pytest.raises(NotImplementedError, match="per-track time steps"):
        tracking.predict_transitions(tr, {"5": np.full((6, 5), R.DT)}, _params())
    with pytest.raises(NotImplementedError, match="comm=None"):
        tracking.predict_transitions(tr, R.DT, _params(), comm=object())
    with pytest.raises(ValueError, match="output"):
        tracking.predict_transitions(tr, R.DT, _params(), output="matrix")
    with pytest.raises(TypeError):
        tracking.predict_transitions(tr, R.DT, [1, 2, 3])
    # the gap rules are those of TrackSet(gaps=True): refused on the host, naming bucket and track, before any device call
    bad = {"5": _tracks(2, 5)}
    bad["5"][2, 0] = np.nan
    with pytest.raises(ValueError, match="track 2"):
        tracking.predict_transitions(bad, R.DT, _params(), gaps=True)
    # nothing to launch: correctly shaped empty arrays, no device needed
    pr, ct = tracking.predict_transitions({"4": np.empty((0, 4, 2)), "9": np.empty((0, 9, 2))}, R.DT, _params(), output="both")
    assert pr["4"].shape == (0, 3, 2, 2) and pr["9"].shape == (0, 8, 2, 2) and ct["4"].shape == (0, 2, 2) and set(pr) == {"4", "9"}


def test_transition_matrix_helper():
    from extrack_amd import tracking
    c = {"3": np.array([[[1.0, 1.0], [0.5, 1.5]], [[np.nan] * 2] * 2]), "5": np.array([[[2.0, 0.0], [0.5, 1.5]]]), "9": np.empty((0, 2, 2))}
    C, P = tracking.transition_matrix(c)
    assert np.array_equal(C, [[3.0, 1.0], [1.0, 3.0]]) and np.allclose(P, [[0.75, 0.25], [0.25, 0.75]])
    with pytest.raises(ValueError):
        tracking.transition_matrix({"9": np.empty((0, 2, 2))})
