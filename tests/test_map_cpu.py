"""CPU checks of the most-likely-state-path feature (no GPU): the numpy restatement of the windowed recursion (tests/map_reference.py)
against the brute-force exact MAP sequence and against fixtures taken from the reference's own sequence matrix
(tests/golden/map_cases.*), the argument contract of ``predict_states``, and the measured agreement table of DESIGN.md section 16."""
import json
import os

import numpy as np
import pytest

import map_reference as R
from extrack_amd import synth
from oracle import oracle_np as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_DT, _PBL, _CELL, _LE = 0.02, 0.1, [1.0], np.array([[[0.02]]])
_MODELS = {
    2: (np.array([0.0005, 0.25]), np.array([[0.9, 0.1], [0.1, 0.9]]), np.array([0.5, 0.5])),
    3: (np.array([0.0005, 0.04, 0.25]), np.array([[0.8, 0.1, 0.1], [0.1, 0.8, 0.1], [0.1, 0.1, 0.8]]), np.array([1 / 3, 1 / 3, 1 / 3])),
}


def _tracks(S, L, N, seed):
    Ds, Tm, Fs = _MODELS[S]
    return synth.brownian_tracks(N, L, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=_DT, dims=2, seed=seed)


@pytest.mark.parametrize("isBL", [0, 1])
@pytest.mark.parametrize("F", [4, 6])
@pytest.mark.parametrize("S", [2, 3])
def test_restatement_is_exact_without_fuse(S, F, isBL):
    """L <= frame_len + 1: nothing is fused, the windowed path IS the exact MAP sequence, and its joint density is at most the track's
    likelihood (a single term of the sum)."""
    Ds, Tm, Fs = _MODELS[S]
    ds = np.sqrt(2 * Ds * _DT)
    for L in sorted(set([2, 3, 5, F, F + 1])):
        Cs = _tracks(S, L, 40, 100 * S + 10 * F + L)
        st, sc, mg = R.map_path(Cs, _LE, ds, Fs, Tm, _PBL, isBL, _CELL, F, 3)
        est, esc, emg = R.exact_map(Cs, _LE, ds, Fs, Tm, _PBL, isBL, _CELL, 3)
        R.compare_paths(st, sc, est, esc, np.minimum(mg, emg), 1e-12, "S=%d F=%d L=%d isBL=%d" % (S, F, L, isBL))
        ll = O.proba_cs(Cs, _LE, ds, Fs, Tm, _PBL, isBL, _CELL, 1, F, 3)
        assert np.all(sc <= ll + 1e-12 * np.abs(ll))


def test_restatement_matches_reference_fixtures():
    """The fixtures hold the argmax of the reference's own P_Cs_inter_bound_stats matrix (tests/golden/make_golden_map.py)."""
    with open(os.path.join(GOLDEN, "map_cases.json")) as f:
        meta = json.load(f)
    data = np.load(os.path.join(GOLDEN, "map_cases.npz"))
    assert len(meta) >= 150
    seen = set()
    for c in meta:
        p = "m%04d_" % c["id"]
        st, sc, mg = R.map_path(data[p + "Cs"], data[p + "LE"], data[p + "ds"], data[p + "Fs"], data[p + "T"], c["pBL"], c["isBL"], c["cell_dims"],
                                c["F"], c["min_len"])
        R.compare_paths(st, sc, data[p + "path"], data[p + "logp"], np.minimum(mg, data[p + "margin"]), 1e-12, "golden case %d" % c["id"])
        seen.add((c["S"], c["D"], c["le"], c["isBL"]))
    assert {s[0] for s in seen} == {2, 3, 4} and {s[1] for s in seen} == {1, 2, 3} and {s[2] for s in seen} == {"scalar", "dim", "peak"}


def test_predict_states_argument_errors():
    """Raised before any device call (this test runs without a GPU)."""
    import extrack_amd
    from extrack_amd import tracking
    from extrack_amd.lmfit_compat import Parameters
    assert extrack_amd.predict_states is tracking.predict_states
    p = Parameters()
    for k, v in dict(D0=1e-3, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1).items():
        p.add(k, value=v)
    tracks = {"5": _tracks(2, 5, 3, 1)}
    with pytest.raises(TypeError):
        tracking.predict_states(tracks, _DT, [1.0, 2.0])
    with pytest.raises(NotImplementedError):
        tracking.predict_states(tracks, _DT, p, fusion="threshold")
    with pytest.raises(NotImplementedError):
        tracking.predict_states(tracks, {"5": np.full((3, 5), _DT)}, p)
    with pytest.raises(ValueError):
        tracking.predict_states(tracks, _DT, p, fusion="nonsense")


@pytest.mark.parametrize("S,L", [(2, 12), (3, 9)])
def test_windowed_score_never_beats_exact(S, L, capsys):
    """The agreement table of DESIGN.md section 16 (printed, 400 tracks per row); asserted: the windowed path is one of the S^L sequences,
    so its joint density under the unfused recursion is at most the exact maximum."""
    Ds, Tm, Fs = _MODELS[S]
    ds = np.sqrt(2 * Ds * _DT)
    Cs = _tracks(S, L, 400, 3)
    est, esc, _ = R.exact_map(Cs, _LE, ds, Fs, Tm, _PBL, 0, _CELL, 3)
    rows = []
    for F in (2, 4, 6):
        st, sc, _ = R.map_path(Cs, _LE, ds, Fs, Tm, _PBL, 0, _CELL, F, 3)
        # the recursion carries the selected sequence's own mean and variance: its score is that sequence's exact joint density
        own = R.sequence_score(st, Cs, _LE, ds, Fs, Tm, _PBL, 0, _CELL, 3)
        assert np.abs(sc - own).max() <= 1e-12 * np.abs(own).max()
        assert np.all(sc <= esc + 1e-12)
        post = O.p_cs_inter_bound_stats(Cs, _LE, ds, Fs, Tm, _PBL, 0, _CELL, 1, F, 1, 3)[1]
        rows.append((F, 100.0 * (st == est).all(axis=1).mean(), 100.0 * (post.argmax(axis=2) == st).all(axis=1).mean()))
    with capsys.disabled():
        for F, a, b in rows:
            print("\n[map agreement] %d states, L %d, frame_len %d: windowed == exact MAP %.2f %%, argmax of posteriors == windowed %.2f %%"
                  % (S, L, F, a, b), end="")
