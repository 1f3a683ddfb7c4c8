"""CPU checks of the fixed-state position refinement (no GPU): the argument contract of ``get_pos_PDF_fixedBs`` and
``refine_along_states`` (everything below is raised on the host before the library is touched), a hand-worked regression of the dense
oracle (tests/cond_reference.py), and its tie to the reference: on the fixtures taken from the reference's own sequence matrix
(tests/golden/map_cases.*) the score of a path minus that path's prior and end term is the oracle's ``logdens``."""
import json
import os

import numpy as np
import pytest

import cond_reference as R
from oracle import oracle_np as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _params():
    from extrack_amd.lmfit_compat import Parameters
    p = Parameters()
    for k, v in dict(D0=1e-3, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1).items():
        p.add(k, value=v)
    return p


def test_get_pos_PDF_fixedBs_argument_errors():
    import extrack_amd
    from extrack_amd import refined_localization as RL
    assert extrack_amd.get_pos_PDF_fixedBs is RL.get_pos_PDF_fixedBs and "get_pos_PDF_fixedBs" in RL.__all__
    Cs = np.random.default_rng(0).normal(size=(4, 6, 2))
    ds, Fs, T = [0.01, 0.1], [0.5, 0.5], [[0.9, 0.1], [0.1, 0.9]]
    Bs = np.zeros((4, 6), dtype=np.int8)
    with pytest.raises(ValueError):
        RL.get_pos_PDF_fixedBs(Cs[0], 0.02, ds, Fs, T, Bs)  # tracks are not [n, len, dims]
    with pytest.raises(ValueError):
        RL.get_pos_PDF_fixedBs(Cs[:, :1], 0.02, ds, Fs, T, Bs[:, :1])  # one position
    with pytest.raises(TypeError):
        RL.get_pos_PDF_fixedBs(Cs, 0.02, ds, Fs, T, Bs.astype(float))  # a float Bs
    with pytest.raises(ValueError):
        RL.get_pos_PDF_fixedBs(Cs, 0.02, ds, Fs, T, Bs[:, :5])
    with pytest.raises(ValueError):
        RL.get_pos_PDF_fixedBs(Cs, 0.02, ds, Fs, T, Bs[:, None, :].repeat(2, axis=1))  # [n, 2, len]
    with pytest.raises(ValueError):
        RL.get_pos_PDF_fixedBs(Cs, 0.02, ds, Fs, T, Bs + 2)  # state 2 of a 2-state model
    with pytest.raises(ValueError):
        RL.get_pos_PDF_fixedBs(Cs, [0.02, 0.03, 0.04], ds, Fs, T, Bs)  # three errors, two dimensions
    with pytest.raises(ValueError):
        RL.get_pos_PDF_fixedBs(Cs, np.full((4, 5, 1), 0.02), ds, Fs, T, Bs)  # per-peak errors of another length
    with pytest.raises(ValueError):
        RL.get_pos_PDF_fixedBs(Cs, 0.02, ds, Fs, np.eye(3), Bs)  # TrMat of another model


def test_refine_along_states_argument_errors():
    import extrack_amd
    from extrack_amd import refined_localization as RL
    assert extrack_amd.refine_along_states is RL.refine_along_states and "refine_along_states" in RL.__all__
    rng = np.random.default_rng(1)
    tracks = {"5": rng.normal(size=(3, 5, 2)), "7": rng.normal(size=(2, 7, 2))}
    st = {"5": np.zeros((3, 5), np.int8), "7": np.ones((2, 7), np.int8)}
    p = _params()
    with pytest.raises(TypeError):
        RL.refine_along_states(tracks, 0.02, [1.0, 2.0], states=st)
    with pytest.raises(NotImplementedError):
        RL.refine_along_states(tracks, {"5": np.full((3, 5), 0.02), "7": np.full((2, 7), 0.02)}, p, states=st)
    with pytest.raises(ValueError):
        RL.refine_along_states(tracks, 0.02, p, states={"5": st["5"]})  # a key is missing
    with pytest.raises(ValueError):
        RL.refine_along_states(tracks, 0.02, p, states=dict(st, **{"9": np.zeros((1, 9), np.int8)}))  # a key too many
    with pytest.raises(ValueError):
        RL.refine_along_states(tracks, 0.02, p, states=[st["5"], st["7"]])  # not a dict
    with pytest.raises(ValueError):
        RL.refine_along_states(tracks, 0.02, p, states=dict(st, **{"7": np.ones((3, 7), np.int8)}))  # rows do not match
    with pytest.raises(TypeError):
        RL.refine_along_states(tracks, 0.02, p, states=dict(st, **{"7": np.ones((2, 7))}))  # float states
    with pytest.raises(ValueError):
        RL.refine_along_states(tracks, 0.02, p, states=dict(st, **{"7": np.full((2, 7), 2, np.int8)}))  # state 2 of a 2-state model
    with pytest.raises(ValueError):
        RL.refine_along_states({"5": tracks["7"]}, 0.02, p, states={"5": st["7"]})  # key and length disagree
    with pytest.raises(ValueError):
        RL.refine_along_states(tracks, 0.02, p, states=st, input_LocErr={"5": np.full((3, 5, 1), 0.02)})  # no errors for a bucket
    with pytest.raises(ValueError):
        RL.refine_along_states(tracks, 0.02, p, input_LocErr={"5": np.full((3, 5, 1), 0.02), "7": np.full((2, 6, 1), 0.02)})  # another length
    with pytest.raises(ValueError):
        RL.refine_along_states(tracks, 0.02, p, states=st, input_LocErr={"5": np.full((3, 5, 3), 0.02), "7": np.full((2, 7, 3), 0.02)})
    four = {"5": rng.normal(size=(3, 5, 4))}
    with pytest.raises(ValueError):
        RL.refine_along_states(four, 0.02, p, states={"5": st["5"]})  # four dimensions
    with pytest.raises(ValueError):
        RL.refine_along_states(four, 0.02, p)  # ... also when the states are to be decoded first


def test_oracle_hand_worked_track():
    """L = 3, D = 1, c = (0, 1, 3), error variance 1, ds = (1, 3), path (0, 0, 1): q = (1, (1 + 9) / 2) = (1, 5).
    Precision  diag(1, 1, 1) + [[1, -1, 0], [-1, 1.2, -.2], [0, -.2, .2]] = [[2, -1, 0], [-1, 2.2, -.2], [0, -.2, 1.2]],  determinant 4;
    its inverse has the diagonal (2.6, 2.4, 3.4) / 4 = (13, 12, 17) / 20, and times c it gives mu = (9, 18, 53) / 20.
    The same by the recursion: f = (0, 2/3, 53/20), a = (1, 2/3, 17/20); J1 = (2/3) / (17/3) = 2/17: mu1 = 2/3 + (2/17)(53/20 - 2/3) = 9/10,
    v1 = 2/3 + (4/289)(17/20 - 17/3) = 3/5; J0 = 1/2: mu0 = 9/20, v0 = 1 + (3/5 - 2) / 4 = 13/20.
    Displacements y = (1, 2) with covariance [[1 + 2, -1], [-1, 5 + 2]] (determinant 20, inverse [[7, 1], [1, 3]] / 20):
    logdens = -log(2 pi) - log(20) / 2 - (7 + 2 + 2 + 12) / 40."""
    Cs = np.array([[[0.0], [1.0], [3.0]]])
    st = np.array([[0, 0, 1]], dtype=np.int8)
    ds = np.array([1.0, 3.0])
    assert np.array_equal(R.step_variances(st, ds), [[1.0, 5.0]])
    mu, sg, ld = R.refine(Cs, st, ds, le=[1.0])
    assert np.abs(mu[0, :, 0] - np.array([9, 18, 53]) / 20).max() < 4e-15
    assert np.abs(sg[0, :, 0] ** 2 - np.array([13, 12, 17]) / 20).max() < 1e-15
    assert abs(ld[0] - (-np.log(2 * np.pi) - 0.5 * np.log(20) - 23 / 40)) < 1e-14
    # one error per dimension: the dimensions do not talk to each other
    C2 = np.concatenate([Cs, 2 * Cs], axis=2)
    mu2, sg2, ld2 = R.refine(C2, st, ds, le=[1.0, 2.0])
    mub, sgb, ldb = R.refine(2 * Cs, st, ds, le=[2.0])
    assert np.array_equal(mu2[:, :, 0], mu[:, :, 0]) and np.array_equal(mu2[:, :, 1], mub[:, :, 0])
    assert np.array_equal(sg2[:, :, 0], sg[:, :, 0]) and np.array_equal(sg2[:, :, 1], sgb[:, :, 0]) and abs(ld2[0] - ld[0] - ldb[0]) < 1e-14
    # special rows
    mu3, sg3, ld3 = R.refine(np.repeat(Cs, 2, axis=0), np.array([[0, -1, 1], [0, 0, 1]], dtype=np.int8), ds, le=[1.0])
    assert np.isnan(mu3[0]).all() and np.isnan(sg3[0]).all() and np.isnan(ld3[0]) and np.array_equal(mu3[1], mu[0]) and ld3[1] == ld[0]


def test_oracle_ties_to_reference_fixtures():
    """The fixtures hold, per track, the exact MAP path of the reference's own sequence matrix and its log joint density.  That density
    is  log Fs[b0] + sum log TrMat[b[t-1]][b[t]] + (stay terms from step max(min_len, 2) on) + (isBL: the summed-out end term)  plus the
    log density of the displacements given the path - the oracle's ``logdens``.  Prior and end term from the tables tests/map_reference.py
    builds (oracle_np.seq_tables / p_stay_table)."""
    with open(os.path.join(GOLDEN, "map_cases.json")) as f:
        meta = json.load(f)
    data = np.load(os.path.join(GOLDEN, "map_cases.npz"))
    worst, n = 0.0, 0
    for c in meta:
        p = "m%04d_" % c["id"]
        Cs, LE, ds, Fs, T = (data[p + k] for k in ("Cs", "LE", "ds", "Fs", "T"))
        path, logp = data[p + "path"], data[p + "logp"]
        N, L, D = Cs.shape
        S = len(ds)
        ok = ~np.isnan(logp)
        LTs, d2s = O.seq_tables(S, 1, ds, T)
        pst = O.p_stay_table(ds, S, 1, c["cell_dims"])
        Lpst = np.log(pst * (1 - c["pBL"]))
        b = path.astype(np.int64)
        prior = np.log(Fs[b[:, 0]])
        for t in range(1, L):
            prior = prior + LTs[b[:, t - 1] * S + b[:, t]]
            if t >= max(c["min_len"], 2):
                prior = prior + Lpst[b[:, t]]
        if c["isBL"]:
            qq = c["pBL"] + (1 - pst) - c["pBL"] * (1 - pst)
            prior = prior + np.log(T @ qq)[b[:, L - 1]]
        assert np.allclose(d2s[b[:, 0] * S + b[:, 1]], R.step_variances(path, ds)[:, 0], rtol=1e-15, atol=0)
        sig = np.broadcast_to(LE, (N, L, LE.shape[2]))
        _, _, ld = R.refine(Cs[ok], path[ok], ds, sigma=sig[ok])
        worst = max(worst, np.abs(logp[ok] - prior[ok] - ld).max())
        n += int(ok.sum())
    print("[cond] %d fixture tracks: |score - prior - logdens| <= %.2e" % (n, worst))
    assert n > 1000 and worst <= 1e-10
