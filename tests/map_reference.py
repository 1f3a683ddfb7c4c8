"""TEST INFRASTRUCTURE: numpy restatement of the windowed most-likely-state-path recursion that
``extrack_map_states`` / ``predict_states`` implement, written per track batch from the oracle's tables, and the brute-force exact MAP
sequence it is compared with.  Not a conftest; imported by tests/test_map_cpu.py, tests/test_emul_map.py and tests/test_hip_map.py.

Notation, tables, initialisation and the expand / integrate step are those of SURVEY.md Appendix A with nb_substeps = 1; digit c of a
sequence index i is (i // S**c) % S, c = 0 the newest.  Two places differ: the fuse of the oldest digit becomes a selection (argmax over
the oldest digit, lowest state on an exact tie, recorded as a back-pointer), and at the end the state after the last position (isBL) is
summed out before the final argmax (lowest index on a tie)."""
import numpy as np

from oracle import oracle_np as O

TIE_MARGIN = 1e-6   # tracks whose smallest best / runner-up gap is below this are left out of PATH comparisons (their score is compared)
TIE_SHARE = 0.01    # ... and may be at most this share of a case


def _top2_gap(x, axis):
    """best - runner-up along ``axis`` (>= 0)."""
    s = np.sort(x, axis=axis)
    return np.take(s, -1, axis=axis) - np.take(s, -2, axis=axis)


def map_path(Cs, LocErr, ds, Fs, TrMat, pBL, isBL, cell_dims, frame_len, min_len):
    """Cs [N, L, D]; LocErr [1 | N, 1 | L, k] as the oracle takes it.  Returns (states int8 [N, L], score [N], margin [N]): the windowed
    most-likely path, the log joint density of track and path under this recursion, and the smallest gap between best and runner-up over
    every select of every group and the final argmax of the track."""
    Cs = np.asarray(Cs, float)
    N, L, D = Cs.shape
    ds, Fs, TrMat = np.asarray(ds, float), np.asarray(Fs, float), np.asarray(TrMat, float)
    S, F = TrMat.shape[0], int(frame_len)
    LocErr = np.asarray(LocErr, float)
    assert LocErr.ndim == 3 and LocErr.shape[1] in (1, L) and L >= 2 and F >= 2
    if LocErr.shape[1] == 1 and L != 1:
        l2 = lambda p: np.broadcast_to(LocErr[:, 0, :] ** 2, (N, LocErr.shape[2]))
    else:
        l2 = lambda p: np.broadcast_to(LocErr[:, p, :] ** 2, (N, LocErr.shape[2]))
    k = LocErr.shape[2]
    LTs, d2s = O.seq_tables(S, 1, ds, TrMat)
    pst = O.p_stay_table(ds, S, 1, cell_dims)
    Lpst = np.log(pst * (1 - pBL))
    bad = np.isnan(Cs).any(axis=(1, 2)) | np.isnan(np.broadcast_to(LocErr, (N,) + LocErr.shape[1:])).any(axis=(1, 2))

    def gauss_log(c, m, s2x):
        return np.sum(-0.5 * np.log(2 * np.pi * s2x) - (c - m) ** 2 / (2 * s2x), axis=2) if s2x.shape[2] == D else \
            D * -0.5 * np.log(2 * np.pi * s2x[:, :, 0]) - np.sum((c - m) ** 2 / (2 * s2x), axis=2)

    n = 2
    idx = np.arange(S ** n)
    LP = np.repeat((LTs[idx] + np.log(Fs[(idx // S) % S]))[None], N, axis=0)
    m = np.repeat(Cs[:, 0, None, :], S ** n, axis=1)
    s2 = l2(0)[:, None, :] + d2s[idx][None, :, None]
    back = []  # back[f][track, j]: the state selected by fuse f (the f-th fuse decides position f) for the S**F index j
    margin = np.full(N, np.inf)
    with np.errstate(invalid="ignore"):
        for t in range(2, L):
            p = t - 1
            n += 1
            idx = np.arange(S ** n)
            par, sm = idx // S, idx % S ** 2
            lp, c = l2(p)[:, None, :], Cs[:, p, None, :]
            mo, s2o = m[:, par], s2[:, par]
            den = lp + s2o
            LC = gauss_log(c, mo, den)
            m = (mo * lp + c * s2o) / den
            d2e = d2s[sm][None, :, None]
            s2 = (d2e * lp + d2e * s2o + lp * s2o) / den
            LP = LP[:, par] + LTs[sm][None] + LC
            if t >= min_len:
                LP = LP + Lpst[idx % S][None]
            if t < L - 1:
                while n > F:
                    LPr = LP.reshape(N, S, -1)
                    q = np.argmax(LPr, axis=1)  # first maximum = lowest state on an exact tie
                    margin = np.minimum(margin, _top2_gap(LPr, 1).min(axis=1))
                    LP = np.take_along_axis(LPr, q[:, None, :], 1)[:, 0]
                    m = np.take_along_axis(m.reshape(N, S, -1, D), q[:, None, :, None], 1)[:, 0]
                    s2 = np.take_along_axis(s2.reshape(N, S, -1, k), q[:, None, :, None], 1)[:, 0]
                    back.append(q)
                    n -= 1
        idx = np.arange(S ** n)
        sc = LP + gauss_log(Cs[:, L - 1, None, :], m, s2 + l2(L - 1)[:, None, :])
        if isBL:
            qq = pBL + (1 - pst) - pBL * (1 - pst)
            sc = sc + np.log(TrMat @ qq)[idx % S][None]
        best = np.argmax(sc, axis=1)
        score = sc[np.arange(N), best]
        margin = np.minimum(margin, _top2_gap(sc, 1))
    states = np.zeros((N, L), dtype=np.int8)
    for c in range(n):
        states[:, L - 1 - c] = (best // S ** c) % S
    j = best.copy()
    for f in range(len(back) - 1, -1, -1):
        j = j // S
        q = back[f][np.arange(N), j]
        states[:, f] = q
        j = q * S ** F + j
    assert len(back) == max(L - 1 - F, 0)
    states[bad] = -1
    score = np.where(bad, np.nan, score)
    return states, score, margin


def exact_map(Cs, LocErr, ds, Fs, TrMat, pBL, isBL, cell_dims, min_len):
    """Brute force over all S**L sequences of the unfused recursion (the oracle's sequence matrix with a window longer than the track);
    with isBL the newest digit (the state after the last position) is summed out first.  Returns (states, score, margin)."""
    Cs = np.asarray(Cs, float)
    N, L, _ = Cs.shape
    S = np.asarray(TrMat).shape[0]
    LP, _ = O.p_cs_inter_bound_stats(Cs, LocErr, ds, Fs, TrMat, pBL, isBL, cell_dims, 1, L + 2, 0, min_len)
    return map_from_matrix(LP, S, L, isBL)


def map_from_matrix(LP, S, L, isBL):
    """Exact MAP path from a full sequence matrix LP [N, S**(L + isBL)] in the reference's column order."""
    LP = np.asarray(LP, float)
    N = LP.shape[0]
    if isBL:
        LPr = LP.reshape(N, S ** L, S)
        mx = LPr.max(axis=2, keepdims=True)
        LP = np.log(np.exp(LPr - mx).sum(axis=2)) + mx[:, :, 0]
    assert LP.shape[1] == S ** L
    best = np.argmax(LP, axis=1)
    states = np.zeros((N, L), dtype=np.int8)
    for c in range(L):
        states[:, L - 1 - c] = (best // S ** c) % S
    return states, LP[np.arange(N), best], _top2_gap(LP, 1)


def sequence_score(states, Cs, LocErr, ds, Fs, TrMat, pBL, isBL, cell_dims, min_len):
    """Log joint density of each track and the GIVEN path under the unfused recursion (for windowed-vs-exact score comparisons)."""
    Cs = np.asarray(Cs, float)
    N, L, _ = Cs.shape
    S = np.asarray(TrMat).shape[0]
    LP, _ = O.p_cs_inter_bound_stats(Cs, LocErr, ds, Fs, TrMat, pBL, isBL, cell_dims, 1, L + 2, 0, min_len)
    if isBL:
        LPr = LP.reshape(N, S ** L, S)
        mx = LPr.max(axis=2, keepdims=True)
        LP = np.log(np.exp(LPr - mx).sum(axis=2)) + mx[:, :, 0]
    i = np.zeros(N, dtype=np.int64)
    for c in range(L):
        i += states[:, L - 1 - c].astype(np.int64) * S ** c
    return LP[np.arange(N), i]


def compare_paths(got_states, got_score, ref_states, ref_score, margin, score_tol, what=""):
    """The tie rule of every path comparison: tracks whose margin is below TIE_MARGIN are left out of the path comparison (at most
    TIE_SHARE of the case), every score is compared."""
    got_states, ref_states = np.asarray(got_states), np.asarray(ref_states)
    assert got_states.shape == ref_states.shape and got_states.dtype == np.int8, (what, got_states.shape, ref_states.shape, got_states.dtype)
    nan = np.isnan(ref_score)
    assert np.array_equal(np.isnan(got_score), nan), what
    keep = (margin >= TIE_MARGIN) | nan
    assert (~keep).sum() <= TIE_SHARE * len(keep), "%s: %d of %d tracks are near-ties: change the seed" % (what, (~keep).sum(), len(keep))
    wrong = np.nonzero((got_states[keep] != ref_states[keep]).any(axis=1))[0]
    assert len(wrong) == 0, "%s: %d of %d paths differ, first %s: got %s want %s" % (
        what, len(wrong), keep.sum(), wrong[:1], got_states[keep][wrong[:1]], ref_states[keep][wrong[:1]])
    err = np.abs(np.asarray(got_score)[~nan] - ref_score[~nan])
    assert err.size == 0 or err.max() <= score_tol, "%s: score differs by %.3e (tolerance %.1e)" % (what, err.max(), score_tol)
