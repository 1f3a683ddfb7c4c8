"""TEST INFRASTRUCTURE: the reference of the pairwise state posteriors, built from the pieces of the numpy oracle
(oracle_np.seq_tables / p_stay_table / _fuse_oldest).  Not a conftest; imported by tests/test_pairs_cpu.py, tests/test_emul_pairs.py and
tests/test_hip_pairs.py.

``windowed`` walks the recursion of oracle_np.p_cs_inter_bound_stats (nb_substeps 1) and keeps, wherever the oracle sums its weight matrix P
down to the posterior of one digit, the sum over all but TWO neighbouring digits as well: trans[n, t, i, j] = P(state t = i, state t+1 = j |
track) from exactly the weights the posterior of position t is taken from.  It returns the posteriors too, so that the restatement can be held
against the unchanged oracle.  ``exact`` takes the pair posterior from the oracle's own final sequence matrix with nothing fused (frame_len
L + 2): independent of the restatement.  Missed detections go through the LAMBDA / fill_gaps device of tests/gap_reference.py."""
import numpy as np

import gap_reference as G
from oracle import oracle_np as O


def windowed(Cs, LocErr, ds, Fs, TrMat, pBL, isBL, cell_dims, frame_len, min_len):
    """Cs [N, L, D], LocErr [1 | N, 1 | L, k].  Returns (preds [N, L, S], trans [N, L-1, S, S])."""
    Cs = np.asarray(Cs, float)
    N, L, D = Cs.shape
    ds, Fs, TrMat, LocErr = np.asarray(ds, float), np.asarray(Fs, float), np.asarray(TrMat, float), np.asarray(LocErr, float)
    S, F = TrMat.shape[0], int(frame_len)
    l2 = (lambda p: LocErr[:, 0, :] ** 2) if LocErr.shape[1] == 1 else (lambda p: LocErr[:, p, :] ** 2)
    k = LocErr.shape[2]
    LTs, d2s = O.seq_tables(S, 1, ds, TrMat)
    pst = O.p_stay_table(ds, S, 1, cell_dims)
    Lpst = np.log(pst * (1 - pBL))
    preds = np.full((N, L, S), -1.0)
    trans = np.full((N, L - 1, S, S), -1.0)

    def gauss_log(c, m, s2x, half):
        return np.sum(-half * np.log(2 * np.pi * s2x) - (c - m) ** 2 / (2 * s2x), axis=2)

    n = 2
    idx = np.arange(S ** n)
    LP = np.repeat((LTs[idx] + np.log(Fs[(idx // S) % S]))[None], N, axis=0)
    m = np.repeat(Cs[:, 0, None, :], S ** n, axis=1)
    s2 = np.broadcast_to(l2(0)[:, None, :] + d2s[idx][None, :, None], (N, S ** n, k)).copy()
    for t in range(2, L):
        p = t - 1
        n += 1
        idx = np.arange(S ** n)
        par, sm = idx // S, idx % S ** 2
        lp, c = l2(p)[:, None, :], Cs[:, p, None, :]
        mo, s2o = m[:, par], s2[:, par]
        den = lp + s2o
        if k == 1:
            LC = D * -0.5 * np.log(2 * np.pi * den[:, :, 0]) - np.sum((c - mo) ** 2 / (2 * den), axis=2)
        else:
            LC = np.sum(-0.5 * np.log(2 * np.pi * den), 2) - np.sum((c - mo) ** 2 / (2 * den), axis=2)
        m = (mo * lp + c * s2o) / den
        d2e = d2s[sm][None, :, None]
        s2 = (d2e * lp + d2e * s2o + lp * s2o) / den
        LP = LP[:, par] + LTs[sm][None] + LC
        if t >= min_len:
            LP = LP + Lpst[idx % S][None]
        if t < L - 1:
            while n > F:
                tl = LP + gauss_log(Cs[:, p + 1, None, :], m, s2 + l2(p + 1)[:, None, :], 1.0)  # the reference's weighting, quirk included
                P = np.exp(tl - tl.max(axis=1, keepdims=True))
                tot = P.sum(axis=1)
                preds[:, t - F, :] = P.reshape(N, S, -1).sum(axis=2) / tot[:, None]
                trans[:, t - F] = P.reshape(N, S, S, -1).sum(axis=3) / tot[:, None, None]  # oldest digit, second-oldest digit
                LP, m, s2 = O._fuse_oldest(LP, m, s2, S)
                n -= 1
    if isBL:
        n += 1
        idx = np.arange(S ** n)
        par, sm = idx // S, idx % S ** 2
        end_p = pst[idx % S]
        LL = np.log(pBL + (1 - end_p) - pBL * (1 - end_p)) + LTs[sm]
        LP, m, s2 = LP[:, par], m[:, par], s2[:, par]
    else:
        idx = np.arange(S ** n)
        LL = 0.0
    LP = LP + gauss_log(Cs[:, L - 1, None, :], m, s2 + l2(L - 1)[:, None, :], 0.5) + LL
    pr, tr = _final_window(LP, S, n, int(isBL), L)
    for pos, v in pr.items():
        preds[:, pos] = v
    for pos, v in tr.items():
        trans[:, pos] = v
    assert not (preds == -1.0).any() and not (trans == -1.0).any()
    return preds, trans


def _final_window(LP, S, n, isBL, L):
    """Posteriors {position: [N, S]} and pairs {position: [N, S, S]} of the digit columns of the final matrix (the state after the last
    position, column 0 with isBL, is no position and forms no pair)."""
    P = np.exp(LP - LP.max(axis=1, keepdims=True))
    tot = P.sum(axis=1)
    idx = np.arange(S ** n)
    dig = [(idx // S ** col) % S for col in range(n)]
    pr, tr = {}, {}
    for col in range(isBL, n):
        pr[(L - 1) - (col - isBL)] = np.stack([P[:, dig[col] == s].sum(axis=1) / tot for s in range(S)], axis=1)
    for col in range(isBL, n - 1):
        v = np.empty((len(P), S, S))
        for i in range(S):
            for j in range(S):
                v[:, i, j] = P[:, (dig[col + 1] == i) & (dig[col] == j)].sum(axis=1) / tot
        tr[(L - 1) - (col + 1 - isBL)] = v
    return pr, tr


def exact(Cs, LocErr, ds, Fs, TrMat, pBL, isBL, cell_dims, min_len):
    """The exact pair posterior [N, L-1, S, S]: nothing fused (the oracle at frame_len L + 2, S^(L+1) <= 3e5 sequences with isBL)."""
    Cs = np.asarray(Cs, float)
    N, L, _ = Cs.shape
    S = np.asarray(TrMat).shape[0]
    assert S ** (L + 1) <= 3e5, "too many sequences for the unfused recursion"
    LP, _ = O.p_cs_inter_bound_stats(Cs, LocErr, ds, Fs, TrMat, pBL, isBL, cell_dims, 1, L + 2, 0, min_len)
    n = L + int(bool(isBL))
    assert LP.shape[1] == S ** n
    _, tr = _final_window(LP, S, n, int(bool(isBL)), L)
    return np.stack([tr[t] for t in range(L - 1)], axis=1)


def _gap_inputs(Cs, LocErr):
    Cs = np.asarray(Cs, float)
    N, L, _ = Cs.shape
    gap, bad = G.gap_rows(Cs)
    LE = np.array(np.broadcast_to(np.asarray(LocErr, float), (N, L, np.shape(LocErr)[2])), dtype=float, copy=True)
    LE[gap] = G.LAMBDA
    bad = bad | np.isnan(LE).any(axis=(1, 2))
    filled = G.fill_gaps(np.where(bad[:, None, None], 0.0, Cs), gap & ~bad[:, None])
    LE[bad] = 1.0
    return filled, LE, bad


def windowed_gaps(Cs, LocErr, ds, Fs, TrMat, pBL, isBL, cell_dims, frame_len, min_len):
    """``windowed`` for tracks with all-NaN rows (missed detections); LocErr is the EFFECTIVE error, its entries at gap rows are ignored.
    Tracks that break a gap rule are NaN."""
    filled, LE, bad = _gap_inputs(Cs, LocErr)
    preds, trans = windowed(filled, LE, ds, Fs, TrMat, pBL, isBL, cell_dims, frame_len, min_len)
    preds[bad] = np.nan
    trans[bad] = np.nan
    return preds, trans


def exact_gaps(Cs, LocErr, ds, Fs, TrMat, pBL, isBL, cell_dims, min_len):
    filled, LE, bad = _gap_inputs(Cs, LocErr)
    trans = exact(filled, LE, ds, Fs, TrMat, pBL, isBL, cell_dims, min_len)
    trans[bad] = np.nan
    return trans


def make_case(S, D, layout, F):
    """gap_reference.make_case plus one bucket of L = frame_len + 2 (exactly one pair leaves the window inside the loop), N = 11, 25 % of
    its interior rows missing and track 0 complete; buckets stay sorted short -> long."""
    from extrack_amd import synth
    case = G.make_case(S, D, layout, F)
    L, N = F + 2, 11
    assert all(b.shape[1] != L for b in case["buckets"])
    Ds, Tm, Fs = G.MODELS[S]
    rng = np.random.default_rng(4000 + 10 * S + F)
    m = rng.random((N, L)) < 0.25
    m[0] = False
    m[:, 0] = m[:, -1] = False
    tr = synth.brownian_tracks(N, L, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=G.DT, dims=D, seed=900 + 7 * S + F)
    tr[m] = np.nan
    at = sum(b.shape[1] < L for b in case["buckets"])
    case["buckets"].insert(at, tr)
    case["masks"].insert(at, m)
    if layout in ("global1", "globalD"):
        case["eff"].insert(at, case["eff"][0])
    elif layout == "peak":
        sg = rng.uniform(0.01, 0.05, (N, L, D))
        sg[m] = 123.0
        case["sig"].insert(at, sg)
        case["eff"].insert(at, sg)
    else:
        sg = rng.uniform(0.01, 0.05, (N, L, 1))
        sg[m] = np.nan
        case["sig"].insert(at, sg)
        case["eff"].insert(at, np.maximum(sg * G.SLOPE_OFFSET[0] + G.SLOPE_OFFSET[1], 1e-6))
    return case


_case_cache = {}


def case_reference(case, gaps=True, extra=None):
    """Per bucket of a gap_reference.make_case (upload order): (preds [N, L, S], trans [N, L-1, S, S]); min_len 3, the longest bucket does not
    end by leaving.  gaps = False: the same buckets with their gap rows filled in (``plain_buckets``).  Computed once per case and shared:
    callers must not write into the arrays."""
    key = (case["S"], case["D"], case["layout"], case["F"], bool(gaps))
    if key not in _case_cache:
        Ds, Tm, Fs = G.MODELS[case["S"]]
        ds = np.sqrt(2 * Ds * G.DT)
        bks = case["buckets"] if gaps else plain_buckets(case)
        Lmax = max(b.shape[1] for b in bks)
        _case_cache[key] = [windowed_gaps(b, eff, ds, Fs, Tm, G.PBL, int(b.shape[1] != Lmax), G.CELL, case["F"], G.MIN_LEN)
                            for b, eff in zip(bks, plain_eff(case) if not gaps else case["eff"])]
    return _case_cache[key]


def plain_buckets(case):
    """The buckets of a case without missed detections: every gap row replaced by the last observed position."""
    return [G.fill_gaps(b, m) for b, m in zip(case["buckets"], case["masks"])]


def plain_sigmas(case):
    """Their per-peak errors (None for the global layouts): the unread entries at former gap rows replaced by a usable value."""
    if case["sig"] is None:
        return None
    return [np.where(m[:, :, None], 0.03, s) for s, m in zip(case["sig"], case["masks"])]


def plain_eff(case):
    if case["sig"] is None:
        return case["eff"]
    if case["slope_offset"] is None:
        return plain_sigmas(case)
    return [np.maximum(s * case["slope_offset"][0] + case["slope_offset"][1], 1e-6) for s in plain_sigmas(case)]
