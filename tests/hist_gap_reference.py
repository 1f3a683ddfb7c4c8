"""TEST INFRASTRUCTURE: the references of the state-duration histograms with missed detections.  Not a conftest;
imported by tests/test_hist_gaps_cpu.py, tests/test_emul_hist_gaps.py and tests/test_hip_hist_gaps.py.

(a) ``limit_reference``: the UNCHANGED numpy oracle (``oracle_hist.p_segment_len``) called with per-peak errors, LAMBDA at the gap rows, and
    the gap rows filled with the last observed position.  A missed detection is the limit of an infinite error at its row; the factor
    (2 pi LAMBDA^2)^(-D/2) every gap row contributes is the same for every sequence of a track and leaves through the per-track
    normalisation, so nothing is taken out.  Each gap costs about 17 D in the oracle's log weights, whose ``exp`` underflows near -745 and
    then ties: at most 4 gaps per track and len <= 30 (a condition on the inputs).
(b) ``p_segment_len_gaps``: a direct restatement of the gap rule - ``oracle_hist.p_segment_len`` operation for operation, with, at a gap
    position, no Gaussian factor, the mean unchanged, the variance carried unreduced, and the predictive density of a missed next position
    dropped from the ranking.  It ranks by the log-probability itself with a stable sort (ties by candidate index), as the kernel does; the
    oracle ranks exp(log-probability), which is the same order until values underflow.

Ties: inside a run of two or more consecutive missed frames distinct histories tie exactly in real arithmetic (the gap states (0, 1) and
(1, 0) between equal end states have the same transition product and the same variance).  Without pruning every sequence is kept and the
order does not matter; with pruning rounding decides it and, through the last-K quirk of the LL terms, shows in the result.  So two
implementations are compared on pruned cases with ISOLATED gaps only, and on runs of gaps only unpruned (max_nb_states >= S^(len - 1))."""
import numpy as np

from gap_reference import fill_gaps, gap_rows
from oracle import oracle_hist as OH
from oracle.oracle_np import p_stay_table

LAMBDA = 1e7
SLOPE_OFFSET = (1.3, 0.004)


def limit_reference(Cs, LocErr, ds, Fs, TrMat, min_l=3, pBL=0.1, isBL=1, cell_dims=(0.5,), max_nb_states=1000, lam=LAMBDA):
    """(a).  Cs [N, L, D] with all-NaN rows; LocErr [1 | N, 1 | L, k] effective errors, entries at gap rows ignored (NaN allowed)."""
    Cs = np.asarray(Cs, float)
    N, L, D = Cs.shape
    gap, bad = gap_rows(Cs)
    assert not bad.any()
    LE = np.array(np.broadcast_to(np.asarray(LocErr, float), (N, L, np.shape(LocErr)[2])), dtype=float, copy=True)
    LE[gap] = lam
    return OH.p_segment_len(fill_gaps(Cs, gap), LE, ds, Fs, TrMat, min_l, pBL, isBL, cell_dims, 1, max_nb_states)


def p_segment_len_gaps(Cs, LocErr, ds, Fs, TrMat, min_l=3, pBL=0.1, isBL=1, cell_dims=(0.5,), max_nb_states=1000):
    """(b).  Arguments as ``limit_reference``.  Returns seg_len_hist[L - 1, S]; all NaN when a track breaks a gap rule (NaN first / last
    row, a row with some NaN coordinates, a NaN error at an observed row), as through the C ABI."""
    Cs = np.asarray(Cs, float)
    N, L, D = Cs.shape
    assert L >= 2
    ds, Fs, TrMat = np.asarray(ds, float), np.asarray(Fs, float), np.asarray(TrMat, float)
    S = len(ds)
    LocErr = np.asarray(LocErr, float)
    assert LocErr.ndim == 3 and LocErr.shape[1] in (1, L)
    kd = LocErr.shape[2]
    gap, bad = gap_rows(Cs)
    LEb = np.broadcast_to(LocErr, (N, L, kd))
    bad = bad | (np.isnan(LEb).any(axis=2) & ~gap).any(axis=1)
    if bad.any():
        return np.full((L - 1, S), np.nan)
    l2 = (lambda p: np.broadcast_to(LocErr[:, 0, :] ** 2, (N, kd))) if LocErr.shape[1] == 1 else (lambda p: np.broadcast_to(LocErr[:, p, :] ** 2, (N, kd)))
    cell_dims = [c for c in cell_dims if c is not None]
    K = int(max_nb_states)
    logT = np.log(TrMat)
    ds2 = ds ** 2
    pst = p_stay_table(ds, S, 1, cell_dims)
    Lpst = np.log(pst * (1 - pBL))

    def gauss(c, m, v):  # the oracle's two forms: one variance for all dims, or one per dim
        if kd == 1:
            return D * -0.5 * np.log(2 * np.pi * v[:, :, 0]) - np.sum((c - m) ** 2 / (2 * v), 2)
        return np.sum(-0.5 * np.log(2 * np.pi * v), 2) - np.sum((c - m) ** 2 / (2 * v), 2)

    i = np.arange(S * S)
    new, old = i % S, i // S
    LP = np.repeat((logT[old, new] + np.log(Fs[old]))[None], N, 0)
    LL = np.zeros((N, S * S)) + (Lpst[new][None] if 1 >= min_l else 0.0)
    m = np.repeat(Cs[:, 0, None, :], S * S, 1)
    s2 = np.broadcast_to(l2(0)[:, None, :] + ((ds2[new] + ds2[old]) / 2)[None, :, None], (N, S * S, kd)).copy()
    hist = np.stack([np.repeat(new[None], N, 0), np.repeat(old[None], N, 0)], -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(2, L):
            p = c - 1
            nB = LP.shape[1]
            r = np.tile(np.arange(S), nB)
            par = np.repeat(np.arange(nB), S)
            prev = hist[:, par, 0]
            gp = gap[:, p]
            lp = l2(p)[:, None, :]
            cp = Cs[:, p, None, :]
            mo, s2o = m[:, par], s2[:, par]
            den = lp + s2o
            LC = np.where(gp[:, None], 0.0, gauss(cp, mo, den))
            m = np.where(gp[:, None, None], mo, (mo * lp + cp * s2o) / den)
            d2 = ((ds2[r][None] + ds2[prev]) / 2)[:, :, None]
            s2 = d2 + np.where(gp[:, None, None], s2o, lp * s2o / den)  # the kernel's form: d2 + l2 s2 / den
            LP = LP[:, par] + logT[prev, r[None]] + LC
            LL = LL[:, par] + (Lpst[r][None] if c >= min_l else 0.0)
            hist = np.concatenate([np.broadcast_to(r[None, :, None], (N, nB * S, 1)), hist[:, par]], -1)
            if c < L - 1 and LP.shape[1] > K:
                gn = gap[:, p + 1]
                ns2 = s2 + l2(p + 1)[:, None, :]
                test = LP + np.where(gn[:, None], 0.0, gauss(Cs[:, p + 1, None, :], m, ns2))
                arg = np.argsort(-test, axis=1, kind="stable")  # descending by the log-probability, ties by candidate index
                m = np.take_along_axis(m, arg[:, :, None], 1)[:, :K]
                s2 = np.take_along_axis(s2, arg[:, :, None], 1)[:, :K]
                LP = np.take_along_axis(LP, arg, 1)[:, :K]
                LL = np.take_along_axis(LL, arg, 1)[:, -K:]  # reference quirk: the LAST K of the ranking
                hist = np.take_along_axis(hist, arg[:, :, None], 1)[:, :K]
    if isBL:
        qq = pBL + (1 - pst) - pBL * (1 - pst)
        LL = LL + np.log(qq[hist[:, :, 0]] + (S - 1) * qq[0])
    LP = LP + gauss(Cs[:, L - 1, None, :], m, s2 + l2(L - 1)[:, None, :])
    W = LP + LL
    P = np.exp(W - W.max(1, keepdims=True))
    P = P / P.sum(1, keepdims=True)
    out = np.zeros((L - 1, S))
    run_state = hist[:, :, 0].copy()
    run_len = np.ones(run_state.shape, int)
    for k in range(1, L):
        brk = hist[:, :, k] != run_state
        for s in range(S):
            sel = brk & (run_state == s)
            np.add.at(out[:, s], run_len[sel] - 1, P[sel])
        run_len = np.where(brk, 1, run_len + 1)
        run_state = hist[:, :, k]
    for s in range(S):
        sel = (run_state == s) & (run_len < L)
        np.add.at(out[:, s], run_len[sel] - 1, P[sel])
    return out


def len_hist_gaps(values, all_tracks, dt, cell_dims=(0.5, None, None), max_nb_states=500):
    """(b) driven bucket by bucket as ``oracle_hist.len_hist`` drives the oracle (keys are frame spans; global localisation error)."""
    from oracle.oracle_np import extract_params
    LocErr, ds, Fs, TrMat, pBL = extract_params(values, dt, 1, 1)
    keys = sorted((k for k in all_tracks if len(all_tracks[k])), key=int)
    out = np.zeros((int(keys[-1]), len(ds)))
    for bi, k in enumerate(keys):
        Css = np.asarray(all_tracks[k], float)
        for a in range(0, len(Css), 50):
            h = p_segment_len_gaps(Css[a:a + 50], LocErr, ds, Fs, TrMat, int(keys[0]), pBL, 0 if bi == len(keys) - 1 else 1, cell_dims, max_nb_states)
            out[:h.shape[0]] += h
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def random_model(S, seed):
    """Asymmetric rates (a model with symmetric rates ties in the ranking), diffusion lengths apart from each other."""
    rng = np.random.default_rng(seed)
    T = rng.uniform(0.03, 0.12, (S, S))
    T[np.arange(S), np.arange(S)] = 0
    T[np.arange(S), np.arange(S)] = 1 - T.sum(1)
    ds = np.linspace(0.01, 0.16, S) * rng.uniform(0.9, 1.1, S)
    Fs = rng.dirichlet(np.ones(S) * 3)
    return ds, Fs, T


def tracks(N, L, D, ds, Fs, T, rng, locerr=0.02):
    """Brownian tracks of the model with localisation noise, [N, L, D]."""
    S = len(ds)
    st = np.zeros((N, L), int)
    st[:, 0] = rng.choice(S, N, p=Fs)
    for t in range(1, L):
        u = rng.random(N)
        st[:, t] = (u[:, None] > np.cumsum(T[st[:, t - 1]], 1)).sum(1).clip(0, S - 1)
    steps = rng.normal(0, 1, (N, L, D)) * ds[st][:, :, None]
    return np.cumsum(steps, 1) + rng.normal(0, locerr, (N, L, D))


def isolated_mask(N, L, rng, share=0.25, max_gaps=None):
    """[N, L] bool: interior rows only, no two neighbours, at most ``max_gaps`` per track."""
    m = np.zeros((N, L), bool)
    for n in range(N):
        for p in rng.permutation(np.arange(1, L - 1)):
            if rng.random() < share and not m[n, p - 1] and not m[n, p + 1] and (max_gaps is None or m[n].sum() < max_gaps):
                m[n, p] = True
    return m


def error_layout(layout, kdim, N, L, mask, rng):
    """(LE as ``P_segment_len`` / the emulator take it, slope_offset or None, the effective errors [1 | N, 1 | L, k] for the references).
    Per-peak errors are NaN at the gap rows: never read."""
    if layout == "global":
        le = np.array([0.02, 0.03, 0.05][:kdim])[None, None]
        return le, None, le
    sg = rng.uniform(0.01, 0.05, (N, L, kdim))
    sg[mask] = np.nan
    if layout == "peak":
        return sg, None, sg
    return sg, SLOPE_OFFSET, np.maximum(sg * SLOPE_OFFSET[0] + SLOPE_OFFSET[1], 1e-6)


SHAPES = ("L2", "L3_mid", "L4", "gap_p1", "gap_Lm2", "gap_next_pruned", "adjacent_unpruned", "all_interior")
COMBOS = [(D, kdim, layout) for layout in ("global", "peak", "affine") for D, kdim in ((1, 1), (2, 1), (2, 2), (3, 1), (3, 3))]
UNPRUNED_L = {2: 7, 3: 6, 4: 5, 5: 5}  # S^(L - 1) = 64, 243, 256, 625 sequences: every one is kept


def shape_case(shape, S, D, kdim, layout, seed):
    """One bucket of the shared case set of the emulator and the GPU tests: dict(Cs, mask, LE, slope_offset, eff, ds, Fs, T, pBL, isBL,
    min_l, K, cell_dims, S, D, name).  Pruned cases hold isolated gaps only; runs of gaps come with K >= S^(L - 1)."""
    rng = np.random.default_rng(7000 + seed)
    ds, Fs, T = random_model(S, 100 + seed)
    if shape == "L2":
        L, N, K = 2, 3, 5
        mask = np.zeros((N, L), bool)
    elif shape == "L3_mid":  # the streamed final step alone, with and without its integration
        L, N, K = 3, 3, 4
        mask = np.zeros((N, L), bool)
        mask[0, 1] = mask[2, 1] = True
    elif shape == "L4":  # one pruned step (S^3 -> S^2): no gap, a gap at p = 1, a gap at L - 2 = p + 1 of the pruned step
        L, N, K = 4, 3, S * S
        mask = np.zeros((N, L), bool)
        mask[1, 1] = mask[2, 2] = True
    elif shape in ("gap_p1", "gap_Lm2", "gap_next_pruned"):
        L, N, K = 9, 4, 2 * S + 1
        mask = isolated_mask(N, L, rng)
        mask[0] = mask[1] = False
        if shape == "gap_p1":
            mask[0, 1] = True
        elif shape == "gap_Lm2":
            mask[0, L - 2] = True
        else:
            mask[0, 4] = mask[0, 6] = True  # steps p = 3 and p = 5 rank without the next position
    else:
        L, N, K = UNPRUNED_L[S], 2, S ** (UNPRUNED_L[S] - 1)
        mask = np.zeros((N, L), bool)
        if shape == "adjacent_unpruned":
            mask[0, 1:3] = True
            mask[1, 2:4] = True
        else:
            mask[0, 1:-1] = True
            mask[1, 1] = True
    Cs = tracks(N, L, D, ds, Fs, T, rng)
    Cs[mask] = np.nan
    LE, so, eff = error_layout(layout, kdim, N, L, mask, rng)
    return dict(name="%s S=%d D=%d k=%d %s" % (shape, S, D, kdim, layout), Cs=Cs, mask=mask, LE=LE, slope_offset=so, eff=eff, ds=ds, Fs=Fs, T=T,
                pBL=0.07, isBL=seed % 2, min_l=2 + seed % 2, K=K, cell_dims=[1.0], S=S, D=D)


def shared_cases():
    """32 buckets: every shape with every number of states 2 - 5; the 15 (D, K, error layout) variants at least twice each."""
    out = []
    for idx in range(32):
        D, kdim, layout = COMBOS[idx % 15]
        out.append(shape_case(SHAPES[idx % 8], 2 + (idx // 8 + idx) % 4, D, kdim, layout, idx))
    return out


def word_boundary_cases():
    """Histories that cross a 64-bit word: 2 states x 70 frames (1 bit per state), 3 states x 40 frames (2 bits); isolated gaps, small K."""
    out = []
    for S, L, K, seed in ((2, 70, 6, 50), (3, 40, 7, 51)):
        rng = np.random.default_rng(7000 + seed)
        ds, Fs, T = random_model(S, 100 + seed)
        mask = isolated_mask(2, L, rng)
        q = 63 if S == 2 else 31  # a missed frame whose digit sits at the word boundary
        mask[0, q - 1:q + 2] = [False, True, False]
        Cs = tracks(2, L, 2, ds, Fs, T, rng)
        Cs[mask] = np.nan
        LE, so, eff = error_layout("global", 1, 2, L, mask, rng)
        out.append(dict(name="word boundary S=%d L=%d" % (S, L), Cs=Cs, mask=mask, LE=LE, slope_offset=so, eff=eff, ds=ds, Fs=Fs, T=T, pBL=0.07, isBL=1,
                        min_l=3, K=K, cell_dims=[1.0], S=S, D=2))
    return out


def reference_of(case):
    """(b) of a case."""
    return p_segment_len_gaps(case["Cs"], case["eff"], case["ds"], case["Fs"], case["T"], case["min_l"], case["pBL"], case["isBL"], case["cell_dims"],
                              case["K"])
