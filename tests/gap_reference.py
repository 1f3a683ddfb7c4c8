"""TEST INFRASTRUCTURE: the reference of the gap-aware likelihood / posteriors, built from the UNCHANGED numpy oracle.
Not a conftest; imported by tests/test_gaps_cpu.py, tests/test_emul_gap.py and tests/test_hip_gaps.py.

A missed detection (a row whose coordinates are all NaN) is the limit of an infinite localisation error at that row.  So the oracle is called
with per-peak errors, LAMBDA at the gap rows, the gap rows filled with the previous observed position (any finite value would do: its
Gaussian factor is flat at that scale), and the factor (2 pi LAMBDA^2)^(-D/2) that every gap row then contributes is taken out again:
+ n_gaps * D * (log(2 pi) / 2 + log LAMBDA) per track.  The bias falls as 1 / LAMBDA^2; at LAMBDA = 1e7 it is below 1e-12 on a log-likelihood
and 1e-12 on a posterior for tracks of up to 40 positions (measured against a direct restatement of the gap rule)."""
import numpy as np

from oracle import oracle_np as O

LAMBDA = 1e7


def gap_rows(Cs):
    """(gap [N, L] bool: all coordinates NaN; bad [N] bool: the track breaks a rule - NaN first / last row or a row with some NaN coordinates)."""
    nan = np.isnan(np.asarray(Cs, float))
    gap = nan.all(axis=2)
    bad = (nan.any(axis=2) & ~gap).any(axis=1) | gap[:, 0] | gap[:, -1]
    return gap, bad


def fill_gaps(Cs, gap):
    """Copy of Cs with every gap row replaced by the last observed position before it."""
    out = np.array(Cs, dtype=float, copy=True)
    for t in range(1, out.shape[1]):
        out[gap[:, t], t] = out[gap[:, t], t - 1]
    return out


def loglik_and_preds(Cs, LocErr, ds, Fs, TrMat, pBL, isBL, cell_dims, frame_len, min_len, do_preds=False):
    """Cs [N, L, D] with NaN rows; LocErr [1 | N, 1 | L, k]: the EFFECTIVE localisation error (affine map already applied), entries at gap
    rows are ignored (NaN allowed).  Returns (LL [N], preds [N, L, S] or None); tracks that break a rule are NaN."""
    Cs = np.asarray(Cs, float)
    N, L, D = Cs.shape
    gap, bad = gap_rows(Cs)
    LE = np.array(np.broadcast_to(np.asarray(LocErr, float), (N, L, np.shape(LocErr)[2])), dtype=float, copy=True)
    LE[gap] = LAMBDA
    bad = bad | np.isnan(LE).any(axis=(1, 2))
    filled = fill_gaps(np.where(bad[:, None, None], 0.0, Cs), gap & ~bad[:, None])
    LE[bad] = 1.0
    LP, preds = O.p_cs_inter_bound_stats(filled, LE, ds, Fs, TrMat, pBL, isBL, cell_dims, 1, frame_len, int(bool(do_preds)), min_len)
    mx = LP.max(axis=1, keepdims=True)
    ll = np.log(np.exp(LP - mx).sum(axis=1)) + mx[:, 0]
    ll = ll + gap.sum(axis=1) * D * (0.5 * O.LOG2PI + np.log(LAMBDA))
    ll[bad] = np.nan
    if preds is not None:
        preds[bad] = np.nan
    return ll, preds


def objective(values, all_tracks, dt, cell_dims=(1,), frame_len=6):
    """-sum of the per-track gap-aware log-likelihoods over a bucket dict {len: [N, len, D]} with a global localisation error: what
    ``cum_Proba_Cs(..., gaps=True)`` returns (min_len / max_len from the keys, as ``oracle_np.cum_proba_cs``)."""
    LocErr, ds, Fs, TrMat, pBL = O.extract_params(values, dt, 1, 1)
    keys = sorted((k for k in all_tracks if len(all_tracks[k])), key=int)
    lens = [int(k) for k in keys]
    tot = 0.0
    for k in keys:
        Cs = np.asarray(all_tracks[k], float)
        ll, _ = loglik_and_preds(Cs, np.asarray(LocErr, float).reshape(1, 1, -1), ds, Fs, TrMat, pBL, int(Cs.shape[1] != max(lens)), cell_dims,
                                 frame_len, max(min(lens), 2))
        tot += ll.sum()
    return -tot


# ---- the shared shapes of the emulator and the GPU tests ---------------------------------------------------------------------------------
DT, PBL, CELL, MIN_LEN = 0.02, 0.1, [1.0], 3
MODELS = {
    2: (np.array([0.001, 0.25]), np.array([[0.9, 0.1], [0.15, 0.85]]), np.array([0.55, 0.45])),
    3: (np.array([0.001, 0.04, 0.25]), np.array([[0.85, 0.1, 0.05], [0.08, 0.85, 0.07], [0.05, 0.1, 0.85]]), np.array([0.3, 0.3, 0.4])),
    4: (np.array([0.001, 0.02, 0.1, 0.4]), np.array([[0.85, 0.05, 0.05, 0.05], [0.04, 0.88, 0.04, 0.04], [0.05, 0.03, 0.86, 0.06],
                                                     [0.02, 0.06, 0.04, 0.88]]), np.array([0.2, 0.3, 0.25, 0.25])),
}
LAYOUTS = ("global1", "globalD", "peak", "affine")
SLOPE_OFFSET = (1.3, 0.004)


def gap_masks(F, seed):
    """{L: mask [N, L]} of the test buckets at frame_len F: L = 2; L = 3 with the only interior row missing (every other track); L = F + 1;
    L = 14 with gaps at t = 1, at t = L - 2, a run longer than the window and a track with every interior row missing; L = 40 with gaps across
    the staging boundary (rows 31..33); N = 37 (ragged: a partial last batch) for L = 14.  Neighbouring tracks differ; the rest is 25 % random."""
    rng = np.random.default_rng(seed)
    out = {}
    for L, N in ((2, 5), (3, 6), (F + 1, 9), (14, 37), (40, 7)):
        m = rng.random((N, L)) < 0.25
        if L == 3:
            m[:, 1] = np.arange(N) % 2 == 0
        if L == F + 1:
            m[1, 1:-1] = True
            m[2] = False
        if L == 14:
            m[0], m[1], m[2], m[3] = False, False, False, False
            m[0, 1] = True
            m[1, L - 2] = True
            m[2, 4:4 + F + 2] = True
            m[3, 1:-1] = True
            m[4, 1] = m[4, L - 2] = True
            m[5] = False
        if L == 40:
            m[0, 31:34] = True
            m[1, 29:32] = True
            m[2, 32] = True
            m[3] = False
            m[4, 1:-1] = True
        m[:, 0] = m[:, -1] = False
        out[L] = m
    return out


def make_case(S, D, layout, F, seed=0):
    """Buckets short -> long (upload order) with their gap rows, the error layout and the effective errors the reference takes."""
    from extrack_amd import synth
    Ds, Tm, Fs = MODELS[S]
    masks = gap_masks(F, 100 * seed + 10 * S + D)
    rng = np.random.default_rng(1000 + seed)
    case = dict(S=S, D=D, F=F, layout=layout, buckets=[], masks=[], sig=None, le=None, slope_offset=None, eff=[])
    if layout in ("peak", "affine"):
        case["sig"] = []
    for i, (L, m) in enumerate(sorted(masks.items())):
        tr = synth.brownian_tracks(len(m), L, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=DT, dims=D, seed=50 * seed + 7 * S + i)
        tr[m] = np.nan
        case["buckets"].append(tr)
        case["masks"].append(m)
        if layout == "global1":
            case["le"] = [0.02]
            case["eff"].append(np.array([[[0.02]]]))
        elif layout == "globalD":
            case["le"] = [0.02, 0.03, 0.05][:D]
            case["eff"].append(np.array(case["le"])[None, None])
        elif layout == "peak":  # one error per dimension; a gap row keeps a finite, absurd value: it must never be read
            sg = rng.uniform(0.01, 0.05, (len(m), L, D))
            sg[m] = 123.0
            case["sig"].append(sg)
            case["eff"].append(sg)
        else:  # affine map of one error per peak; NaN at the gap rows
            sg = rng.uniform(0.01, 0.05, (len(m), L, 1))
            sg[m] = np.nan
            case["sig"].append(sg)
            case["slope_offset"] = SLOPE_OFFSET
            case["eff"].append(np.maximum(sg * SLOPE_OFFSET[0] + SLOPE_OFFSET[1], 1e-6))
    return case


def case_reference(case, preds):
    """Per bucket (upload order): LL [N], or posteriors [N, L, S]; min_len 3, the longest bucket does not end by leaving (isBL = 0)."""
    Ds, Tm, Fs = MODELS[case["S"]]
    ds = np.sqrt(2 * Ds * DT)
    Lmax = max(b.shape[1] for b in case["buckets"])
    out = []
    for b, eff in zip(case["buckets"], case["eff"]):
        ll, pr = loglik_and_preds(b, eff, ds, Fs, Tm, PBL, int(b.shape[1] != Lmax), CELL, case["F"], MIN_LEN, do_preds=preds)
        out.append(pr if preds else ll)
    return out
