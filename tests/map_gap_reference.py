"""TEST INFRASTRUCTURE: numpy restatement of the windowed most-likely-state-path recursion with missed detections
that ``extrack_map_states_gaps`` / ``predict_states(gaps=True)`` implement, and the score of a GIVEN path computed without the recursion.
Not a conftest; imported by tests/test_map_gaps_cpu.py, tests/test_cond_gaps_cpu.py, tests/test_emul_map_gaps.py,
tests/test_emul_cond_gaps.py, tests/test_hip_map_gaps.py and tests/test_hip_cond_gaps.py.

``map_path`` is ``map_reference.map_path`` with the gap rule at a row whose coordinates are all NaN: no Gaussian factor, the mean stays,
the variance carried forward grows by the step variance (the limit of an infinite error at that row); select, back-pointers and the final
argmax are unchanged.  On a gap-free track every operation is the one of ``map_reference.map_path``: the results are identical.

Path comparison with gaps (``compare_paths``): inside a run of two or more consecutive gap rows the joint density depends only on how many
rows of the run each state occupies and on the transitions, not on where inside the run an excursion sits, so distinct paths tie exactly
(select margins of 0 or ~3e-14) and the tie rule decides.  Hence (a) every score within ``score_tol`` of the restatement's, (b) for every
unpoisoned track ``path_score`` of the RETURNED path within 2e-10 of the returned score (the decoder's 1e-10 plus the dense logdens's
1e-10): the path is a real path with that density, (c) states equal the restatement's for every track whose margin is >= TIE_MARGIN, (d)
the tracks (c) leaves out are at most ``max_ties`` and each has a run of at least two consecutive gap rows."""
import numpy as np

import cond_gap_reference as CG
from gap_reference import gap_rows
from map_reference import TIE_MARGIN, TIE_SHARE, _top2_gap  # noqa: F401
from oracle import oracle_np as O

PATH_SCORE_TOL = 2e-10
MAX_TIES_PER_CASE = 4  # of the 64 tracks of a gap_reference.make_case (measured with the reference alone on all 72 cases at seed 0)


def map_path(Cs, LocErr, ds, Fs, TrMat, pBL, isBL, cell_dims, frame_len, min_len):
    """Cs [N, L, D] with all-NaN rows; LocErr [1 | N, 1 | L, k], entries at gap rows ignored (NaN allowed).  Returns (states int8 [N, L],
    score [N], margin [N]) as ``map_reference.map_path``; tracks that break a gap rule have states -1 and score NaN."""
    Cs = np.asarray(Cs, float)
    N, L, D = Cs.shape
    ds, Fs, TrMat = np.asarray(ds, float), np.asarray(Fs, float), np.asarray(TrMat, float)
    S, F = TrMat.shape[0], int(frame_len)
    LocErr = np.asarray(LocErr, float)
    assert LocErr.ndim == 3 and LocErr.shape[1] in (1, L) and L >= 2 and F >= 2
    gap, bad = gap_rows(Cs)
    LEb = np.broadcast_to(LocErr, (N, L, LocErr.shape[2]))
    bad = bad | (np.isnan(LEb).any(axis=2) & ~gap).any(axis=1)
    if LocErr.shape[1] == 1 and L != 1:
        l2 = lambda p: np.broadcast_to(LocErr[:, 0, :] ** 2, (N, LocErr.shape[2]))
    else:
        l2 = lambda p: np.broadcast_to(LocErr[:, p, :] ** 2, (N, LocErr.shape[2]))
    k = LocErr.shape[2]
    LTs, d2s = O.seq_tables(S, 1, ds, TrMat)
    pst = O.p_stay_table(ds, S, 1, cell_dims)
    Lpst = np.log(pst * (1 - pBL))

    def gauss_log(c, m, s2x):
        return np.sum(-0.5 * np.log(2 * np.pi * s2x) - (c - m) ** 2 / (2 * s2x), axis=2) if s2x.shape[2] == D else \
            D * -0.5 * np.log(2 * np.pi * s2x[:, :, 0]) - np.sum((c - m) ** 2 / (2 * s2x), axis=2)

    n = 2
    idx = np.arange(S ** n)
    LP = np.repeat((LTs[idx] + np.log(Fs[(idx // S) % S]))[None], N, axis=0)
    m = np.repeat(Cs[:, 0, None, :], S ** n, axis=1)
    s2 = l2(0)[:, None, :] + d2s[idx][None, :, None]
    back = []
    margin = np.full(N, np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(2, L):
            p = t - 1
            n += 1
            idx = np.arange(S ** n)
            par, sm = idx // S, idx % S ** 2
            gp = gap[:, p]
            lp, c = l2(p)[:, None, :], Cs[:, p, None, :]
            mo, s2o = m[:, par], s2[:, par]
            den = lp + s2o
            LC = np.where(gp[:, None], 0.0, gauss_log(c, mo, den))
            m = np.where(gp[:, None, None], mo, (mo * lp + c * s2o) / den)
            d2e = d2s[sm][None, :, None]
            s2 = np.where(gp[:, None, None], d2e + s2o, (d2e * lp + d2e * s2o + lp * s2o) / den)
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
        sc = np.where(bad[:, None], 0.0, sc)
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


def log_prior(states, ds, Fs, TrMat, pBL, isBL, cell_dims, min_len):
    """Log prior of given paths [N, L]: initial fraction, transitions, stay terms from step max(min_len, 2) on, and with isBL the summed-out
    end term - the terms written out in tests/test_cond_cpu.py (test_oracle_ties_to_reference_fixtures)."""
    ds, Fs, TrMat = np.asarray(ds, float), np.asarray(Fs, float), np.asarray(TrMat, float)
    S = len(ds)
    b = np.asarray(states).astype(np.int64)
    L = b.shape[1]
    LTs, _ = O.seq_tables(S, 1, ds, TrMat)
    pst = O.p_stay_table(ds, S, 1, cell_dims)
    Lpst = np.log(pst * (1 - pBL))
    prior = np.log(Fs[b[:, 0]])
    for t in range(1, L):
        prior = prior + LTs[b[:, t - 1] * S + b[:, t]]
        if t >= max(min_len, 2):
            prior = prior + Lpst[b[:, t]]
    if isBL:
        qq = pBL + (1 - pst) - pBL * (1 - pst)
        prior = prior + np.log(TrMat @ qq)[b[:, L - 1]]
    return prior


def path_score(states, Cs, LocErr, ds, Fs, TrMat, pBL, isBL, cell_dims, min_len):
    """Log joint density of the observed positions and the GIVEN path, without the recursion: the path's log prior plus the gap-aware dense
    ``logdens`` of that path (tests/cond_gap_reference.py).  LocErr [1 | N, 1 | L, k] effective errors.  NaN for tracks that break a gap rule
    or hold a negative state."""
    Cs = np.asarray(Cs, float)
    N, L, D = Cs.shape
    states = np.asarray(states)
    LE = np.array(np.broadcast_to(np.asarray(LocErr, float), (N, L, np.shape(LocErr)[2])), dtype=float)
    _, _, ld = CG.refine(Cs, states, ds, sigma=LE)
    ok = ~np.isnan(ld)
    out = np.full(N, np.nan)
    if ok.any():
        out[ok] = log_prior(states[ok], ds, Fs, TrMat, pBL, isBL, cell_dims, min_len) + ld[ok]
    return out


def has_gap_run(mask):
    """[N] bool: the track has two or more consecutive gap rows."""
    mask = np.asarray(mask, bool)
    return (mask[:, 1:] & mask[:, :-1]).any(axis=1)


def compare_paths(got_states, got_score, ref, Cs, LocErr, model, score_tol, what="", show=True):
    """Rules (a) - (c) of the module docstring for one bucket.  ``ref``: (states, score, margin) of ``map_path``; ``model``: the arguments
    (ds, Fs, TrMat, pBL, isBL, cell_dims, min_len) of ``path_score``.  Returns the [N] bool of the tracks (c) left out, for rule (d)."""
    ref_states, ref_score, margin = ref
    got_states, got_score = np.asarray(got_states), np.asarray(got_score)
    assert got_states.shape == ref_states.shape and got_states.dtype == np.int8, (what, got_states.shape, ref_states.shape, got_states.dtype)
    nan = np.isnan(ref_score)
    assert np.array_equal(np.isnan(got_score), nan), what
    assert np.all(got_states[nan] == -1) and not np.any(got_states[~nan] < 0), what
    e_sc = np.abs(got_score[~nan] - ref_score[~nan]).max() if (~nan).any() else 0.0  # (a)
    ps = path_score(got_states, Cs, LocErr, *model)                                  # (b)
    assert np.array_equal(np.isnan(ps), nan), what
    e_ps = np.abs(ps[~nan] - got_score[~nan]).max() if (~nan).any() else 0.0
    out = ~nan & ~(margin >= TIE_MARGIN)
    if show:
        print("[map gaps] %s: |score - ref| %.2e, |path_score(path) - score| %.2e, %d of %d tracks left out of the path comparison"
              % (what, e_sc, e_ps, out.sum(), len(out)))
    assert e_sc <= score_tol, "%s: score differs by %.3e (tolerance %.1e)" % (what, e_sc, score_tol)
    assert e_ps <= PATH_SCORE_TOL, "%s: the returned path scores %.3e away from the returned score (tolerance %.1e)" % (what, e_ps, PATH_SCORE_TOL)
    keep = ~out
    wrong = np.nonzero((got_states[keep] != ref_states[keep]).any(axis=1))[0]                                                 # (c)
    assert len(wrong) == 0, "%s: %d of %d paths differ, first %s: got %s want %s" % (
        what, len(wrong), keep.sum(), wrong[:1], got_states[keep][wrong[:1]], ref_states[keep][wrong[:1]])
    return out


def check_exclusions(left_out, masks, max_ties=MAX_TIES_PER_CASE, what=""):
    """Rule (d) over the buckets of a case: a condition, not a measurement."""
    n = sum(int(o.sum()) for o in left_out)
    assert n <= max_ties, "%s: %d tracks are near-ties (at most %d)" % (what, n, max_ties)
    for o, m in zip(left_out, masks):
        assert np.all(has_gap_run(m)[o]), "%s: a track without a run of two gap rows has a margin below %.0e" % (what, TIE_MARGIN)
