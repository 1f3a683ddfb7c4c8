"""TEST INFRASTRUCTURE: the dense oracle of the fixed-state position refinement with missed detections that
``extrack_refine_fixed_states_gaps`` / ``refine_along_states(gaps=True)`` implement.  Not a conftest; imported by
tests/test_cond_gaps_cpu.py, tests/test_map_gaps_cpu.py, tests/test_emul_cond_gaps.py, tests/test_hip_cond_gaps.py and
tests/map_gap_reference.py.

It extends ``cond_reference.smooth`` and, like it, is NOT the kernel's recursion: a missed detection (a row whose coordinates are all NaN)
is an observation of infinite error, so the diagonal ``1 / l2`` of the tridiagonal posterior precision is 0 at that row and the row does
not enter the right-hand side; the log density is that of the displacements between consecutive OBSERVED rows, a multivariate normal with
covariance ``Dobs (C + diag(l2)) Dobs^T`` - C[i, j] = sum of q[s] over s < min(i, j), the covariance of the real positions relative to the
first one, and Dobs the first-difference matrix over the observed rows.  Tolerances are those of ``cond_reference``."""
import numpy as np

import cond_reference as R
from gap_reference import gap_rows

MU_ATOL, SIGMA_RTOL, LOGDENS_ATOL = R.MU_ATOL, R.SIGMA_RTOL, R.LOGDENS_ATOL


def smooth(Cs, l2, q, gap):
    """Cs [N, L, D] (gap rows NaN), l2 [N, L, K] (entries at gap rows ignored), q [N, L - 1], gap [N, L] bool with the first and the last
    row observed  ->  (mu [N, L, D], sigma [N, L, K], logdens [N])."""
    Cs, l2, q, gap = np.asarray(Cs, float), np.asarray(l2, float), np.asarray(q, float), np.asarray(gap, bool)
    N, L, D = Cs.shape
    K = l2.shape[2]
    assert K in (1, D) and l2.shape[:2] == (N, L) and q.shape == (N, L - 1) and gap.shape == (N, L) and L >= 2
    assert not gap[:, 0].any() and not gap[:, -1].any()
    i, j = np.arange(L), np.arange(L - 1)
    mu, sig, ld = np.empty((N, L, D)), np.empty((N, L, K)), np.zeros(N)
    x = np.where(gap[:, :, None], 0.0, Cs - Cs[:, :1])
    for k in range(K):
        dims = list(range(D)) if K == 1 else [k]
        w = np.where(gap, 0.0, 1.0 / np.where(gap, 1.0, l2[:, :, k]))  # the precision of an observation: 0 at a gap row
        prec = np.zeros((N, L, L))
        prec[:, i, i] = w
        prec[:, j, j] += 1.0 / q
        prec[:, j + 1, j + 1] += 1.0 / q
        prec[:, j, j + 1] = prec[:, j + 1, j] = -1.0 / q
        cov = np.linalg.inv(prec)
        sig[:, :, k] = np.sqrt(cov[:, i, i])
        mu[:, :, dims] = np.linalg.solve(prec, x[:, :, dims] * w[:, :, None]) + Cs[:, :1, dims]
        for n in range(N):  # the observed rows differ from track to track
            o = np.nonzero(~gap[n])[0]
            cq = np.concatenate([[0.0], np.cumsum(q[n])])
            C = cq[np.minimum.outer(i, i)]
            full = (C + np.diag(np.where(gap[n], 0.0, l2[n, :, k])))[np.ix_(o, o)]
            Dobs = np.zeros((len(o) - 1, len(o)))
            Dobs[np.arange(len(o) - 1), np.arange(len(o) - 1)] = -1.0
            Dobs[np.arange(len(o) - 1), np.arange(1, len(o))] = 1.0
            ycov = Dobs @ full @ Dobs.T
            _, logdet = np.linalg.slogdet(ycov)
            y = x[n][o][1:][:, dims] - x[n][o][:-1][:, dims]
            ld[n] += -0.5 * (np.sum(y * np.linalg.solve(ycov, y)) + len(dims) * (logdet + (len(o) - 1) * np.log(2 * np.pi)))
    return mu, sig, ld


def refine(Cs, states, ds, le=None, sigma=None, slope_offset=None):
    """The oracle on the kernel's inputs.  NaN in all three outputs: a NaN first or last row, a row with only some NaN coordinates, a NaN
    error at an observed row, a negative state anywhere (gap rows included).  The error of a gap row is never looked at."""
    Cs = np.asarray(Cs, float)
    states = np.asarray(states)
    N, L, D = Cs.shape
    gap, bad = gap_rows(Cs)
    l2 = R.error_variances(Cs.shape, le, sigma, slope_offset)
    bad = bad | (np.isnan(l2).any(axis=2) & ~gap).any(axis=1) | (states < 0).any(axis=1)
    ok = ~bad
    mu, sig, ld = np.full((N, L, D), np.nan), np.full((N, L, l2.shape[2]), np.nan), np.full(N, np.nan)
    if ok.any():
        mu[ok], sig[ok], ld[ok] = smooth(Cs[ok], l2[ok], R.step_variances(states[ok], ds), gap[ok])
    return mu, sig, ld


def recursion(Cs, l2, q, gap):
    """The forward / backward rule of csrc/xt_cond.h with GAPS, restated in numpy for ONE error channel layout (K = 1 or D): used by the
    CPU tests to tie the rule to the dense oracle on every mask.  Same arguments and results as ``smooth``."""
    Cs, l2, q, gap = np.asarray(Cs, float), np.asarray(l2, float), np.asarray(q, float), np.asarray(gap, bool)
    N, L, D = Cs.shape
    K = l2.shape[2]
    ch = lambda v: v if K == D else np.repeat(v, D, axis=-1)  # [.., K] -> [.., D]
    f, a = np.empty((N, L, D)), np.empty((N, L, D))
    f[:, 0], a[:, 0] = Cs[:, 0], ch(l2[:, 0])
    ld = np.zeros(N)
    for t in range(1, L):
        g = gap[:, t]
        p = a[:, t - 1] + q[:, t - 1, None]
        lt = ch(np.where(g[:, None], 1.0, l2[:, t]))
        w = p + lt
        r = np.where(g[:, None], 0.0, Cs[:, t]) - f[:, t - 1]
        f[:, t] = np.where(g[:, None], f[:, t - 1], f[:, t - 1] + p / w * r)
        a[:, t] = np.where(g[:, None], p, p / w * lt)
        ld += np.where(g, 0.0, np.sum(-0.5 * np.log(2 * np.pi * w) - r * r / (2 * w), axis=1))
    mu, v = f.copy(), a.copy()
    for t in range(L - 2, -1, -1):
        J = a[:, t] / (a[:, t] + q[:, t, None])
        mu[:, t] = f[:, t] + J * (mu[:, t + 1] - f[:, t])
        v[:, t] = a[:, t] + J * J * (v[:, t + 1] - a[:, t] - q[:, t, None])
    sig = np.sqrt(v if K == D else v[:, :, :1])
    return mu, sig, ld


compare = R.compare
