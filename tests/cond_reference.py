"""TEST INFRASTRUCTURE: the independent oracle of the fixed-state position refinement that
``extrack_refine_fixed_states`` / ``get_pos_PDF_fixedBs`` / ``refine_along_states`` implement.  Not a conftest; imported by
tests/test_cond_cpu.py, tests/test_emul_cond.py and tests/test_hip_cond.py.

It is NOT the forward / backward recursion of the kernel: per track and error channel it builds the tridiagonal posterior precision
``diag(1 / l2) + Dt diag(1 / q) D`` of the real positions (D: the (L - 1) x L first-difference matrix; flat prior on the first position)
and solves it densely for the posterior means and variances, and it evaluates the log density of the observed displacements ``D c`` as a
multivariate normal with covariance ``diag(q) + D diag(l2) Dt``.  Positions are taken relative to the track's first one for the solve (the
model is translation invariant), which keeps the dense solve's rounding at the scale of the displacements."""
import numpy as np

MU_ATOL, SIGMA_RTOL, LOGDENS_ATOL = 1e-12, 1e-12, 1e-10  # the comparison tolerances of every test


def step_variances(states, ds):
    """q [N, L - 1] = (ds[b[t]]**2 + ds[b[t + 1]]**2) / 2: the likelihood's step variance for nb_substeps = 1."""
    ds2 = np.asarray(ds, float) ** 2
    b = np.asarray(states).astype(np.int64)
    return 0.5 * (ds2[b[:, :-1]] + ds2[b[:, 1:]])


def error_variances(shape, le=None, sigma=None, slope_offset=None):
    """l2 [N, L, K] from a global error (1 or D values) or per-peak errors [N, L, K] (optionally through slope / offset, floor 1e-6)."""
    N, L = shape[:2]
    if sigma is None:
        v = np.atleast_1d(np.asarray(le, float)).ravel()
        return np.broadcast_to(v[None, None] ** 2, (N, L, len(v))).copy()
    s = np.asarray(sigma, float)
    if slope_offset is not None:
        s = np.maximum(s * slope_offset[0] + slope_offset[1], 1e-6)
    return s ** 2


def smooth(Cs, l2, q):
    """Cs [N, L, D], l2 [N, L, K] (K = 1 or D), q [N, L - 1]  ->  (mu [N, L, D], sigma [N, L, K], logdens [N])."""
    Cs, l2, q = np.asarray(Cs, float), np.asarray(l2, float), np.asarray(q, float)
    N, L, D = Cs.shape
    K = l2.shape[2]
    assert K in (1, D) and l2.shape[:2] == (N, L) and q.shape == (N, L - 1) and L >= 2
    i, j = np.arange(L), np.arange(L - 1)
    mu, sig, ld = np.empty((N, L, D)), np.empty((N, L, K)), np.zeros(N)
    x = Cs - Cs[:, :1]
    for k in range(K):
        dims = range(D) if K == 1 else [k]
        prec = np.zeros((N, L, L))  # diag(1 / l2) + Dt diag(1 / q) D, written out entry by entry
        prec[:, i, i] = 1.0 / l2[:, :, k]
        prec[:, j, j] += 1.0 / q
        prec[:, j + 1, j + 1] += 1.0 / q
        prec[:, j, j + 1] = prec[:, j + 1, j] = -1.0 / q
        cov = np.linalg.inv(prec)
        sig[:, :, k] = np.sqrt(cov[:, i, i])
        ycov = np.zeros((N, L - 1, L - 1))  # diag(q) + D diag(l2) Dt
        ycov[:, j, j] = q + l2[:, :-1, k] + l2[:, 1:, k]
        ycov[:, j[:-1], j[:-1] + 1] = ycov[:, j[:-1] + 1, j[:-1]] = -l2[:, 1:-1, k]
        _, logdet = np.linalg.slogdet(ycov)
        dims = list(dims)  # one solve for all the dimensions of the channel
        mu[:, :, dims] = np.linalg.solve(prec, x[:, :, dims] / l2[:, :, k:k + 1]) + Cs[:, :1, dims]
        y = x[:, 1:, dims] - x[:, :-1, dims]
        ld += -0.5 * (np.einsum("ntd,ntd->n", y, np.linalg.solve(ycov, y)) + len(dims) * (logdet + (L - 1) * np.log(2 * np.pi)))
    return mu, sig, ld


def refine(Cs, states, ds, le=None, sigma=None, slope_offset=None):
    """The oracle on the kernel's inputs.  Tracks with a NaN position or error, or with a negative state, are NaN in all three outputs."""
    Cs = np.asarray(Cs, float)
    states = np.asarray(states)
    N, L, D = Cs.shape
    l2 = error_variances(Cs.shape, le, sigma, slope_offset)
    bad = np.isnan(Cs).any(axis=(1, 2)) | np.isnan(l2).any(axis=(1, 2)) | (states < 0).any(axis=1)
    ok = ~bad
    mu, sig, ld = np.full((N, L, D), np.nan), np.full((N, L, l2.shape[2]), np.nan), np.full(N, np.nan)
    if ok.any():
        mu[ok], sig[ok], ld[ok] = smooth(Cs[ok], l2[ok], step_variances(states[ok], ds))
    return mu, sig, ld


def compare(got, ref, what="", show=True):
    """(mu, sigma, logdens | None) against the oracle's: NaN rows must coincide; mu within MU_ATOL absolute, sigma within SIGMA_RTOL
    relative, logdens within LOGDENS_ATOL.  Prints the three figures before asserting."""
    (mu, sg, ld), (rmu, rsg, rld) = got, ref
    assert mu.shape == rmu.shape and sg.shape == rsg.shape, (what, mu.shape, rmu.shape, sg.shape, rsg.shape)
    nan = np.isnan(rld)
    assert np.array_equal(np.isnan(mu).all(axis=(1, 2)), nan) and np.array_equal(np.isnan(mu).any(axis=(1, 2)), nan), what
    assert np.array_equal(np.isnan(sg).all(axis=(1, 2)), nan) and np.array_equal(np.isnan(sg).any(axis=(1, 2)), nan), what
    ok = ~nan
    e_mu = np.abs(mu[ok] - rmu[ok]).max() if ok.any() else 0.0
    e_sg = (np.abs(sg[ok] - rsg[ok]) / rsg[ok]).max() if ok.any() else 0.0
    e_ld = 0.0
    if ld is not None:
        assert ld.shape == rld.shape and np.array_equal(np.isnan(ld), nan), what
        e_ld = np.abs(ld[ok] - rld[ok]).max() if ok.any() else 0.0
    if show:
        print("[cond] %s: |mu - ref| %.2e, sigma rel. %.2e, |logdens - ref| %.2e" % (what, e_mu, e_sg, e_ld))
    assert e_mu <= MU_ATOL, "%s: mu differs by %.3e (tolerance %.1e)" % (what, e_mu, MU_ATOL)
    assert e_sg <= SIGMA_RTOL, "%s: sigma differs by %.3e relative (tolerance %.1e)" % (what, e_sg, SIGMA_RTOL)
    assert e_ld <= LOGDENS_ATOL, "%s: logdens differs by %.3e (tolerance %.1e)" % (what, e_ld, LOGDENS_ATOL)
    return e_mu, e_sg, e_ld
