"""Standard errors of fitted parameters: per-track scores, the outer product of gradients and the observed information.

``param_fitting`` minimises -sum_n LL_n(theta).  The tracks are independent, so at the optimum three matrices estimate the
information the data hold about theta (all with respect to the VALUES of the free parameters, ``gradient.free_names``):

    B = sum_n s_n s_n^T,  s_n = d LL_n / d theta      outer product of gradients (OPG), from ONE scores evaluation
                                                      (extrack_loglik_scores: the forward-mode kernels keep every track's score
                                                      and reduce the outer products on the device)
    H = d^2 (-sum LL) / d theta^2                     observed information, by central differences of the exact gradient
                                                      (2 p gradient evaluations)

and give the covariance of the estimate as

    "opg"       B^-1            (BHHH)      correct model, large sample; always positive semi-definite
    "hessian"   H^-1                        correct model; the curvature the optimiser actually saw
    "sandwich"  H^-1 B H^-1     (Huber / White)   stays valid when the model is misspecified

What is refused rather than papered over (the message says which; nothing is written then):
  * a non-finite matrix (a NaN position poisons its track's score, as it poisons its LL);
  * a matrix that is not positive definite or numerically singular.  Rule: with d = diag(M) (every d_i must be > 0) and
    M_s = d^-1/2 M d^-1/2 - the scaling takes out the units of the parameters, D ~ 1e-3 against fractions ~ 0.5 - the
    eigenvalues of M_s must be > 0 and cond_2(M_s) = l_max / l_min <= 1 / (p * eps), eps = 2^-52.  The inverse is
    d^-1/2 M_s^-1 d^-1/2: a true inverse, never a pseudo-inverse.

A free parameter ON A BOUND (within 1e-6 of its range - 1.0 for one-sided bounds - of ``min`` or ``max``: the rule by which
``lmfit_compat._own_minimize`` moves a start value off a bound) has no two-sided neighbourhood and no normal approximation: it is dropped
from the matrices, gets ``stderr = None`` and is named in the message.  ``expr`` parameters (F1 = 1 - F0) get their standard error
by the delta method, J C J^T with J = d value / d free values from the complex-step plumbing of ``gradient._values_batched``.
"""
import numpy as np

from . import engine, gradient
from .lmfit_compat import _OwnParameters, _to_own_parameters

METHODS = ("opg", "hessian", "sandwich")
_EPS = 2.0 ** -52
_BOUND_TOL = 1e-6
_REL_STEP = 1e-4


def resolve_method(uncertainties):
    """None for no uncertainties (None / False), else the method name (True = "opg")."""
    if uncertainties is None or uncertainties is False:
        return None
    if uncertainties is True:
        return "opg"
    if uncertainties not in METHODS:
        raise ValueError("uncertainties must be None, a bool or one of %s" % (METHODS,))
    return uncertainties


def on_bound(p):
    """Does the parameter sit within 1e-6 of its range (1.0 for one-sided bounds) of a bound?  The comparison carries a relative slack of
    1e-6 so that a parameter the optimiser left exactly at its 1e-6 starting offset counts as on the bound."""
    lo, hi = p.min, p.max
    rng = (hi - lo) if (np.isfinite(lo) and np.isfinite(hi)) else 1.0
    tol = _BOUND_TOL * rng * (1.0 + 1e-6)
    return bool((np.isfinite(lo) and p.value - lo <= tol) or (np.isfinite(hi) and hi - p.value <= tol))


def split_on_bounds(params, names=None):
    """(free parameters kept, free parameters dropped because they sit on a bound)."""
    names = gradient.free_names(params) if names is None else list(names)
    kept = [k for k in names if not on_bound(params[k])]
    return kept, [k for k in names if k not in kept]


def hessian_steps(params, names):
    """Differencing step of every parameter: h_i = 1e-4 |value_i| (1e-4 of the range, or 1e-4, at value 0), at most half the distance to
    the nearer bound.  With the exact gradient g the central difference (g(x + h) - g(x - h)) / 2h has the truncation error
    h^2 / 6 |d^3 g| ~ 1e-8 relative and the rounding error eps_g / h ~ 1e-12 / 1e-4 of the gradient's own rounding: the two meet there."""
    h = []
    for k in names:
        p = params[k]
        v = p.value
        rng = (p.max - p.min) if (np.isfinite(p.min) and np.isfinite(p.max)) else 1.0
        hi = _REL_STEP * (abs(v) if v != 0.0 else rng)
        for b in (p.min, p.max):
            if np.isfinite(b):
                hi = min(hi, 0.5 * abs(v - b))
        h.append(hi)
    return np.array(h)


def hessian_from_gradient(fgrad, x, h):
    """Jacobian of the gradient ``fgrad(x) -> g [p]`` at ``x`` by central differences with the per-coordinate steps ``h``, symmetrised:
    row i = (g(x + h_i e_i) - g(x - h_i e_i)) / (2 h_i), H = (J + J^T) / 2.  2 p calls of ``fgrad``."""
    x = np.asarray(x, float)
    p = len(x)
    h = np.broadcast_to(np.asarray(h, float), (p,))
    J = np.empty((p, p))
    for i in range(p):
        xp, xm = x.copy(), x.copy()
        xp[i] += h[i]
        xm[i] -= h[i]
        J[i] = (np.asarray(fgrad(xp), float) - np.asarray(fgrad(xm), float)) / (xp[i] - xm[i])  # the step actually taken
    return 0.5 * (J + J.T)


def _inverse_pd(M, what):
    """(M^-1, None), or (None, reason) under the rule of the module docstring."""
    p = len(M)
    if not np.all(np.isfinite(M)):
        why = "a differencing step left the valid parameter region, or a track has a NaN input" if what == "the Hessian" else \
            "a track with a NaN position or localisation error has a NaN score"
        return None, "%s is not finite (%s)" % (what, why)
    d = np.diag(M)
    if np.any(d <= 0):
        return None, "%s is not positive definite (diagonal entry <= 0)" % what
    r = 1.0 / np.sqrt(d)
    Ms = M * r[:, None] * r[None, :]
    Ms = 0.5 * (Ms + Ms.T)
    w = np.linalg.eigvalsh(Ms)
    if w[0] <= 0:
        return None, "%s is not positive definite (smallest eigenvalue of the scaled matrix %.3g)" % (what, w[0])
    if w[-1] / w[0] > 1.0 / (p * _EPS):
        return None, "%s is numerically singular (condition number of the scaled matrix %.3g > 1 / (p eps))" % (what, w[-1] / w[0])
    inv = np.linalg.inv(Ms) * r[:, None] * r[None, :]
    return 0.5 * (inv + inv.T), None


def covariance(method, opg=None, hessian=None):
    """(covariance, None) of the chosen method from the OPG matrix B and / or the Hessian H of -sum LL, or (None, reason)."""
    if method not in METHODS:
        raise ValueError("method must be one of %s" % (METHODS,))
    if method == "opg":
        return _inverse_pd(np.asarray(opg, float), "the outer product of gradients")
    Hi, why = _inverse_pd(np.asarray(hessian, float), "the Hessian")
    if Hi is None or method == "hessian":
        return Hi, why
    B = np.asarray(opg, float)
    if not np.all(np.isfinite(B)):
        return None, "the outer product of gradients is not finite (a track with a NaN position or localisation error has a NaN score)"
    C = Hi @ B @ Hi
    return 0.5 * (C + C.T), None


def value_jacobian(params, names):
    """{parameter name: d value / d (values of the free parameters ``names``) [len(names)]} through the constraint expressions."""
    if not names:
        return {k: np.zeros(0) for k in params}
    vals = gradient._values_batched(params, names)
    return {k: np.imag(v) / gradient._H for k, v in vals.items()}


def assemble(params, names, method, opg=None, hessian=None, dropped=()):
    """The result dict of ``parameter_uncertainties`` from the matrices over the kept free parameters ``names`` (pure host code):
    var_names, covar [p, p] or None, stderr {every parameter: float or None}, correl {kept name: {other kept name: r}}, opg, hessian,
    method, message.  ``dropped``: free parameters left out because they sit on a bound."""
    names = list(names)
    out = dict(var_names=names, covar=None, stderr={k: None for k in params}, correl={}, opg=opg, hessian=hessian, method=method, message="")
    notes = ["%s is on a bound: dropped, no standard error" % k for k in dropped]
    if not names:
        out["message"] = "; ".join(notes + ["no free parameter left"])
        return out
    C, why = covariance(method, opg, hessian)
    if C is None:
        out["message"] = "; ".join(notes + ["no uncertainties: " + why])
        return out
    if np.any(np.diag(C) <= 0):
        out["message"] = "; ".join(notes + ["no uncertainties: the covariance has a non-positive diagonal entry"])
        return out
    out["covar"] = C
    sd = np.sqrt(np.diag(C))
    J = value_jacobian(params, names)
    for k, p in params.items():
        if k in names:
            out["stderr"][k] = float(sd[names.index(k)])
        elif getattr(p, "expr", None):  # delta method
            out["stderr"][k] = float(np.sqrt(max(J[k] @ C @ J[k], 0.0)))
    R = C / np.outer(sd, sd)
    out["correl"] = {a: {b: float(R[i, j]) for j, b in enumerate(names) if b != a} for i, a in enumerate(names)}
    out["message"] = "; ".join(notes + ["%s covariance of %d parameters" % (method, len(names))])
    return out


def _own(params):
    return params if isinstance(params, _OwnParameters) else _to_own_parameters(params)


def _open(all_tracks, dt, input_LocErr, device, gaps=False):
    """(TrackSet, owned, bucket keys) - a TrackSet is used as is (a gapped one included); ``gaps``: the dict's all-NaN rows are missed detections."""
    if isinstance(all_tracks, engine.TrackSet):
        ts, owned, keys = all_tracks, False, None
    else:
        if isinstance(dt, (dict, list)):
            raise NotImplementedError("per-track scores with per-track time steps are not built (the fixed-window kernels take a scalar dt)")
        _, tracks, sigmas = engine.sort_buckets(all_tracks, input_LocErr)
        ts, owned = engine.TrackSet(tracks, sigmas, device=0 if device is None else int(device), gaps=gaps), True
        keys = [str(t.shape[1]) for t in tracks]
    if ts.has_dt:
        if owned:
            ts.close()
        raise NotImplementedError("per-track scores with per-track time steps are not built (the fixed-window kernels take a scalar dt)")
    return ts, owned, keys


def _scores_call(params, names, ts, dt, cell_dims, nb_states, nb_substeps, frame_len, Matrix_type, scores=False):
    """ctx.loglik_scores at ``params`` along the free parameters ``names``; None for invalid parameters."""
    from .tracking import _objective_model
    model = _objective_model(params, ts, dt, cell_dims, None, nb_states, nb_substeps, frame_len, Matrix_type)
    if model is None:
        return None
    tang = gradient.model_tangents(params, dt, nb_substeps, Matrix_type, cell_dims, names, has_sigma=ts.has_sigma)
    if ts.gaps:  # the gap-aware forward-mode kernels (extrack_loglik_scores_gaps)
        return ts.ctx.loglik_scores(model, tang, scores=scores, gaps=True)
    return ts.ctx.loglik_scores(model, tang, scores=scores)


def track_scores(all_tracks, dt, params, nb_states=2, nb_substeps=1, frame_len=6, cell_dims=[1], input_LocErr=None, Matrix_type=1,
                 device=None, gaps=False):
    """{str(len): ndarray [n_tracks, p]}: every track's d LL_n / d (value of the free parameter), columns in the order of
    ``gradient.free_names(params)``, rows in the order of the bucket.  The chain rule from the parameters to the model goes through
    ``gradient.model_tangents``, the recursion through the forward-mode gradient kernels (extrack_loglik_scores).
    ``gaps``: all-NaN rows of the track dict are missed detections (``extrack_amd.gaps``; extrack_loglik_scores_gaps); a gapped
    ``TrackSet`` is used as it is."""
    params = _own(params)
    names = gradient.free_names(params)
    ts, owned, keys = _open(all_tracks, dt, input_LocErr, device, gaps)
    try:
        if keys is None:
            keys = [str(s[1]) for s in ts.shapes]
        res = _scores_call(params, names, ts, dt, cell_dims, nb_states, nb_substeps, frame_len, Matrix_type, scores=True)
        if res is None:
            raise ValueError("invalid parameters (extrack/tracking.py:1017): no score")
        sc, out, r0 = res[3], {}, 0
        for k, shp in zip(keys, ts.shapes):
            out[k] = sc[r0:r0 + shp[0]]
            r0 += shp[0]
        return out
    finally:
        if owned:
            ts.close()


def parameter_uncertainties(all_tracks, dt, params, nb_states=2, nb_substeps=1, frame_len=6, cell_dims=[1], input_LocErr=None,
                            Matrix_type=1, device=None, method="opg", comm=None, gaps=False):
    """Covariance and standard errors of the fitted ``params`` (see the module docstring for the three methods, the refusal rules and
    the treatment of bounds and ``expr`` parameters).  ``all_tracks``: the track dict, or a ``TrackSet`` (with ``comm``: this rank's
    shard - every rank evaluates its own tracks, the p x p matrix and the (1 + p) vector {sum LL, gradient} are summed with
    ``comm.allreduce_vector``; scores are never gathered).  Returns a dict: var_names (free parameters not on a bound), covar, stderr
    {name: float | None}, correl, opg, hessian (None when the method does not need it), method, message, loglik, gradient.

    Hessian: central differences of ``gradient.objective_and_gradient`` with the steps of ``hessian_steps`` (1e-4 of the value, at
    most half the distance to the nearer bound), symmetrised.

    ``gaps``: all-NaN rows of the track dict are missed detections (a gapped ``TrackSet`` is used as it is): scores and gradient come from
    the gap-aware forward-mode kernels, all three methods work; one GPU only (``comm`` raises NotImplementedError)."""
    if method not in METHODS:
        raise ValueError("method must be one of %s" % (METHODS,))
    if comm is not None and (gaps or (isinstance(all_tracks, engine.TrackSet) and all_tracks.gaps)):
        raise NotImplementedError("missed detections (gaps=True) are not built for distributed evaluation: comm must be None")
    params = _own(params)
    kept, dropped = split_on_bounds(params)
    ts, owned, _ = _open(all_tracks, dt, input_LocErr, device, gaps)
    try:
        B = H = ll = g = None
        p = len(kept)
        if p and method in ("opg", "sandwich"):
            res = _scores_call(params, kept, ts, dt, cell_dims, nb_states, nb_substeps, frame_len, Matrix_type) if ts.n_tracks else \
                (0.0, np.zeros(p), np.zeros((p, p)))
            if comm is not None:
                ok = comm.allreduce_scalar(0.0 if res is not None else 1.0) == 0.0
                res = res if ok else None
            if res is None:
                out = assemble(params, [], method, dropped=dropped)
                out["message"] = "no uncertainties: invalid parameters"
                return out
            ll, g, B = res[0], res[1], res[2]
            if comm is not None:
                v = comm.allreduce_vector(np.concatenate([[ll], g]))
                ll, g = float(v[0]), np.asarray(v[1:])
                B = np.asarray(comm.allreduce_vector(B.ravel())).reshape(p, p)
        if p and method in ("hessian", "sandwich"):
            work = params.copy()

            def fgrad(x):
                for k, xi in zip(kept, x):
                    work[k].value = xi
                work.update_constraints()
                f, gg = gradient.objective_and_gradient(work, ts, dt, cell_dims, nb_states, nb_substeps, frame_len, Matrix_type, comm, kept)
                return gg if np.isfinite(f) else np.full(p, np.nan)
            H = hessian_from_gradient(fgrad, [params[k].value for k in kept], hessian_steps(params, kept))
        out = assemble(params, kept, method, opg=B, hessian=H, dropped=dropped)
        out["loglik"], out["gradient"] = ll, g
        return out
    finally:
        if owned:
            ts.close()


def attach(fit, res):
    """Writes a result of ``parameter_uncertainties`` into a MinimizerResult the way lmfit reports its own error bars: ``fit.covar``,
    ``fit.params[name].stderr`` / ``.correl``, ``fit.errorbars``; plus ``fit.uncertainty_method`` / ``fit.uncertainty_message``."""
    fit.uncertainty_method, fit.uncertainty_message = res["method"], res["message"]
    fit.uncertainty_var_names = list(res["var_names"])
    if res["covar"] is None:
        return fit
    fit.covar = res["covar"]
    for k, p in fit.params.items():
        p.stderr = res["stderr"][k]
        p.correl = res["correl"].get(k)
    fit.errorbars = True
    return fit
