"""CPU checks of extrack_amd.uncertainty: the central-difference Hessian helper against a function with a known Hessian, and the assembly
of covariance / standard errors / correlations from hand-made matrices (bounds, delta method, refusals).  No GPU, no library."""
import numpy as np
import pytest

from extrack_amd import uncertainty as U
from extrack_amd.lmfit_compat import _OwnParameters as Parameters


def test_hessian_from_gradient_on_a_quartic_with_known_hessian():
    """f(x) = sum_i a_i x_i^4 / 12 + x^T Q x / 2 (bounded below: a > 0, Q positive definite).  Gradient g_j = a_j x_j^3 / 3 + (Q x)_j,
    Hessian H = diag(a x^2) + Q.  The central difference of g_j along e_i with step h is exact for the linear part; for the cubic part
    (a_i / 3) ((x + h)^3 - (x - h)^3) / (2 h) = a_i x^2 + a_i h^2 / 3: the truncation error is h^2 / 6 times the third derivative of g
    (= the fourth derivative of f, 2 a_i), on the diagonal only.  Bound: max_i a_i h_i^2 / 3 plus the rounding of the difference,
    8 eps max|g| / min h."""
    rng = np.random.default_rng(3)
    p = 5
    a = rng.uniform(0.5, 2.0, p)
    A = rng.normal(size=(p, p))
    Q = A @ A.T + p * np.eye(p)
    x = rng.uniform(-1.5, 1.5, p)
    grad = lambda y: a * y ** 3 / 3 + Q @ y
    calls = []

    def fgrad(y):
        calls.append(1)
        return grad(y)

    h = 1e-3 * np.maximum(np.abs(x), 0.1)
    H = U.hessian_from_gradient(fgrad, x, h)
    assert len(calls) == 2 * p
    assert np.array_equal(H, H.T)
    exact = np.diag(a * x ** 2) + Q
    bound = (a * h ** 2 / 3).max() + 8 * np.finfo(float).eps * np.abs(grad(x)).max() / h.min()
    assert np.abs(H - exact).max() <= bound, (np.abs(H - exact).max(), bound)
    # the truncation term is really there (order h^2): a 10 times larger step misses the tight bound and meets its own
    H10 = U.hessian_from_gradient(grad, x, 10 * h)
    err10 = np.abs(H10 - exact).max()
    assert bound < err10 <= (a * (10 * h) ** 2 / 3).max() + 8 * np.finfo(float).eps * np.abs(grad(x)).max() / h.min()
    # a gradient that is not symmetric in its Jacobian (not a gradient at all) still comes back symmetrised
    Hn = U.hessian_from_gradient(lambda y: np.array([y[1], 3 * y[0]]), np.array([1.0, 2.0]), 1e-3)
    assert np.allclose(Hn, [[0, 2], [2, 0]], atol=1e-9)


def _params(F0=0.4, D0=0.01, D0_min=0.0):
    p = Parameters()
    p.add("D0", value=D0, min=D0_min, max=1.0)
    p.add("D1", value=0.25, min=0.0, max=3.0)
    p.add("F0", value=F0, min=0.001, max=0.99)
    p.add("F1", expr="1 - F0")
    p.add("LocErr", value=0.02, vary=False)
    p.add("p01", value=0.1, min=0.0001, max=1.0)
    p.add("twoF", expr="2 * F0 + p01")
    return p


def _scores(n, names, seed=0):
    rng = np.random.default_rng(seed)
    scale = np.array([300.0, 4.0, 2.0, 10.0])[:len(names)]  # the scores of a small parameter are large
    return rng.normal(size=(n, len(names))) * scale + 0.3 * rng.normal(size=(n, 1)) * scale


def test_opg_covariance_stderr_correl_and_delta_method():
    p = _params()
    names = ["D0", "D1", "F0", "p01"]
    assert U.split_on_bounds(p) == (names, [])
    S = _scores(200, names)
    B = S.T @ S
    r = U.assemble(p, names, "opg", opg=B)
    C = np.linalg.inv(B)
    assert r["covar"] is not None and np.array_equal(r["covar"], r["covar"].T)
    sd = np.sqrt(np.diag(C))
    assert np.abs(r["covar"] - C).max() <= 1e-12 * 1.0 and np.all(np.abs(r["covar"] - C) <= 1e-10 * np.outer(sd, sd))
    for i, k in enumerate(names):
        assert abs(r["stderr"][k] - sd[i]) <= 1e-10 * sd[i]
    # delta method: F1 = 1 - F0 has the standard error of F0; twoF = 2 F0 + p01 combines two
    assert abs(r["stderr"]["F1"] - r["stderr"]["F0"]) <= 1e-12 * r["stderr"]["F0"]
    want = np.sqrt(4 * r["covar"][2, 2] + r["covar"][3, 3] + 4 * r["covar"][2, 3])
    assert abs(r["stderr"]["twoF"] - want) <= 1e-12 * want
    assert r["stderr"]["LocErr"] is None  # fixed
    assert abs(r["correl"]["D0"]["F0"] - C[0, 2] / (sd[0] * sd[2])) <= 1e-9 and "D0" not in r["correl"]["D0"]
    assert r["correl"]["D0"]["F0"] == r["correl"]["F0"]["D0"]
    assert "opg" in r["message"] and r["method"] == "opg" and r["var_names"] == names


def test_hessian_and_sandwich_formulas():
    p = _params()
    names = ["D0", "D1", "F0", "p01"]
    S = _scores(300, names, 1)
    B = S.T @ S
    rng = np.random.default_rng(5)
    A = rng.normal(size=(4, 4))
    H = B + 0.05 * (A @ A.T) * np.sqrt(np.outer(np.diag(B), np.diag(B)))
    Hi = np.linalg.inv(H)
    rh = U.assemble(p, names, "hessian", opg=None, hessian=H)
    rs = U.assemble(p, names, "sandwich", opg=B, hessian=H)
    sdh = np.sqrt(np.diag(Hi))
    assert np.all(np.abs(rh["covar"] - Hi) <= 1e-10 * np.outer(sdh, sdh))
    Cs = Hi @ B @ Hi
    sds = np.sqrt(np.diag(Cs))
    assert np.all(np.abs(rs["covar"] - Cs) <= 1e-10 * np.outer(sds, sds)) and np.array_equal(rs["covar"], rs["covar"].T)
    # information equality: with H == B the three coincide
    r3 = [U.assemble(p, names, m, opg=B, hessian=B)["covar"] for m in U.METHODS]
    assert np.all(np.abs(r3[0] - r3[1]) <= 1e-10 * np.abs(r3[0])) and np.all(np.abs(r3[0] - r3[2]) <= 1e-9 * np.outer(*[np.sqrt(np.diag(r3[0]))] * 2))
    # an indefinite Hessian (not at a minimum) is refused, not inverted
    Hbad = H.copy()
    Hbad[1, 1] = -Hbad[1, 1]
    r = U.assemble(p, names, "hessian", hessian=Hbad)
    assert r["covar"] is None and "positive definite" in r["message"]
    v = np.linalg.eigh(H)[1][:, 0]
    Hind = H - 2.0 * np.linalg.eigvalsh(H)[0] * np.outer(v, v)  # smallest eigenvalue flipped, diagonal still positive
    r = U.assemble(p, names, "sandwich", opg=B, hessian=Hind)
    assert r["covar"] is None and "positive definite" in r["message"]


def test_parameter_on_a_bound_is_dropped_and_reported():
    # D0 within 1e-6 of its range of the lower bound (where _own_minimize leaves a start value that sat on the bound)
    p = _params(D0=1e-6)
    kept, dropped = U.split_on_bounds(p)
    assert dropped == ["D0"] and kept == ["D1", "F0", "p01"]
    assert U.split_on_bounds(_params(D0=2e-6))[1] == [] and U.split_on_bounds(_params(F0=0.99))[1] == ["F0"]
    q = Parameters()
    q.add("a", value=1e-7, min=0.0)        # one-sided: range 1.0
    q.add("b", value=5.0, max=5.0 + 5e-7)
    q.add("c", value=0.0)                  # unbounded: never on a bound
    assert U.split_on_bounds(q) == (["c"], ["a", "b"])
    S = _scores(100, kept, 2)
    B = S.T @ S
    r = U.assemble(p, kept, "opg", opg=B, dropped=dropped)
    assert r["var_names"] == kept and r["covar"].shape == (3, 3)
    assert r["stderr"]["D0"] is None and r["stderr"]["D1"] > 0 and "D0" in r["message"] and "bound" in r["message"]
    assert "D0" not in r["correl"] and "D0" not in r["correl"]["D1"]
    sd = np.sqrt(np.diag(np.linalg.inv(B)))
    assert abs(r["stderr"]["F1"] - sd[1]) <= 1e-10 * sd[1]


def test_nan_row_and_rank_deficient_scores_are_refused_with_a_message():
    p = _params()
    names = ["D0", "D1", "F0", "p01"]
    S = _scores(50, names, 4)
    Sn = S.copy()
    Sn[7] = np.nan
    r = U.assemble(p, names, "opg", opg=Sn.T @ Sn)
    assert r["covar"] is None and "not finite" in r["message"] and all(v is None for v in r["stderr"].values()) and r["correl"] == {}
    r = U.assemble(p, names, "sandwich", opg=Sn.T @ Sn, hessian=S.T @ S)
    assert r["covar"] is None and "not finite" in r["message"]
    # rank deficient: one column is a combination of two others (a redundant parametrisation) - no pseudo-inverse
    Sd = S.copy()
    Sd[:, 3] = 2.0 * Sd[:, 1] - 0.5 * Sd[:, 2]
    r = U.assemble(p, names, "opg", opg=Sd.T @ Sd)
    assert r["covar"] is None and ("singular" in r["message"] or "positive definite" in r["message"])
    # fewer tracks than parameters
    r = U.assemble(p, names, "opg", opg=S[:3].T @ S[:3])
    assert r["covar"] is None
    # the scaling is not what refuses: the same well-conditioned problem in other units passes
    sc = np.array([1e-6, 1.0, 1e4, 1.0])
    assert U.assemble(p, names, "opg", opg=(S * sc).T @ (S * sc))["covar"] is not None


def test_attach_and_method_resolution():
    from extrack_amd.lmfit_compat import MinimizerResult
    assert U.resolve_method(None) is None and U.resolve_method(False) is None and U.resolve_method(True) == "opg"
    assert U.resolve_method("sandwich") == "sandwich"
    with pytest.raises(ValueError):
        U.resolve_method("bootstrap")
    p = _params()
    names = ["D0", "D1", "F0", "p01"]
    S = _scores(80, names, 6)
    fit = MinimizerResult(params=p.copy(), errorbars=False)
    U.attach(fit, U.assemble(p, names, "opg", opg=S.T @ S))
    assert fit.errorbars is True and fit.uncertainty_method == "opg" and fit.covar.shape == (4, 4)
    assert fit.params["F1"].stderr == pytest.approx(fit.params["F0"].stderr, rel=1e-12) and fit.params["LocErr"].stderr is None
    assert set(fit.params["D1"].correl) == {"D0", "F0", "p01"}
    fit2 = MinimizerResult(params=p.copy(), errorbars=False)
    Sn = S.copy()
    Sn[0, 0] = np.nan
    U.attach(fit2, U.assemble(p, names, "opg", opg=Sn.T @ Sn))
    assert fit2.errorbars is False and fit2.params["D1"].stderr is None and not hasattr(fit2, "covar") and "not finite" in fit2.uncertainty_message


def test_hessian_steps_respect_value_and_bounds():
    p = _params(D0=3e-6)
    h = U.hessian_steps(p, ["D0", "D1", "F0"])
    assert h[1] == pytest.approx(1e-4 * 0.25) and h[2] == pytest.approx(1e-4 * 0.4)
    assert h[0] == pytest.approx(min(1e-4 * 3e-6, 0.5 * 3e-6)) and 0 < h[0] <= 0.5 * 3e-6


def test_param_fitting_refuses_uncertainties_for_threshold_fusion_up_front():
    from extrack_amd import tracking as T
    tr = {"5": np.zeros((3, 5, 2))}
    with pytest.raises(NotImplementedError):
        T.param_fitting(tr, 0.02, fusion="threshold", uncertainties=True)
    with pytest.raises(NotImplementedError):
        T.param_fitting(tr, {"5": np.full((3, 5), 0.02)}, fusion="threshold", uncertainties="opg")
    with pytest.raises(ValueError):
        T.param_fitting(tr, 0.02, uncertainties="bootstrap")
