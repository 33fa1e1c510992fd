"""rat_policy_gradient / rat_policy_tail_gradient without a device: the exports, the compile-only check and its refusals, and the NumPy
model (tests/policy_gradient_model.py) against central finite differences of its own sample functionals on fixed draws, a closed form
and the plain standard error."""
import ctypes as C

import numpy as np
import pytest

import policy_gradient_model as pg
import ratilqr.jl_amd as rat
import tail_risk_model as trm
import user_noise_model as un
import worst_case_model as wcm
from ratilqr.jl_amd import _native as nv

EPS = np.finfo(np.float64).eps


def test_exports_and_prototypes():
    lib = nv.lib()
    for name in ("rat_policy_gradient", "rat_policy_tail_gradient", "rat_policy_gradient_check"):
        assert name in nv.EXPORTS and hasattr(lib, name)
    assert len(lib.rat_policy_gradient.argtypes) == 10 and lib.rat_policy_gradient.argtypes[-1] == C.POINTER(C.c_int64)
    assert len(lib.rat_policy_tail_gradient.argtypes) == 8 and len(lib.rat_policy_gradient_check.argtypes) == 5


@pytest.mark.parametrize("case", [pg.ScalarLQ(), pg.Lin2(), pg.Pendulum(), pg.Pendulum(source=pg.PEND_JAC), pg.SqrtCost(),
                                  pg.LqCubic(5, 3, 2), pg.LqCubic(12, 4, 3)], ids=lambda c: f"{type(c).__name__}{c.n}x{c.m}")
def test_check_compiles_the_cases(case):
    rat.policy_gradient_check(case.source, **case.dims())


def test_check_refuses_with_the_documented_codes():
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_UNSUPPORTED.*defines RAT_USER_POLICY"):
        rat.policy_gradient_check("#define RAT_USER_POLICY\n" + un.PEND_DIAG, 2, 1, 2, 0)
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_ARG.*does not define RAT_USER_NOISE"):
        rat.policy_gradient_check(un.PEND_PLAIN, 2, 1, 0, 0)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*n <= 12"):
        rat.policy_gradient_check(un.PEND_DIAG, 13, 1, 2, 0)


# ---- the model against central differences of its own sample functionals ----------------------------------------------------------------
K_FD, SEED = 256, 11
FUNCTIONALS = {
    "mean": (dict(thetas=[0.0]), lambda J: J.mean()),
    "entropic": (dict(thetas=[0.7]), lambda J: np.log(np.exp(np.longdouble(0.7) * (J - J.max())).mean()) / np.longdouble(0.7) + J.max()),
    "kl": (dict(kl_bounds=[0.05]), lambda J: wcm.direct(np.asarray(J, float), 0.05)["bound"]),
    "cvar": (dict(alphas=[0.9]), lambda J: trm.direct(np.asarray(J, float), 0.9)["cvar"]),
}


def fd_gradient(case, x_nom, l, L, z, F, step, dtype):
    """central differences of F(costs) over every entry of l and L"""
    def val(lq, Lq):
        return F(pg.rollout(case, x_nom, lq, Lq, z, dtype)[0])
    gl, gL = np.zeros(l.shape, dtype=dtype), np.zeros(L.shape, dtype=dtype)
    for idx in np.ndindex(*l.shape):
        a, b = l.copy(), l.copy()
        a[idx] += step; b[idx] -= step
        gl[idx] = (val(a, L) - val(b, L)) / (dtype(a[idx]) - dtype(b[idx]))
    for idx in np.ndindex(*L.shape):
        a, b = L.copy(), L.copy()
        a[idx] += step; b[idx] -= step
        gL[idx] = (val(l, a) - val(l, b)) / (dtype(a[idx]) - dtype(b[idx]))
    return gl, gL


@pytest.mark.parametrize("name", ["mean", "cvar"])
def test_lq_quadratic_functionals_match_central_differences(name):
    """Linear dynamics and a quadratic cost: the mean, and CVaR while its tail set stands, are quadratic in the policy, so a central
    difference has no truncation error and what is left is rounding: two costs of size max|J|, each a sum of K terms rounded at eps,
    over 2 step.  The tolerance is 8 eps max|J| / step (a factor 8 for the accumulated roundings of the N + 1 cost terms and the mean),
    computed here."""
    case, N, step = pg.Lin2(), 3, 2.0 ** -10
    x_nom, l, L = pg.policy(case, N)
    z = pg.draws(case, SEED, K_FD, N)
    kw, F = FUNCTIONALS[name]
    mod = pg.model(case, x_nom, l, L, K_FD, SEED, **kw)
    if name == "cvar":                                                # the step is small enough that the tail set does not change
        v = trm.direct(np.asarray(mod["J"]), 0.9)["var"]
        tail = set(np.flatnonzero(mod["J"] >= v))
        for arr, base in ((l, "l"), (L, "L")):
            for idx in np.ndindex(*arr.shape):
                for sgn in (1.0, -1.0):
                    a = arr.copy(); a[idx] += sgn * step
                    J = pg.rollout(case, x_nom, a if base == "l" else l, a if base == "L" else L, z)[0]
                    assert set(np.flatnonzero(J >= trm.direct(J, 0.9)["var"])) == tail
    gl, gL = fd_gradient(case, x_nom, l, L, z, lambda J: np.float64(F(J)), step, np.float64)
    tol = 8 * EPS * np.abs(mod["J"]).max() / step
    print(f"{name}: tol {tol:.3e}, grad_l err {np.abs(gl - mod['grad_l'][0]).max():.3e}, grad_L err {np.abs(gL - mod['grad_L'][0]).max():.3e}")
    assert np.abs(gl - mod["grad_l"][0]).max() <= tol and np.abs(gL - mod["grad_L"][0]).max() <= tol


@pytest.mark.parametrize("name", ["mean", "entropic", "kl", "cvar"])
@pytest.mark.parametrize("case", [pg.Lin2(), pg.Pendulum()], ids=["lin2", "pendulum"])
def test_functionals_match_central_differences_in_extended_precision(case, name):
    """The functionals that are not quadratic (the entropic risk and the KL bound everywhere, everything on the pendulum).  The central
    difference is taken in np.longdouble and Richardson-extrapolated, D(h) = (4 d(h / 2) - d(h)) / 3, whose truncation error is
    O(h^4).  The step is the one of 2^-4, 2^-6, 2^-8, 2^-10 that minimises the reference's own error estimate |D(h) - D(h / 2)|
    (printed: 2^-4 .. 2^-10 here, estimates 4e-18 .. 2e-15, and 6e-14 .. 1.3e-13 for the KL bound, whose bisection for theta* in
    worst_case_model.direct shows through the division by h).  The tolerance is 4 times that estimate plus 64 eps of the largest
    gradient entry for the float64 model's own sums over K = 256 rollouts: 3e-15 .. 5e-13 here, against errors of 2e-17 .. 1.3e-13."""
    N = 3
    x_nom, l, L = pg.policy(case, N)
    z = pg.draws(case, SEED, K_FD, N)
    kw, F = FUNCTIONALS[name]
    mod = pg.model(case, x_nom, l, L, K_FD, SEED, **kw)
    if name == "cvar":
        tail = set(np.flatnonzero(mod["y"][0] > 0))

    def Fc(J):
        if name == "cvar":                                            # the tail set must not change under any perturbation used
            J64 = np.asarray(J, float)
            assert set(np.flatnonzero(J64 >= trm.direct(J64, 0.9)["var"])) == tail
            return trm_cvar_ld(J, 0.9)
        return F(J)

    def D(h):
        a, b = fd_gradient(case, x_nom, l, L, z, Fc, h, np.longdouble), fd_gradient(case, x_nom, l, L, z, Fc, h / 2, np.longdouble)
        return (4 * b[0] - a[0]) / 3, (4 * b[1] - a[1]) / 3
    best = None
    for e in (4, 6, 8, 10):
        h = 2.0 ** -e
        try:
            d1, d2 = D(h), D(h / 2)
        except AssertionError:
            continue                                                  # (CVaR: a step that moves the tail set is no candidate)
        est = float(max(np.abs(d1[0] - d2[0]).max(), np.abs(d1[1] - d2[1]).max()))
        if best is None or est < best[0]:
            best = (est, h, d2)
    assert best is not None
    est, h, (gl, gL) = best
    tol = 4 * est + 64 * EPS * float(max(np.abs(gl).max(), np.abs(gL).max()))
    e_l, e_L = float(np.abs(gl - mod["grad_l"][0]).max()), float(np.abs(gL - mod["grad_L"][0]).max())
    print(f"{name}: step 2^{int(np.log2(h))}, reference error estimate {est:.3e}, tol {tol:.3e}, errors {e_l:.3e} {e_L:.3e}")
    assert e_l <= tol and e_L <= tol


def trm_cvar_ld(J, alpha):
    """CVaR_alpha of the sample in the dtype of J, tail_risk_model.direct's rule: v + sum (J - v)+ / (n - n alpha)"""
    n = J.size
    av = np.float64(n) * alpha
    k = int(min(max(np.ceil(av), 1), n))
    v = np.sort(J)[k - 1]
    return v + np.where(J > v, J - v, 0).sum() / (J.dtype.type(n) - J.dtype.type(av))


def test_closed_form_scalar_open_loop_mean():
    """x+ = a x + b u + w, N = 2, open loop: J = (q x0^2 + r l0^2) / 2 + (q x1^2 + r l1^2) / 2 + qf x2^2 / 2 with x1 = a x0 + b l0 + w0,
    x2 = a x1 + b l1 + w1, so dJ/dl1 = r l1 + qf b x2 and dJ/dl0 = r l0 + q b x1 + qf a b x2; the sample mean of those, written out."""
    case = pg.ScalarLQ()
    a, b, q, r, qf, _ = case.p
    x0, l = np.array([0.7]), np.array([[0.3], [-0.2]])
    K = 64
    mod = pg.model(case, x0, l, None, K, SEED, thetas=[0.0])
    x1, x2 = mod["x"][:, 1, 0], mod["x"][:, 2, 0]
    want = np.array([(r * l[0, 0] + q * b * x1 + qf * a * b * x2).mean(), (r * l[1, 0] + qf * b * x2).mean()])
    assert mod["grad_L"] is None and mod["n_nonfinite"] == 0
    assert np.abs(mod["grad_l"][0, :, 0] - want).max() <= 8 * EPS * np.abs(want).max()


def test_standard_error_at_theta_zero_is_the_sample_standard_deviation():
    case, N, K = pg.Pendulum(), 3, 200
    x_nom, l, L = pg.policy(case, N)
    mod = pg.model(case, x_nom, l, L, K, SEED, thetas=[0.0])
    want = mod["gu"].std(axis=0) / np.sqrt(K)                         # (population form: sum p^2 (g - mean)^2 with p = 1 / K)
    assert np.abs(mod["grad_l_se"][0] - want).max() <= 1e-9 * want.max()


def test_nonfinite_sensitivities_are_left_out_of_numerator_and_denominator():
    case = pg.SqrtCost([0.5, 0.5, 0.0, 0.0, 1.0, 0.3])
    x_nom, l, L = np.array([[1.0], [1.0], [0.0]]), np.array([[1.0], [0.0]]), np.array([[[0.5]], [[0.5]]])
    mod = pg.model(case, x_nom, l, L, 64, SEED, thetas=[0.0])
    bad = ~mod["fin"]
    assert 0 < mod["n_nonfinite"] == bad.sum() < 64 and np.isfinite(mod["J"]).all()
    assert np.array_equal(bad, mod["u"][:, 1, 0] == 0.0)
    keep = ~bad
    assert np.allclose(mod["grad_l"][0], mod["gu"][keep].mean(axis=0), rtol=1e-13, atol=0)
