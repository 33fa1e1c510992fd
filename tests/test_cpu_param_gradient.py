"""rat_policy_param_gradient / rat_policy_tail_param_gradient without a device: the exports, the compile-only check and its refusals, the
claim that a RAT_USER_PARAMS_AD source still compiles as every other kernel kind, and the NumPy model (tests/param_gradient_model.py)
against Richardson-extrapolated longdouble central differences in p and x_0, a closed form, the u + p identity and the exclusion of
non-finite rollouts."""
import ctypes as C

import numpy as np
import pytest

import param_gradient_model as pp
import policy_gradient_model as pgm
import ratilqr.jl_amd as rat
import tail_risk_model as trm
import worst_case_model as wcm
from ratilqr.jl_amd import _native as nv

EPS = np.finfo(np.float64).eps
K_FD, SEED = 256, 11

CASES = {
    "scalar": lambda: pp.ScalarLQ(), "sqrt": lambda: pp.SqrtParam(), "lin2": lambda: pp.Lin2(), "pendulum": lambda: pp.Pendulum(),
    "pendulum_jac": lambda: pp.Pendulum(source=pp.PEND_AD_JAC), "lq5x3p17": lambda: pp.LqCubic(5, 3, 17),
    "lq12x4p32": lambda: pp.LqCubic(12, 4, 32), "lq5x3p15": lambda: pp.LqCubic(5, 3, 15), "lq5x3p16": lambda: pp.LqCubic(5, 3, 16),
    "uplusp": lambda: pp.UPlusP(),
}


def test_exports_and_prototypes():
    lib = nv.lib()
    for name in ("rat_policy_param_gradient", "rat_policy_tail_param_gradient", "rat_policy_param_gradient_check"):
        assert name in nv.EXPORTS and hasattr(lib, name)
    assert len(lib.rat_policy_param_gradient.argtypes) == 11 and lib.rat_policy_param_gradient.argtypes[-1] == C.POINTER(C.c_int64)
    assert len(lib.rat_policy_tail_param_gradient.argtypes) == 9 and len(lib.rat_policy_param_gradient_check.argtypes) == 6
    assert hasattr(rat.Context, "policy_param_gradient") and hasattr(rat.Context, "policy_tail_param_gradient")


@pytest.mark.parametrize("name", list(CASES))
def test_check_compiles_the_cases(name):
    case = CASES[name]()
    rat.policy_param_gradient_check(case.source, **case.dims(), n_params=case.n_params)


def test_check_compiles_without_parameters():
    case = pp.Pendulum()                                              # (n_params = 0: lambda_0 alone, p is never seeded)
    rat.policy_param_gradient_check(case.source, **case.dims(), n_params=0)


def test_check_refuses_with_the_documented_codes():
    pend = pp.Pendulum()
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_UNSUPPORTED.*does not define RAT_USER_PARAMS_AD"):
        rat.policy_param_gradient_check(pgm.Pendulum().source, 2, 1, 2, 0, 3)
    plain = pend.source.replace("template <class T, class P>", "template <class T>").replace("const P *p", "const double *p")
    assert "RAT_USER_PARAMS_AD" in plain
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_ARG.*does not compile.*rat_user_") as e:
        rat.policy_param_gradient_check(plain, 2, 1, 2, 0, 3)
    assert "error:" in str(e.value)                                   # (the compiler's log)
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_UNSUPPORTED.*defines RAT_USER_POLICY"):
        rat.policy_param_gradient_check("#define RAT_USER_POLICY\n" + pend.source, 2, 1, 2, 0, 3)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*n_params = 33 is above 32"):
        rat.policy_param_gradient_check(pend.source, 2, 1, 2, 0, 33)


@pytest.mark.parametrize("name", list(CASES))
def test_an_opted_in_source_passes_the_existing_checks(name):
    """P deduces to double wherever p arrives as const double *: the source compiles as the policy gradient's adjoint, as the
    Monte-Carlo rollout and as the solver's rollout and linearisation (rat_dual and rat_hdual for T)."""
    case = CASES[name]()
    rat.policy_gradient_check(case.source, **case.dims())
    nv.user_noise_check(case.source, **case.dims())
    nv.source_check(case.source, case.n, case.m)


# ---- the model against central differences of its own sample functionals ----------------------------------------------------------------
def trm_cvar_ld(J, alpha):
    """CVaR_alpha of the sample in the dtype of J, tail_risk_model.direct's rule: v + sum (J - v)+ / (n - n alpha)"""
    n = J.size
    av = np.float64(n) * alpha
    k = int(min(max(np.ceil(av), 1), n))
    v = np.sort(J)[k - 1]
    return v + np.where(J > v, J - v, 0).sum() / (J.dtype.type(n) - J.dtype.type(av))


FUNCTIONALS = {
    "mean": (dict(thetas=[0.0]), lambda J: J.mean()),
    "entropic": (dict(thetas=[0.7]), lambda J: np.log(np.exp(np.longdouble(0.7) * (J - J.max())).mean()) / np.longdouble(0.7) + J.max()),
    "kl": (dict(kl_bounds=[0.05]), lambda J: wcm.direct(np.asarray(J, float), 0.05)["bound"]),
    "cvar": (dict(alphas=[0.9]), lambda J: trm.direct(np.asarray(J, float), 0.9)["cvar"]),
}


def fd_gradient(case, x_nom, l, L, z, F, step, dtype):
    """central differences of F(costs) over every parameter and every component of the initial state (the law stays on x_nom)"""
    P, n = case.n_params, case.n
    gp, gx = np.zeros(P, dtype=dtype), np.zeros(n, dtype=dtype)
    base = case.p.astype(dtype)
    for i in range(P):
        a, b = base.copy(), base.copy()
        a[i] += step; b[i] -= step
        va, vb = (F(pp.rollout(case.at(q), x_nom, l, L, z, dtype)[0]) for q in (a, b))
        gp[i] = (va - vb) / (a[i] - b[i])
    for i in range(n):
        d = np.zeros(n, dtype=dtype)
        d[i] = step
        gx[i] = (F(pp.rollout(case, x_nom, l, L, z, dtype, dx0=d)[0]) - F(pp.rollout(case, x_nom, l, L, z, dtype, dx0=-d)[0])) / (2 * d[i])
    return gp, gx


@pytest.mark.parametrize("name", ["mean", "entropic", "kl", "cvar"])
@pytest.mark.parametrize("cname", ["lin2", "pendulum", "lq5x3p17"])
def test_functionals_match_central_differences_in_extended_precision(cname, name):
    """The rule of the sibling's test of the same name: the central difference is taken in np.longdouble and Richardson-extrapolated,
    D(h) = (4 d(h / 2) - d(h)) / 3; the step is the one of 2^-4, 2^-6, 2^-8, 2^-10 that minimises the reference's own error estimate
    |D(h) - D(h / 2)|; the tolerance is 4 times that estimate plus 64 eps of the largest gradient entry (the float64 model's own sums
    over K = 256 rollouts).  Closed loop, so the x_0 direction is the one the header means: the law stays centred on x_nom_0."""
    case, N = CASES[cname](), 3
    x_nom, l, L = pgm.policy(case, N)
    z = pgm.draws(case, SEED, K_FD, N)
    kw, F = FUNCTIONALS[name]
    mod = pp.model(case, x_nom, l, L, K_FD, SEED, **kw)
    assert mod["n_nonfinite"] == 0
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
    est, h, (gp, gx) = best
    tol = 4 * est + 64 * EPS * float(max(np.abs(gp).max(), np.abs(gx).max()))
    e_p, e_x = float(np.abs(gp - mod["grad_p"][0]).max()), float(np.abs(gx - mod["grad_x0"][0]).max())
    print(f"{cname} {name}: step 2^{int(np.log2(h))}, reference error estimate {est:.3e}, tol {tol:.3e}, errors {e_p:.3e} {e_x:.3e}")
    assert e_p <= tol and e_x <= tol


def test_open_loop_x0_is_the_plain_shift():
    case, N = pp.Pendulum(), 3
    x0, l, _ = pgm.policy(case, N, closed=False)
    z = pgm.draws(case, SEED, 64, N)
    mod = pp.model(case, x0, l, None, 64, SEED, thetas=[0.0])
    h = 2.0 ** -8

    def d(step):
        return fd_gradient(case, x0, l, None, z, lambda J: J.mean(), step, np.longdouble)[1]
    d1, d2 = (4 * d(h / 2) - d(h)) / 3, (4 * d(h / 4) - d(h / 2)) / 3
    tol = 4 * float(np.abs(d1 - d2).max()) + 64 * EPS * float(np.abs(d2).max())
    assert np.abs(d2 - mod["grad_x0"][0]).max() <= tol


def test_closed_form_scalar_open_loop_mean():
    """x+ = a x + b u + w, N = 2, open loop: J = (q x0^2 + r l0^2) / 2 + (q x1^2 + r l1^2) / 2 + qf x2^2 / 2 with x1 = a x0 + b l0 + w0,
    x2 = a x1 + b l1 + w1 and w frozen: dx1/da = x0, dx2/da = x1 + a x0, dx1/db = l0, dx2/db = l1 + a l0, dx1/dx0 = a, dx2/dx0 = a^2; the
    sample means of the derivatives, written out.  sigma moves the noise alone, which is frozen: its entry is exactly 0."""
    case = pp.ScalarLQ()
    a, b, q, r, qf, _ = case.p
    x0, l = np.array([0.7]), np.array([[0.3], [-0.2]])
    K = 64
    mod = pp.model(case, x0, l, None, K, SEED, thetas=[0.0])
    x1, x2 = mod["x"][:, 1, 0], mod["x"][:, 2, 0]
    want_p = np.array([(q * x1 * x0[0] + qf * x2 * (x1 + a * x0[0])).mean(), (q * x1 * l[0, 0] + qf * x2 * (l[1, 0] + a * l[0, 0])).mean(),
                       (0.5 * (x0[0] ** 2 + x1 ** 2)).mean(), 0.5 * (l[0, 0] ** 2 + l[1, 0] ** 2), (0.5 * x2 ** 2).mean(), 0.0])
    want_x = (q * x0[0] + q * x1 * a + qf * x2 * a * a).mean()
    assert mod["n_nonfinite"] == 0 and mod["grad_p"][0, 5] == 0.0
    assert np.abs(mod["grad_p"][0] - want_p).max() <= 8 * EPS * np.abs(want_p).max()
    assert abs(mod["grad_x0"][0, 0] - want_x) <= 8 * EPS * abs(want_x)


@pytest.mark.parametrize("closed", [True, False], ids=["closed", "open"])
def test_u_plus_p_is_the_sum_of_the_policy_gradient_over_the_steps(closed):
    """c and f read u + p, so dJ_k / dp_j = sum_t dJ_k / du_t[j] with the loop closed downstream: grad_p against the sibling model's own
    grad_l, summed over t (two different sums of the same K N terms: 64 eps of the largest)"""
    case, N, K = pp.UPlusP(), 4, 128
    pol = pgm.policy(case, N, closed)
    mod = pp.model(case, *pol, K, SEED, kl_bounds=[0.05], thetas=[0.0, 0.7])
    sib = pgm.model(case, *pol, K, SEED, kl_bounds=[0.05], thetas=[0.0, 0.7])
    assert np.array_equal(mod["J"], sib["J"])
    want = sib["grad_l"].sum(axis=1)
    assert np.abs(mod["grad_p"] - want).max() <= 64 * EPS * np.abs(want).max()


def test_standard_error_at_theta_zero_is_the_sample_standard_deviation():
    case, N, K = pp.Pendulum(), 3, 200
    mod = pp.model(case, *pgm.policy(case, N), K, SEED, thetas=[0.0])
    for key, v in (("grad_p_se", mod["gp"]), ("grad_x0_se", mod["lam0"])):
        want = v.std(axis=0) / np.sqrt(K)
        assert np.abs(mod[key][0] - want).max() <= 1e-9 * want.max()


def test_nonfinite_sensitivities_are_left_out_of_numerator_and_denominator():
    case = pp.SqrtParam()
    x_nom, l, L = np.array([[1.0], [1.0], [0.0]]), np.array([[1.0], [0.0]]), np.array([[[0.5]], [[0.5]]])
    mod = pp.model(case, x_nom, l, L, 64, SEED, thetas=[0.0])
    bad = ~mod["fin"]
    assert 0 < mod["n_nonfinite"] == bad.sum() < 64 and np.isfinite(mod["J"]).all()
    assert np.array_equal(bad, mod["x"][:, 2, 0] == 0.5)              # h = sqrt(|p4 (x_N - 1/2)|) at x_N == 1/2
    assert np.isnan(mod["gp"][bad, 4]).all()                          # h_p: Inf times the zero tangent
    keep = ~bad
    assert np.isfinite(mod["grad_p"]).all() and np.isfinite(mod["grad_x0"]).all()
    assert np.allclose(mod["grad_p"][0], mod["gp"][keep].mean(axis=0), rtol=1e-13, atol=0)
    assert np.allclose(mod["grad_x0"][0], mod["lam0"][keep].mean(axis=0), rtol=1e-13, atol=0)
