"""rat_policy_param_gradient / rat_policy_tail_param_gradient on the device against tests/param_gradient_model.py.

Tolerance of the device-against-model cases: the rule of tests/test_gpu_policy_gradient.py -- MULT = 8 times the distance between the
float64 and the np.longdouble run of the NumPy model on the same case, with a floor of MULT eps times the row's largest component.  The
standard errors are held in their square, with 4 eps sum p^2 v^2 added to the models' distance (the three uncentred terms and the
division, each rounded at eps of that size)."""
import ctypes as C

import numpy as np
import pytest

import param_gradient_model as pp
import policy_gradient_model as pgm
import ratilqr.jl_amd as rat
from ratilqr.jl_amd import _native as nv

pytestmark = pytest.mark.gpu
MULT, EPS, SEED = 8, np.finfo(np.float64).eps, 11
KL, TH, AL = [0.05, np.inf], [0.0, 0.7], [0.0, 0.9]
KS = (1, 3, 4, 5, 63, 64, 65)
_cache = {}


def context(case, N):
    prob = rat.DeviceSourceProblem(case.source, case.n, case.m, N, np.eye(case.n), params=case.p)
    return rat.Context(prob, max_batch=1, device=0)


def evaluate(ctx, case, pol, K, seed=SEED):
    x_nom, l, L = pol
    return ctx.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(case.npn, 0, seed=seed), K=K, want_costs=True)


def reference(key, case, pol, K, **kw):
    """the float64 and the longdouble model of one case, computed once"""
    if key not in _cache:
        _cache[key] = tuple(pp.model(case, *pol, K, SEED, dtype=dt, **kw) for dt in (np.float64, np.longdouble))
    return _cache[key]


def close(name, got, m64, mld, scale=None):
    """every row of got against the float64 model within MULT times the models' own distance (floor: MULT eps of the row's largest entry);
    scale (a standard error: sum p^2 v^2 per entry): the squares are compared, with 4 eps scale added to the distance"""
    for r in range(got.shape[0]):
        if m64[r].size == 0:
            continue
        if np.isnan(m64[r]).all():
            assert np.isnan(got[r]).all(), (name, r)
            continue
        if scale is not None:
            a, b = m64[r] ** 2, mld[r].astype(np.float64) ** 2
            tolv = MULT * (np.abs(a - b) + 4 * EPS * scale[r])
            errv = np.abs(got[r] ** 2 - a)
            print(f"{name} row {r}: square's tolerance {float(tolv.max()):.3e}, device error {float(errv.max()):.3e}")
            assert (errv <= tolv).all(), (name, r, errv, tolv)
            continue
        dist = float(np.abs(m64[r] - mld[r].astype(np.float64)).max())
        tol = MULT * max(dist, EPS * float(np.abs(m64[r]).max()))
        err = float(np.abs(got[r] - m64[r]).max())
        print(f"{name} row {r}: model distance {dist:.3e}, tolerance {tol:.3e}, device error {err:.3e}, error / tolerance {err / tol if tol else 0:.3f}")
        assert err <= tol, (name, r, err, tol)


KEYS = (("grad_p", None), ("grad_x0", None), ("grad_p_se", "p_scale"), ("grad_x0_se", "x0_scale"))


def hold(name, ctx, case, pol, K, key, q=None):
    """one evaluation: both calls against the model, the rows against the trajectory calls' bit for bit"""
    g, t = ctx.policy_param_gradient(kl_bounds=KL, thetas=TH), ctx.policy_tail_param_gradient(AL)
    wt, tt = ctx.policy_worst_case_trajectory(kl_bounds=KL, thetas=TH), ctx.policy_tail_trajectory(AL)
    for part in ("bounds", "thetas"):
        for k in nv.WC_SLOTS:
            assert np.array_equal(g[part][k], wt[part][k], equal_nan=True), (K, part, k)
    for k in nv.TR_SLOTS:
        assert np.array_equal(t[k], tt[k], equal_nan=True), (K, k)
    m64, mld = reference(key + ("wc",), case, pol, K, kl_bounds=KL, thetas=TH, q=q)
    t64, tld = reference(key + ("tail",), case, pol, K, alphas=AL, q=q)
    for k, sc in KEYS:
        got = np.concatenate([g["bounds"][k], g["thetas"][k]])
        close(f"{name} K={K} {k}", got, m64[k], mld[k], m64[sc] if sc else None)
        close(f"{name} K={K} tail {k}", t[k], t64[k], tld[k], t64[sc] if sc else None)
    assert g["thetas"]["n_nonfinite"] == m64["n_nonfinite"] == t["n_nonfinite"]
    return g, t, m64


CASES = [("scalar", lambda: pp.ScalarLQ()), ("pendulum", lambda: pp.Pendulum()), ("pendulum_jac", lambda: pp.Pendulum(source=pp.PEND_AD_JAC)),
         ("lq5x3p17", lambda: pp.LqCubic(5, 3, 17)), ("lq12x4p32", lambda: pp.LqCubic(12, 4, 32))]


@pytest.mark.parametrize("closed", [True, False], ids=["closed", "open"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_device_matches_the_model(name, make, N, closed):
    case = make()
    ctx = context(case, N)
    pol = pgm.policy(case, N, closed)
    for K in KS:
        evaluate(ctx, case, pol, K)
        hold(name, ctx, case, pol, K, (name, N, closed, K))


@pytest.mark.parametrize("NP", [15, 16])
def test_the_boundary_between_the_parameter_tiles(NP):
    case, N, K = pp.LqCubic(5, 3, NP), 3, 5
    ctx, pol = context(case, N), pgm.policy(case, N)
    evaluate(ctx, case, pol, K)
    g, _, m64 = hold(f"lq5x3p{NP}", ctx, case, pol, K, ("tiles", NP))
    assert g["thetas"]["grad_p"].shape == (2, NP) and (m64["grad_p"][2] != 0).all()   # (every parameter is live in the theta = 0 row)


def test_across_a_chunk_boundary():
    case, N, K = pp.Lin2(), 2, 65536 + 5
    ctx, pol = context(case, N), pgm.policy(case, N)
    evaluate(ctx, case, pol, K)
    g, t = ctx.policy_param_gradient(thetas=TH), ctx.policy_tail_param_gradient(AL)
    m64, mld = reference(("chunk", "wc"), case, pol, K, thetas=TH)
    t64, tld = reference(("chunk", "tail"), case, pol, K, alphas=AL)
    for k, sc in KEYS:
        close(f"chunk {k}", g["thetas"][k], m64[k], mld[k], m64[sc] if sc else None)
        close(f"chunk tail {k}", t[k], t64[k], tld[k], t64[sc] if sc else None)


def test_same_bits_twice_and_a_row_alone():
    case, N, K = pp.LqCubic(5, 3, 17), 2, 65
    ctx, pol = context(case, N), pgm.policy(case, N)
    evaluate(ctx, case, pol, K)
    a, b = ctx.policy_param_gradient(kl_bounds=KL, thetas=TH), ctx.policy_param_gradient(kl_bounds=KL, thetas=TH)
    alone = ctx.policy_param_gradient(thetas=[0.7])
    ta, tb, talone = ctx.policy_tail_param_gradient(AL), ctx.policy_tail_param_gradient(AL), ctx.policy_tail_param_gradient([0.9])
    for k, _ in KEYS:
        for part in ("bounds", "thetas"):
            assert np.array_equal(a[part][k], b[part][k])
        assert np.array_equal(alone["thetas"][k][0], a["thetas"][k][1])
        assert np.array_equal(ta[k], tb[k]) and np.array_equal(talone[k][0], ta[k][1])
    assert np.array_equal(ta["grad_p"][0], a["thetas"]["grad_p"][0])  # alpha = 0 is the theta = 0 row


def test_grad_p_against_central_differences_of_the_devices_own_mean():
    """The linear source at (2, 1), N = 3, K = 64: MEAN is at most quadratic in each parameter (an additive drift, a cost weight), so a
    central difference of rat_policy_evaluate_noise's MEAN under rat_problem_set_params(p +- step) and the same seed has no truncation
    error; its rounding is that of two means of size |MEAN| over 2 step: tolerance 8 eps |MEAN| / step, step = 2^-10, as in the sibling."""
    case, N, K, step = pp.Lin2(), 3, 64, 2.0 ** -10
    ctx, pol = context(case, N), pgm.policy(case, N)
    mean0 = evaluate(ctx, case, pol, K)["mean"]
    g = ctx.policy_param_gradient(thetas=[0.0])["thetas"]["grad_p"][0]
    tol = 8 * EPS * abs(mean0) / step
    for i in range(case.n_params):
        a, b = case.p.copy(), case.p.copy()
        a[i] += step; b[i] -= step
        ctx.set_params(a)
        ma = evaluate(ctx, case, pol, K)["mean"]
        ctx.set_params(b)
        mb = evaluate(ctx, case, pol, K)["mean"]
        fd = (ma - mb) / (a[i] - b[i])
        print(f"p[{i}]: fd {fd:.15e} device {g[i]:.15e} tol {tol:.2e}")
        assert abs(fd - g[i]) <= tol, i


def test_grad_x0_open_loop_against_central_differences_of_the_devices_own_mean():
    """The same way by shifting the initial state of an open-loop evaluation (row 0 of x_nom): MEAN is quadratic in x_0."""
    case, N, K, step = pp.Lin2(), 3, 64, 2.0 ** -10
    ctx = context(case, N)
    x0, l, _ = pgm.policy(case, N, closed=False)
    mean0 = evaluate(ctx, case, (x0, l, None), K)["mean"]
    g = ctx.policy_param_gradient(thetas=[0.0])["thetas"]["grad_x0"][0]
    tol = 8 * EPS * abs(mean0) / step
    for i in range(case.n):
        a, b = x0.copy(), x0.copy()
        a[i] += step; b[i] -= step
        fd = (evaluate(ctx, case, (a, l, None), K)["mean"] - evaluate(ctx, case, (b, l, None), K)["mean"]) / (a[i] - b[i])
        print(f"x0[{i}]: fd {fd:.15e} device {g[i]:.15e} tol {tol:.2e}")
        assert abs(fd - g[i]) <= tol, i


def test_parameter_sampling_differentiates_at_every_rollouts_own_q():
    case, N, K = pp.Pendulum(source=pp.PEND_AD_JAC_SAMPLED), 3, 65
    ctx, pol = context(case, N), pgm.policy(case, N)
    ctx.set_param_sampling(rat.ParamSampling(2, 1))
    evaluate(ctx, case, pol, K)
    q = ctx.sample_params(K, seed=SEED)
    assert q.shape == (K, 3) and (q != case.p).all()
    hold("sampled", ctx, case, pol, K, ("sampled",), q=q)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*parameter sampling is on"):
        ctx.policy_gradient(thetas=[0.0])                             # (the sibling's refusal stands)


def test_nonfinite_sensitivities_are_counted_and_left_out():
    case = pp.SqrtParam()
    pol = (np.array([[1.0], [1.0], [0.0]]), np.array([[1.0], [0.0]]), np.array([[[0.5]], [[0.5]]]))
    ctx, K = context(case, 2), 64
    assert evaluate(ctx, case, pol, K)["n_ok"] == K
    g, t = ctx.policy_param_gradient(thetas=TH), ctx.policy_tail_param_gradient([0.0])
    m64, mld = reference(("sqrt",), case, pol, K, thetas=TH)
    assert 0 < m64["n_nonfinite"] < K and g["thetas"]["n_nonfinite"] == m64["n_nonfinite"] == t["n_nonfinite"]
    for k, sc in KEYS:
        assert np.isfinite(g["thetas"][k]).all()
        close(f"sqrt {k}", g["thetas"][k], m64[k], mld[k], m64[sc] if sc else None)
    assert np.array_equal(t["grad_p"][0], g["thetas"]["grad_p"][0])


def test_refusals_leave_the_handle_usable():
    case, N, K = pp.Pendulum(), 3, 16
    ctx, pol = context(case, N), pgm.policy(case, N)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no evaluation to replay"):
        ctx.policy_param_gradient(thetas=[0.0])
    evaluate(ctx, case, pol, K)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*nothing to compute"):
        ctx.policy_param_gradient()
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*alpha must be in"):
        ctx.policy_tail_param_gradient([1.0])
    good = ctx.policy_param_gradient(thetas=[0.0])["thetas"]["grad_p"]
    assert np.isfinite(good).all()
    # a family: write the model as source
    prob, x0, u = rat.synthetic_lq_problem()
    cf = rat.Context(prob, max_batch=1, device=0)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*write the model as source"):
        cf.policy_param_gradient(thetas=[0.0])
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*write the model as source"):
        cf.policy_tail_param_gradient([0.5])
    # a source without the define (sampling off): the other calls serve it, this one names its reason
    plain = pgm.Pendulum()
    cp = context(plain, N)
    evaluate(cp, plain, pol, K)
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_UNSUPPORTED.*does not define RAT_USER_PARAMS_AD"):
        cp.policy_param_gradient(thetas=[0.0])
    assert np.isfinite(cp.policy_gradient(thetas=[0.0])["thetas"]["grad_l"]).all()
    # no parameters: grad_x0 alone is served, grad_p_out is refused
    none = pp.Pendulum()
    none.source = none.source.replace("/ p[0]", "/ 1.3").replace("p[1] *", "0.1 *").replace("p[2] *", "0.8 *")
    c0 = rat.Context(rat.DeviceSourceProblem(none.source, 2, 1, N, np.eye(2), params=np.zeros(0)), max_batch=1, device=0)
    evaluate(c0, none, pol, K)
    g0 = c0.policy_param_gradient(thetas=[0.0])["thetas"]
    assert g0["grad_p"].shape == (1, 0)                               # (the same model with its parameters as literals)
    assert np.allclose(g0["grad_x0"], ctx.policy_param_gradient(thetas=[0.0])["thetas"]["grad_x0"], rtol=1e-12, atol=0)
    th, rows, buf, gx = np.zeros(1), np.zeros(nv.WC_NSTAT), np.zeros(4), np.full(2, 7.0)
    rc = nv.lib().rat_policy_param_gradient(c0.h, None, C.c_int32(0), nv.P(th), C.c_int32(1), nv.P(rows), nv.P(buf), None, nv.P(gx), None, None)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*no parameters"):
        nv.check(rc)
    assert (gx == 7.0).all()
    # the replay guard
    ctx.set_params([1.3, 0.12, 0.8])
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*changed since the evaluation"):
        ctx.policy_param_gradient(thetas=[0.0])
    evaluate(ctx, case, pol, K)
    assert not np.array_equal(ctx.policy_param_gradient(thetas=[0.0])["thetas"]["grad_p"], good)
