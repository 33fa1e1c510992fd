"""rat_policy_gradient / rat_policy_tail_gradient on the device against tests/policy_gradient_model.py.

Tolerance of the device-against-model cases: MULT times the distance between the float64 and the np.longdouble run of the NumPy model on
the same case (measured on the CPU, recorded per case in profiles/policy_gradient.md), with a floor of MULT eps times the row's largest
component where that distance is 0.  MULT = 8: the device is a third float64 evaluation of the same sums -- another summation order (four
rollouts per MFMA, 32 wavefront partials, 8 slots), fused multiply-adds in f, c and the adjoint's dot products, the device's sin / exp --
so its distance from the model is of the size of the model's own distance from extended precision, a few times over; a single digit.
The standard error is held in its square: the header forms it from uncentred sums, (sum y^2 gu^2 - 2 mean sum y^2 gu + mean^2 sum y^2) /
(sum y)^2, three terms of size S = sum p^2 gu^2 each rounded at eps, so its square carries an absolute error of a few eps S whatever the
variance is (on a saturated row, one rollout with all the weight, the variance is 0 and the square root of that error, 1e-8 gu, is all
there is).  The square's tolerance is MULT times (the models' distance in the square + 4 eps S): 4 for the three terms and the division."""
import numpy as np
import pytest

import policy_gradient_model as pg
import ratilqr.jl_amd as rat
import user_noise_model as un

pytestmark = pytest.mark.gpu
MULT, EPS, SEED = 8, np.finfo(np.float64).eps, 11
KL, TH, AL = [0.05, np.inf], [0.0, 0.7], [0.0, 0.9]
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
        _cache[key] = tuple(pg.model(case, *pol, K, SEED, dtype=dt, **kw) for dt in (np.float64, np.longdouble))
    return _cache[key]


def close(name, got, m64, mld, scale=None):
    """every row of got against the float64 model within MULT times the models' own distance (floor: MULT eps of the row's largest entry);
    scale (the standard error: sum p^2 gu^2 per entry): the squares are compared, with 4 eps scale added to the distance"""
    for r in range(got.shape[0]):
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
        print(f"{name} row {r}: model distance {dist:.3e}, tolerance {tol:.3e}, device error {err:.3e}")
        assert err <= tol, (name, r, err, tol)


CASES = [("scalar", lambda: pg.ScalarLQ(), 1), ("pend3", lambda: pg.Pendulum(), 3), ("pend10", lambda: pg.Pendulum(), 10),
         ("lq5x3", lambda: pg.LqCubic(5, 3, 2), 2), ("lq12x4", lambda: pg.LqCubic(12, 4, 3), 3)]


@pytest.mark.parametrize("closed", [True, False], ids=["closed", "open"])
@pytest.mark.parametrize("name,make,N", CASES, ids=[c[0] for c in CASES])
def test_device_matches_the_model(name, make, N, closed):
    case = make()
    ctx = context(case, N)
    pol = pg.policy(case, N, closed)
    for K in (1, 3, 4, 5, 63, 64, 65):
        evaluate(ctx, case, pol, K)
        wc, tr = ctx.policy_worst_case(kl_bounds=KL, thetas=TH), ctx.policy_tail_risk(AL)
        g, t = ctx.policy_gradient(kl_bounds=KL, thetas=TH), ctx.policy_tail_gradient(AL)
        for part in ("bounds", "thetas"):                             # rows_out: the rows of rat_policy_worst_case, bit for bit
            for k in wc[part]:
                assert np.array_equal(g[part][k], wc[part][k], equal_nan=True), (K, part, k)
        for k in ("alpha", "var", "cvar", "cvar_se", "tail_n", "ess", "kl", "flag"):
            assert np.array_equal(t[k], tr[k], equal_nan=True), (K, k)
        m64, mld = reference((name, closed, K, "wc"), case, pol, K, kl_bounds=KL, thetas=TH)
        t64, tld = reference((name, closed, K, "tail"), case, pol, K, alphas=AL)
        got_l = np.concatenate([g["bounds"]["grad_l"], g["thetas"]["grad_l"]])
        close(f"{name} K={K} grad_l", got_l, m64["grad_l"], mld["grad_l"])
        close(f"{name} K={K} tail grad_l", t["grad_l"], t64["grad_l"], tld["grad_l"])
        close(f"{name} K={K} grad_l_se", np.concatenate([g["bounds"]["grad_l_se"], g["thetas"]["grad_l_se"]]), m64["grad_l_se"], mld["grad_l_se"], m64["se_scale"])
        if closed:
            close(f"{name} K={K} grad_L", np.concatenate([g["bounds"]["grad_L"], g["thetas"]["grad_L"]]), m64["grad_L"], mld["grad_L"])
            close(f"{name} K={K} tail grad_L", t["grad_L"], t64["grad_L"], tld["grad_L"])
        else:
            assert g["thetas"]["grad_L"] is None and t["grad_L"] is None
        assert g["thetas"]["n_nonfinite"] == 0 and t["n_nonfinite"] == 0


def test_across_a_chunk_boundary():
    case, N, K = pg.Lin2(), 2, 65536 + 5
    ctx, pol = context(case, N), pg.policy(case, N)
    evaluate(ctx, case, pol, K)
    g, t = ctx.policy_gradient(thetas=TH), ctx.policy_tail_gradient(AL)
    m64, mld = reference(("chunk", "wc"), case, pol, K, thetas=TH)
    t64, tld = reference(("chunk", "tail"), case, pol, K, alphas=AL)
    for k in ("grad_l", "grad_L", "grad_l_se"):
        close(f"chunk {k}", g["thetas"][k], m64[k], mld[k], m64["se_scale"] if k == "grad_l_se" else None)
        close(f"chunk tail {k}", t[k], t64[k], tld[k], t64["se_scale"] if k == "grad_l_se" else None)


def test_device_against_central_differences_of_its_own_mean():
    """The linear source with a quadratic cost at (2, 1), N = 3, K = 64: MEAN is quadratic in the policy, so a central difference of
    rat_policy_evaluate_noise's MEAN under the same seed has no truncation error; its rounding is that of two means of size |MEAN|, eps
    each times a factor 8 for the K + N sums behind them, over 2 step: tolerance 8 eps |MEAN| / step, step = 2^-10."""
    case, N, K, step = pg.Lin2(), 3, 64, 2.0 ** -10
    ctx = context(case, N)
    x_nom, l, L = pg.policy(case, N)
    mean0 = evaluate(ctx, case, (x_nom, l, L), K)["mean"]
    g = ctx.policy_gradient(thetas=[0.0])["thetas"]
    tol = 8 * EPS * abs(mean0) / step
    for arr, key in ((l, "grad_l"), (L, "grad_L")):
        for idx in np.ndindex(*arr.shape):
            a, b = arr.copy(), arr.copy()
            a[idx] += step; b[idx] -= step
            pa, pb = ((x_nom, a, L), (x_nom, b, L)) if key == "grad_l" else ((x_nom, l, a), (x_nom, l, b))
            fd = (evaluate(ctx, case, pa, K)["mean"] - evaluate(ctx, case, pb, K)["mean"]) / (a[idx] - b[idx])
            print(f"{key}{idx}: fd {fd:.15e} device {g[key][(0,) + idx]:.15e} tol {tol:.2e}")
            assert abs(fd - g[key][(0,) + idx]) <= tol, (key, idx)


def test_jacobian_hook_gives_the_models_gradient():
    case, N, K = pg.Pendulum(source=pg.PEND_JAC), 3, 65
    ctx, pol = context(case, N), pg.policy(case, N)
    evaluate(ctx, case, pol, K)
    g = ctx.policy_gradient(kl_bounds=[0.05], thetas=TH)
    m64, mld = reference(("jac",), case, pol, K, kl_bounds=[0.05], thetas=TH)
    for k in ("grad_l", "grad_L"):
        close(f"jacobian {k}", np.concatenate([g["bounds"][k], g["thetas"][k]]), m64[k], mld[k])


def test_nonfinite_sensitivities_are_counted_and_left_out():
    case = pg.SqrtCost([0.5, 0.5, 0.0, 0.0, 1.0, 0.3])
    pol = (np.array([[1.0], [1.0], [0.0]]), np.array([[1.0], [0.0]]), np.array([[[0.5]], [[0.5]]]))
    ctx, K = context(case, 2), 64
    ev = evaluate(ctx, case, pol, K)
    assert ev["n_ok"] == K
    g, t = ctx.policy_gradient(thetas=TH), ctx.policy_tail_gradient([0.0])
    m64, mld = reference(("sqrt",), case, pol, K, thetas=TH)
    assert 0 < m64["n_nonfinite"] < K and g["thetas"]["n_nonfinite"] == m64["n_nonfinite"] == t["n_nonfinite"]
    for k in ("grad_l", "grad_L", "grad_l_se"):
        assert np.isfinite(g["thetas"][k]).all()
        close(f"sqrt {k}", g["thetas"][k], m64[k], mld[k], m64["se_scale"] if k == "grad_l_se" else None)
    assert np.array_equal(t["grad_l"][0], g["thetas"]["grad_l"][0])   # alpha = 0 is the theta = 0 row


def test_same_bits_twice_and_a_row_alone():
    case, N, K = pg.LqCubic(5, 3, 2), 2, 65
    ctx, pol = context(case, N), pg.policy(case, N)
    evaluate(ctx, case, pol, K)
    before = ctx.policy_worst_case_trajectory(kl_bounds=[0.05], thetas=TH)
    a, b = ctx.policy_gradient(kl_bounds=KL, thetas=TH), ctx.policy_gradient(kl_bounds=KL, thetas=TH)
    alone = ctx.policy_gradient(thetas=[0.7])
    ta, tb, talone = ctx.policy_tail_gradient(AL), ctx.policy_tail_gradient(AL), ctx.policy_tail_gradient([0.9])
    after = ctx.policy_worst_case_trajectory(kl_bounds=[0.05], thetas=TH)
    for k in ("grad_l", "grad_L", "grad_l_se"):
        for part in ("bounds", "thetas"):
            assert np.array_equal(a[part][k], b[part][k])
        assert np.array_equal(alone["thetas"][k][0], a["thetas"][k][1])
        assert np.array_equal(ta[k], tb[k]) and np.array_equal(talone[k][0], ta[k][1])
    for part in ("bounds", "thetas"):                                 # the existing replay's outputs are what they were
        for k in before[part]:
            assert np.array_equal(before[part][k], after[part][k], equal_nan=True), (part, k)


def test_refusals_leave_the_handle_usable():
    case, N, K = pg.Pendulum(), 3, 16
    ctx, pol = context(case, N), pg.policy(case, N)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no evaluation to replay"):
        ctx.policy_gradient(thetas=[0.0])
    evaluate(ctx, case, pol, K)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*nothing to compute"):
        ctx.policy_gradient()
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*alpha must be in"):
        ctx.policy_tail_gradient([1.0])
    good = ctx.policy_gradient(thetas=[0.0])["thetas"]["grad_l"]
    # rows x N above the cap: 16 + 16 rows at N = 106 is 3392 > 3360
    big = pg.Pendulum()
    cb, pb = context(big, 106), pg.policy(big, 106)
    evaluate(cb, big, pb, 4)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rows x N = 3392 is above 3360"):
        cb.policy_gradient(kl_bounds=np.full(16, 0.1), thetas=np.full(16, 0.5))
    assert np.isfinite(cb.policy_gradient(thetas=[0.0])["thetas"]["grad_l"]).all()
    # a family: write the model as source
    prob, x0, u = rat.synthetic_lq_problem()
    cf = rat.Context(prob, max_batch=1, device=0)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*write the model as source"):
        cf.policy_gradient(thetas=[0.0])
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*write the model as source"):
        cf.policy_tail_gradient([0.5])
    # a source with rat_user_policy
    hook = "#define RAT_USER_POLICY\n__device__ void rat_user_policy(int k, const double *x, const double *u_prev, double *u, const double *p) {}\n"
    cp = pg.Pendulum(source=hook + un.PEND_DIAG)
    cc = context(cp, N)
    evaluate(cc, cp, pol, K)
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_UNSUPPORTED.*defines RAT_USER_POLICY"):
        cc.policy_gradient(thetas=[0.0])
    assert cc.policy_worst_case_trajectory(thetas=[0.0])["thetas"]["mean_x"].shape == (1, N + 1, 2)
    # what the rollouts run changed behind the evaluation (the policy pack on the device is the evaluation's own, so the parameters are
    # what a caller can change): the replay guard refuses, and an evaluation later the call serves again
    assert np.array_equal(ctx.policy_gradient(thetas=[0.0])["thetas"]["grad_l"], good)
    ctx.set_params([0.1, 0.07, 0.1])
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*changed since the evaluation"):
        ctx.policy_gradient(thetas=[0.0])
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*changed since the evaluation"):
        ctx.policy_tail_gradient([0.5])
    evaluate(ctx, case, pol, K)
    assert not np.array_equal(ctx.policy_gradient(thetas=[0.0])["thetas"]["grad_l"], good)
    # parameter sampling switched on
    import user_params_model as upm
    cs = pg.Pendulum(source=upm.source(un.PEND_DIAG, "scale", 1, 2, 0, 0.0))
    cx = context(cs, N)
    cx.set_param_sampling(rat.ParamSampling(upm.PARAM_NORMALS, upm.PARAM_UNIFORMS))
    evaluate(cx, cs, pol, K)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*parameter sampling is on"):
        cx.policy_gradient(thetas=[0.0])
    cx.set_param_sampling(None)
    evaluate(cx, cs, pol, K)
    assert np.isfinite(cx.policy_gradient(thetas=[0.0])["thetas"]["grad_l"]).all()


def test_an_empty_sample_is_nan_and_ok():
    case, N, K = pg.Pendulum(source=un.PEND_NAN, p=(0.1, np.nan)), 3, 8
    case.npn = 1
    ctx, pol = context(case, N), pg.policy(case, N)
    ev = evaluate(ctx, case, pol, K)                                  # every draw NaN: every rollout a DomainError
    assert ev["n_ok"] == 0
    g, t = ctx.policy_gradient(kl_bounds=[0.1], thetas=[0.0]), ctx.policy_tail_gradient([0.5])
    assert np.isnan(g["thetas"]["grad_l"]).all() and np.isnan(g["bounds"]["grad_L"]).all() and np.isnan(t["grad_l"]).all()
    assert g["thetas"]["n_nonfinite"] == 0
