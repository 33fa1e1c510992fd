"""rat_policy_margin_gradient on the device against tests/margin_gradient_model.py.

Tolerance of the device-against-model cases, the method of tests/test_gpu_policy_gradient.py: MULT = 8 times the distance between the
float64 and the np.longdouble run of the NumPy model on the same case (recorded per case in profiles/policy_margin_gradient.md), with a
floor of MULT eps times the row's largest component where that distance is 0; the standard error is compared in its square with 4 eps
sum p^2 gu^2 added to the distance (the uncentred form subtracts three terms of that size).  The device is a third float64 evaluation of
the same sums: another summation order, fused multiply-adds in f and in the dot products with lambda, g_z at t* summed over the padded
tile.  The tail's membership and the arg-max step are discrete: tests/test_cpu_margin_gradient.py checks, without a device, that the two
models agree on both for every case here, so no case is skipped on those grounds; the device's own arg-max steps are not visible, its
margins are (the rows), and those are held bit for bit against rat_policy_events' below."""
import numpy as np
import pytest

import margin_gradient_model as mg
import policy_gradient_model as pg
import ratilqr.jl_amd as rat
import user_noise_model as un

pytestmark = pytest.mark.gpu
MULT, EPS, SEED, AL = 8, np.finfo(np.float64).eps, mg.SEED, mg.ALPHAS
ROW_KEYS = ("alpha", "var", "cvar", "cvar_se", "tail_n", "ess", "kl", "flag")
GRAD_KEYS = ("grad_l", "grad_L", "grad_l_se")


def context(case, N):
    prob = rat.DeviceSourceProblem(case.source, case.n, case.m, N, np.eye(case.n), params=case.p)
    return rat.Context(prob, max_batch=1, device=0)


def evaluate(ctx, case, pol, K, seed=SEED):
    x_nom, l, L = pol
    return ctx.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(case.npn, 0, seed=seed), K=K, want_costs=True)


def call(ctx, evs, alphas=AL):
    return ctx.policy_margin_gradient([mg.to_rat(rat, e) for e in evs], alphas)


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


def close_event(name, got, m64, mld, e, closed=True):
    close(f"{name} grad_l", got["grad_l"], m64["grad_l"][e], mld["grad_l"][e])
    close(f"{name} grad_l_se", got["grad_l_se"], m64["grad_l_se"][e], mld["grad_l_se"][e], m64["se_scale"][e])
    if closed:
        close(f"{name} grad_L", got["grad_L"], m64["grad_L"][e], mld["grad_L"][e])
    else:
        assert got["grad_L"] is None
    assert got["n_nonfinite"] == m64["n_nonfinite"][e]


def same_bits(a, b):
    for k in ROW_KEYS + GRAD_KEYS:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["n_nonfinite"] == b["n_nonfinite"]


@pytest.mark.parametrize("closed", [True, False], ids=["closed", "open"])
@pytest.mark.parametrize("name,make,N", mg.CASES, ids=[c[0] for c in mg.CASES])
def test_device_matches_the_model(name, make, N, closed):
    """Events: four at once mixing both kinds (four_events: a linear one with a window of one step at t = N, a quadratic one over the
    whole window 0 .. N, a linear one over 0 .. N - 1, a quadratic one over 1 .. N) and the same four one at a time -- the first two of
    those are the single linear and the single quadratic case; a row's bits must not depend on the other events of the call."""
    case = make()
    ctx = context(case, N)
    pol = pg.policy(case, N, closed)
    evs = mg.four_events(case, N)
    for K in mg.KS:
        evaluate(ctx, case, pol, K)
        m64, mld = mg.reference((name, closed, K), case, pol, K, evs)
        joint = call(ctx, evs)
        assert len(joint) == 4
        for e in range(4):
            close_event(f"{name} K={K} event {e}", joint[e], m64, mld, e, closed)
            alone = call(ctx, [evs[e]])
            assert len(alone) == 1
            same_bits(alone[0], joint[e])


def test_rows_are_tail_risk_of_the_margins_bit_for_bit():
    case, N, K = pg.LqCubic(5, 3, 2), 2, 65
    ctx, other, pol = context(case, N), context(case, N), pg.policy(case, N)
    evs = mg.four_events(case, N)
    evaluate(ctx, case, pol, K)
    evaluate(other, case, pol, K)
    before = ctx.policy_tail_gradient(AL)
    got = call(ctx, evs)
    margins = other.policy_events([mg.to_rat(rat, e) for e in evs], thetas=[0.0], want_margins=True)["margins"]
    for e in range(4):
        want = other.policy_tail_risk(AL, costs=margins[e])           # (uploaded costs end `other`'s evaluation: hence a second context)
        for k in ROW_KEYS:
            assert np.array_equal(got[e][k], want[k], equal_nan=True), (e, k)
    after = ctx.policy_tail_gradient(AL)                              # the first context's evaluation is still replayable, to the same bits
    for k in ROW_KEYS + GRAD_KEYS:
        assert np.array_equal(before[k], after[k], equal_nan=True), k


def test_across_a_chunk_boundary():
    case, N, K = pg.Lin2(), 2, 65536 + 5
    ctx, pol = context(case, N), pg.policy(case, N)
    evs = [mg.linear_event(case, N, 21, N)]
    evaluate(ctx, case, pol, K)
    got = call(ctx, evs)
    m64, mld = mg.reference(("chunk",), case, pol, K, evs)
    close_event("chunk", got[0], m64, mld, 0)


def test_jacobian_hook_gives_the_models_gradient():
    case, N, K = pg.Pendulum(source=pg.PEND_JAC), 3, 65
    ctx, pol = context(case, N), pg.policy(case, N)
    evs = mg.four_events(case, N)
    evaluate(ctx, case, pol, K)
    got = call(ctx, evs)
    m64, mld = mg.reference(("jac",), case, pol, K, evs)
    for e in range(4):
        close_event(f"jacobian event {e}", got[e], m64, mld, e)


def test_device_against_central_differences_of_its_own_margin_mean():
    """The linear source at (2, 1), N = 3, K = 64 and a linear event with t_lo == t_hi = N: per rollout M_k = a' x_N + b is affine in
    every single entry of l and of L (x_N is multilinear in the gains of different steps), so a central difference of
    rat_policy_events' MARGIN_MEAN (theta = 0 row) under the same seed has no truncation error.  Its rounding: each MARGIN_MEAN is a
    sum of K margins of size |M_k| -- not of size |mean|, the margins change sign and their mean can be small -- each rounded at eps, a
    factor 8 for the N steps of sums behind a margin and the K-term mean, two of them over 2 step: tolerance 8 eps mean|M_k| / step with
    step = 2^-10."""
    case, N, K, step = pg.Lin2(), 3, 64, 2.0 ** -10
    ctx = context(case, N)
    x_nom, l, L = pg.policy(case, N)
    ev = mg.linear_event(case, N, 21, N)
    rev = [mg.to_rat(rat, ev)]

    def margin_mean(pol):
        evaluate(ctx, case, pol, K)
        return ctx.policy_events(rev, thetas=[0.0], want_margins=True)
    base = margin_mean((x_nom, l, L))
    g = call(ctx, [ev], [0.0])[0]
    tol = 8 * EPS * float(np.abs(base["margins"][0]).mean()) / step
    for arr, key in ((l, "grad_l"), (L, "grad_L")):
        for idx in np.ndindex(*arr.shape):
            a, b = arr.copy(), arr.copy()
            a[idx] += step; b[idx] -= step
            pa, pb = ((x_nom, a, L), (x_nom, b, L)) if key == "grad_l" else ((x_nom, l, a), (x_nom, l, b))
            fa, fb = (margin_mean(p)["thetas"]["margin_mean"][0, 0] for p in (pa, pb))
            fd = (fa - fb) / (a[idx] - b[idx])
            print(f"{key}{idx}: fd {fd:.15e} device {g[key][(0,) + idx]:.15e} tol {tol:.2e}")
            assert abs(fd - g[key][(0,) + idx]) <= tol, (key, idx)


def test_same_bits_twice_and_the_other_replays_are_undisturbed():
    case, N, K = pg.LqCubic(5, 3, 2), 2, 65
    ctx, pol = context(case, N), pg.policy(case, N)
    evs = mg.four_events(case, N)
    evaluate(ctx, case, pol, K)
    before = ctx.policy_gradient(kl_bounds=[0.05], thetas=[0.0, 0.7])
    costs_before = ctx.policy_tail_risk(AL)
    a, b = call(ctx, evs), call(ctx, evs)
    for e in range(4):
        same_bits(a[e], b[e])
    after = ctx.policy_gradient(kl_bounds=[0.05], thetas=[0.0, 0.7])  # policy_gradient returns the bits it returned before the call
    for part in ("bounds", "thetas"):
        for k in before[part]:
            if isinstance(before[part][k], np.ndarray):
                assert np.array_equal(before[part][k], after[part][k], equal_nan=True), (part, k)
            else:
                assert before[part][k] == after[part][k], (part, k)
    costs_after = ctx.policy_tail_risk(AL)                            # ... and the stored costs are what they were
    for k in ROW_KEYS:
        assert np.array_equal(costs_before[k], costs_after[k], equal_nan=True), k


def test_nonfinite_sensitivities_are_counted_and_left_out():
    case, pol = mg.sqrt_dyn_setup()
    ctx, K = context(case, 2), 64
    ev = [(None, np.array([1.0, 0.0]), -0.3, 2, 2)]
    assert evaluate(ctx, case, pol, K)["n_ok"] == K
    got = call(ctx, ev)[0]
    m64, mld = mg.reference(("sqrtdyn",), case, pol, K, ev)
    assert 0 < m64["n_nonfinite"][0] < K and got["n_nonfinite"] == m64["n_nonfinite"][0]
    for k in GRAD_KEYS:
        assert np.isfinite(got[k]).all()
    close_event("sqrt dynamics", got, m64, mld, 0)
    # an event that seeds above the step where f_u is Inf never multiplies it: nothing is flagged
    early = call(ctx, [(None, np.array([1.0, 0.5]), -0.3, 1, 1)], [0.0])[0]
    assert early["n_nonfinite"] == 0 and np.isfinite(early["grad_l"]).all() and np.all(early["grad_l"][:, 1] == 0.5)


def test_an_empty_sample_is_nan_and_ok():
    case, N, K = pg.Pendulum(source=un.PEND_NAN, p=(0.1, np.nan)), 3, 8
    case.npn = 1
    ctx, pol = context(case, N), pg.policy(case, N)
    assert evaluate(ctx, case, pol, K)["n_ok"] == 0                   # every draw NaN: every rollout a DomainError
    got = call(ctx, mg.four_events(case, N))
    for e in range(4):
        assert np.isnan(got[e]["grad_l"]).all() and np.isnan(got[e]["grad_L"]).all() and np.isnan(got[e]["grad_l_se"]).all()
        assert got[e]["n_nonfinite"] == 0 and np.all(got[e]["flag"] == 2)


def test_refusals_leave_the_handle_usable():
    case, N, K = pg.Pendulum(), 3, 16
    ctx, pol = context(case, N), pg.policy(case, N)
    evs = mg.four_events(case, N)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no evaluation to replay"):
        call(ctx, evs[:1])
    evaluate(ctx, case, pol, K)
    good = call(ctx, evs[:1])[0]["grad_l"]
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*alpha must be in"):
        call(ctx, evs[:1], [1.0])
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*n_alpha must be in"):
        call(ctx, evs[:1], [])
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*n_event must be at least 1"):
        call(ctx, [])
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*n_event = 5 is above 4"):
        call(ctx, evs + evs[:1])
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*the window must satisfy"):
        call(ctx, [(None, np.ones(3), 0.0, 2, N + 1)])
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*must be finite"):
        call(ctx, [(None, np.array([1.0, np.inf, 0.0]), 0.0, 0, N)])
    assert np.array_equal(call(ctx, evs[:1])[0]["grad_l"], good)
    # rows x N above the cap: 4 events x 16 levels at N = 53 is 3392 > 3360
    big = pg.Pendulum()
    cb, pb = context(big, 53), pg.policy(big, 53)
    evaluate(cb, big, pb, 4)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rows x N = 3392 is above 3360"):
        call(cb, mg.four_events(big, 53), np.linspace(0.0, 0.9, 16))
    assert np.isfinite(call(cb, mg.four_events(big, 53)[:1], [0.0])[0]["grad_l"]).all()
    # a family: write the model as source
    prob, x0, u = rat.synthetic_lq_problem()
    cf = rat.Context(prob, max_batch=1, device=0)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*write the model as source"):
        cf.policy_margin_gradient([rat.halfspace(np.ones(prob.n), 0.0)], [0.5])
    # a source with rat_user_policy
    hook = "#define RAT_USER_POLICY\n__device__ void rat_user_policy(int k, const double *x, const double *u_prev, double *u, const double *p) {}\n"
    cp = pg.Pendulum(source=hook + un.PEND_DIAG)
    cc = context(cp, N)
    evaluate(cc, cp, pol, K)
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_UNSUPPORTED.*defines RAT_USER_POLICY"):
        call(cc, evs[:1])
    assert cc.policy_worst_case_trajectory(thetas=[0.0])["thetas"]["mean_x"].shape == (1, N + 1, 2)
    # the replay guard: the parameters changed behind the evaluation; an evaluation later the call serves again
    ctx.set_params([0.1, 0.07, 0.1])
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*changed since the evaluation"):
        call(ctx, evs[:1])
    evaluate(ctx, case, pol, K)
    assert not np.array_equal(call(ctx, evs[:1])[0]["grad_l"], good)
    # parameter sampling switched on
    import user_params_model as upm
    cs = pg.Pendulum(source=upm.source(un.PEND_DIAG, "scale", 1, 2, 0, 0.0))
    cx = context(cs, N)
    cx.set_param_sampling(rat.ParamSampling(upm.PARAM_NORMALS, upm.PARAM_UNIFORMS))
    evaluate(cx, cs, pol, K)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*parameter sampling is on"):
        call(cx, evs[:1])
    cx.set_param_sampling(None)
    evaluate(cx, cs, pol, K)
    assert np.isfinite(call(cx, evs[:1])[0]["grad_l"]).all()
