"""Model parameters drawn per rollout on the GPU (rat_user_params, include/ratilqr.h "source models"; csrc/source_params.h in
rat_src_user_noisy_rollout, both variants of rat_src_rare_rollout and rat_src_user_events): injected draws against the NumPy restatement
of tests/user_params_model.py, sampling off against the source without the hook (bit for bit), the NaN rule, the replays (worst-case
trajectory and disturbance moments, a user-written event that reads a drawn parameter, the replay guard), rare events against a plain
count, the generator's invariants, the refusals, and the closed form of tests/test_cpu_user_params.py.

Shapes (tests/user_params_model.Case): the pendulum 2 x 1 at N = 8, K = 256; the LQ + cubic source 12 x 4 at N = 4, K = 128 with twelve
normals and a uniform per step; the same source at 5 x 3, K = 65 (padding lanes, a ragged last wave).

Tolerance against the model: 1e-12 relative -- costs and statistics element by element; states and controls relative to the largest entry
of the rollout set, as tests/test_gpu_user_noise.py holds them.  The drawn parameters themselves (sample_params) are held bit for bit on
injected draws; under the generator, whose Box-Muller NumPy restates to rounding, to 1e-13."""
import numpy as np
import pytest

import rare_event_noise_model as rn
import ratilqr.jl_amd as rat
import user_params_model as pm
from test_gpu_user_noise import check_stats, rel
from test_gpu_user_policy import against_model, same_evaluation, same_rare
from test_gpu_wc_disturbance import check as check_disturbance
from test_gpu_wc_trajectory import check as check_trajectory
from wc_trajectory_model import centre

pytestmark = pytest.mark.gpu
THETAS = (0.0, 0.4)
_CTX = {}


def context(name, hook, event=False):
    """one handle per (case, hook): every test sets the sampling state it needs and the nominal parameters"""
    key = (name, hook, event)
    if key not in _CTX:
        _CTX[key] = rat.Context(pm.case(name).problem(hook, event=event), max_batch=64)
    ctx = _CTX[key]
    ctx.set_params(pm.case(name).p)
    ctx.set_param_sampling(None)
    return ctx


def evaluate(ctx, c, closed, **kw):
    x_nom, l, L = c.args(closed)
    return ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(zn=c.zn, zu=c.zu), thetas=THETAS, want_costs=True, want_trajectories=True, **kw)


def ulps(a, b):
    return int(np.abs(a.view(np.int64) - b.view(np.int64)).max())


# ---- 1. injected draws against the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("name", pm.CASE_NAMES)
def test_injected_draws_against_the_model(name, closed):
    c = pm.case(name)
    ctx = context(name, "scale")
    ctx.set_param_sampling(c.sampling())
    q = ctx.sample_params(c.K, seed=3)                               # (injected: the seed is not read)
    ref = c.q("scale")
    print(f"{name}: sample_params against the model: {ulps(q, ref)} ulp")
    assert q.shape == (c.K, c.p.size) and np.array_equal(q, ref)
    moved = np.any(q != c.p[None], axis=0)
    assert np.array_equal(np.nonzero(moved)[0], sorted((c.idx["pi0"], c.idx["pi1"], c.idx["pi2"])))      # the other entries stay nominal
    r = evaluate(ctx, c, closed)
    model = c.model("scale", closed)
    against_model(r, model, f"{name} closed={closed}")
    check_stats(r, THETAS)
    free, _, _ = c.model(None, closed)
    assert not np.allclose(r["costs"], free, rtol=1e-4, atol=0.0)    # the costs are those of the drawn parameters, not of the nominal ones
    # a shorter call reads the same rows
    x_nom, l, L = c.args(closed)
    K2 = c.K // 2 + 1
    r2 = ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(zn=c.zn[:K2], zu=None if c.zu is None else c.zu[:K2]), want_costs=True)
    assert np.array_equal(r2["costs"], r["costs"][:K2])


# ---- 2. off is invisible ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pm.CASE_NAMES)
def test_sampling_off_is_invisible(name):
    c = pm.case(name)
    plain, hooked, ident = context(name, None, event=True), context(name, "scale", event=True), context(name, "identity", event=True)
    x_nom, l, L = c.policy
    for closed in (False, True):
        xa, la, La = c.args(closed)
        a, b = evaluate(plain, c, closed), evaluate(hooked, c, closed)
        same_evaluation(a, b, (name, closed, "injected"))
        gen = dict(noise=c.user_noise(seed=77), thetas=THETAS, K=300, want_costs=True, want_trajectories=True)
        ga, gb = plain.policy_evaluate_noise(xa, la, La, **gen), hooked.policy_evaluate_noise(xa, la, La, **gen)
        same_evaluation(ga, gb, (name, closed, "generator"))
        ea, eb = plain.policy_events_user(1, thetas=[0.0], want_margins=True), hooked.policy_events_user(1, thetas=[0.0], want_margins=True)
        assert np.array_equal(ea["margins"], eb["margins"]) and np.array_equal(ea["thetas"]["n_viol"], eb["thetas"]["n_viol"])
        rare = dict(noise=c.user_noise(seed=5), n_iter=2, rho=0.1, want_margins=True, want_logw=True)
        same_rare(plain.policy_rare_event_user(xa, la, La, 1, 0, 1000, **rare), hooked.policy_rare_event_user(xa, la, La, 1, 0, 1000, **rare), (name, closed))
        # sampling on with a hook that leaves q alone: the sampling-off bits, trajectories included (the step counters are untouched)
        ident.set_param_sampling(c.sampling(injected=False))
        same_evaluation(ga, ident.policy_evaluate_noise(xa, la, La, **gen), (name, closed, "identity hook"))
        same_evaluation(a, evaluate(ident, c, closed), (name, closed, "identity hook, injected"))
        ident.set_param_sampling(None)
    theta = np.linspace(0.0, 0.5, 64)
    for va, vb in zip(plain.solve_batch(x_nom[0], l, theta), hooked.solve_batch(x_nom[0], l, theta)):
        assert np.array_equal(va, vb, equal_nan=True)


# ---- 3. the NaN rule --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pend", "lq12"])
def test_a_nan_from_the_hook_is_a_domain_error(name):
    c = pm.case(name)
    ctx = context(name, "nan", event=True)
    p = c.p.copy()
    p[c.idx["pnan"]] = 1.2                                           # the first parameter normal beyond 1.2: about one rollout in nine
    ctx.set_params(p)
    ctx.set_param_sampling(c.sampling())
    bad = c.zpn[:, 0] > 1.2
    assert 5 < bad.sum() < c.K // 4
    r = evaluate(ctx, c, True)
    cost, xs, us = c.model("nan", True, p=p)
    assert np.array_equal(np.isnan(cost), bad)
    assert np.array_equal(np.isnan(r["costs"]), bad) and r["n_domain"] == bad.sum() and r["n_ok"] == c.K - bad.sum()
    assert np.allclose(r["costs"][~bad], cost[~bad], rtol=1e-12, atol=0.0) and rel(r["x"][~bad], xs[~bad]) < 1e-12
    check_stats(r, THETAS)
    assert np.array_equal(np.isnan(ctx.sample_params(c.K)[:, c.idx["pi0"]]), bad)
    x_nom, l, L = c.policy
    got = ctx.policy_rare_event_user(x_nom, l, L, 1, 0, c.K, noise=c.user_noise(seed=9), n_iter=0, want_margins=True)
    assert got.n_domain == bad.sum() and got.n_ok == c.K - bad.sum() and np.array_equal(np.isnan(got.margins), bad)
    ev = rat.halfspace(np.eye(c.n + c.m)[0], 0.0)
    got = ctx.policy_rare_event_noise(x_nom, l, L, ev, c.K, noise=c.user_noise(seed=9), n_iter=0, want_margins=True)
    assert got.n_domain == bad.sum() and np.array_equal(np.isnan(got.margins), bad)


# ---- 4. replays see the rollout's parameters -------------------------------------------------------------------------------------------------
def lqc_w(q, seed, x, u):
    """w [K, N, n] of LQC's sampler under the generator's step draws and the parameters q [K, 14] of the rollouts"""
    K, N, n = u.shape[0], u.shape[1], x.shape[2]
    xi, un = rn.normals(seed, 0, K, N, n), rn.uniforms(seed, 0, K, N, 1)
    second = un[:, :, 0] < q[:, None, 8]
    q_ = lambda i: q[:, None, None, i]
    return np.where(second[:, :, None], q_(9) + q_(10) * xi, q_(11) * (xi + 0.5 * np.roll(xi, -1, axis=2)))


def test_replays_see_the_rollouts_parameters():
    c = pm.case("lq12")
    K, seed = 2048, 21
    # the obstacle's radius p[12] is drawn: scaled by 1 + 0.2 z0; the first component's scale by 1 + 0.2 z1; a shifted by 0.1 v
    idx = dict(pi0=12, pi1=11, pi2=0, psh=0.1)
    src = pm.source(pm.LQC, "scale", **idx) + "#define EVP 12\n" + pm.EVENT
    ctx = rat.Context(rat.DeviceSourceProblem(src, c.n, c.m, c.N, c.W, params=c.p))
    ctx.set_param_sampling(rat.ParamSampling(2, 1))
    x_nom, l, L = c.policy
    kw = dict(noise=c.user_noise(seed=seed), K=K, want_costs=True, want_trajectories=True)
    r = ctx.policy_evaluate_noise(x_nom, l, L, **kw)
    assert r["n_ok"] == K
    # the nominal radius at the median over the rollouts of the closest approach to the origin: about half of them enter an obstacle of
    # that radius.  The radius is read by the event alone, so the rollouts -- evaluated again for the replays -- do not move
    p = c.p.copy()
    p[12] = float(np.median(np.abs(r["x"][:, :, 0]).min(axis=1)))
    ctx.set_params(p)
    r2 = ctx.policy_evaluate_noise(x_nom, l, L, **kw)
    assert np.array_equal(r2["costs"], r["costs"]) and np.array_equal(r2["x"], r["x"])
    q = ctx.sample_params(K, seed)
    zpn, zpu = pm.gen_draws(seed, K, 2, 1)
    assert np.allclose(q, pm.np_params("scale", p, zpn, zpu, **idx), rtol=1e-13, atol=0.0)
    # the trajectories continue under each rollout's own parameters: x_{t+1} = f(x_t, u_t; q_j) + w_t(q_j)
    w = lqc_w(q, seed, r["x"], r["u"])
    xn = np.array([[pm.lqc_f(r["x"][j, t], r["u"][j, t], q[j]) for t in range(c.N)] for j in range(K)])
    assert rel(xn + w, r["x"][:, 1:]) < 1e-10
    w_nom = lqc_w(np.repeat(p[None], K, axis=0), seed, r["x"], r["u"])
    assert rel(xn + w_nom, r["x"][:, 1:]) > 1e-3                      # (the nominal parameters would not)
    thetas = (0.0, 1.0 / np.sqrt(r["var"]))
    cz = centre(x_nom, l)
    check_trajectory(ctx, r["x"], r["u"], r["costs"], cz, (0.2,), thetas, "drawn parameters", far=True)
    check_disturbance(ctx, w, r["x"], r["u"], r["costs"], cz, (0.2,), thetas, "drawn parameters", far=True)
    # the user's event reads the drawn radius: g = q_j[12] - |x_0| on the device's own trajectories, single operations, exact
    g = q[:, None, 12] - np.abs(r["x"][:, :, 0])
    ev = ctx.policy_events_user(1, thetas=[0.0], want_margins=True)
    n_viol = int((g > 0).any(axis=1).sum())
    g_nom = p[12] - np.abs(r["x"][:, :, 0])
    print(f"replays: {n_viol} of {K} rollouts enter the obstacle of their own radius, {int((g_nom > 0).any(axis=1).sum())} the nominal one")
    assert 0 < n_viol < K and n_viol != int((g_nom > 0).any(axis=1).sum())
    assert ev["thetas"]["n_viol"][0, 0] == n_viol and np.array_equal(ev["margins"][0], g.max(axis=1))
    # the rare-event kernel hands the event the same parameters: without a shift, the margins of the replay
    r0 = ctx.policy_rare_event_user(x_nom, l, L, 1, 0, K, noise=c.user_noise(seed=seed), n_iter=0, want_margins=True)
    assert np.array_equal(r0.margins, ev["margins"][0])
    # the guard: sampling switched off behind the evaluation is another set of rollouts
    ctx.set_param_sampling(None)
    for call in (lambda: ctx.policy_worst_case_trajectory(thetas=(0.0,)), lambda: ctx.policy_worst_case_disturbance(thetas=(0.0,)),
                 lambda: ctx.policy_events_user(1, thetas=[0.0])):
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*changed since the evaluation"):
            call()
    ctx.set_param_sampling(rat.ParamSampling(2, 1))
    assert ctx.policy_events_user(1, thetas=[0.0])["thetas"]["n_viol"][0, 0] == n_viol


# ---- 5. rare events against a plain count ----------------------------------------------------------------------------------------------------
def test_rare_events_against_a_plain_count():
    """the pendulum with rat_user_event g = x[0] - p[3] and the hook scaling p[3] by 1 + 0.2 z0: the nominal threshold sits where about one
    rollout in a hundred of a plain run of 2^16 exceeds its own threshold; the importance-sampling estimate under another seed lies within
    4 of its own standard errors of that count."""
    c = pm.case("pend")
    x_nom, l, L = c.policy
    K = 1 << 16
    event = "#define RAT_USER_EVENT\n__device__ void rat_user_event(int k, const double *x, const double *u, double *g, const double *p) {\n" \
            "    g[0] = x[0] - p[3];\n}\n"
    src = pm.source(c.base, "scale", pi0=3, pi1=2, pi2=0, psh=0.02) + event
    ctx = rat.Context(rat.DeviceSourceProblem(src, 2, 1, c.N, c.W, params=c.p))
    ctx.set_param_sampling(rat.ParamSampling(2, 1))
    r = ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=1), K=K, want_trajectories=True)
    scale = ctx.sample_params(K, 1)[:, 3] / c.p[3]                    # 1 + 0.2 z0 of every rollout
    s = np.sort(r["x"][:, :, 0].max(axis=1) / scale)
    i = int(0.99 * K)
    p = c.p.copy()
    p[3] = 0.5 * (s[i] + s[i + 1])
    assert scale.min() > 0 and p[3] > 0
    ctx.set_params(p)
    ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=1), K=K)
    n_viol = int(ctx.policy_events_user(1, thetas=[0.0])["thetas"]["n_viol"][0, 0])
    plain = n_viol / K
    assert abs(n_viol - (K - 1 - i)) <= 2 and 5e-3 < plain < 2e-2
    got = ctx.policy_rare_event_user(x_nom, l, L, 1, 0, K, noise=c.user_noise(seed=2), n_iter=4, rho=0.1)
    print(f"rare: PROB {got.prob:.5e} SE {got.prob_se:.2e}; plain count {plain:.5e}: {abs(got.prob - plain) / got.prob_se:.2f} sigma")
    assert got.flag == 0 and got.n_domain == 0 and got.prob_se > 0
    assert abs(got.prob - plain) <= 4.0 * got.prob_se


# ---- 6. generator invariants -----------------------------------------------------------------------------------------------------------------
def test_generator_invariants():
    c = pm.case("pend")
    N, K = 2, (1 << 16) + 37
    x_nom, l, L = pm.um.pend_policy(N)
    ctx = rat.Context(c.problem("scale", N=N))
    ctx.set_param_sampling(c.sampling(injected=False))
    noise = c.user_noise(seed=77)
    a = ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=K, want_costs=True, want_trajectories=True)     # two chunks, the second of 37
    b = ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=K + 64, want_costs=True)                        # one launch
    assert a["n_ok"] == K and np.array_equal(a["costs"], b["costs"][:K]) and np.unique(a["costs"][-8:]).size == 8
    same_evaluation(a, ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=K, want_costs=True, want_trajectories=True), "repeat")
    # the parameters behind those costs: keyed by the global rollout index across the chunk boundary, the model's draws to rounding
    q = ctx.sample_params(K, 77)
    assert np.array_equal(q, ctx.sample_params(K + 64, 77)[:K]) and not np.array_equal(q, ctx.sample_params(K, 78))
    zpn, zpu = pm.gen_draws(77, K, pm.PARAM_NORMALS, pm.PARAM_UNIFORMS)
    err = float(np.abs(q / c.q("scale", zpn=zpn, zpu=zpu) - 1).max())
    print(f"generator: sample_params against the Python Philox {err:.2e}")
    assert err < 1e-13 and np.unique(q[-37:, 1]).size == 37
    # the last rollouts' costs are c(0) + c(1) + h on their own trajectories (the cost reads no drawn parameter but through x)
    x, u = a["x"][-3:], a["u"][-3:]
    ref = sum(pm.um.pend_c(t, x[:, t].T, u[:, t].T, c.p) for t in range(N)) + pm.um.pend_h(x[:, N].T, c.p)
    assert np.allclose(a["costs"][-3:], ref, rtol=1e-10, atol=0.0)
    # x_1 = f(x_0, u_0; dt_j) + w_0: the drawn dt of rollout j, in both chunks
    j = np.array([0, 1, K - 2, K - 1])
    xn0 = np.stack([pm.um.pend_f(a["x"][i, 0], a["u"][i, 0], q[i]) for i in j])
    assert np.allclose(a["x"][j, 1, 0], xn0[:, 0] + q[j, 1] * np.abs(a["x"][j, 0, 0]) * rn.normals(77, 0, K, N, 3)[j, 0, 0], rtol=1e-12, atol=0.0)


def test_the_scalar_closed_form():
    a0, s, x0, N, K, seed = 0.9, 0.05, 1.5, 6, 1 << 14, 2024
    ctx = rat.Context(rat.DeviceSourceProblem(pm.SCALAR, 1, 1, N, 1e-3 * np.eye(1), params=[a0, s]))
    ctx.set_param_sampling(rat.ParamSampling(1, 0))
    r = ctx.policy_evaluate_noise(np.array([x0]), np.zeros((N, 1)), None, noise=rat.UserNoise(1, 0, seed=seed), K=K)
    ref = pm.scalar_mean_cost(a0, s, x0, N)
    print(f"closed form {ref:.6f}, device mean {r['mean']:.6f}, se {r['se_mean']:.2e}: {abs(r['mean'] - ref) / r['se_mean']:.2f} sigma")
    assert r["n_ok"] == K and abs(r["mean"] - ref) <= 4.0 * r["se_mean"]


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_handle_goes_on():
    c = pm.case("pend")
    x_nom, l, L = c.policy
    ctx = context("pend", "over")
    ctx.set_param_sampling(c.sampling())
    for call in (lambda: evaluate(ctx, c, True), lambda: ctx.sample_params(8),
                 lambda: ctx.policy_rare_event_noise(x_nom, l, L, rat.halfspace(np.eye(3)[0], 0.0), 64, noise=c.user_noise(seed=1), n_iter=0)):
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*rat_user_params drew more.*param_normals = 2, param_uniforms = 1"):
            call()
    ctx.set_param_sampling(rat.ParamSampling(3, 1, zpn=np.concatenate([c.zpn, np.ones((c.K, 1))], axis=1), zpu=c.zpu))     # declared in full
    r = evaluate(ctx, c, True)
    assert r["n_ok"] == c.K and np.array_equal(ctx.sample_params(c.K)[:, 1], c.q("scale")[:, 1])
    # more rollouts than the injected parameter draws hold
    ok = context("pend", "scale")
    ok.set_param_sampling(rat.ParamSampling(2, 1, zpn=c.zpn[:100], zpu=c.zpu[:100]))
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*above the 100 rollouts"):
        evaluate(ok, c, True)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*above the 100 rollouts"):
        ok.sample_params(101)
    assert ok.sample_params(100).shape == (100, c.p.size)
    for ps in (rat.ParamSampling(2, 1, zpn=c.zpn), rat.ParamSampling(2, 1, zpu=c.zpu)):
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*every declared stream"):
            ok.set_param_sampling(ps)
    for ps in (rat.ParamSampling(-1, 1), rat.ParamSampling(2, -1)):
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*must not be negative"):
            ok.set_param_sampling(ps)
    assert ok.sample_params(100).shape == (100, c.p.size)            # a refused call leaves the state as it was
    # a source without the hook, with sampling on
    plain = context("pend", None)
    plain.set_param_sampling(c.sampling())
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_ARG.*does not define RAT_USER_PARAMS"):
        evaluate(plain, c, True)
    plain.set_param_sampling(None)
    assert evaluate(plain, c, True)["n_ok"] == c.K
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*sampling is off"):
        plain.sample_params(4)
    # a source without parameters, and a family
    none = rat.Context(rat.DeviceSourceProblem(pm.um.PEND_FCH.replace("p[0]", "0.1"), 2, 1, 4, 1e-2 * np.eye(2)))
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no parameters"):
        none.set_param_sampling(rat.ParamSampling(1, 0))
    fam = rat.Context(rat.LQRiskSensitiveProblem(np.eye(2), np.ones((2, 1)), Q=np.eye(2), R=np.eye(1), N=4, W=1e-2 * np.eye(2), Qf=np.eye(2)))
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*not a source model"):
        fam.set_param_sampling(rat.ParamSampling(1, 0))
    fam.set_param_sampling(None)
