"""The controller the user writes on the GPU (rat_user_policy, include/ratilqr.h "source models"; csrc/source_policy.h in the four
Monte-Carlo rollout kernels of source models): injected draws against the NumPy restatement of tests/user_policy_model.py, the rate
limiter's u_prev, a hook that leaves u alone and the solver (bit for bit against the source without the hook), the NaN rule, the replays
(worst-case trajectory and disturbance moments, quadratic and user-written events on u), set_params, the rare-event calls, and the
generator's two invariants of tests/test_gpu_user_noise.py.

Shapes (tests/user_policy_model.Case): the pendulum 2 x 1 at N = 8, K = 256; the LQ + cubic source 12 x 4 at N = 4, K = 128 with twelve
normals and a uniform per step (the kernel's tightest register regime); the same source at 5 x 3, K = 65 (padding lanes of x and u).

Tolerance against the model: 1e-12 relative -- costs and statistics element by element; states and controls relative to the largest entry
of the rollout set, as tests/test_gpu_user_noise.py holds them, because a state component can pass through zero (the element-wise
figures are printed beside them)."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
import user_event_model as ue
import user_noise_model as um
import user_policy_model as up
from policy_mc_model import reduce_costs
from test_cpu_wc_disturbance import CPU_DEV_COV as CPU_DEV_COV_W
from test_cpu_wc_disturbance import CPU_DEV_FAR_WZ
from test_cpu_wc_disturbance import CPU_DEV_MEAN as CPU_DEV_MEAN_W
from test_cpu_wc_trajectory import CPU_DEV_FAR_COV, CPU_DEV_FAR_MEAN
from test_gpu_user_noise import check_stats, rel
from test_gpu_wc_disturbance import check as check_disturbance
from test_gpu_wc_disturbance import parts, source_w
from test_gpu_wc_trajectory import check as check_trajectory
from test_gpu_wc_trajectory import full
from wc_disturbance_model import centre_w, z_offset
from wc_disturbance_model import deviation as deviation_w
from wc_disturbance_model import direct as direct_w
from wc_trajectory_model import centre
from wc_trajectory_model import deviation as deviation_z
from wc_trajectory_model import direct as direct_z

pytestmark = pytest.mark.gpu
RTOL = 1e-12
THETAS = (0.0, 0.4)
_CTX = {}


def context(name, hook):
    """one handle per (case, hook): the code objects are cached per process by the source text, the handle keeps the loaded modules"""
    if (name, hook) not in _CTX:
        _CTX[name, hook] = rat.Context(up.case(name).problem(hook), max_batch=64)
    ctx = _CTX[name, hook]
    ctx.set_params(up.case(name).params())
    return ctx


def evaluate(ctx, c, closed, gaussian, **kw):
    x_nom, l, L = c.args(closed)
    if gaussian:
        return ctx.policy_evaluate(x_nom, l, L, z=c.z, thetas=THETAS, want_costs=True, **kw)
    return ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(zn=c.zn, zu=c.zu), thetas=THETAS, want_costs=True, want_trajectories=True, **kw)


def against_model(r, model, label):
    """costs, statistics, x_out and u_out of an evaluation against the NumPy rollouts"""
    cost, xs, us = model
    ok = ~np.isnan(cost)
    ec = float(np.abs(r["costs"][ok] / cost[ok] - 1).max())
    line = f"{label}: cost err {ec:.2e}"
    assert np.array_equal(np.isnan(r["costs"]), ~ok), label
    if r.get("x") is not None:
        fin = np.isfinite(xs)
        assert np.array_equal(np.isfinite(r["x"]), fin) and np.array_equal(np.isfinite(r["u"]), np.isfinite(us)), label
        ex, eu = rel(r["x"][fin], xs[fin]), rel(r["u"][np.isfinite(us)], us[np.isfinite(us)])
        with np.errstate(divide="ignore", invalid="ignore"):
            exe = float(np.nanmax(np.abs(r["x"][fin] / xs[fin] - 1)))
        line += f", x err {ex:.2e} (element-wise {exe:.2e}), u err {eu:.2e}"
    mdl = reduce_costs(cost, THETAS)
    es = max(float(np.abs(np.asarray(r[k]) / np.asarray(mdl[k]) - 1).max()) for k in ("mean", "var", "min", "max", "se_mean", "risk", "risk_se"))
    print(line + f", statistics err {es:.2e}")
    assert np.allclose(r["costs"][ok], cost[ok], rtol=RTOL, atol=0.0), label
    assert r["n_ok"] == mdl["n_ok"] and r["n_domain"] == mdl["n_domain"], label
    for k in ("mean", "var", "min", "max", "se_mean", "risk", "risk_se"):
        assert np.allclose(r[k], mdl[k], rtol=RTOL, atol=0.0), (label, k)
    if r.get("x") is not None:
        assert ex < RTOL and eu < RTOL, label


# ---- 1. injected draws against the model --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("gaussian", [False, True])
@pytest.mark.parametrize("name", up.CASE_NAMES)
def test_injected_draws_against_the_model(name, gaussian, closed):
    """policy_evaluate_noise on zn / zu and policy_evaluate on z under the clamp: the model's numbers, and no control outside the clamp.
    (On a library without the hook every u_out entry is the affine law's: the clamp assertions fail.)"""
    c = up.case(name)
    ctx = context(name, "clamp")
    r = evaluate(ctx, c, closed, gaussian)
    against_model(r, c.model("clamp", closed, gaussian=gaussian), f"{name} gaussian={gaussian} closed={closed}")
    check_stats(r, THETAS)
    _, _, u_free = c.model(None, closed, gaussian=gaussian)
    assert (np.abs(u_free) > c.q[0]).any()                           # the affine law does leave the limits on these draws
    if not gaussian:                                                 # (rat_policy_evaluate has no trajectory output)
        assert r["u"].shape == (c.K, c.N, c.m) and np.abs(r["u"]).max() == c.q[0]
        assert np.all(np.abs(r["u"]) <= c.q[0])
        at = np.abs(u_free) > c.q[0]
        assert np.all(np.abs(r["u"][:, 0][at[:, 0]]) == c.q[0])      # step 0: the same state on both sides, so exactly the clamped entries
    else:
        # the costs are those of the clamped loop, not of the affine law's
        free, _, _ = c.model(None, closed, gaussian=True)
        assert not np.allclose(r["costs"], free, rtol=1e-6, atol=0.0)


# ---- 2. the rate limiter reads u_prev ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("name", up.CASE_NAMES)
def test_the_rate_limiter_reads_u_prev(name, closed):
    c = up.case(name)
    ctx = context(name, "rate")
    clamp, rate = c.q[0], c.q[1]
    for gaussian in (False, True):
        r = evaluate(ctx, c, closed, gaussian)
        against_model(r, c.model("rate", closed, gaussian=gaussian), f"rate {name} gaussian={gaussian} closed={closed}")
    r = evaluate(ctx, c, closed, False)
    u = r["u"]
    assert np.all(np.abs(u[:, 0]) <= rate)                           # step 0 is limited against u_prev = 0 ...
    _, l, _ = c.args(closed)
    if not closed:
        assert np.array_equal(u[:, 0], np.broadcast_to(np.clip(l[0], -rate, rate), u[:, 0].shape)) and (np.abs(l[0]) > rate).any()
    steps = np.diff(u, axis=1)                                       # ... and step t against the control applied at t - 1
    assert np.abs(steps).max() <= rate * (1 + 1e-15) and np.abs(u).max() <= clamp
    assert (np.abs(steps) >= rate * (1 - 1e-15)).mean() > 0.1


# ---- 3. a hook that leaves u alone is invisible -------------------------------------------------------------------------------------------
def same_evaluation(a, b, label):
    for k in ("n_ok", "n_domain", "mean", "var", "min", "max", "se_mean"):
        assert a[k] == b[k], (label, k)
    for k in ("risk", "risk_se", "costs", "x", "u"):
        if a.get(k) is not None or b.get(k) is not None:
            assert np.array_equal(a[k], b[k], equal_nan=True), (label, k)


def same_rare(a, b, label):
    for k in ("prob", "prob_se", "ess", "n_viol", "n_ok", "n_domain", "logw_max", "logw_min", "flag", "n_iter", "level"):
        assert getattr(a, k) == getattr(b, k) or (np.isnan(getattr(a, k)) and np.isnan(getattr(b, k))), (label, k)
    for k in ("shift", "trace", "margins", "logw"):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), (label, k)


@pytest.mark.parametrize("name", up.CASE_NAMES)
def test_a_hook_that_leaves_u_alone_is_invisible(name):
    c = up.case(name)
    plain, ident = context(name, None), context(name, "identity")
    x_nom, l, L = c.policy
    ev = rat.halfspace(np.eye(c.n + c.m)[0], -float(x_nom[:, 0].max()) - 0.5)
    for closed in (False, True):
        xa, la, La = c.args(closed)
        for gaussian in (False, True):
            same_evaluation(evaluate(plain, c, closed, gaussian), evaluate(ident, c, closed, gaussian), (name, closed, gaussian))
        gen = dict(noise=c.user_noise(seed=77), thetas=THETAS, K=300, want_costs=True, want_trajectories=True)
        same_evaluation(plain.policy_evaluate_noise(xa, la, La, **gen), ident.policy_evaluate_noise(xa, la, La, **gen), (name, closed, "generator"))
        same_evaluation(plain.policy_evaluate(xa, la, La, thetas=THETAS, K=300, seed=9, want_costs=True),
                        ident.policy_evaluate(xa, la, La, thetas=THETAS, K=300, seed=9, want_costs=True), (name, closed, "N(0, W) generator"))
        rare = dict(noise=c.user_noise(seed=5), n_iter=2, rho=0.1, want_margins=True, want_logw=True)
        a, b = plain.policy_rare_event_noise(xa, la, La, ev, 1000, **rare), ident.policy_rare_event_noise(xa, la, La, ev, 1000, **rare)
        assert np.isfinite(a.margins).all() and np.unique(a.margins).size > 100      # (open loop many rollouts peak at the shared x_0)
        same_rare(a, b, (name, closed))


# ---- 4. the solver does not see the hook ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pend", "lq5"])
def test_the_solver_does_not_see_the_hook(name):
    c = up.case(name)
    plain, clamp = context(name, None), context(name, "clamp")
    x_nom, l, _ = c.policy
    a, b = plain.solve(x_nom[0], l, 0.3), clamp.solve(x_nom[0], l, 0.3)
    for k in ("x", "l", "L", "eps_history"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert (a["value"], a["status"], a["iters"], a["hist_n"]) == (b["value"], b["status"], b["iters"], b["hist_n"])
    assert a["iters"] >= 1
    theta = np.linspace(0.0, 2.0, 64)
    for va, vb in zip(plain.solve_batch(x_nom[0], l, theta), clamp.solve_batch(x_nom[0], l, theta)):
        assert np.array_equal(va, vb, equal_nan=True)
    # the deterministic rollouts are the solver's as well
    assert np.array_equal(plain.rollout_open(x_nom[0], l), clamp.rollout_open(x_nom[0], l))


# ---- 5. a NaN from the hook is a DomainError -------------------------------------------------------------------------------------------------
def nan_threshold(c, closed, gaussian):
    """(q with the NaN threshold between the largest and the second largest first state the clamped model reaches at a step the hook
    sees, that rollout)"""
    _, xs, _ = c.model("clamp", closed, gaussian=gaussian)
    top = xs[:, 1:-1, 0].max(axis=1)                                 # (x_0 is the same point on every rollout)
    order = np.argsort(top)
    q = c.q.copy()
    q[2] = 0.5 * (top[order[-1]] + top[order[-2]])
    assert q[2] > xs[0, 0, 0]
    return q, int(order[-1])


@pytest.mark.parametrize("gaussian", [False, True])
@pytest.mark.parametrize("name", ["pend", "lq12"])
def test_a_nan_from_the_hook_is_a_domain_error(name, gaussian):
    c = up.case(name)
    ctx = context(name, "nan")
    q, j = nan_threshold(c, True, gaussian)
    ctx.set_params(c.params(q))
    r = evaluate(ctx, c, True, gaussian)
    cost, xs, us = c.model("nan", True, gaussian=gaussian, q=q)
    assert np.array_equal(np.isnan(cost), np.arange(c.K) == j)
    assert np.array_equal(np.isnan(r["costs"]), np.arange(c.K) == j) and r["n_domain"] == 1 and r["n_ok"] == c.K - 1
    ok = np.arange(c.K) != j
    assert np.isclose(r["mean"], cost[ok].mean(), rtol=1e-10)         # the mean is that of the others
    against_model(r, (cost, xs, us), f"nan {name} gaussian={gaussian}")
    check_stats(r, THETAS)
    if not gaussian:
        assert np.isnan(r["u"][j]).any() and np.all(np.isfinite(r["u"][ok]))
    ctx.set_params(c.params())
    assert evaluate(ctx, c, True, gaussian)["n_domain"] == 0          # out of reach again: no rollout fails


# ---- 6. replays see applied controls --------------------------------------------------------------------------------------------------------
REPLAY_N, REPLAY_K, REPLAY_SEED = 6, 4096, 21
REPLAY_P = [0.1, 0.05, 0.08]                                          # dt, s0, s1 of PEND_UDEP
REPLAY_CLAMP = 0.15


def replay_problem(hook):
    """PEND_UDEP (a sampler that reads u) with the hook and rat_user_event g[0] = u[0] - q[0]; p = model | clamp, rate, NaN | event"""
    src = up.PEND_UDEP if hook is None else up.source(up.PEND_UDEP, 3, hook)
    p = np.concatenate([REPLAY_P, [REPLAY_CLAMP, 0.5 * REPLAY_CLAMP, 1e300], [REPLAY_CLAMP]])
    return rat.DeviceSourceProblem(up.with_u_event(src, 6), 2, 1, REPLAY_N, 1e-3 * np.eye(2), params=p)


def test_replays_see_applied_controls():
    x_nom, l, L = um.pend_policy(REPLAY_N)
    L = 4.0 * L
    noise = rat.UserNoise(2, 0, seed=REPLAY_SEED)
    kw = dict(noise=noise, K=REPLAY_K, want_costs=True, want_trajectories=True)
    ev_u = rat.halfspace(np.array([0.0, 0.0, 1.0]), -REPLAY_CLAMP)    # u_0 > limit at any step
    res = {}
    for hook in ("clamp", None):
        ctx = rat.Context(replay_problem(hook))
        r = ctx.policy_evaluate_noise(x_nom, l, L, **kw)
        assert r["n_ok"] == REPLAY_K
        quad = ctx.policy_events([ev_u], thetas=[0.0], want_margins=True)
        user = ctx.policy_events_user(1, thetas=[0.0], want_margins=True)
        res[hook] = (ctx, r, quad, user)
    ctx, r, quad, user = res["clamp"]
    free = res[None][1]
    share = up.beyond(free["u"], REPLAY_CLAMP)
    print(f"replays: the hookless policy is beyond the clamp in {share:.3f} of the pairs")
    assert share > 0.25 and np.abs(r["u"]).max() == REPLAY_CLAMP
    # u_out holds applied controls, and rat_user_noise received them: w restated on the host from the device's own (x, u) continues x
    w = source_w(up.udep_noise, REPLAY_P, REPLAY_SEED, 2, r["x"], r["u"])
    xn = np.stack([um.pend_f(r["x"][:, t].T, r["u"][:, t].T, REPLAY_P).T for t in range(REPLAY_N)], axis=1)
    assert rel(xn + w, r["x"][:, 1:]) < 1e-10
    w_aff = source_w(up.udep_noise, REPLAY_P, REPLAY_SEED, 2, r["x"], l + np.einsum("tij,ktj->kti", L, r["x"][:, :-1] - x_nom[:-1]))
    assert rel(xn + w_aff, r["x"][:, 1:]) > 1e-4                      # (the affine control in the sampler would not)
    # the moments of the replays are the host combination of these trajectories: tests/test_gpu_wc_trajectory.py's and
    # tests/test_gpu_wc_disturbance.py's own checks and tolerances, u rows and columns included; the centre stays (x_nom, l)
    thetas = (0.0, 1.0 / np.sqrt(r["var"]))
    c = centre(x_nom, l)
    out = check_trajectory(ctx, r["x"], r["u"], r["costs"], c, (0.2,), thetas, "clamped pendulum", far=True)
    mu = np.concatenate([out["bounds"]["mean_u"], out["thetas"]["mean_u"]])
    assert np.all(np.abs(mu) <= REPLAY_CLAMP) and np.abs(mu).max() > 0.5 * REPLAY_CLAMP
    dis = check_disturbance(ctx, w, r["x"], r["u"], r["costs"], c, (0.2,), thetas, "clamped pendulum", far=True)
    # the same with rat_policy_worst_case's weights_out at the radius in place of weights rebuilt from theta*: u_out combined on the
    # host in np.longdouble, held to what those files hold `direct` to
    y = ctx.policy_worst_case(kl_bounds=(0.2,), want_weights=True)["weights"][None]
    alive = np.array([False])
    cd = c[:, [0, 1, 12]]
    mean, cov = full({k: v[:1] for k, v in out["bounds"].items()}, 2, 1)
    mean_d, cov_d = direct_z(r["x"], r["u"], r["costs"], y, alive)
    em, ec = deviation_z(mean, cov, mean_d, cov_d, cd, K=REPLAY_K)
    zs = z_offset(mean_d[:, :-1], cov_d[:, :-1], cd[:-1])
    got = parts({k: v[:1] for k, v in dis["bounds"].items()})
    dm, dc, dz = deviation_w(got, direct_w(w, r["x"], r["u"], r["costs"], y, alive), centre_w(w, r["costs"])[:, :2], zs, K=REPLAY_K)
    print(f"replays against weights_out: mean {em:.2e} cov {ec:.2e}; mean_w {dm:.2e} cov_w {dc:.2e} cov_wz {dz:.2e}")
    assert em <= 10 * CPU_DEV_FAR_MEAN and ec <= 10 * CPU_DEV_FAR_COV
    assert dm <= 10 * CPU_DEV_MEAN_W and dc <= 10 * CPU_DEV_COV_W and dz <= 10 * CPU_DEV_FAR_WZ
    assert np.abs(dis["bounds"]["cov_wu"]).max() > 0
    # events on u: exactly 0 with the clamp, positive without; rat_user_event on u agrees with the quadratic event
    for hook, (_, _, q_, u_) in res.items():
        for k in ("prob", "n_viol"):
            assert np.array_equal(q_["thetas"][k], u_["thetas"][k]), (hook, k)
        assert np.array_equal(q_["margins"], u_["margins"])
    assert quad["thetas"]["prob"][0, 0] == 0.0 and quad["thetas"]["n_viol"][0, 0] == 0 and quad["margins"].max() == 0.0
    free_q = res[None][2]
    assert free_q["thetas"]["prob"][0, 0] > 0.25 and free_q["margins"].max() > 0.0


# ---- 7. set_params moves the limit without a recompile ----------------------------------------------------------------------------------------
def test_set_params_moves_the_limit_without_a_recompile():
    c = up.case("pend")
    prob = c.problem("clamp")
    ctx = rat.Context(prob)
    x_nom, l, L = c.policy
    kw = dict(noise=c.user_noise(seed=8), K=500, want_costs=True, want_trajectories=True)
    assert ctx.debug_get("src_un_loads") == 0
    a = ctx.policy_evaluate_noise(x_nom, l, L, **kw)
    assert np.abs(a["u"]).max() == c.q[0] and ctx.debug_get("src_un_loads") == 1
    ctx.policy_worst_case_trajectory(thetas=(0.0,))
    q = c.q.copy()
    q[0] = 0.5 * c.q[0]
    ctx.set_params(c.params(q))
    # a replay before the new evaluation runs under the new limit: its costs are not the stored ones
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*changed since the evaluation"):
        ctx.policy_worst_case_trajectory(thetas=(0.0,))
    b = ctx.policy_evaluate_noise(x_nom, l, L, **kw)
    assert np.abs(b["u"]).max() == q[0] and not np.array_equal(a["costs"], b["costs"])
    assert ctx.debug_get("src_un_loads") == 1                        # the module of the first call served both
    fresh = rat.Context(c.problem("clamp", q=q)).policy_evaluate_noise(x_nom, l, L, **kw)
    same_evaluation(b, fresh, "set_params")
    mu = ctx.policy_worst_case_trajectory(thetas=(0.0,))["thetas"]["mean_u"]
    assert np.all(np.abs(mu) <= q[0])
    # rat_policy_evaluate's kernel reads the same parameters
    g0 = rat.Context(prob).policy_evaluate(x_nom, l, L, K=500, seed=3, want_costs=True)["costs"]
    g1 = ctx.policy_evaluate(x_nom, l, L, K=500, seed=3, want_costs=True)["costs"]
    assert not np.array_equal(g0, g1)


# ---- 8. rare events -------------------------------------------------------------------------------------------------------------------------
def test_rare_events_against_a_plain_count():
    """the clamp source of the pendulum with rat_user_event g[0] = x[0] - q[0]: the threshold sits at the 0.99 quantile of a plain run of
    2^18 rollouts (between two neighbouring margins), so the plain count is about 2^18 / 100; the two importance-sampling estimates at
    K = 2^16 under other seeds lie within five combined standard errors of it (the count's binomial one and the estimate's own)."""
    c = up.case("pend")
    x_nom, l, L = c.policy
    K_PLAIN, K_IS = 1 << 18, 1 << 16
    evoff = 3 + up.N_HOOK_PARAMS
    src = ue.source(up.source(c.base, c.poff, "clamp"), "half", evoff)
    ctx = rat.Context(rat.DeviceSourceProblem(src, 2, 1, c.N, c.W, params=np.concatenate([c.params(), [0.0]])))
    ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=1), K=K_PLAIN)
    ex = np.array([1.0, 0.0, 0.0])
    M = np.sort(ctx.policy_events([rat.halfspace(ex, 0.0)], thetas=[0.0], want_margins=True)["margins"][0])
    i = int(0.99 * K_PLAIN)
    thr = 0.5 * (M[i] + M[i + 1])
    ctx.set_params(np.concatenate([c.params(), [thr]]))
    ev = rat.halfspace(ex, -thr)
    plain = ctx.policy_events([ev], thetas=[0.0])["thetas"]
    p = float(plain["n_viol"][0, 0]) / K_PLAIN
    assert 1e-3 < p < 1e-1 and plain["n_viol"][0, 0] == ctx.policy_events_user(1, thetas=[0.0])["thetas"]["n_viol"][0, 0]
    se_plain = np.sqrt(p * (1 - p) / K_PLAIN)
    a = ctx.policy_rare_event_noise(x_nom, l, L, ev, K_IS, noise=c.user_noise(seed=2), n_iter=4, rho=0.1)
    b = ctx.policy_rare_event_user(x_nom, l, L, 1, 0, K_IS, noise=c.user_noise(seed=3), n_iter=4, rho=0.1)
    for r, label in ((a, "quadratic"), (b, "user")):
        comb = np.hypot(r.prob_se, se_plain)
        print(f"rare {label}: PROB {r.prob:.5e} SE {r.prob_se:.2e}; plain {p:.5e} SE {se_plain:.2e}: {abs(r.prob - p) / comb:.2f} combined sigma")
        assert r.flag == 0 and r.n_domain == 0 and r.prob_se > 0
        assert abs(r.prob - p) <= 5.0 * comb
    # the two calls are one kernel text: under the same seed and shift, the same margins
    a0 = ctx.policy_rare_event_noise(x_nom, l, L, ev, 4096, noise=c.user_noise(seed=2), shift=a.shift, n_iter=0, want_margins=True, want_logw=True)
    b0 = ctx.policy_rare_event_user(x_nom, l, L, 1, 0, 4096, noise=c.user_noise(seed=2), shift=a.shift, n_iter=0, want_margins=True, want_logw=True)
    assert np.array_equal(a0.margins, b0.margins) and np.array_equal(a0.logw, b0.logw)
    # without a shift the margins are rat_policy_events' behind the evaluation at that seed: the rare kernel clamps as the rollout kernel does
    r0 = ctx.policy_rare_event_noise(x_nom, l, L, ev, 1000, noise=c.user_noise(seed=1), n_iter=0, want_margins=True)
    ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=1), K=1000)
    assert np.array_equal(r0.margins, ctx.policy_events([ev], thetas=[0.0], want_margins=True)["margins"][0])


def test_rare_events_set_dom_for_a_nan_from_the_hook():
    c = up.case("pend")
    x_nom, l, L = c.policy
    K = 2000
    evoff = 3 + up.N_HOOK_PARAMS
    src = ue.source(up.source(c.base, c.poff, "nan"), "half", evoff)
    ctx = rat.Context(rat.DeviceSourceProblem(src, 2, 1, c.N, c.W, params=np.concatenate([c.params(), [0.0]])))
    r = ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=9), K=K, want_costs=True, want_trajectories=True)
    assert r["n_domain"] == 0
    q = c.q.copy()
    q[2] = float(np.quantile(r["x"][:, :-1, 0].max(axis=1), 0.98))   # about forty rollouts cross it
    ctx.set_params(np.concatenate([c.params(q), [0.0]]))
    ref = ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=9), K=K, want_costs=True)
    assert 10 < ref["n_domain"] < 100
    ev = rat.halfspace(np.array([0.0, 1.0, 0.0]), 0.0)
    for call in (lambda **kw: ctx.policy_rare_event_noise(x_nom, l, L, ev, K, **kw), lambda **kw: ctx.policy_rare_event_user(x_nom, l, L, 1, 0, K, **kw)):
        got = call(noise=c.user_noise(seed=9), n_iter=0, want_margins=True)
        assert got.n_domain == ref["n_domain"] and got.n_ok == ref["n_ok"]
        assert np.array_equal(np.isnan(got.margins), np.isnan(ref["costs"]))


# ---- 9. generator runs -------------------------------------------------------------------------------------------------------------------------
def test_generator_repeats_bit_for_bit():
    c = up.case("pend")
    ctx = context("pend", "clamp")
    x_nom, l, L = c.policy
    K = 300
    kw = dict(noise=c.user_noise(seed=0x1234567890ABCDEF), thetas=(0.0, 0.7), K=K, want_costs=True, want_trajectories=True)
    a, b = ctx.policy_evaluate_noise(x_nom, l, L, **kw), ctx.policy_evaluate_noise(x_nom, l, L, **kw)
    same_evaluation(a, b, "repeat")
    assert a["n_ok"] == K and a["costs"].std() > 0 and np.unique(a["x"][:, c.N, 1]).size == K and np.abs(a["u"]).max() == c.q[0]
    check_stats(a, (0.0, 0.7))
    other = ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=2), K=K, want_costs=True)
    assert not np.array_equal(other["costs"], a["costs"])
    for tpw in (16, 32):                                             # every packing of the kernel
        ctx.debug_set("src_mc_tpw", tpw)
        assert np.array_equal(ctx.policy_evaluate_noise(x_nom, l, L, **kw)["costs"], a["costs"])
    ctx.debug_set("src_mc_tpw", 64)


def test_the_chunk_boundary_is_invisible():
    """rollout j has the same noise whatever K is and however the call is cut into launches: with trajectories the call runs in chunks of
    2^16 rollouts (two here, the second of 3); without them in one launch"""
    c = up.case("pend")
    N, K = 2, (1 << 16) + 3
    x_nom, l, L = um.pend_policy(N)
    L = 4.0 * L
    ctx = rat.Context(rat.DeviceSourceProblem(up.source(c.base, c.poff, "clamp"), 2, 1, N, c.W, params=c.params()))
    noise = c.user_noise(seed=77)
    a = ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=K, want_costs=True, want_trajectories=True)
    b = ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=K + 64, want_costs=True)
    assert a["n_ok"] == K and np.array_equal(a["costs"], b["costs"][:K])
    assert np.unique(a["costs"][-8:]).size == 8 and np.all(a["x"][-3:, 0] == x_nom[0]) and np.all(a["x"][-3:, N] != 0.0)
    assert np.abs(a["u"]).max() == c.q[0] and up.beyond(a["u"][-3:], 0.999 * c.q[0]) > 0
    # the trajectories of the second chunk are those of the costs: c(0) + c(1) + h on them
    x, u = a["x"][-3:], a["u"][-3:]
    ref = sum(um.pend_c(t, x[:, t].T, u[:, t].T, [0.1]) for t in range(N)) + um.pend_h(x[:, N].T, [0.1])
    assert np.allclose(a["costs"][-3:], ref, rtol=1e-10, atol=0.0)
