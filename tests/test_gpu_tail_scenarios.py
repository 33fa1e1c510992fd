"""rat_policy_tail_trajectory / _disturbance / _params on the GPU (csrc/policy_mc.hip: tlt_levels, tlt_weights and the liveness schedule
tlt_moments / tld_moments / tlp_moments behind the replay).

Per case: the rows against policy_tail_risk bit for bit; the moments against np.longdouble (`direct` of the worst-case models) under the
weights of tests/tail_scenarios_model.tail_weights on the evaluation's own costs and trajectories, held to MARGIN = 8 times the
restatement's own distance from np.longdouble that tests/test_cpu_tail_scenarios.py measures on the host (CPU_DEV_MEAN, CPU_DEV_COV);
alpha = 0 against the theta = 0 row of the worst-case sibling bit for bit, and the liveness schedule against the dense kernels on the
same weights (switch tail_dense) bit for bit -- the bit-neutrality of the skip; a level alone against the level among sixteen.

Shapes: (n, m, N) = (1, 1, 1), (5, 3, 4), (12, 4, 3); K = 1, 3 (the K tail inside a group), 4 WT_WAVES WT_SLOTS + 1 = 129 (one slot gets
a second group) and 2^16 + 5 (a second chunk of five rollouts).  Levels 0, 0.5, 0.9 and 1 - 0.5 / K (thinner than one rollout).  The
parameter call: the fourteen parameters of the LQ + cubic source (one tile) and the tiny source of tests/wc_params_model.py with P = 17
(a second tile with one live row) and P = 32 (full), the two-tile kernels."""
import numpy as np
import pytest

import rare_event_noise_model as rn
import ratilqr.jl_amd as rat
import tail_scenarios_model as ts
import user_noise_model as um
import user_params_model as pm
import wc_params_model as wp
from test_cpu_tail_scenarios import CLOSED_ALPHAS, CLOSED_K, CLOSED_SEED, CLOSED_SIGMA, KS, SHAPES, closed_form_check, levels
from test_cpu_wc_params import lqc_p
from test_gpu_user_noise import pend_problem
from test_gpu_wc_params import tiny_context, tiny_evaluate
from test_gpu_wc_disturbance import family_w
from test_gpu_wc_trajectory import full
from wc_disturbance_model import centre_w
from wc_disturbance_model import deviation as deviation_w
from wc_disturbance_model import direct as direct_w
from wc_disturbance_model import z_offset
from wc_trajectory_model import centre, deviation, direct

pytestmark = pytest.mark.gpu
MOMENT_KEYS_T = ("mean_x", "cov_x", "mean_u", "cov_u", "cov_xu")


def lq(n, m, N):
    prob, x0, _ = rat.synthetic_lq_problem(n=n, m=m, N=N, seed=n + N, w=0.09)
    r = np.random.default_rng(n)
    return prob, x0, 0.5 * r.standard_normal((N, m)), 0.1 * r.standard_normal((N, m, n))


def same(a, b, label, keys=None):
    for k in (a if keys is None else keys):
        assert np.array_equal(a[k], b[k], equal_nan=True), (label, k)


def rows_are_tail_risk(ctx, out, alphas, label):
    tr = ctx.policy_tail_risk(alphas)
    for k in tr:
        if k != "weights":
            assert np.array_equal(out[k], tr[k], equal_nan=True), (label, k)


def check_trajectory(ctx, x, u, costs, c, alphas, label):
    n, m = x.shape[2], u.shape[2]
    out = ctx.policy_tail_trajectory(alphas)
    rows_are_tail_risk(ctx, out, alphas, label)
    y, dead, info = ts.tail_weights(costs, alphas)
    assert np.array_equal(out["flag"], info["flag"]) and np.array_equal(out["var"], info["v"], equal_nan=True)
    mean, cov = full(out, n, m)
    mean_d, cov_d = direct(x, u, costs, y, dead)
    em, ec = deviation(mean, cov, mean_d, cov_d, c[:, list(range(n)) + list(range(12, 12 + m))], K=costs.size)
    print(f"{label}: longdouble mean {em:.2e} cov {ec:.2e}")
    assert em <= ts.MARGIN * ts.CPU_DEV_MEAN and ec <= ts.MARGIN * ts.CPU_DEV_COV, (label, em, ec)
    assert np.array_equal(cov, cov.swapaxes(-1, -2), equal_nan=True)
    ctx.debug_set("tail_dense", 1)                                   # the dense kernels on the same weights: the same bits
    try:
        same(out, ctx.policy_tail_trajectory(alphas), (label, "dense"))
    finally:
        ctx.debug_set("tail_dense", 0)
    return out


def check_disturbance(ctx, w, x, u, costs, c, alphas, label):
    n, m = x.shape[2], u.shape[2]
    out = ctx.policy_tail_disturbance(alphas)
    rows_are_tail_risk(ctx, out, alphas, label)
    y, dead, _ = ts.tail_weights(costs, alphas)
    got = (out["mean_w"], out["cov_w"], np.concatenate([out["cov_wx"], out["cov_wu"]], axis=-1))
    c_w = centre_w(w, costs)
    mean_z, cov_z = direct(x, u, costs, y, dead)
    zs = z_offset(mean_z[:, :-1], cov_z[:, :-1], c[:-1][:, list(range(n)) + list(range(12, 12 + m))])
    em, ec, ez = deviation_w(got, direct_w(w, x, u, costs, y, dead), c_w[:, :n], zs, K=costs.size)
    print(f"{label}: longdouble mean_w {em:.2e} cov_w {ec:.2e} cov_wz {ez:.2e}")
    assert em <= ts.MARGIN * ts.CPU_DEV_MEAN and ec <= ts.MARGIN * ts.CPU_DEV_COV and ez <= ts.MARGIN * ts.CPU_DEV_COV, (label, em, ec, ez)
    plain = ctx.policy_tail_disturbance(alphas, cross=False)
    assert "cov_wx" not in plain
    same(plain, out, (label, "cross=False"))
    ctx.debug_set("tail_dense", 1)
    try:
        same(out, ctx.policy_tail_disturbance(alphas), (label, "dense"))
    finally:
        ctx.debug_set("tail_dense", 0)
    return out


# ---- the LQ family -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES)
def test_lq_family(shape, K):
    n, m, N = shape
    prob, x0, l, L = lq(n, m, N)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)
    r = ctx.policy_evaluate(x_det, l, L, K=K, seed=5, want_costs=True)
    x, u, cost, _ = ctx.rollout_noisy(x_det, l, L, K=K, seed=5)
    assert np.array_equal(cost, r["costs"])
    al, c, label = levels(K), centre(x_det, l), f"lq {n} x {m}, N = {N}, K = {K}"
    out = check_trajectory(ctx, x, u, cost, c, al, label)
    assert out["flag"][-1] == 1 and np.array_equal(out["flag"], [1 if K - K * a < 1.0 else 0 for a in al])   # 1 - 0.5 / K: thinner than one rollout
    sat = int(np.argmax(cost))
    assert np.abs(out["mean_x"][-1] - x[sat]).max() <= 8 * np.finfo(float).eps * np.abs(x).max()
    outw = check_disturbance(ctx, family_w(prob, 5, K), x, u, cost, c, al, label)
    # alpha = 0 is the nominal row of the worst-case siblings, bit for bit
    same(ctx.policy_worst_case_trajectory(thetas=(0.0,))["thetas"], {k: out[k][:1] for k in MOMENT_KEYS_T}, (label, "alpha = 0"), MOMENT_KEYS_T)
    wd = ctx.policy_worst_case_disturbance(thetas=(0.0,))["thetas"]
    same(wd, {k: outw[k][:1] for k in ("mean_w", "cov_w", "cov_wx", "cov_wu")}, (label, "alpha = 0, w"), ("mean_w", "cov_w", "cov_wx", "cov_wu"))


def test_row_by_row_and_sixteen_levels():
    prob, x0, l, L = lq(5, 3, 4)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)
    ctx.policy_evaluate(x_det, l, L, K=301, seed=4)
    al = tuple(0.06 * i for i in range(16))                           # 0, 0.06 ... 0.9
    a = ctx.policy_tail_trajectory(al)
    same(a, ctx.policy_tail_trajectory(al), "again")
    rows_are_tail_risk(ctx, a, al, "sixteen")
    aw = ctx.policy_tail_disturbance(al)
    for i in (0, 7, 15):                                              # a level alone and among sixteen: the same bits
        one, onew = ctx.policy_tail_trajectory((al[i],)), ctx.policy_tail_disturbance((al[i],))
        for k in one:
            assert np.array_equal(one[k][0], a[k][i], equal_nan=True), (i, k)
        for k in onew:
            assert np.array_equal(onew[k][0], aw[k][i], equal_nan=True), (i, k)


def check_params(ctx, q, costs, alphas, label):
    """the parameter call against the rows, np.longdouble, the sibling's theta = 0 row, itself without the cost sums and the dense kernels"""
    op = ctx.policy_tail_params(alphas)
    rows_are_tail_risk(ctx, op, alphas, label)
    R, P = len(alphas), q.shape[1]
    assert op["mean_q"].shape == (R, P) and op["cov_q"].shape == (R, P, P) and op["cov_qJ"].shape == (R, P)
    y, dead, _ = ts.tail_weights(costs, alphas)
    c_q, c_J = wp.centre(q, costs)
    with np.errstate(all="ignore"):
        mean_J = np.array([(y[i] * costs).sum() / y[i].sum() for i in range(R)])
    dm, dc, dj = wp.deviation((op["mean_q"], op["cov_q"], op["cov_qJ"]), wp.direct(q, costs, y, dead), c_q, c_J, mean_J)
    print(f"{label}: parameters against longdouble mean {dm:.2e} cov_q {dc:.2e} cov_qJ {dj:.2e}")
    assert dm <= ts.MARGIN * ts.CPU_DEV_MEAN and dc <= ts.MARGIN * ts.CPU_DEV_COV and dj <= ts.MARGIN * ts.CPU_DEV_COV, (label, dm, dc, dj)
    assert np.array_equal(op["cov_q"], op["cov_q"].swapaxes(-1, -2), equal_nan=True)
    wq = ctx.policy_worst_case_params(thetas=(0.0,))["thetas"]
    same(wq, {k: op[k][:1] for k in ("mean_q", "cov_q", "cov_qJ")}, (label, "alpha = 0, q"), ("mean_q", "cov_q", "cov_qJ"))
    plain = ctx.policy_tail_params(alphas, cost=False)
    assert "cov_qJ" not in plain
    same(plain, op, (label, "cost=False"))
    ctx.debug_set("tail_dense", 1)
    try:
        same(op, ctx.policy_tail_params(alphas), (label, "dense, q"))
    finally:
        ctx.debug_set("tail_dense", 0)
    return op


# ---- a source model under rat_user_noise, and its parameters -------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_source_model_with_parameters(K):
    """the fourteen-parameter LQ + cubic source of tests/test_gpu_user_params.py: all three calls on one evaluation"""
    c = pm.case("lq12")
    N, p = 3, lqc_p()
    ctx = rat.Context(c.problem("scale", p=p, N=N))
    ctx.set_param_sampling(rat.ParamSampling(pm.PARAM_NORMALS, pm.PARAM_UNIFORMS))
    r0 = np.random.default_rng(3)
    x_nom, l, L = 0.5 * r0.standard_normal((N + 1, c.n)), 0.8 * r0.standard_normal((N, c.m)), 0.1 * r0.standard_normal((N, c.m, c.n))
    r = ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=21), K=K, want_costs=True, want_trajectories=True)
    q = ctx.sample_params(K, seed=21)
    assert r["n_ok"] == K
    al, label = levels(K), f"lqc14 K = {K}"
    out = check_trajectory(ctx, r["x"], r["u"], r["costs"], centre(x_nom, l), al, label)
    same(ctx.policy_worst_case_trajectory(thetas=(0.0,))["thetas"], {k: out[k][:1] for k in MOMENT_KEYS_T}, (label, "alpha = 0"), MOMENT_KEYS_T)
    # the disturbances: the rows, alpha = 0 against the sibling, the schedule against the dense kernels
    ow = ctx.policy_tail_disturbance(al)
    rows_are_tail_risk(ctx, ow, al, label)
    keys_w = ("mean_w", "cov_w", "cov_wx", "cov_wu")
    same(ctx.policy_worst_case_disturbance(thetas=(0.0,))["thetas"], {k: ow[k][:1] for k in keys_w}, (label, "alpha = 0, w"), keys_w)
    ctx.debug_set("tail_dense", 1)
    try:
        same(ow, ctx.policy_tail_disturbance(al), (label, "dense, w"))
    finally:
        ctx.debug_set("tail_dense", 0)
    # the parameters against np.longdouble
    op = check_params(ctx, q, r["costs"], al, label)
    if K == 1:                                                        # one rollout: every level is that rollout, and exactly no covariance
        assert np.array_equal(op["flag"], [0, 1, 1, 1]) and not op["cov_q"].any()
        assert np.abs(op["mean_q"] - q[0]).max() <= 4 * np.finfo(float).eps * np.abs(q).max()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("P", [17, 32])
def test_parameters_in_two_tiles(P, K):
    """more than sixteen parameters: the two-tile instantiations of tlp_moments, on the tiny source of tests/test_gpu_wc_params.py"""
    ctx, _ = tiny_context(P)
    r = tiny_evaluate(ctx, K, seed=7)
    q = ctx.sample_params(K, seed=7)
    assert r["n_ok"] == K
    check_params(ctx, q, r["costs"], levels(K), f"tiny P = {P}, K = {K}")
    if K == 129:
        al = tuple(0.06 * i for i in range(16))                       # sixteen levels: two row batches
        a = check_params(ctx, q, r["costs"], al, f"tiny P = {P}, K = {K}, sixteen levels")
        one = ctx.policy_tail_params((al[15],))
        for k in one:
            assert np.array_equal(one[k][0], a[k][15], equal_nan=True), k


_CLOSED = {}


def closed_context():
    if "ctx" not in _CLOSED:
        _CLOSED["ctx"] = rat.Context(rat.DeviceSourceProblem(CLOSED_SRC, 1, 1, 1, np.eye(1), params=[CLOSED_SIGMA]))
    return _CLOSED["ctx"]


@pytest.mark.parametrize("K", KS)
def test_source_model_disturbances_against_longdouble(K):
    """the 1 x 1 source of the closed form: w_0 = sigma z_0 under the generator's normals, against np.longdouble"""
    x0, u0, seed = 0.3, -0.1, 17
    ctx = closed_context()
    l = np.array([[u0]])
    r = ctx.policy_evaluate_noise(np.array([x0]), l, None, noise=rat.UserNoise(1, 0, seed=seed), K=K, want_costs=True, want_trajectories=True)
    assert r["n_ok"] == K
    w = CLOSED_SIGMA * rn.normals(seed, 0, K, 1, 1)
    assert np.abs(r["x"][:, 1] - (x0 + u0 + w[:, 0])).max() <= 4 * np.finfo(float).eps  # (w is the sampler's, to the rounding of the sum)
    c = centre(np.array([[x0], [x0 + u0]]), l)
    check_disturbance(ctx, w, r["x"], r["u"], r["costs"], c, levels(K), f"1 x 1 source, K = {K}")


# ---- ties, DomainErrors, Inf: one small source --------------------------------------------------------------------------------------------
# x_0' = x_0 + u + w_0 with w_0 a step function of the draw, in quarters of p[0], and the cost is x_0 at the end: hundreds of rollouts tie;
# x_1 overflows to Inf where the draw is low (p[1] on) -- rollouts whose cost is small; the sampler returns NaN where the draw is above p[2]
STEP_SRC = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) {
    xn[0] = x[0] + u[0];
    xn[1] = x[1];
}
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) { return 0.0 * x[0]; }
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return x[0]; }
""" + um.NOISE_HEAD + r"""
    const double z = rng.normal();
    w[0] = (z > p[2]) ? sqrt(p[2] - z) : p[0] * 0.25 * floor(4.0 * z);
    w[1] = (p[1] != 0.0 && z < -1.0) ? 1e308 * 10.0 : 0.0;
}
"""


X0_TINY, L_TINY = np.array([0.3]), np.zeros((2, 1))                  # (the tiny source's open-loop policy, as tests/test_gpu_wc_params.py has it)


def step_context(inf=0.0, nan_above=1e9):
    return rat.Context(rat.DeviceSourceProblem(STEP_SRC, 2, 1, 1, 1e-3 * np.eye(2), params=[0.5, inf, nan_above]))


def step_eval(ctx, K, seed=9):
    return ctx.policy_evaluate_noise(np.array([0.1, 0.0]), np.zeros((1, 1)), None, noise=rat.UserNoise(1, 0, seed=seed), K=K, want_costs=True,
                                     want_trajectories=True)


def test_ties_at_the_quantile():
    ctx = step_context()
    K = 4001
    r = step_eval(ctx, K)
    J = r["costs"]
    assert np.array_equal(J, r["x"][:, 1, 0]) and np.unique(J).size < 60
    al = (0.0, 0.5, 0.9)
    y, dead, info = ts.tail_weights(J, al)
    assert all((J == info["v"][i]).sum() > 100 for i in (1, 2))       # hundreds tie at the quantiles inside the sample (level 0: the minimum)
    out = check_trajectory(ctx, r["x"], r["u"], J, centre(np.array([[0.1, 0.0], [0.1, 0.0]]), np.zeros((1, 1))), al, "ties")
    # the atom's weight: S0 of the level is tail_n, and the ESS is that of the model's weights
    assert np.allclose(out["ess"], y.sum(axis=1) ** 2 / (y ** 2).sum(axis=1), rtol=1e-13)
    w0 = ctx.policy_tail_risk((0.0,), want_weights=True)["weights"]
    assert abs(w0.sum() - 1.0) <= 1e-13
    for i, a in enumerate(al):                                        # the normalised weights of every level, level by level
        w = ctx.policy_tail_risk((a,), want_weights=True)["weights"]
        assert np.allclose(w, y[i] / y[i].sum(), rtol=1e-13, atol=0)


def test_domain_errors_carry_no_weight_and_an_empty_sample_is_nan():
    ctx = step_context(nan_above=1.0)
    r = step_eval(ctx, 2000)
    bad = np.isnan(r["costs"])
    assert 0.05 * 2000 < bad.sum() < 0.3 * 2000
    out = check_trajectory(ctx, r["x"], r["u"], r["costs"], centre(np.array([[0.1, 0.0], [0.1, 0.0]]), np.zeros((1, 1))), (0.0, 0.5, 0.9), "nan")
    assert out["tail_n"][0] == (~bad).sum() and np.isfinite(out["cov_x"]).all()
    ctx.set_params([0.5, 0.0, -1e9])                                  # every draw fails
    r = step_eval(ctx, 9)
    assert r["n_ok"] == 0
    for out in (ctx.policy_tail_trajectory((0.0, 0.9)), ctx.policy_tail_disturbance((0.0, 0.9))):
        assert np.all(out["flag"] == 2)
        assert all(np.isnan(out[k]).all() for k in out if k.startswith(("mean", "cov")))


def test_a_rollout_without_weight_that_overflows_is_left_out():
    ctx = step_context(inf=1.0)
    r = step_eval(ctx, 1000)
    J, x = r["costs"], r["x"]
    blown = np.isinf(x[:, 1, 1])
    assert 100 < blown.sum() < 250 and np.isfinite(J).all()
    out = ctx.policy_tail_trajectory((0.0, 0.9))
    y, _, info = ts.tail_weights(J, (0.0, 0.9))
    assert not (y[1][blown] != 0).any()                               # the overflowing rollouts are all below the 0.9 quantile
    assert not np.isfinite(out["mean_x"][0, 1, 1])                    # the whole sample holds them: Inf or NaN there
    assert np.isfinite(out["mean_x"][1]).all() and np.isfinite(out["cov_x"][1]).all()
    keep = y[1] != 0
    ref = (y[1][keep] * x[keep, 1, 0]).sum() / y[1][keep].sum()
    assert abs(out["mean_x"][1, 1, 0] - ref) <= 1e-13 and out["mean_x"][1, 1, 1] == 0.0 and out["cov_x"][1, 1, 1, 1] == 0.0


# ---- the closed form -----------------------------------------------------------------------------------------------------------------------
CLOSED_SRC = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) { xn[0] = x[0] + u[0]; }
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) { return 0.0 * x[0]; }
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return x[0]; }
""" + um.NOISE_HEAD + r"""
    w[0] = p[0] * rng.normal();
}
"""


def test_closed_form_on_the_device():
    x0, u0 = 0.3, -0.1
    ctx = closed_context()
    r = ctx.policy_evaluate_noise(np.array([x0]), np.array([[u0]]), None, noise=rat.UserNoise(1, 0, seed=CLOSED_SEED), K=CLOSED_K, want_costs=True)
    assert r["n_ok"] == CLOSED_K
    out = ctx.policy_tail_trajectory(CLOSED_ALPHAS)
    assert np.all(out["flag"] == 0)
    closed_form_check(None, r["costs"], out["mean_x"][:, 1, 0], out["cov_x"][:, 1, 0, 0], x0, u0, "device")
    assert np.allclose(out["mean_x"][:, 1, 0], out["cvar"], rtol=1e-12)     # J = x_1: the tail's mean state is the CVaR
    ow = ctx.policy_tail_disturbance(CLOSED_ALPHAS)
    assert np.allclose(ow["mean_w"][:, 0, 0], out["mean_x"][:, 1, 0] - (x0 + u0), rtol=1e-10, atol=1e-13)


# ---- the refusals --------------------------------------------------------------------------------------------------------------------------
RAT_ERR_ARG = 1                                                       # (include/ratilqr.h)


def test_refusals_of_the_parameter_call():
    mu, Cq, a, b = wp.tiny_tables(3)
    ctx = rat.Context(rat.DeviceSourceProblem(wp.tiny_source(3, Cq, a, b, "gauss", None), 1, 1, 2, np.eye(1), params=mu))
    ctx.set_param_sampling(rat.ParamSampling(3, 0))
    name, f = "rat_policy_tail_params", ctx.policy_tail_params
    with pytest.raises(rat.RatError, match=f"RAT_ERR_ARG.*{name}.*no evaluation"):           # nothing to replay yet
        f((0.5,))
    tiny_evaluate(ctx, 20, seed=1)
    for bad in ((1.0,), (-0.1,), (np.nan,), (), tuple(0.05 * i for i in range(17))):          # rat_policy_tail_risk's rules
        with pytest.raises(rat.RatError, match=f"RAT_ERR_ARG.*{name}"):
            f(bad)
    good = f((0.0, 0.5))
    assert good["ess"][0] == 20                                                              # ... leave the handle usable
    lib, nv = rat.native.lib(), rat.native
    al, rows = nv.f64(np.array([0.5])), np.zeros(8)
    assert lib.rat_policy_tail_params(ctx.h, nv.P(al), 1, nv.P(rows), None, None, None) == RAT_ERR_ARG       # null outputs
    assert b"rat_policy_tail_params: null alpha / output" in lib.rat_last_error()
    assert lib.rat_policy_tail_params(ctx.h, nv.P(al), 1, None, nv.P(np.zeros(3)), nv.P(np.zeros(9)), None) == RAT_ERR_ARG
    assert b"rat_policy_tail_params: null alpha / output" in lib.rat_last_error()
    ctx.policy_tail_risk((0.5,), costs=np.arange(20.0))                                      # uploaded costs are no evaluation's
    with pytest.raises(rat.RatError, match=f"RAT_ERR_ARG.*{name}.*no evaluation's"):
        f((0.5,))
    ctx.policy_evaluate(X0_TINY, L_TINY, K=16, seed=1)                                       # under N(0, W)
    with pytest.raises(rat.RatError, match=f"RAT_ERR_UNSUPPORTED.*{name}.*rat_user_noise"):
        f((0.5,))
    ctx.policy_evaluate_noise(X0_TINY, L_TINY, None, noise=rat.UserNoise(1, 0, zn=np.zeros((4, 2, 1))))      # injected draws are not kept
    with pytest.raises(rat.RatError, match=f"RAT_ERR_UNSUPPORTED.*{name}.*injected"):
        f((0.5,))
    tiny_evaluate(ctx, 20, seed=1)
    ctx.set_params(mu + 0.5)                                                                 # the parameters changed behind the evaluation
    with pytest.raises(rat.RatError, match=f"RAT_ERR_ARG.*{name}.*20 replayed.*changed since the evaluation"):
        f((0.5,))
    ctx.set_params(mu)
    tiny_evaluate(ctx, 20, seed=1)
    same(good, f((0.0, 0.5)), "after the refusals")
    wide_prob, wx0, wu = rat.synthetic_lq_problem(n=16, m=4, N=5, seed=3, w=1e-2)             # general sizes
    wide = rat.Context(wide_prob)
    wide.policy_evaluate(wx0, wu, K=8, seed=1)
    with pytest.raises(rat.RatError, match=f"RAT_ERR_UNSUPPORTED.*{name}"):
        wide.policy_tail_params((0.5,))
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rat_policy_tail_disturbance.*n <= 12"):
        wide.policy_tail_disturbance((0.5,))


def test_refusals():
    prob, x0, l, L = lq(5, 3, 4)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)
    calls = (("rat_policy_tail_trajectory", ctx.policy_tail_trajectory), ("rat_policy_tail_disturbance", ctx.policy_tail_disturbance))
    for name, f in calls:
        with pytest.raises(rat.RatError, match=f"RAT_ERR_ARG.*{name}.*no evaluation"):       # nothing to replay yet
            f((0.5,))
    ctx.policy_evaluate(x_det, l, L, K=20, seed=1)
    for name, f in calls:
        for bad in ((1.0,), (-0.1,), (np.nan,), (), tuple(0.05 * i for i in range(17))):      # rat_policy_tail_risk's rules
            with pytest.raises(rat.RatError, match=f"RAT_ERR_ARG.*{name}"):
                f(bad)
        assert f((0.0,))["ess"][0] == 20                                                     # ... leave the handle usable
    lib, nv = rat.native.lib(), rat.native
    al, rows = nv.f64(np.array([0.5])), np.zeros(8)
    assert lib.rat_policy_tail_trajectory(ctx.h, nv.P(al), 1, nv.P(rows), None, None) == RAT_ERR_ARG      # null outputs
    assert b"rat_policy_tail_trajectory: null alpha / output" in lib.rat_last_error()
    assert lib.rat_policy_tail_disturbance(ctx.h, nv.P(al), 1, nv.P(rows), None, None, None) == RAT_ERR_ARG
    assert b"rat_policy_tail_disturbance: null alpha / output" in lib.rat_last_error()
    assert lib.rat_policy_tail_trajectory(ctx.h, None, 1, nv.P(rows), nv.P(np.zeros(40)), nv.P(np.zeros(320))) == RAT_ERR_ARG
    assert b"rat_policy_tail_trajectory: null alpha / output" in lib.rat_last_error() and ctx.policy_tail_trajectory((0.0,))["ess"][0] == 20
    ctx.policy_tail_risk((0.5,), costs=np.arange(20.0))                                      # uploaded costs are no evaluation's
    for name, f in calls:
        with pytest.raises(rat.RatError, match=f"RAT_ERR_ARG.*{name}.*no evaluation's"):
            f((0.5,))
    ctx.policy_evaluate(x_det, l, L, z=np.random.default_rng(0).standard_normal((8, 4, 5)))  # injected draws are not kept
    for name, f in calls:
        with pytest.raises(rat.RatError, match=f"RAT_ERR_UNSUPPORTED.*{name}.*injected"):
            f((0.5,))
    # the problem changed behind the evaluation: the replay guard's count
    ctx.policy_evaluate(x_det, l, L, K=50, seed=1)
    good = ctx.policy_tail_trajectory((0.5,))
    p2, _, _ = rat.synthetic_lq_problem(n=5, m=3, N=4, seed=10, w=0.09)                      # (another A and B; lq's seed is n + N = 9)
    ctx.set_problem(p2)
    for name, f in calls:
        with pytest.raises(rat.RatError, match=f"RAT_ERR_ARG.*{name}.*50 replayed.*changed since the evaluation"):
            f((0.5,))
    ctx.set_problem(prob)
    assert ctx.policy_evaluate(x_det, l, L, K=50, seed=1)["n_ok"] == 50
    same(good, ctx.policy_tail_trajectory((0.5,)), "after the refusals")
    # the parameter call: not a source model; sampling off
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rat_policy_tail_params.*not a source model"):
        ctx.policy_tail_params((0.5,))
    # a source under N(0, W); the parameter call without sampling
    N = 3
    x_nom, pl, pL = um.pend_policy(N)
    src = rat.Context(pend_problem(um.PEND_STATE, N, um.PEND_STATE_P))
    src.policy_evaluate(x_nom, pl, pL, K=16, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rat_policy_tail_trajectory.*rat_user_noise"):
        src.policy_tail_trajectory((0.5,))
    assert src.policy_evaluate_noise(x_nom, pl, pL, noise=rat.UserNoise(3, 0, seed=1), K=16)["n_ok"] == 16
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*rat_policy_tail_params.*rat_policy_params_sampling"):
        src.policy_tail_params((0.5,))
    assert src.policy_tail_disturbance((0.5,))["flag"][0] == 0
    # general sizes
    wide_prob, wx0, wu = rat.synthetic_lq_problem(n=16, m=4, N=5, seed=3, w=1e-2)
    wide = rat.Context(wide_prob)
    wide.policy_evaluate(wx0, wu, K=8, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rat_policy_tail_trajectory.*n <= 12"):
        wide.policy_tail_trajectory((0.5,))
    # rows x steps above the caps
    long_prob = rat.LQRiskSensitiveProblem(np.eye(2), np.eye(2), Q=np.eye(2), R=np.eye(2), N=400, W=np.eye(2), Qf=np.eye(2))
    lc = rat.Context(long_prob)
    lc.policy_evaluate(np.zeros(2), np.zeros((400, 2)), K=4, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rat_policy_tail_trajectory.*3640"):
        lc.policy_tail_trajectory(tuple(0.05 * i for i in range(10)))
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rat_policy_tail_disturbance.*1899"):
        lc.policy_tail_disturbance(tuple(0.05 * i for i in range(5)))
    assert lc.policy_tail_trajectory((0.5,))["mean_x"].shape == (1, 401, 2)
