"""Monte-Carlo evaluation of a source model's policy under user-written process noise on the GPU (rat_policy_evaluate_noise,
Context.policy_evaluate_noise, csrc/source_user_noise.h).  Checked against the NumPy restatement of tests/user_noise_model.py on injected
draws, against rat_policy_evaluate for a sampler that is the model's own Gaussian, against itself across chunkings of K, and
statistically against NumPy's generator.

Tolerances are those tests/test_gpu_source_pets.py holds the same models' injected-draw costs to: 1e-10 relative for the pendulum
(device and host sin differ by ulps), 1e-11 for the LQ family written as source.  Costs are held element by element; states and controls
relative to the largest entry of the rollout set, because a state component can pass through zero."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
from policy_mc_model import reduce_costs
import user_noise_model as um

pytestmark = pytest.mark.gpu
TOL_PEND, TOL_LQ = 1e-10, 1e-11


def close(got, ref, tol):
    return np.all(np.isfinite(ref)) and np.all(np.abs(got - ref) <= tol * np.abs(ref))


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def pend_problem(src, N, params, W=None):
    return rat.DeviceSourceProblem(src, 2, 1, N, 1e-3 * np.eye(2) if W is None else W, params=params)


def check_stats(r, thetas):
    """The statistics are the reduction (tests/policy_mc_model.py restates its order) of the device's own costs, as
    tests/test_gpu_policy_mc.py checks rat_policy_evaluate."""
    mdl = reduce_costs(r["costs"], thetas)
    assert r["n_ok"] == mdl["n_ok"] and r["n_domain"] == mdl["n_domain"]
    for key in ("mean", "var", "se_mean", "risk", "risk_se"):
        assert np.allclose(r[key], mdl[key], rtol=1e-12, atol=0.0, equal_nan=True), key
    ok = ~np.isnan(r["costs"])
    if ok.any():
        assert r["min"] == r["costs"][ok].min() and r["max"] == r["costs"][ok].max()


# ---- 1. injected draws against NumPy ----------------------------------------------------------------------------------------------------
_REF = {}


def injected_case(model):
    """(context, NumPy f / c / h / noise, p, policy, draws for 65 rollouts, draw counts, tolerance), built once per model."""
    if model not in _REF:
        rng = np.random.default_rng(5)
        K, N = 65, 3
        if model == "pendulum":
            x_nom, l, L = um.pend_policy(N)
            ctx = rat.Context(pend_problem(um.PEND_STATE, N, um.PEND_STATE_P))
            fns = (um.pend_f, um.pend_c, um.pend_h, um.pend_state_noise)
            _REF[model] = (ctx, fns, um.PEND_STATE_P, (x_nom, l, L), rng.standard_normal((K, N, 3)), None, 3, 0, TOL_PEND)
        else:
            gp = um.lq_generative(Nh=N)
            mdl = um.LqNumpy(gp)
            ctx = rat.Context(um.lq_source_problem(gp))
            x_nom = rng.standard_normal((N + 1, 12))
            l, L = 0.3 * rng.standard_normal((N, 4)), 0.1 * rng.standard_normal((N, 4, 12))
            _REF[model] = (ctx, (mdl.f, mdl.c, mdl.h, mdl.noise), None, (x_nom, l, L), rng.standard_normal((K, N, 12)), rng.random((K, N, 1)),
                           12, 1, TOL_LQ)
    return _REF[model]


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("K", [1, 65])
@pytest.mark.parametrize("model", ["pendulum", "lq"])
def test_injected_draws_against_numpy(model, K, closed):
    ctx, fns, p, (x_nom, l, L), zn, zu, npn, npu, tol = injected_case(model)
    xa, La = (x_nom, L) if closed else (x_nom[0], None)
    zn_k, zu_k = zn[:K], None if zu is None else zu[:K]
    thetas = (0.0, 0.4)
    r = ctx.policy_evaluate_noise(xa, l, La, noise=rat.UserNoise(npn, npu, zn=zn_k, zu=zu_k), thetas=thetas, want_costs=True,
                                  want_trajectories=True)
    cost, xs, us = um.np_rollouts(*fns, p, xa, l, La, K, zn_k.ravel(), None if zu_k is None else zu_k.ravel(), npn, npu)
    print(f"{model} K={K} closed={closed}: cost err {np.abs(r['costs'] / cost - 1).max():.2e}, x err {rel(r['x'], xs):.2e}, u err {rel(r['u'], us):.2e}")
    assert r["costs"].shape == (K,) and r["x"].shape == xs.shape and r["u"].shape == us.shape
    assert r["n_ok"] == K and r["n_domain"] == 0
    assert close(r["costs"], cost, tol) and rel(r["x"], xs) < tol and rel(r["u"], us) < tol
    if model == "lq" and K == 65:
        assert np.unique(zu_k < 0.3).size == 2                      # both mixture components occur
    if closed:
        assert rel(us, np.broadcast_to(l, us.shape)) > 1e-3         # the feedback term is exercised
    check_stats(r, thetas)
    # without the trajectories (one launch, no staging) and without the costs on the host: the same bits
    r2 = ctx.policy_evaluate_noise(xa, l, La, noise=rat.UserNoise(npn, npu, zn=zn_k, zu=zu_k), thetas=thetas, want_costs=True)
    assert r2["x"] is None and r2["u"] is None and np.array_equal(r2["costs"], r["costs"]) and r2["mean"] == r["mean"]
    r3 = ctx.policy_evaluate_noise(xa, l, La, noise=rat.UserNoise(npn, npu, zn=zn_k, zu=zu_k), thetas=thetas)
    assert r3["costs"] is None and r3["mean"] == r["mean"] and np.array_equal(r3["risk"], r["risk"])


# ---- 2. the Gaussian special case ---------------------------------------------------------------------------------------------------
def test_a_diagonal_gaussian_sampler_reproduces_policy_evaluate():
    """w_i = s_i z_i with injected z is the model noise chol(diag(s^2)) z of rat_policy_evaluate on the same z.  Not bit for bit: the add
    of w may contract differently across the inlined user code."""
    N, K = 6, 65
    s = np.array([0.03, 0.05])
    x_nom, l, L = um.pend_policy(N)
    ctx = rat.Context(pend_problem(um.PEND_DIAG, N, [0.1, s[0], s[1]], W=np.diag(s ** 2)))
    z = np.random.default_rng(9).standard_normal((K, N, 2))
    for xa, La in ((x_nom[0], None), (x_nom, L)):
        a = ctx.policy_evaluate(xa, l, La, z=z, want_costs=True)
        b = ctx.policy_evaluate_noise(xa, l, La, noise=rat.UserNoise(2, 0, zn=z), want_costs=True)
        print(f"gaussian special case: cost err {np.abs(b['costs'] / a['costs'] - 1).max():.2e}")
        assert a["n_ok"] == b["n_ok"] == K and close(b["costs"], a["costs"], TOL_PEND)


# ---- 3. generator mode -----------------------------------------------------------------------------------------------------------------
def test_generator_repeats_bit_for_bit():
    N, K = 5, 300
    x_nom, l, L = um.pend_policy(N)
    ctx = rat.Context(pend_problem(um.PEND_STATE, N, um.PEND_STATE_P))
    kw = dict(noise=rat.UserNoise(3, 0, seed=0x1234567890ABCDEF), thetas=(0.0, 0.7), K=K, want_costs=True, want_trajectories=True)
    a, b = ctx.policy_evaluate_noise(x_nom, l, L, **kw), ctx.policy_evaluate_noise(x_nom, l, L, **kw)
    for key in ("n_ok", "mean", "var", "min", "max", "se_mean"):
        assert a[key] == b[key], key
    for key in ("risk", "risk_se", "costs", "x", "u"):
        assert np.array_equal(a[key], b[key]), key
    assert a["n_ok"] == K and a["costs"].std() > 0 and np.unique(a["x"][:, N, 1]).size == K
    check_stats(a, (0.0, 0.7))
    c = ctx.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(3, 0, seed=2), K=K, want_costs=True)
    assert not np.array_equal(c["costs"], a["costs"])
    # every packing of the kernel
    for tpw in (16, 32):
        ctx.debug_set("src_mc_tpw", tpw)
        assert np.array_equal(ctx.policy_evaluate_noise(x_nom, l, L, **kw)["costs"], a["costs"])
    ctx.debug_set("src_mc_tpw", 64)


def test_the_chunk_boundary_is_invisible():
    """The generator counts rollouts globally: rollout j has the same noise whatever K is and however the call is cut into launches.  With
    trajectories the call runs in chunks of 2^16 rollouts (two here, the second of 3); without them in one launch."""
    N, K = 2, (1 << 16) + 3
    x_nom, l, L = um.pend_policy(N)
    ctx = rat.Context(pend_problem(um.PEND_MIX, N, [0.1, 0.02, 0.03, 0.25, 0.2]))
    noise = rat.UserNoise(2, 1, seed=77)
    a = ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=K, want_costs=True, want_trajectories=True)
    b = ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=K + 64, want_costs=True)
    assert a["n_ok"] == K and np.array_equal(a["costs"], b["costs"][:K])
    assert np.unique(a["costs"][-8:]).size == 8 and np.all(a["x"][-3:, 0] == x_nom[0]) and np.all(a["x"][-3:, N] != 0.0)
    # the trajectories of the second chunk are those of the costs: c(0) + c(1) + h on them
    x, u = a["x"][-3:], a["u"][-3:]
    ref = sum(um.pend_c(t, x[:, t].T, u[:, t].T, [0.1]) for t in range(N)) + um.pend_h(x[:, N].T, [0.1])
    assert close(a["costs"][-3:], ref, TOL_PEND)


def test_generator_mean_against_numpys_generator():
    """Other streams, the same distribution: the device mean of K = 20 000 costs lies within 5 of its own standard errors of the mean of a
    NumPy run of the same sampler (tests/test_cpu_user_noise.py checks that two NumPy runs agree at that margin)."""
    N, K = 10, 20000
    x_nom, l, L = um.pend_policy(N)
    ctx = rat.Context(pend_problem(um.PEND_STATE, N, um.PEND_STATE_P))
    r = ctx.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(3, 0, seed=314159), K=K)
    ref = um.np_pend_state_costs(um.PEND_STATE_P, x_nom, l, L, K, seed=101)
    print(f"generator: device mean {r['mean']:.6f} se {r['se_mean']:.2e}, NumPy mean {ref.mean():.6f}, var ratio {r['var'] / ref.var(ddof=1):.4f}")
    assert r["n_ok"] == K and r["se_mean"] > 0
    assert abs(r["mean"] - ref.mean()) <= 5.0 * r["se_mean"]


# ---- 4. DomainError ------------------------------------------------------------------------------------------------------------------
def test_a_nan_from_the_sampler_is_a_domain_error():
    N, K = 4, 70
    x0, l = np.array([0.4, -0.3]), 0.1 * np.ones((N, 1))
    zn = np.random.default_rng(2).uniform(-2.0, 2.0, (K, N, 1))
    zn[66, 2, 0] = 3.5                                               # beyond 3: sqrt of a negative number in rollout 66 alone
    ctx = rat.Context(pend_problem(um.PEND_NAN, N, [0.1, 0.05]))
    r = ctx.policy_evaluate_noise(x0, l, noise=rat.UserNoise(1, 0, zn=zn), thetas=(0.0, 1.0), want_costs=True, want_trajectories=True)
    cost, xs, _ = um.np_rollouts(um.pend_f, um.pend_c, um.pend_h, um.pend_nan_noise, [0.1, 0.05], x0, l, None, K, zn.ravel(), None, 1, 0)
    assert r["n_ok"] == K - 1 and r["n_domain"] == 1
    assert np.array_equal(np.isnan(r["costs"]), np.arange(K) == 66) and np.isnan(cost[66])
    ok = np.arange(K) != 66
    assert close(r["costs"][ok], cost[ok], TOL_PEND)
    check_stats(r, (0.0, 1.0))
    assert np.isclose(r["mean"], cost[ok].mean(), rtol=1e-10)
    # the failed rollout wrote what it computed: sound up to the step of the NaN, NaN from there
    assert rel(r["x"][66, :3], xs[66, :3]) < TOL_PEND and np.isnan(r["x"][66, 3, 1]) and np.all(np.isfinite(r["x"][ok]))


# ---- 5. overdraw -----------------------------------------------------------------------------------------------------------------------
def test_an_overdraw_is_an_error_and_the_handle_goes_on():
    N, K = 3, 10
    x_nom, l, L = um.pend_policy(N)
    ctx = rat.Context(pend_problem(um.PEND_OVER, N, [0.1, 0.03, 0.05]))
    zn = np.random.default_rng(4).standard_normal((K, N, 2))
    for noise in (rat.UserNoise(2, 0, zn=zn), rat.UserNoise(2, 0, seed=3)):
        with pytest.raises(rat.RatError, match=r"RAT_ERR_ARG.*normals_per_step = 2, uniforms_per_step = 0"):
            ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=K, want_costs=True)
    # declared in full, the same source runs -- on the same handle -- and is PEND_DIAG (the extra draw is multiplied by zero)
    zn3 = np.concatenate([zn, np.ones((K, N, 1))], axis=2)
    r = ctx.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(3, 0, zn=zn3), want_costs=True)
    d = rat.Context(pend_problem(um.PEND_DIAG, N, [0.1, 0.03, 0.05])).policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(2, 0, zn=zn),
                                                                                             want_costs=True)
    assert r["n_ok"] == K and close(r["costs"], d["costs"], TOL_PEND)
    assert ctx.policy_evaluate(x_nom, l, L, K=8, seed=1)["n_ok"] == 8


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_policy_evaluate_is_untouched():
    N = 4
    x_nom, l, L = um.pend_policy(N)
    fam = rat.LQRiskSensitiveProblem(np.eye(2), np.ones((2, 1)), Q=np.eye(2), R=np.eye(1), N=N, W=1e-2 * np.eye(2), Qf=np.eye(2))
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*not a source model"):
        rat.Context(fam).policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(2, 0), K=4)
    plain = rat.Context(pend_problem(um.PEND_PLAIN, N, [0.1]))
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_ARG.*does not define RAT_USER_NOISE"):
        plain.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(2, 0), K=4)
    assert plain.policy_evaluate(x_nom, l, L, K=4, seed=1)["n_ok"] == 4
    prob = pend_problem(um.PEND_MIX, N, [0.1, 0.02, 0.03, 0.25, 0.2])
    ctx = rat.Context(prob)
    fresh = rat.Context(prob).policy_evaluate(x_nom, l, L, thetas=(0.0, 0.5), K=500, seed=11, want_costs=True)
    before = ctx.policy_evaluate(x_nom, l, L, thetas=(0.0, 0.5), K=500, seed=11, want_costs=True)
    zn, zu = np.zeros((4, N, 2)), np.full((4, N, 1), 0.5)
    for noise in (rat.UserNoise(2, 1, zn=zn), rat.UserNoise(2, 1, zu=zu)):               # injected draws need every declared stream
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*every declared stream"):
            ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=4)
    for noise in (rat.UserNoise(-1, 1), rat.UserNoise(2, -1)):
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*must not be negative"):
            ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=4)
    for kw in (dict(K=0), dict(K=(1 << 27) + 1), dict(K=4, thetas=(-0.1,)), dict(K=4, thetas=np.zeros(17))):
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG"):
            ctx.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(2, 1), **kw)
    assert ctx.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(2, 1, zn=zn, zu=zu), want_costs=True)["n_ok"] == 4
    assert rat.evaluate_policy(prob, x_nom, l, L, K=64, noise=rat.UserNoise(2, 1, seed=5))["mean"] == \
        ctx.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(2, 1, seed=5), K=64)["mean"]
    after = ctx.policy_evaluate(x_nom, l, L, thetas=(0.0, 0.5), K=500, seed=11, want_costs=True)
    for r in (before, after):
        assert np.array_equal(r["costs"], fresh["costs"]) and np.array_equal(r["risk"], fresh["risk"])
        assert all(r[k] == fresh[k] for k in ("n_ok", "mean", "var", "min", "max", "se_mean"))


# ---- 7. parameters ---------------------------------------------------------------------------------------------------------------------
def test_set_params_changes_the_sampler_without_a_recompile():
    N, K = 5, 40
    x_nom, l, L = um.pend_policy(N)
    ctx = rat.Context(pend_problem(um.PEND_STATE, N, um.PEND_STATE_P))
    zn = np.random.default_rng(6).standard_normal((K, N, 3))
    noise = rat.UserNoise(3, 0, zn=zn)
    assert ctx.debug_get("src_un_loads") == 0
    c0 = ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, want_costs=True)["costs"]
    assert ctx.debug_get("src_un_loads") == 1
    p1 = [0.1, 0.5, 0.1]
    ctx.set_params(p1)
    c1 = ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, want_costs=True)["costs"]
    g1 = ctx.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(3, 0, seed=8), K=K, want_costs=True)["costs"]
    assert ctx.debug_get("src_un_loads") == 1                        # the module of the first call served all three
    fresh = rat.Context(pend_problem(um.PEND_STATE, N, p1))
    assert np.array_equal(c1, fresh.policy_evaluate_noise(x_nom, l, L, noise=noise, want_costs=True)["costs"])
    assert np.array_equal(g1, fresh.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(3, 0, seed=8), K=K, want_costs=True)["costs"])
    assert not np.array_equal(c0, c1)
    ref, _, _ = um.np_rollouts(um.pend_f, um.pend_c, um.pend_h, um.pend_state_noise, p1, x_nom, l, L, K, zn.ravel(), None, 3, 0)
    assert close(c1, ref, TOL_PEND)
    # other draw counts are another kernel
    ctx.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(4, 0, seed=8), K=K)
    assert ctx.debug_get("src_un_loads") == 2
