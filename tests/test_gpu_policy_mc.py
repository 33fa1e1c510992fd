"""Monte-Carlo policy evaluation on the device (rat_policy_evaluate, Context.policy_evaluate): K noisy rollouts of a policy on a problem
of any model kind, reduced on the device (csrc/policy_mc.hip); source models run rat_src_noisy_rollout (csrc/source_noisy.h).

rat_rollout_noisy keeps refusing source models (tests/test_gpu_source_model.py pins that); this entry point is the way to their
Monte-Carlo costs.  Checked against rat_rollout_noisy bit for bit, the oracle, NumPy on the returned costs, the LQ family for a source
model, a NumPy restatement of the pendulum, and the closed-form entropic risk of tests/leqg_exact.py."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
from oracle import oracle as orc
from leqg_exact import breakdown_theta, exact_value, random_lq
from policy_mc_model import direct, reduce_costs
from test_gpu_source_model import N_P, DT, W_P, lq_pair, source_pendulum

pytestmark = pytest.mark.gpu
N = 10


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def noisy_problems():
    """The two problems of _noisy_problems() in tests/test_gpu_ileqg.py, rebuilt, and a power-law problem (the third model family that
    rat_rollout_noisy serves): (problem, x0, l, L)."""
    rng = np.random.default_rng(3)
    n, m, Nn = 12, 4, 20
    Qo, _ = np.linalg.qr(rng.standard_normal((n, n)))
    G = rng.standard_normal((Nn, n, n))
    Wtv = 1e-2 * (np.einsum("tij,tkj->tik", G, G) / n + np.eye(n))           # time-varying dense SPD covariances
    lq = rat.LQRiskSensitiveProblem(0.9 * Qo, rng.standard_normal((n, m)) / np.sqrt(n), Q=np.eye(n), R=0.1 * np.eye(m),
                                    P=0.05 * rng.standard_normal((m, n)), N=Nn, W=Wtv, Qf=np.eye(n), kappa=0.02,
                                    qv=0.1 * rng.standard_normal(n), rv=0.1 * rng.standard_normal(m), q0=0.3)
    small = rat.LQRiskSensitiveProblem(np.eye(2), np.eye(2), Q=np.eye(2), R=2 * np.eye(2), P=np.eye(2), N=N, W=np.array([[2.0, 0.6], [0.6, 1.0]]),
                                       Qf=np.eye(2))
    pl = rat.PowerLawRiskSensitiveProblem(2, N, 1e-4 * np.eye(2), a=1.3, b=1.5, p=2.5, hconst=1.0)
    return (lq, rng.standard_normal(n), 0.1 * rng.standard_normal((Nn, m)), 0.2 * rng.standard_normal((Nn, m, n))), \
           (small, np.array([0.5, -1.0]), np.ones((N, 2)), 0.3 * np.ones((N, 2, 2))), \
           (pl, np.array([0.6, 0.4]), 0.2 * np.ones((N, 2)), 0.05 * np.ones((N, 2, 2)))


# ---- 1. family parity on injected noise --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
def test_family_costs_are_rollout_noisys_bit_for_bit_and_the_oracles(which):
    prob, x0, l, L = noisy_problems()[which]
    P = orc.Problem(prob)
    ctx = rat.Context(prob)
    K = 37                                                          # ragged: not a multiple of the 4 rollouts per wavefront
    z = np.random.default_rng(11).standard_normal((K, prob.N, prob.n))
    x_det = ctx.rollout_open(x0, l)
    for x_nom, gains in ((x0, None), (x_det, L)):                   # open loop, and under the affine policy
        r = ctx.policy_evaluate(x_nom, l, gains, z=z, want_costs=True)
        _, _, c_old, dom = ctx.rollout_noisy(x_nom, l, gains, z=z, want_x=False, want_u=False)
        assert not dom and r["n_ok"] == K and r["n_domain"] == 0
        assert np.array_equal(r["costs"], c_old)
        rc, _, _, co = orc.simulate_noisy(P, x_nom, l, gains, z)
        assert rc == 0 and rel(r["costs"], co) < 1e-12
        # the device generator: same seed, same costs, beyond one chunk of 65536 rollouts too
        for Kg in (16, 70000):
            rg = ctx.policy_evaluate(x_nom, l, gains, K=Kg, seed=7, want_costs=True)
            _, _, cg, _ = ctx.rollout_noisy(x_nom, l, gains, K=Kg, seed=7, want_x=False, want_u=False)
            assert np.array_equal(rg["costs"], cg, equal_nan=True)
    assert ctx.policy_evaluate(x0, l, K=8, seed=1)["costs"] is None


def test_general_size_costs_are_rollout_noisys_bit_for_bit():
    prob, x0, u = rat.synthetic_lq_problem(n=16, m=4, N=20, seed=3, kappa=0.02, w=1e-2)
    ctx = rat.Context(prob)
    assert ctx.get_path(1) == "wide"
    rng = np.random.default_rng(4)
    L = 0.1 * rng.standard_normal((20, 4, 16))
    x_det = ctx.rollout_open(x0, u)
    z = rng.standard_normal((41, 20, 16))
    for x_nom, gains in ((x0, None), (x_det, L)):
        r = ctx.policy_evaluate(x_nom, u, gains, thetas=(0.0, 0.5), z=z, want_costs=True)
        _, _, c_old, _ = ctx.rollout_noisy(x_nom, u, gains, z=z, want_x=False, want_u=False)
        assert np.array_equal(r["costs"], c_old) and r["n_ok"] == 41
        d = direct(r["costs"], (0.0, 0.5))
        assert all(np.allclose(r[k], d[k], rtol=1e-11, atol=0.0) for k in ("mean", "var", "min", "max", "se_mean", "risk", "risk_se"))
        rg = ctx.policy_evaluate(x_nom, u, gains, K=1000, seed=5, want_costs=True)
        _, _, cg, _ = ctx.rollout_noisy(x_nom, u, gains, K=1000, seed=5, want_x=False, want_u=False)
        assert np.array_equal(rg["costs"], cg)


# ---- 2. statistics -----------------------------------------------------------------------------------------------------------------
def test_statistics_equal_numpy_on_the_returned_costs_and_repeat_bit_for_bit():
    """Tolerance 1e-11 relative: a fixed-order fp64 sum of K <= 2^13 terms of one sign errs by at most about K 2^-53 ~ 1e-12 relative,
    the shift by the maximum keeps every exponent <= 0, and 1e-11 leaves a decade over that bound."""
    prob, x0, l, L = noisy_problems()[0]
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)
    thetas = (0.0, 0.1, 1.0)
    r = ctx.policy_evaluate(x_det, l, L, thetas=thetas, K=5000, seed=3, want_costs=True)
    assert r["n_ok"] == 5000 and r["n_domain"] == 0 and np.all(np.isfinite(r["costs"])) and r["costs"].std() > 0
    d = direct(r["costs"], thetas)
    for key in ("mean", "var", "min", "max", "se_mean", "risk", "risk_se"):
        assert np.allclose(r[key], d[key], rtol=1e-11, atol=0.0), key
    assert r["min"] == r["costs"].min() and r["max"] == r["costs"].max()
    assert r["risk"][0] == r["mean"] and r["risk_se"][0] == r["se_mean"]
    assert r["mean"] < r["risk"][1] < r["risk"][2] <= r["max"]      # the entropic risk grows with theta, from the mean to the maximum
    # the NumPy model of the reduction restates the device's summation order: what is left are ulps of exp / log and contracted
    # multiply-adds, each ~1e-16 relative per term; 1e-12 leaves decades over that
    mdl = reduce_costs(r["costs"], thetas)
    for key in ("mean", "var", "se_mean", "risk", "risk_se"):
        assert np.allclose(r[key], mdl[key], rtol=1e-12, atol=0.0), key
    r2 = ctx.policy_evaluate(x_det, l, L, thetas=thetas, K=5000, seed=3, want_costs=True)
    for key in ("mean", "var", "min", "max", "se_mean"):
        assert r[key] == r2[key], key
    assert np.array_equal(r["risk"], r2["risk"]) and np.array_equal(r["risk_se"], r2["risk_se"]) and np.array_equal(r["costs"], r2["costs"])
    # without the costs on the host the statistics are the same bits
    r3 = ctx.policy_evaluate(x_det, l, L, thetas=thetas, K=5000, seed=3)
    assert r3["costs"] is None and r3["mean"] == r["mean"] and np.array_equal(r3["risk"], r["risk"])
    # sixteen thetas, and none
    th16 = np.linspace(0.0, 1.5, 16)
    r16 = ctx.policy_evaluate(x_det, l, L, thetas=th16, K=5000, seed=3)
    d16 = direct(r["costs"], th16)
    assert np.allclose(r16["risk"], d16["risk"], rtol=1e-11, atol=0.0) and np.allclose(r16["risk_se"], d16["risk_se"], rtol=1e-11, atol=0.0)
    r0 = ctx.policy_evaluate(x_det, l, L, K=5000, seed=3)
    assert r0["risk"].size == 0 and r0["mean"] == r["mean"]


def test_argument_errors_on_a_live_handle():
    prob, x0, l, L = noisy_problems()[1]
    ctx = rat.Context(prob)
    for kw in (dict(thetas=np.zeros(17), K=4), dict(thetas=(-0.1,), K=4), dict(K=0), dict(K=(1 << 27) + 1)):
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG"):
            ctx.policy_evaluate(x0, l, **kw)
    with pytest.raises(rat.RatError, match="RAT_ERR_NO_PROBLEM"):
        rat.Context(None).policy_evaluate(x0, l, K=4)
    bad = rat.LQRiskSensitiveProblem(np.eye(2), np.eye(2), Q=np.eye(2), R=np.eye(2), N=N, W=np.array([[1.0, 2.0], [2.0, 1.0]]), Qf=np.eye(2))
    with pytest.raises(rat.RatError, match="not positive definite"):
        rat.Context(bad).policy_evaluate(x0, l, K=4)


# ---- 3. source model against the family ------------------------------------------------------------------------------------------------
def test_lq_source_costs_equal_the_familys_on_the_same_noise():
    fam, src, x0, u = lq_pair()
    cf, cs = rat.Context(fam), rat.Context(src)
    sol = cf.solve(x0, u, 1.5)
    assert sol["status"] == 0
    z = np.random.default_rng(21).standard_normal((500, fam.N, fam.n))
    for x_nom, l, L in ((x0, u, None), (sol["x"], sol["l"], sol["L"])):
        a = cf.policy_evaluate(x_nom, l, L, thetas=(0.0, 1.5), z=z, want_costs=True)
        b = cs.policy_evaluate(x_nom, l, L, thetas=(0.0, 1.5), z=z, want_costs=True)
        assert b["n_ok"] == 500 and rel(b["costs"], a["costs"]) < 1e-12
        assert np.allclose(b["risk"], a["risk"], rtol=1e-11, atol=0.0) and np.isclose(b["var"], a["var"], rtol=1e-9)
        # the same seed names the same noise: the Philox keying is shared, chunk offsets included (70000 rollouts are two chunks)
        for K in (64, 70000):
            a = cf.policy_evaluate(x_nom, l, L, K=K, seed=12345, want_costs=True)
            b = cs.policy_evaluate(x_nom, l, L, K=K, seed=12345, want_costs=True)
            assert rel(b["costs"], a["costs"]) < 1e-12
        # ... for every packing of the rollout kernel
        for tpw in (16, 32):
            cs.debug_set("src_mc_tpw", tpw)
            assert np.array_equal(cs.policy_evaluate(x_nom, l, L, K=70000, seed=12345, want_costs=True)["costs"], b["costs"])
        cs.debug_set("src_mc_tpw", 64)
    assert rat.evaluate_policy(src, sol["x"], sol["l"], sol["L"], thetas=(1.5,), K=64, seed=12345)["mean"] == \
        cs.policy_evaluate(sol["x"], sol["l"], sol["L"], K=64, seed=12345)["mean"]


# ---- 4. source model against NumPy ----------------------------------------------------------------------------------------------------
def test_pendulum_under_its_solved_policy_against_numpy():
    """Tolerance 1e-10 relative, as the NumPy comparison of the same pendulum in tests/test_gpu_source_pets.py: device and host sin
    differ by ulps."""
    prob = source_pendulum()
    ctx = rat.Context(prob)
    sol = ctx.solve(np.array([1.0, 0.0]), np.zeros((N_P, 1)), 0.5)
    assert sol["status"] == 0
    xb, l, L = sol["x"], sol["l"], sol["L"]
    K = 300
    z = np.random.default_rng(8).standard_normal((K, N_P, 2))
    r = ctx.policy_evaluate(xb, l, L, thetas=(0.0, 0.5), z=z, want_costs=True)
    ref = np.zeros(K)
    for k in range(K):
        x, c = xb[0].copy(), 0.0
        for t in range(N_P):
            u = l[t] + L[t] @ (x - xb[t])
            c += 0.5 * (x @ x) + 0.05 * (u @ u) + 0.01 * t * x[0]
            xn = np.array([x[0] + DT * x[1], x[1] + DT * (-np.sin(x[0]) - 0.1 * x[1] + u[0])])
            x = xn + np.linalg.cholesky(W_P(t)) @ z[k, t]
        ref[k] = c + 2.0 * (x @ x)
    assert r["n_ok"] == K and np.all(np.abs(r["costs"] - ref) <= 1e-10 * np.abs(ref))
    d = direct(ref, (0.0, 0.5))
    assert np.isclose(r["mean"], d["mean"], rtol=1e-10) and np.allclose(r["risk"], d["risk"], rtol=1e-10)
    # open loop from x_0 alone
    ro = ctx.policy_evaluate(xb[0], l, None, z=z[:5], want_costs=True)
    x, c = xb[0].copy(), 0.0
    for t in range(N_P):
        c += 0.5 * (x @ x) + 0.05 * (l[t] @ l[t]) + 0.01 * t * x[0]
        x = np.array([x[0] + DT * x[1], x[1] + DT * (-np.sin(x[0]) - 0.1 * x[1] + l[t, 0])]) + np.linalg.cholesky(W_P(t)) @ z[0, t]
    assert abs(ro["costs"][0] - (c + 2.0 * (x @ x))) <= 1e-10 * abs(c)


# ---- 5. domain errors -------------------------------------------------------------------------------------------------------------------
SQRT_MODEL = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) { xn[0] = sqrt(x[0]) + u[0]; }
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) { return x[0] * x[0] + u[0] * u[0]; }
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return x[0] * x[0]; }
"""


def test_domain_errors_are_counted_and_left_out():
    prob = rat.DeviceSourceProblem(SQRT_MODEL, 1, 1, 10, np.eye(1) * 1e-2)
    ctx = rat.Context(prob)
    K = 4000
    z = np.random.default_rng(13).standard_normal((K, 10, 1))
    x0, u = np.array([0.5]), -0.2 * np.ones((10, 1))                 # sqrt(x) - 0.2 holds x near 0.52; the noise (sd 0.1) pushes some below zero
    ref, x = np.zeros(K), np.full(K, 0.5)
    with np.errstate(invalid="ignore"):
        for t in range(10):
            ref += x * x + 0.04
            x = (np.sqrt(x) - 0.2) + 0.1 * z[:, t, 0]
        ref += x * x
    failed = np.isnan(ref)
    assert 0 < failed.sum() < K, failed.sum()                        # the inputs: some rollouts cross zero and some do not
    r = ctx.policy_evaluate(x0, u, thetas=(0.0, 2.0), z=z, want_costs=True)
    assert r["n_ok"] + r["n_domain"] == K and r["n_ok"] > 0 and r["n_domain"] > 0
    assert np.array_equal(np.isnan(r["costs"]), failed) and r["n_domain"] == failed.sum()
    assert rel(r["costs"][~failed], ref[~failed]) < 1e-12
    d = direct(r["costs"], (0.0, 2.0))
    for key in ("mean", "var", "min", "max", "se_mean", "risk", "risk_se"):
        assert np.allclose(r[key], d[key], rtol=1e-11, atol=0.0), key
    # every rollout fails: RAT_OK, NaN statistics
    ra = ctx.policy_evaluate(x0, -np.ones((10, 1)), thetas=(0.0, 2.0), K=64, seed=1, want_costs=True)
    assert ra["n_ok"] == 0 and ra["n_domain"] == 64 and np.all(np.isnan(ra["costs"]))
    assert all(np.isnan(ra[k]) for k in ("mean", "var", "min", "max", "se_mean")) and np.all(np.isnan(ra["risk"])) and np.all(np.isnan(ra["risk_se"]))
    # the power-law family flags its DomainErrors apart from the cost: the same exclusion
    pl = rat.PowerLawRiskSensitiveProblem(2, N, 1e-2 * np.eye(2), a=1.3, b=1.5, p=2.5, hconst=1.0)
    cp = rat.Context(pl)
    rp = cp.policy_evaluate(np.array([0.1, 0.1]), 0.2 * np.ones((N, 2)), K=2000, seed=2, want_costs=True)
    _, _, c_old, dom = cp.rollout_noisy(np.array([0.1, 0.1]), 0.2 * np.ones((N, 2)), K=2000, seed=2, want_x=False, want_u=False)
    assert dom and 0 < rp["n_domain"] < 2000 and np.array_equal(rp["costs"], c_old, equal_nan=True)
    assert rp["n_domain"] == np.isnan(c_old).sum() and np.isclose(rp["mean"], np.nanmean(c_old), rtol=1e-11)


# ---- 6. the LEQG identity, statistically ------------------------------------------------------------------------------------------
def test_entropic_risk_of_the_solved_policy_is_the_solvers_value():
    """risk(theta) of K = 200 000 rollouts lies within 5 risk_se of the closed-form (1/theta) log E exp(theta J) of the policy solve
    returned at theta (tests/leqg_exact.py), and the mean within 5 se_mean of the closed form at theta = 0.  The estimator's variance
    is finite only where the closed form at 2 theta is: asserted first."""
    n, m, Nn = 12, 4, 50
    prob, x0, u = random_lq(n, m, Nn, seed=212)
    assert prob.kappa == 0.0
    # on the CPU, before the GPU is touched: theta is 0.3 of the open-loop plan's breakdown (what the identity tests solve at, halved
    # below), and twice the theta used is feasible for the open-loop plan already
    Z = np.zeros((Nn, m, n))
    th_bd = breakdown_theta(prob, x0, u, Z, np.zeros((Nn + 1, n)))
    theta = 0.15 * th_bd
    assert exact_value(prob, x0, u, None, Z, np.zeros((Nn + 1, n)), 2.0 * theta)[1]
    ctx = rat.Context(prob)
    sol = ctx.solve(x0, u, theta)
    assert sol["status"] == 0
    ex, ok = exact_value(prob, x0, sol["l"], None, sol["L"], sol["x"], theta)
    assert ok and abs(sol["value"] - ex) <= 1e-10 * abs(ex)
    assert exact_value(prob, x0, sol["l"], None, sol["L"], sol["x"], 2.0 * theta)[1]        # the solved policy: finite variance
    ex0, _ = exact_value(prob, x0, sol["l"], None, sol["L"], sol["x"], 0.0)
    r = ctx.policy_evaluate(sol["x"], sol["l"], sol["L"], thetas=(theta, 0.0), K=200000, seed=2024)
    assert r["n_ok"] == 200000 and r["risk_se"][0] > 0 and r["se_mean"] > 0
    assert abs(r["risk"][0] - ex) <= 5.0 * r["risk_se"][0], (r["risk"][0], ex, r["risk_se"][0])
    assert abs(r["mean"] - ex0) <= 5.0 * r["se_mean"], (r["mean"], ex0, r["se_mean"])
    assert r["risk"][1] == r["mean"] and ex > ex0 and r["risk"][0] > r["mean"]


# ---- 7. refusals that stay ---------------------------------------------------------------------------------------------------------------
def test_rollout_noisy_still_refuses_source_models():
    ctx = rat.Context(source_pendulum())
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED"):
        ctx.rollout_noisy(np.zeros((N_P + 1, 2)), np.zeros((N_P, 1)), K=4)
    assert ctx.policy_evaluate(np.zeros(2), np.zeros((N_P, 1)), K=4, seed=0, want_costs=True)["costs"].shape == (4,)
