"""Worst-case disturbance moments on the device (rat_policy_worst_case_disturbance, Context.policy_worst_case_disturbance): the mean and
covariance of w_t and its covariance with (x_t, u_t) under q and under p* ~ exp(theta* J) q, formed by replaying the last evaluation with
the rollouts keeping w (csrc/policy_mc.hip: wcd_centre, wcd_moments, wcd_final).

The reference w never comes from the call under test.  Families: rare_event_model.normals(seed, 0, K, N, n), the NumPy model of the device
generator at rat_policy_evaluate's keying, times np.linalg.cholesky(W(t)).  Source models under rat_user_noise:
rare_event_noise_model.normals and NumPy restatements of the samplers, evaluated at the device's own x_t, u_t.  x and u: rat_rollout_noisy
with the same seed for the families (it returns policy_evaluate's costs bit for bit, which every case asserts again),
policy_evaluate_noise's x / u for source models.  From them tests/wc_disturbance_model.py: `moments` restates the device's summation
order (held to 1e-12 of the step's scale, the project's figure for a restated order) and `direct` is np.longdouble (held to ten times the
deviation tests/test_cpu_wc_disturbance.py measures between the two).  Scales: wc_disturbance_model.deviation."""
import numpy as np
import pytest

import rare_event_model as rm
import rare_event_noise_model as rn
import ratilqr.jl_amd as rat
import user_noise_model as um
from test_cpu_wc_disturbance import (CF_FACTOR, CF_K, CF_SEED, CPU_DEV_COV, CPU_DEV_FAR_WZ, CPU_DEV_MEAN, CPU_DEV_WZ, closed_form_cases,
                                     det_rollout, within_se)
from test_gpu_user_noise import pend_problem
from test_gpu_wc_trajectory import both, family
from wc_disturbance_model import centre_w, closed_form, deviation, direct, moments, z_offset
from wc_trajectory_model import centre, weights_from_rows
from wc_trajectory_model import direct as direct_z

pytestmark = pytest.mark.gpu
TOL_MODEL = 1e-12
KS = (1, 3, 4, 5, 63, 64, 65)
K_CHUNK = 65536 + 5


def family_w(prob, seed, K):
    """w [K, N, n] of rat_policy_evaluate(seed=seed, K=K) on a family: the generator's normals times the host's Cholesky factors"""
    z = rm.normals(seed, 0, K, prob.N, prob.n)
    return np.einsum("tij,ktj->kti", rm.chol_factors(prob), z)


def parts(o):
    return o["mean_w"], o["cov_w"], (np.concatenate([o["cov_wx"], o["cov_wu"]], axis=-1) if "cov_wx" in o else None)


def same_bits(a, b, label):
    for part in ("bounds", "thetas"):
        assert a[part].keys() == b[part].keys()
        for k in a[part]:
            assert np.array_equal(a[part][k], b[part][k], equal_nan=True), (label, part, k)


def check(ctx, w, x, u, costs, c_z, bounds, thetas, label, far=False):
    """the call against policy_worst_case's rows (bit for bit), the model and the extended-precision answer; cross=False against the
    same mean_w / cov_w bits; returns the parts.  far: the (x, u) centre is the caller's x_nom several standard deviations from where
    the rollouts go (CPU_DEV_FAR_WZ: cov_wz alone reads it)"""
    n, m = x.shape[2], u.shape[2]
    out = ctx.policy_worst_case_disturbance(kl_bounds=bounds, thetas=thetas)
    wc = ctx.policy_worst_case(kl_bounds=bounds, thetas=thetas)
    for part in ("bounds", "thetas"):
        for k in wc[part]:
            assert np.array_equal(out[part][k], wc[part][k], equal_nan=True), (label, part, k)
    o = both(out)
    got = parts(o)
    N = u.shape[1]
    assert got[0].shape[1:] == (N, n) and got[1].shape[1:] == (N, n, n) and got[2].shape[1:] == (N, n, n + m)
    y, dead = weights_from_rows(costs, o["theta"], o["flag"])
    c_w = centre_w(w, costs)
    mean_z, cov_z = direct_z(x, u, costs, y, dead)
    zs = z_offset(mean_z[:, :-1], cov_z[:, :-1], c_z[:-1][:, list(range(n)) + list(range(12, 12 + m))])
    dm, dc, dz = deviation(got, moments(w, x, u, costs, c_w, c_z, y, dead)[:3], c_w[:, :n], zs, K=costs.size)
    em, ec, ez = deviation(got, direct(w, x, u, costs, y, dead), c_w[:, :n], zs, K=costs.size)
    print(f"{label}: model mean {dm:.2e} cov_w {dc:.2e} cov_wz {dz:.2e}; longdouble mean {em:.2e} cov_w {ec:.2e} cov_wz {ez:.2e}")
    assert dm <= TOL_MODEL and dc <= TOL_MODEL and dz <= TOL_MODEL, (label, dm, dc, dz)
    assert em <= 10 * CPU_DEV_MEAN and ec <= 10 * CPU_DEV_COV and ez <= 10 * (CPU_DEV_FAR_WZ if far else CPU_DEV_WZ), (label, em, ec, ez)
    assert np.array_equal(got[1], got[1].swapaxes(-1, -2), equal_nan=True)
    plain = ctx.policy_worst_case_disturbance(kl_bounds=bounds, thetas=thetas, cross=False)
    for part in ("bounds", "thetas"):
        assert "cov_wx" not in plain[part] and "cov_wu" not in plain[part]
        for k in plain[part]:
            assert np.array_equal(plain[part][k], out[part][k], equal_nan=True), (label, part, k)
    return out


def run_family(which, N, K, closed, seed=5):
    prob, x0, l, L = family(which, N)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)
    x_nom, gains = (x_det, L) if closed else (x0, None)
    r = ctx.policy_evaluate(x_nom, l, gains, K=K, seed=seed, want_costs=True)
    x, u, cost, _ = ctx.rollout_noisy(x_nom, l, gains, K=K, seed=seed)
    assert np.array_equal(cost, r["costs"], equal_nan=True)
    # Rows: a searched radius, a saturated one, the nominal distribution and a tilt of one standard deviation of the costs (the reasons:
    # tests/test_gpu_wc_trajectory.run_family)
    sd = np.sqrt(r["var"]) if r["n_ok"] >= 2 and r["var"] > 0 else 1.0
    out = check(ctx, family_w(prob, seed, K), x, u, cost, centre(x_det, l), (0.1, 1e9), (0.0, 1.0 / sd), f"family {which} N={N} K={K} closed={closed}")
    if r["n_ok"] > 0:
        assert out["bounds"]["flag"][1] == 1
    return r, out, ctx


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("N", [1, 2, 3, 10])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_families_against_model_and_longdouble(which, N, closed):
    """K = 1, 3, 4, 5 (the MFMA tail), 63, 64, 65 (more than one wavefront per slot) per problem, horizon and loop; odd and even N: one
    Box-Muller transform serves two steps.  Open loop u_t is its centre l_t, and x_0 is its centre always: those covariances are
    exact zeros, not small numbers."""
    for K in KS:
        _, out, _ = run_family(which, N, K, closed)
        for part in ("bounds", "thetas"):
            live = ~np.isnan(out[part]["mean_w"][:, 0, 0])
            assert np.all(out[part]["cov_wx"][live, 0] == 0.0)
            if not closed:
                assert np.all(out[part]["cov_wu"][live] == 0.0)


@pytest.mark.parametrize("which,N,closed", [(0, 3, True), (1, 1, False), (2, 3, True), (2, 10, False)])
def test_families_across_a_chunk(which, N, closed):
    """K = 65536 + 5: the second chunk holds five rollouts, under its own Philox key.  The power-law runs lose rollouts to DomainErrors,
    whose w and trajectories may hold NaN: selected out."""
    r, out, _ = run_family(which, N, K_CHUNK, closed)
    if which == 2:
        assert r["n_domain"] > 0
    assert np.all(out["thetas"]["ess"][0] == r["n_ok"])


def test_size_one_by_one_at_one_step():
    """n = m = 1, N = 1: eleven padding lanes of w, fifteen of (x, u), one step.  (12 x 4 at N = 1 is family 0 above.)"""
    prob = rat.LQRiskSensitiveProblem(np.array([[0.9]]), np.array([[1.0]]), Q=np.eye(1), R=np.eye(1), N=1, W=np.array([[0.5]]), Qf=2 * np.eye(1))
    ctx = rat.Context(prob)
    x0, l, L = np.array([0.7]), np.array([[0.2]]), np.array([[[-0.4]]])
    x_det = ctx.rollout_open(x0, l)
    for K in (1, 5, 65):
        r = ctx.policy_evaluate(x_det, l, L, K=K, seed=3, want_costs=True)
        x, u, cost, _ = ctx.rollout_noisy(x_det, l, L, K=K, seed=3)
        assert np.array_equal(cost, r["costs"])
        out = check(ctx, family_w(prob, 3, K), x, u, cost, centre(x_det, l), (0.1,), (0.0,), f"1 x 1 K={K}")
        assert out["thetas"]["mean_w"].shape == (1, 1, 1) and np.all(out["thetas"]["cov_wx"] == 0.0) and np.all(out["thetas"]["cov_wu"] == 0.0)
    assert abs(out["thetas"]["cov_w"][0, 0, 0, 0] - 0.5) < 6 * 0.5 * np.sqrt(2.0 / 65)        # Var of a sample variance of Gaussians


# ---- source models under rat_user_noise ----------------------------------------------------------------------------------------------
# a sampler whose mean is far from zero (p[3], p[4]: ten and twenty standard deviations), and one whose mean follows the state
PEND_SHIFT = um.PEND_FCH + um.NOISE_HEAD + r"""
    for (int i = 0; i < 2; ++i) w[i] = p[3 + i] + p[1 + i] * rng.normal();
}
"""
PEND_SHIFT_P = [0.1, 0.05, 0.02, 0.5, -0.4]
PEND_DRIFT = um.PEND_FCH + um.NOISE_HEAD + r"""
    const double z0 = rng.normal();
    const double z1 = rng.normal();
    w[0] = p[1] * z0;
    w[1] = p[3] * x[0] + p[2] * z1;
}
"""
PEND_DRIFT_P = [0.1, 0.2, 0.1, -0.5]


class StepRng:
    """rat_rng's normals of one step over all rollouts, in draw order"""

    def __init__(self, xi_t):
        self.xi, self.i = xi_t, 0

    def normal(self):
        self.i += 1
        return self.xi[:, self.i - 1]


def shift_noise(k, x, u, rng, p):
    return np.stack([p[3] + p[1] * rng.normal(), p[4] + p[2] * rng.normal()], axis=1)


def drift_noise(k, x, u, rng, p):
    z0, z1 = rng.normal(), rng.normal()
    return np.stack([p[1] * z0, p[3] * x[:, 0] + p[2] * z1], axis=1)


def source_w(noise, p, seed, npn, x, u):
    """w [K, N, n] the sampler restated in NumPy writes at the device's own (x_t, u_t) under the generator's normals"""
    K, N = u.shape[:2]
    xi = rn.normals(seed, 0, K, N, npn)
    with np.errstate(invalid="ignore"):
        return np.stack([noise(t, x[:, t], u[:, t], StepRng(xi[:, t]), np.asarray(p, float)) for t in range(N)], axis=1)


def run_pendulum(src, p, noise, npn, N, K, closed, seed, bounds=(0.2,)):
    x_nom, l, L = um.pend_policy(N)
    ctx = rat.Context(pend_problem(src, N, p))
    x_det = ctx.rollout_open(x_nom[0], l)
    xa, La = (x_nom, L) if closed else (x_nom[0], None)
    r = ctx.policy_evaluate_noise(xa, l, La, noise=rat.UserNoise(npn, 0, seed=seed), K=K, want_costs=True, want_trajectories=True)
    w = source_w(noise, p, seed, npn, r["x"], r["u"])
    c = centre(x_nom if closed else x_det, l)
    # the tilt of one standard deviation of the costs, as run_family's: PEND_STATE's costs spread so far that theta = 0.5 leaves the weight
    # on a handful of rollouts, where a covariance is what is left of (mean - c)^2 and no order keeps its digits
    thetas = (0.0, 1.0 / np.sqrt(r["var"]) if r["n_ok"] >= 2 and r["var"] > 0 else 1.0)
    out = check(ctx, w, r["x"], r["u"], r["costs"], c, bounds, thetas, f"pendulum {noise.__name__} K={K} closed={closed}", far=closed)
    return ctx, r, w, out


@pytest.mark.parametrize("closed", [False, True])
def test_pendulum_under_a_shifted_sampler(closed):
    """E w = (0.5, -0.4) with standard deviations (0.05, 0.02): c_w = 0 would cost two to three digits of cov_w (test_cpu_wc_disturbance
    measures that road); the device's centre is a draw."""
    for K in (5, 2000):
        _, r, w, out = run_pendulum(PEND_SHIFT, PEND_SHIFT_P, shift_noise, 2, 4, K, closed, seed=21)
        if K == 2000:
            m0, c0 = out["thetas"]["mean_w"][0], out["thetas"]["cov_w"][0]
            assert np.all(np.abs(m0 - [0.5, -0.4]) <= 6 * np.array([0.05, 0.02]) / np.sqrt(K))
            assert np.all(np.abs(np.sqrt(np.diagonal(c0, axis1=-2, axis2=-1)) - [0.05, 0.02]) <= 6 * np.array([0.05, 0.02]) / np.sqrt(2 * K))


def test_pendulum_under_a_sampler_that_fails_across_a_chunk():
    """PEND_NAN draws NaN beyond three standard deviations: DomainError rollouts whose w holds NaN from that step.  K = 65536 + 5: the
    generator counts rollouts globally."""
    ctx, r, w, out = run_pendulum(um.PEND_NAN, [0.1, 0.05], rn.pend_nan_noise, 1, 4, K_CHUNK, True, seed=21)
    bad = np.isnan(r["costs"])
    assert r["n_domain"] > 0 and np.isnan(w[bad]).any() and np.all(out["thetas"]["ess"][0] == r["n_ok"])
    assert np.all(out["thetas"]["cov_w"][:, :, 0, :] == 0.0)          # the sampler leaves w[0] alone: zero, and its covariances exact zeros


def test_a_state_dependent_sampler_shows_in_cov_wx():
    """PEND_STATE scales its noise with |x_t|, PEND_DRIFT adds p[3] x_t[0] to w_t[1].  At theta = 0 a family's cov_wx is zero to
    Monte-Carlo error; PEND_DRIFT's is Cov(w_t[1], x_t) = p[3] Cov(x_t[0], x_t) + p[2] Cov(z, x_t) -- the first term from the
    trajectory call's cov_x at the SAME step, the second zero to Monte-Carlo error: sd(x_t) p[2] / sqrt(K) per entry, six of them allowed.
    Held against x_{t+1} instead the relation fails."""
    N, K = 4, 4000
    run_pendulum(um.PEND_STATE, um.PEND_STATE_P, rn.pend_state_noise, 3, N, 2000, True, seed=6)
    ctx, r, w, out = run_pendulum(PEND_DRIFT, PEND_DRIFT_P, drift_noise, 2, N, K, True, seed=8)
    cov_wx = out["thetas"]["cov_wx"][0]
    cov_x = ctx.policy_worst_case_trajectory(thetas=(0.0,))["thetas"]["cov_x"][0]
    p = PEND_DRIFT_P
    wrong = 0
    for t in range(1, N):
        sdx = np.sqrt(np.diag(cov_x[t]))
        slack = 6 * p[2] * sdx / np.sqrt(K)
        assert np.all(np.abs(cov_wx[t, 1] - p[3] * cov_x[t, 0]) <= slack), t
        assert abs(cov_wx[t, 1, 0]) > 5 * slack[0]                                         # far from zero
        wrong += np.any(np.abs(cov_wx[t, 1] - p[3] * cov_x[t + 1, 0]) > slack)
    assert wrong > 0
    # a family at theta = 0: zero to Monte-Carlo error, sqrt(W_ii Cov(x)_jj / K) per entry
    prob, x0, l, L = family(1, 3)
    fam = rat.Context(prob)
    x_det = fam.rollout_open(x0, l)
    fam.policy_evaluate(x_det, l, L, K=K, seed=2)
    f_wx = fam.policy_worst_case_disturbance(thetas=(0.0,))["thetas"]["cov_wx"][0]
    f_x = fam.policy_worst_case_trajectory(thetas=(0.0,))["thetas"]["cov_x"][0]
    for t in range(3):
        se = np.sqrt(np.outer(np.diag(prob.W(t)), np.diag(f_x[t])) / K)
        assert np.all(np.abs(f_wx[t]) <= 6 * se)


# ---- the closed form of the tilted law -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 1])
def test_closed_form_on_the_device(case):
    """The problems, theta, K and seed of test_cpu_wc_disturbance's closed-form test through policy_evaluate and the call: within 6 SE of
    closed_form, the SE from rollout_noisy's trajectories, the reference w and the host weights."""
    label, prob, x0, l, L = closed_form_cases()[case]
    ctx = rat.Context(prob)
    x_det = det_rollout(prob, x0, l)
    r = ctx.policy_evaluate(x_det, l, L, K=CF_K, seed=CF_SEED, want_costs=True)
    x, u, cost, _ = ctx.rollout_noisy(x_det, l, L, K=CF_K, seed=CF_SEED)
    assert np.array_equal(cost, r["costs"])
    theta = CF_FACTOR / closed_form(prob, x0, l, L, x_det, 0.0)[4]
    out = ctx.policy_worst_case_disturbance(thetas=(theta, 0.0))["thetas"]
    print(f"{label}: theta {theta:.4g}, ESS / K = {out['ess'][0] / CF_K:.4f}")
    assert out["ess"][0] >= CF_K / 4 and out["ess"][1] == CF_K
    y, dead = weights_from_rows(cost, [theta, 0.0], [0, 0])
    se = direct(family_w(prob, CF_SEED, CF_K), x, u, cost, y, dead, want_se=True)[3]
    got = parts(out)
    for r_, th in enumerate((theta, 0.0)):
        ref = closed_form(prob, x0, l, L, x_det, th)
        within_se(tuple(g[r_] for g in got), tuple(s[r_] for s in se), ref[:3], f"device {label} theta={th:.3g}")


# ---- repeatability -------------------------------------------------------------------------------------------------------------------
def test_same_bits_again_and_row_by_row():
    prob, x0, l, L = family(0, 3)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)
    ctx.policy_evaluate(x_det, l, L, K=301, seed=4)
    bounds = tuple(0.01 * (i + 1) ** 2 for i in range(15)) + (np.inf,)
    a = ctx.policy_worst_case_disturbance(kl_bounds=bounds, thetas=(0.0, 0.4))
    b = ctx.policy_worst_case_disturbance(kl_bounds=bounds, thetas=(0.0, 0.4))
    same_bits(a, b, "again")
    assert a["bounds"]["flag"][-1] == 1 and np.all(a["bounds"]["flag"][:-1] == 0)
    for i, d in enumerate(bounds):
        one = ctx.policy_worst_case_disturbance(kl_bounds=(d,))["bounds"]
        for k in one:
            assert np.array_equal(one[k][0], a["bounds"][k][i], equal_nan=True), (i, k)


def test_the_existing_surface_is_untouched():
    """rollout_noisy, policy_evaluate and policy_worst_case_trajectory return the same bits before and after a disturbance call on the
    same handle (their w_out is null; the staging buffer is the new call's own)."""
    prob, x0, l, L = family(0, 3)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)

    def surface():
        r = ctx.policy_evaluate(x_det, l, L, K=301, seed=4, want_costs=True)
        t = ctx.policy_worst_case_trajectory(kl_bounds=(0.1,), thetas=(0.0,))
        return r, t, ctx.rollout_noisy(x_det, l, L, K=301, seed=4)
    r0, t0, n0 = surface()
    ctx.policy_evaluate(x_det, l, L, K=301, seed=4)
    ctx.policy_worst_case_disturbance(kl_bounds=(0.1,), thetas=(0.0,))
    r1, t1, n1 = surface()
    same_bits(t0, t1, "trajectory")
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(n0, n1))
    assert r0.keys() == r1.keys() and all(np.array_equal(r0[k], r1[k], equal_nan=True) for k in r0)


# ---- the guard and the refusals ----------------------------------------------------------------------------------------------------------
def test_a_changed_problem_is_caught_and_the_handle_goes_on():
    N = 3
    x_nom, l, L = um.pend_policy(N)
    ctx = rat.Context(pend_problem(um.PEND_STATE, N, um.PEND_STATE_P))
    noise = rat.UserNoise(3, 0, seed=6)
    ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=100)
    good = ctx.policy_worst_case_disturbance(thetas=(0.0,))
    ctx.set_params([0.1, 0.25, 0.02])
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*changed since the evaluation"):
        ctx.policy_worst_case_disturbance(thetas=(0.0,))
    assert ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=100)["n_ok"] == 100
    other = ctx.policy_worst_case_disturbance(thetas=(0.0,))
    assert not np.array_equal(other["thetas"]["cov_w"], good["thetas"]["cov_w"])
    # a family: the same tables with another Q
    prob, x0, l2, L2 = family(1, 3)
    fam = rat.Context(prob)
    x_det = fam.rollout_open(x0, l2)
    fam.policy_evaluate(x_det, l2, L2, K=50, seed=1)
    fam.policy_worst_case_disturbance(kl_bounds=(0.1,))
    fam.set_problem(rat.LQRiskSensitiveProblem(np.eye(2), np.eye(2), Q=3 * np.eye(2), R=2 * np.eye(2), P=np.eye(2), N=3,
                                               W=np.array([[2.0, 0.6], [0.6, 1.0]]), Qf=np.eye(2)))
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*changed since the evaluation"):
        fam.policy_worst_case_disturbance(kl_bounds=(0.1,))
    assert fam.policy_evaluate(x_det, l2, L2, K=50, seed=1)["n_ok"] == 50
    assert fam.policy_worst_case_disturbance(kl_bounds=(0.1,))["bounds"]["flag"][0] == 0


def test_refusals():
    prob, x0, l, L = family(1, 3)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no evaluation"):                    # nothing to replay yet
        ctx.policy_worst_case_disturbance(thetas=(0.0,))
    ctx.policy_evaluate(x_det, l, L, K=20, seed=1)
    for kw in (dict(), dict(kl_bounds=(-0.1,)), dict(kl_bounds=(np.nan,)), dict(thetas=(np.inf,)), dict(thetas=(-1.0,)),
               dict(kl_bounds=np.ones(17)), dict(thetas=np.ones(17))):                       # rat_policy_worst_case's argument refusals
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG"):
            ctx.policy_worst_case_disturbance(**kw)
    assert ctx.policy_worst_case_disturbance(thetas=(0.0,))["thetas"]["ess"][0] == 20        # ... leave the handle usable
    ctx.policy_worst_case(kl_bounds=(0.1,), costs=np.arange(20.0))                           # uploaded costs are no evaluation's
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no evaluation"):
        ctx.policy_worst_case_disturbance(thetas=(0.0,))
    z = np.random.default_rng(0).standard_normal((8, 3, 2))
    ctx.policy_evaluate(x_det, l, L, z=z)                                                    # injected draws are not kept
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*injected"):
        ctx.policy_worst_case_disturbance(thetas=(0.0,))
    # a source model under N(0, W); and under its sampler with injected draws
    N = 3
    x_nom, pl, pL = um.pend_policy(N)
    src = rat.Context(pend_problem(um.PEND_STATE, N, um.PEND_STATE_P))
    src.policy_evaluate(x_nom, pl, pL, K=16, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rat_user_noise"):
        src.policy_worst_case_disturbance(thetas=(0.0,))
    src.policy_evaluate_noise(x_nom, pl, pL, noise=rat.UserNoise(3, 0, zn=np.zeros((4, N, 3))))
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*injected"):
        src.policy_worst_case_disturbance(thetas=(0.0,))
    assert src.policy_evaluate_noise(x_nom, pl, pL, noise=rat.UserNoise(3, 0, seed=1), K=16)["n_ok"] == 16
    assert src.policy_worst_case_disturbance(thetas=(0.0,))["thetas"]["flag"][0] == 0
    # general sizes
    wide_prob, wx0, wu = rat.synthetic_lq_problem(n=16, m=4, N=5, seed=3, w=1e-2)
    wide = rat.Context(wide_prob)
    wide.policy_evaluate(wx0, wu, K=8, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*n <= 12"):
        wide.policy_worst_case_disturbance(thetas=(0.0,))
    # too many rows x steps for the partial sums: the cap of its own
    long_prob = rat.LQRiskSensitiveProblem(np.eye(2), np.eye(2), Q=np.eye(2), R=np.eye(2), N=400, W=np.eye(2), Qf=np.eye(2))
    lc = rat.Context(long_prob)
    lc.policy_evaluate(np.zeros(2), np.zeros((400, 2)), K=4, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*1899"):
        lc.policy_worst_case_disturbance(kl_bounds=0.1 * np.arange(1, 6))
    assert lc.policy_worst_case_disturbance(kl_bounds=0.1 * np.arange(1, 5))["bounds"]["mean_w"].shape == (4, 400, 2)


def test_an_empty_sample_is_nan():
    """Every rollout of the power-law problem fails when it starts below zero: RAT_WC_EMPTY rows, NaN moments (and no rollout to take
    c_w from: zero)."""
    prob, _, l, _ = family(2, 3)
    ctx = rat.Context(prob)
    r = ctx.policy_evaluate(np.array([-0.5, -0.5]), l, K=9, seed=1)
    assert r["n_ok"] == 0
    out = ctx.policy_worst_case_disturbance(kl_bounds=(0.1,), thetas=(0.0,))
    for part in ("bounds", "thetas"):
        assert out[part]["flag"][0] == 2 and all(np.isnan(out[part][k]).all() for k in ("mean_w", "cov_w", "cov_wx", "cov_wu"))
