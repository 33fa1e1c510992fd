"""Worst-case trajectory moments on the device (rat_policy_worst_case_trajectory, Context.policy_worst_case_trajectory): the mean and
covariance of (x_t, u_t) under q and under p* ~ exp(theta* J) q, formed by replaying the last evaluation (csrc/policy_mc.hip).

Reference trajectories: rat_rollout_noisy with the same seed for the families (it returns policy_evaluate's costs bit for bit, which every
case asserts again), policy_evaluate_noise's x / u for a source model.  From them tests/wc_trajectory_model.py: `moments` restates the
device's summation order (held to 1e-12 of the step's scale, the project's figure for a restated order) and `direct` is np.longdouble
(held to ten times the deviation tests/test_cpu_wc_trajectory.py measures between the two: contracted multiply-adds and the ulps of exp
are what the device adds).  Scales: wc_trajectory_model.deviation."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
import user_noise_model as um
from test_cpu_wc_trajectory import CPU_DEV_COV, CPU_DEV_FAR_COV, CPU_DEV_FAR_MEAN, CPU_DEV_MEAN
from test_gpu_policy_mc import noisy_problems
from test_gpu_user_noise import pend_problem
from wc_trajectory_model import centre, deviation, direct, moments, weights_from_rows

pytestmark = pytest.mark.gpu
TOL_MODEL = 1e-12
KS = (1, 3, 4, 5, 63, 64, 65)
K_CHUNK = 65536 + 5


def family(which, N):
    """The problems of tests/test_gpu_policy_mc.py::noisy_problems at horizon N: the same tables and policies, cut or rebuilt to N steps
    (0: 12 x 4 LQ with time-varying dense W and a cubic term, 1: the 2 x 2 LQ problem), and (2) a power-law problem started so close to
    zero that the noise drives states negative: DomainErrors."""
    lq, small, _ = noisy_problems()
    if which == 0:
        p, x0, l, L = lq
        prob = rat.LQRiskSensitiveProblem(p.A, p.B, Q=np.eye(12), R=0.1 * np.eye(4), P=p.P, N=N, W=np.asarray(p.Wtab)[:N], Qf=np.eye(12), kappa=0.02,
                                          qv=p.qv, rv=p.rv, q0=0.3)
        return prob, x0, l[:N], L[:N]
    if which == 1:
        prob = rat.LQRiskSensitiveProblem(np.eye(2), np.eye(2), Q=np.eye(2), R=2 * np.eye(2), P=np.eye(2), N=N, W=np.array([[2.0, 0.6], [0.6, 1.0]]),
                                          Qf=np.eye(2))
        return prob, np.array([0.5, -1.0]), np.ones((N, 2)), 0.3 * np.ones((N, 2, 2))
    prob = rat.PowerLawRiskSensitiveProblem(2, N, 1e-4 * np.eye(2), a=1.3, b=1.5, p=2.5, hconst=1.0)
    return prob, np.array([0.03, 0.03]), 0.01 * np.ones((N, 2)), 0.05 * np.ones((N, 2, 2))


def full(part, n, m):
    """mean [R, N+1, n+m] and cov [R, N+1, n+m, n+m] from the parts the context returns (u at step N: zero)"""
    R, T = part["mean_x"].shape[:2]
    mean, cov = np.zeros((R, T, n + m)), np.zeros((R, T, n + m, n + m))
    mean[:, :, :n], mean[:, :T - 1, n:] = part["mean_x"], part["mean_u"]
    cov[:, :, :n, :n], cov[:, :T - 1, n:, n:] = part["cov_x"], part["cov_u"]
    cov[:, :T - 1, :n, n:], cov[:, :T - 1, n:, :n] = part["cov_xu"], part["cov_xu"].swapaxes(-1, -2)
    dead = np.isnan(part["mean_x"][:, 0, 0])                         # (an empty or non-finite sample: the parts not returned are NaN too)
    mean[dead], cov[dead] = np.nan, np.nan
    return mean, cov


def both(out):
    return {k: np.concatenate([out["bounds"][k], out["thetas"][k]]) for k in out["bounds"]}


def check(ctx, x, u, costs, c, bounds, thetas, label, far=False):
    """the call against policy_worst_case's rows (bit for bit), the model and the extended-precision answer; returns the parts.  far: the
    centre is the caller's x_nom several standard deviations from where the rollouts go (test_cpu_wc_trajectory measures that case
    apart: CPU_DEV_FAR_*)"""
    n, m = x.shape[2], u.shape[2]
    out = ctx.policy_worst_case_trajectory(kl_bounds=bounds, thetas=thetas)
    wc = ctx.policy_worst_case(kl_bounds=bounds, thetas=thetas)
    for part in ("bounds", "thetas"):
        for k in wc[part]:
            assert np.array_equal(out[part][k], wc[part][k], equal_nan=True), (label, part, k)
    o = both(out)
    mean, cov = full(o, n, m)
    y, dead = weights_from_rows(costs, o["theta"], o["flag"])
    cd = c[:, list(range(n)) + list(range(12, 12 + m))]
    mean_m, cov_m, _ = moments(x, u, costs, c, y, dead)
    dm, dc = deviation(mean, cov, mean_m, cov_m, cd, K=costs.size)
    mean_d, cov_d = direct(x, u, costs, y, dead)
    em, ec = deviation(mean, cov, mean_d, cov_d, cd, K=costs.size)
    print(f"{label}: model mean {dm:.2e} cov {dc:.2e}; longdouble mean {em:.2e} cov {ec:.2e}")
    assert dm <= TOL_MODEL and dc <= TOL_MODEL, (label, dm, dc)
    assert em <= 10 * (CPU_DEV_FAR_MEAN if far else CPU_DEV_MEAN) and ec <= 10 * (CPU_DEV_FAR_COV if far else CPU_DEV_COV), (label, em, ec)
    assert np.array_equal(cov, cov.swapaxes(-1, -2), equal_nan=True)
    return out


def run_family(which, N, K, closed, seed=5):
    prob, x0, l, L = family(which, N)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)
    x_nom, gains = (x_det, L) if closed else (x0, None)
    r = ctx.policy_evaluate(x_nom, l, gains, K=K, seed=seed, want_costs=True)
    x, u, cost, _ = ctx.rollout_noisy(x_nom, l, gains, K=K, seed=seed)
    assert np.array_equal(cost, r["costs"], equal_nan=True)
    # Rows: a searched radius, the nominal distribution and a tilt of one standard deviation of the costs, theta = 1 / sd(J).  A fixed
    # theta would be 30 standard deviations on the 2 x 2 problem: all the weight on one rollout, where the covariance is the difference
    # of two numbers (mean - c)^2 that agree to its last digits and no summation order can be held to 1e-12 of what is left.
    sd = np.sqrt(r["var"]) if r["n_ok"] >= 2 and r["var"] > 0 else 1.0
    # the centre: (x_nom, l) under the policy, the noise-free trajectory open loop
    out = check(ctx, x, u, cost, centre(x_det, l), (0.1,), (0.0, 1.0 / sd), f"family {which} N={N} K={K} closed={closed}")
    return r, out


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("N", [1, 3, 10])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_families_against_model_and_longdouble(which, N, closed):
    """K = 1, 3, 4, 5 (the MFMA tail), 63, 64, 65 (more than one wavefront per slot) per problem, horizon and loop."""
    for K in KS:
        run_family(which, N, K, closed)


@pytest.mark.parametrize("which,N,closed", [(0, 3, True), (1, 1, False), (2, 3, True), (2, 10, False)])
def test_families_across_a_chunk(which, N, closed):
    """K = 65536 + 5: the second chunk holds five rollouts, under its own Philox key.  The power-law runs lose rollouts to DomainErrors,
    whose trajectories hold NaN: selected out."""
    r, out = run_family(which, N, K_CHUNK, closed)
    if which == 2:
        assert r["n_domain"] > 0
    assert np.all(out["thetas"]["ess"][0] == r["n_ok"])


def test_the_problems_of_noisy_problems_at_their_own_horizon():
    for which in (0, 1):
        prob, x0, l, L = noisy_problems()[which]
        ctx = rat.Context(prob)
        x_det = ctx.rollout_open(x0, l)
        r = ctx.policy_evaluate(x_det, l, L, K=65, seed=9, want_costs=True)
        x, u, cost, _ = ctx.rollout_noisy(x_det, l, L, K=65, seed=9)
        assert np.array_equal(cost, r["costs"])
        check(ctx, x, u, cost, centre(x_det, l), (0.05, 1e9), (0.0,), f"noisy_problems[{which}]")      # (1e9: a saturated row)


# ---- source model under rat_user_noise ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("closed", [False, True])
def test_pendulum_under_a_sampler_that_fails(closed):
    """PEND_NAN draws NaN beyond three standard deviations: about one rollout in 190 at N = 4 is a DomainError whose trajectory holds NaN
    from that step on.  K = 65536 + 5 crosses a chunk (the generator counts rollouts globally).  Closed loop the centre is pend_policy's
    x_nom, "a nominal trajectory that is not the rollout of l": seven standard deviations from the closed-loop mean in the velocity, so
    the covariance is the difference of two numbers fifty times its size (measured on the MI355X at K = 65541: 2.9e-14 of the step's
    scale against np.longdouble, 4.1e-15 against the restated order; the far-centre figures of test_cpu_wc_trajectory apply)."""
    N = 4
    x_nom, l, L = um.pend_policy(N)
    ctx = rat.Context(pend_problem(um.PEND_NAN, N, [0.1, 0.05]))
    x_det = ctx.rollout_open(x_nom[0], l)
    for K in (5, 2000, K_CHUNK):
        xa, La = (x_nom, L) if closed else (x_nom[0], None)
        r = ctx.policy_evaluate_noise(xa, l, La, noise=rat.UserNoise(1, 0, seed=21), K=K, want_costs=True, want_trajectories=True)
        if K >= 2000:
            assert r["n_domain"] > 0 and np.isnan(r["x"][np.isnan(r["costs"])]).any()
        c = centre(x_nom if closed else x_det, l)
        out = check(ctx, r["x"], r["u"], r["costs"], c, (0.2,), (0.0, 1.0), f"pendulum K={K} closed={closed}", far=closed)
        # the theta = 0 row is the plain sample mean of the rollouts that have a cost
        ok = ~np.isnan(r["costs"])
        # (taken in np.longdouble: a float64 sum down the rollout axis adds one term at a time and errs by up to K ulps itself;
        # held to what `direct` is held to, against the mean's largest entry)
        sm = r["x"][ok].astype(np.longdouble).mean(axis=0).astype(np.float64)
        dev = np.abs(out["thetas"]["mean_x"][0] - sm).max() / np.abs(sm).max()
        print(f"pendulum K={K} closed={closed}: theta = 0 mean against the plain sample mean {dev:.2e}")
        assert dev <= 10 * (CPU_DEV_FAR_MEAN if closed else CPU_DEV_MEAN)
        # a run without trajectories (one launch of K) replays in chunks to the same bits
        ctx.policy_evaluate_noise(xa, l, La, noise=rat.UserNoise(1, 0, seed=21), K=K)
        again = ctx.policy_worst_case_trajectory(kl_bounds=(0.2,), thetas=(0.0, 1.0))
        for part in ("bounds", "thetas"):
            for k in out[part]:
                assert np.array_equal(out[part][k], again[part][k], equal_nan=True), (part, k)


# ---- closed form at theta = 0 ------------------------------------------------------------------------------------------------------------
def test_lq_covariance_recursion_at_theta_zero():
    """Closed-loop 2 x 2 LQ, K = 2^18: x_t is Gaussian with mean the noise-free closed-loop trajectory and covariance
    S_{t+1} = (A + B L_t) S_t (A + B L_t)' + W, S_0 = 0.  Five standard errors: sqrt(S_ii / K) for a mean and, for a sample covariance of
    Gaussians, sqrt((S_ii S_jj + S_ij^2) / K) (Isserlis); the population form's bias S / K is 1 / 512 of a standard error."""
    N, K = 10, 1 << 18
    prob, x0, l, L = family(1, N)
    ctx = rat.Context(prob)
    x_nom = ctx.rollout_open(x0, l)
    ctx.policy_evaluate(x_nom, l, L, K=K, seed=2024)
    out = ctx.policy_worst_case_trajectory(thetas=(0.0,))["thetas"]
    A, B, W = np.eye(2), np.eye(2), np.array([[2.0, 0.6], [0.6, 1.0]])
    S, xb = np.zeros((2, 2)), x0.copy()
    for t in range(N + 1):
        se_m = np.sqrt(np.diag(S) / K)
        se_c = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S * S) / K)
        dm, dc = np.abs(out["mean_x"][0, t] - xb), np.abs(out["cov_x"][0, t] - S)
        print(f"t={t}: mean {np.max(dm / np.maximum(se_m, 1e-300)) if t else 0.0:.2f} se, cov {np.max(dc / np.maximum(se_c, 1e-300)) if t else 0.0:.2f} se")
        assert np.all(dm <= 5 * se_m + 1e-15 * np.abs(xb).max()) and np.all(dc <= 5 * se_c + 1e-14 * max(np.abs(S).max(), 1e-30) + (1e-28 if t == 0 else 0.0))
        if t < N:
            F = A + B @ L[t]
            xb = A @ xb + B @ (l[t] + L[t] @ (xb - x_nom[t]))
            S = F @ S @ F.T + W
    assert out["ess"][0] == K and out["flag"][0] == 0


# ---- repeatability ---------------------------------------------------------------------------------------------------------------------
def test_same_bits_again_and_row_by_row():
    prob, x0, l, L = family(0, 3)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)
    ctx.policy_evaluate(x_det, l, L, K=301, seed=4)
    bounds = tuple(0.01 * (i + 1) ** 2 for i in range(15)) + (np.inf,)
    a = ctx.policy_worst_case_trajectory(kl_bounds=bounds, thetas=(0.0, 0.4))
    b = ctx.policy_worst_case_trajectory(kl_bounds=bounds, thetas=(0.0, 0.4))
    for part in ("bounds", "thetas"):
        for k in a[part]:
            assert np.array_equal(a[part][k], b[part][k], equal_nan=True), (part, k)
    assert a["bounds"]["flag"][-1] == 1 and np.all(a["bounds"]["flag"][:-1] == 0)
    for i, d in enumerate(bounds):
        one = ctx.policy_worst_case_trajectory(kl_bounds=(d,))["bounds"]
        for k in one:
            assert np.array_equal(one[k][0], a["bounds"][k][i], equal_nan=True), (i, k)


# ---- the guard and the refusals ----------------------------------------------------------------------------------------------------------
def test_a_changed_problem_is_caught_and_the_handle_goes_on():
    N = 3
    x_nom, l, L = um.pend_policy(N)
    ctx = rat.Context(pend_problem(um.PEND_STATE, N, um.PEND_STATE_P))
    noise = rat.UserNoise(3, 0, seed=6)
    ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=100)
    good = ctx.policy_worst_case_trajectory(thetas=(0.0,))
    ctx.set_params([0.1, 0.25, 0.02])
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*changed since the evaluation"):
        ctx.policy_worst_case_trajectory(thetas=(0.0,))
    assert ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=100)["n_ok"] == 100
    other = ctx.policy_worst_case_trajectory(thetas=(0.0,))
    assert not np.array_equal(other["thetas"]["cov_x"], good["thetas"]["cov_x"])
    # a family: the same tables with another Q
    prob, x0, l2, L2 = family(1, 3)
    fam = rat.Context(prob)
    x_det = fam.rollout_open(x0, l2)
    fam.policy_evaluate(x_det, l2, L2, K=50, seed=1)
    fam.policy_worst_case_trajectory(kl_bounds=(0.1,))
    fam.set_problem(rat.LQRiskSensitiveProblem(np.eye(2), np.eye(2), Q=3 * np.eye(2), R=2 * np.eye(2), P=np.eye(2), N=3,
                                               W=np.array([[2.0, 0.6], [0.6, 1.0]]), Qf=np.eye(2)))
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*changed since the evaluation"):
        fam.policy_worst_case_trajectory(kl_bounds=(0.1,))
    assert fam.policy_evaluate(x_det, l2, L2, K=50, seed=1)["n_ok"] == 50
    assert fam.policy_worst_case_trajectory(kl_bounds=(0.1,))["bounds"]["flag"][0] == 0


def test_refusals():
    prob, x0, l, L = family(1, 3)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no evaluation"):                    # nothing to replay yet
        ctx.policy_worst_case_trajectory(thetas=(0.0,))
    ctx.policy_evaluate(x_det, l, L, K=20, seed=1)
    for kw in (dict(), dict(kl_bounds=(-0.1,)), dict(kl_bounds=(np.nan,)), dict(thetas=(np.inf,)), dict(thetas=(-1.0,)),
               dict(kl_bounds=np.ones(17)), dict(thetas=np.ones(17))):                       # rat_policy_worst_case's argument refusals
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG"):
            ctx.policy_worst_case_trajectory(**kw)
    assert ctx.policy_worst_case_trajectory(thetas=(0.0,))["thetas"]["ess"][0] == 20         # ... leave the handle usable
    ctx.policy_worst_case(kl_bounds=(0.1,), costs=np.arange(20.0))                           # uploaded costs are no evaluation's
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no evaluation"):
        ctx.policy_worst_case_trajectory(thetas=(0.0,))
    z = np.random.default_rng(0).standard_normal((8, 3, 2))
    ctx.policy_evaluate(x_det, l, L, z=z)                                                    # injected draws are not kept
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*injected"):
        ctx.policy_worst_case_trajectory(thetas=(0.0,))
    # a source model under N(0, W); and under its sampler with injected draws
    N = 3
    x_nom, pl, pL = um.pend_policy(N)
    src = rat.Context(pend_problem(um.PEND_STATE, N, um.PEND_STATE_P))
    src.policy_evaluate(x_nom, pl, pL, K=16, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rat_user_noise"):
        src.policy_worst_case_trajectory(thetas=(0.0,))
    src.policy_evaluate_noise(x_nom, pl, pL, noise=rat.UserNoise(3, 0, zn=np.zeros((4, N, 3))))
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*injected"):
        src.policy_worst_case_trajectory(thetas=(0.0,))
    assert src.policy_evaluate_noise(x_nom, pl, pL, noise=rat.UserNoise(3, 0, seed=1), K=16)["n_ok"] == 16
    assert src.policy_worst_case_trajectory(thetas=(0.0,))["thetas"]["flag"][0] == 0
    # general sizes
    wide_prob, wx0, wu = rat.synthetic_lq_problem(n=16, m=4, N=5, seed=3, w=1e-2)
    wide = rat.Context(wide_prob)
    wide.policy_evaluate(wx0, wu, K=8, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*n <= 12"):
        wide.policy_worst_case_trajectory(thetas=(0.0,))
    # too many rows x steps for the partial sums
    long_prob = rat.LQRiskSensitiveProblem(np.eye(2), np.eye(2), Q=np.eye(2), R=np.eye(2), N=400, W=np.eye(2), Qf=np.eye(2))
    lc = rat.Context(long_prob)
    lc.policy_evaluate(np.zeros(2), np.zeros((400, 2)), K=4, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*3640"):
        lc.policy_worst_case_trajectory(kl_bounds=0.1 * np.arange(1, 11))
    assert lc.policy_worst_case_trajectory(kl_bounds=(0.1,))["bounds"]["mean_x"].shape == (1, 401, 2)


def test_an_empty_sample_is_nan():
    """Every rollout of the power-law problem fails when it starts below zero: RAT_WC_EMPTY rows, NaN moments."""
    prob, _, l, _ = family(2, 3)
    ctx = rat.Context(prob)
    r = ctx.policy_evaluate(np.array([-0.5, -0.5]), l, K=9, seed=1)
    assert r["n_ok"] == 0
    out = ctx.policy_worst_case_trajectory(kl_bounds=(0.1,), thetas=(0.0,))
    for part in ("bounds", "thetas"):
        assert out[part]["flag"][0] == 2 and np.isnan(out[part]["mean_x"]).all() and np.isnan(out[part]["cov_u"]).all()
