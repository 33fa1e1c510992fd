"""The NumPy model of rat_policy_worst_case_disturbance's moment kernels (tests/wc_disturbance_model.py) against a direct np.longdouble
answer, the whole pipeline on the host against the closed form of the tilted Gaussian, and the Python mirror of the entry point."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
import rare_event_model as rm
from leqg_exact import random_lq
from ratilqr.jl_amd import _native as nv
from wc_disturbance_model import centre_w, closed_form, deviation, direct, moments, z_offset
from wc_trajectory_model import centre, row_weights, weights_from_rows
from wc_trajectory_model import direct as direct_z

# The deviation of the restated order from the extended-precision answer that test_model_against_longdouble measures (worst over its
# cases, each relative to its step's scale -- wc_disturbance_model.deviation): the GPU tests allow the device ten times this.
CPU_DEV_MEAN, CPU_DEV_COV, CPU_DEV_WZ = 2.2e-16, 8.3e-15, 2.8e-16
# ... with the (x, u) centre seven standard deviations from where the rollouts go (a caller's x_nom that is not the closed-loop mean):
# only cov_wz reads that centre
CPU_DEV_FAR_WZ = 7.6e-15
# ... and what c_w = 0 would cost under a sampler whose mean is seven standard deviations from zero: recorded, the device does not do it
CPU_DEV_ZERO_CENTRE_COV = 4.7e-14


def sample(K, seed, n=3, m=2, N=2, nan_every=0, w_mean=0.0, first_off=4.0):
    """Rollouts the way a feedback adversary leaves them: w_t with a mean and a spread of 0.3, x_{t+1} depending on w_t, u_t on x_t, a
    cost that grows with them.  The first rollout -- the one the device takes c_w from -- is put first_off standard deviations from the
    mean in every component of w: a centre as far off as one draw in ten thousand is."""
    rng = np.random.default_rng(seed)
    x_nom, l = rng.standard_normal((N + 1, n)) * 3.0, rng.standard_normal((N, m))
    w = w_mean + 0.3 * rng.standard_normal((K, N, n))
    w[0] = w_mean + 0.3 * first_off
    x = np.empty((K, N + 1, n))
    x[:, 0] = x_nom[0]
    for t in range(N):
        x[:, t + 1] = x_nom[t + 1] + 0.5 * (x[:, t] - x_nom[t]) + (w[:, t] - w_mean)
    u = l[None] + 0.2 * (x[:, :N, :m] - x_nom[None, :N, :m]) + 0.01 * rng.standard_normal((K, N, m))
    J = 5.0 + ((x - x_nom[None]) ** 2).sum(axis=(1, 2)) + 0.3 * rng.standard_normal(K)
    if nan_every:
        bad = np.arange(K) % nan_every == 1
        J[bad] = np.nan
        w[bad, 1:], x[bad, 1:], u[bad, 1:] = np.nan, np.nan, np.nan   # a DomainError rollout holds NaN from the step it failed at
    return w, x, u, J, x_nom, l


def z_scales(x, u, J, y, dead, c_z, n, m):
    mean_z, cov_z = direct_z(x, u, J, y, dead)
    return z_offset(mean_z[:, :-1], cov_z[:, :-1], c_z[:-1][:, list(range(n)) + list(range(12, 12 + m))])


CASES = [(K, e) for K in (1, 3, 4, 5, 257) for e in (0, 3)] + [(65536 + 5, 7)]


@pytest.mark.parametrize("K,nan_every", CASES)
def test_model_against_longdouble(K, nan_every):
    """Rows: a searched radius, a saturated one (d = +Inf), the nominal distribution and a tilt.  K = 65536 + 5 crosses a chunk.  The
    sampler's mean is seven standard deviations from zero; c_w is the device's (the first rollout with a cost, here four standard
    deviations from the mean in every component, so that S2 / S0 and m m' are seventeen times the covariance each).  Measured here,
    worst over the eleven cases: mean 2.12e-16 and cov_w 8.25e-15 (K = 65541; 7.4e-15 at K = 257), cov_wz 2.71e-16 (K = 5) of the step's
    scale.  CPU_DEV_* round these up; asserted."""
    w, x, u, J, x_nom, l = sample(K, 10 * K + nan_every, N=2 if K < 1000 else 1, nan_every=nan_every, w_mean=2.1)
    c_z, c_w = centre(x_nom, l), centre_w(w, J)
    assert np.array_equal(c_w[:, :3], w[0])
    y, dead, wc = row_weights(J, kl_bounds=(0.05, np.inf), thetas=(0.0, 0.7))
    assert wc["bounds"]["flag"][1] == 1 and not dead.any()
    mw, cw, cwz, ess = moments(w, x, u, J, c_w, c_z, y, dead)
    ref = direct(w, x, u, J, y, dead)
    dm, dc, dz = deviation((mw, cw, cwz), ref, c_w[:, :3], z_scales(x, u, J, y, dead, c_z, 3, 2), K=K)
    print(f"K={K} nan_every={nan_every}: mean {dm:.2e} cov_w {dc:.2e} cov_wz {dz:.2e}")
    assert dm <= CPU_DEV_MEAN and dc <= CPU_DEV_COV and dz <= CPU_DEV_WZ
    assert np.array_equal(cw, cw.swapaxes(-1, -2))
    assert np.all(cwz[:, 0, :, :3] == 0.0)                            # x_0 is the centre: no product is formed about it
    ess_rows = np.concatenate([wc["bounds"]["ess"], wc["thetas"]["ess"]])
    assert np.allclose(ess, ess_rows, rtol=1e-12, atol=0.0)
    # without the cross product the other two are the same bits
    mw2, cw2, none, _ = moments(w, x, u, J, c_w, c_z, y, dead, cross=False)
    assert none is None and np.array_equal(mw2, mw) and np.array_equal(cw2, cw)
    # the saturated row is the rollout attaining the maximum
    k = int(np.nanargmax(J))
    assert np.allclose(mw[1], w[k], rtol=0, atol=1e-14 * 10) and np.abs(cw[1]).max() < 1e-13 and np.abs(cwz[1]).max() < 1e-13


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("K,seed", [(257, 1), (257, 2), (65536 + 5, 1), (65536 + 5, 2)])
def test_model_against_longdouble_with_far_centres(K, seed, flat):
    """The (x, u) centre 0.35 beside trajectories of spread 0.05 (test_cpu_wc_trajectory's far-centre case): cov_wz is the difference of
    two numbers up to fifty times sd(w) sd(z), the scale it is held against together with that offset.  Measured: cov_wz 5.17e-16
    (K = 65541, seed 2) where every component varies, and 7.50e-15 (K = 65541, seed 2; 2.7e-16 at K = 257) with `flat`: a component of
    (x, u) that does not vary but sits beside its centre, whose sum y Dw a and (sum y Dw) a cancel to the rounding of two sums of K terms --
    it grows with K as those do; mean_w and cov_w do not read that centre (cov_w 5.2e-16 at most here, the first rollout being an ordinary draw).
    And the road not taken, c_w = 0 under the same sampler (mean seven standard deviations from zero): cov_w 4.65e-14 (K = 65541,
    seed 2) against 3.5e-16 with the device's centre on the same rollouts -- two digits the device's centre keeps."""
    rng = np.random.default_rng(seed)
    n, m, N = 3, 2, 1
    x_nom, l = rng.standard_normal((N + 1, n)), rng.standard_normal((N, m))
    w = 0.35 + 0.05 * rng.standard_normal((K, N, n))
    x = x_nom[None] + 0.05 * rng.standard_normal((K, N + 1, n))
    x[:, 1] += w[:, 0] - 0.35
    u = l[None] + 0.05 * rng.standard_normal((K, N, m))
    if flat:
        # a sampler that leaves w[0] alone (PEND_NAN of tests/user_noise_model.py), and state and control components that do not vary but sit
        # beside their centre: the pendulum's position one step on.  Their products sum y Dw a and (sum y Dw) a are rounded apart.
        w[:, :, 0], x[:, :, 0], u[:, :, 0] = 0.0, x_nom[None, :, 0], l[None, :, 0]
    J = 5.0 + (x ** 2).sum(axis=(1, 2)) * 0.1 + rng.standard_normal(K)
    bad = np.arange(K) % 7 == 1
    J[bad], w[bad], x[bad, 1:], u[bad] = np.nan, np.nan, np.nan, np.nan
    c_z, c_w = centre(x_nom + 0.35, l + 0.35), centre_w(w, J)
    y, dead, _ = row_weights(J, kl_bounds=(0.05, np.inf), thetas=(0.0, 0.7))
    ref = direct(w, x, u, J, y, dead)
    zs = z_scales(x, u, J, y, dead, c_z, n, m)
    dm, dc, dz = deviation(moments(w, x, u, J, c_w, c_z, y, dead)[:3], ref, c_w[:, :n], zs, K=K)
    zm, zc, _ = deviation(moments(w, x, u, J, 0.0 * c_w, c_z, y, dead)[:3], ref, 0.0 * c_w[:, :n], zs, K=K)
    print(f"far centres K={K} seed={seed} flat={flat}: mean {dm:.2e} cov_w {dc:.2e} cov_wz {dz:.2e}; with c_w = 0: mean {zm:.2e} cov_w {zc:.2e}")
    assert dm <= CPU_DEV_MEAN and dc <= CPU_DEV_COV and dz <= CPU_DEV_FAR_WZ
    assert zc <= CPU_DEV_ZERO_CENTRE_COV


def test_empty_sample_is_nan_and_nan_disturbances_do_not_leak():
    w, x, u, J, x_nom, l = sample(5, 1)
    y, dead, _ = row_weights(np.full(5, np.nan), kl_bounds=(0.1,), thetas=(0.0,))
    assert dead.all()
    nanJ = np.full(5, np.nan)
    assert np.all(centre_w(w, nanJ) == 0.0)                           # no rollout has a cost: the centre is zero
    mw, cw, cwz, _ = moments(w, x, u, nanJ, centre_w(w, nanJ), centre(x_nom, l), y, dead)
    assert np.isnan(mw).all() and np.isnan(cw).all() and np.isnan(cwz).all()
    w, x, u, J, x_nom, l = sample(9, 2, nan_every=2)
    y, dead, _ = row_weights(J, thetas=(0.0, 1.5))
    mw, cw, cwz, _ = moments(w, x, u, J, centre_w(w, J), centre(x_nom, l), y, dead)
    assert np.isfinite(mw).all() and np.isfinite(cw).all() and np.isfinite(cwz).all()
    assert mw.shape == (2, 2, 3) and cw.shape == (2, 2, 3, 3) and cwz.shape == (2, 2, 3, 5)
    # a centre entry that is not finite is replaced by zero, and any centre gives the same moments
    w[0, 1, 0] = np.inf
    J2 = J.copy()
    c2 = centre_w(w, J2)
    assert c2[1, 0] == 0.0 and c2[1, 1] == w[0, 1, 1]
    w[0, 1, 0] = 0.3
    mw2, cw2, cwz2, _ = moments(w, x, u, J, 0.0 * c2, centre(x_nom, l), y, dead)
    mw3, cw3, cwz3, _ = moments(w, x, u, J, centre_w(w, J), centre(x_nom, l), y, dead)
    assert np.allclose(mw2, mw3, rtol=0, atol=1e-13) and np.allclose(cw2, cw3, rtol=0, atol=1e-12) and np.allclose(cwz2, cwz3, rtol=0, atol=1e-12)


# ---- the closed form: the tilted law of the stacked noise --------------------------------------------------------------------------------
CF_K, CF_SEED, CF_FACTOR, CF_NSE = 1 << 16, 2026, 0.3, 6.0


def closed_form_cases():
    """(label, prob, x0, l, L): the 2 x 2 LQ problem of tests/test_gpu_wc_trajectory.family(1, 3) and a random 4 x 2 one with N = 5 under a
    small random gain"""
    small = rat.LQRiskSensitiveProblem(np.eye(2), np.eye(2), Q=np.eye(2), R=2 * np.eye(2), P=np.eye(2), N=3, W=np.array([[2.0, 0.6], [0.6, 1.0]]),
                                       Qf=np.eye(2))
    prob, x0, l = random_lq(4, 2, 5, seed=11)
    L = 0.1 * np.random.default_rng(12).standard_normal((5, 2, 4))
    return [("2x2 N=3", small, np.array([0.5, -1.0]), np.ones((3, 2)), 0.3 * np.ones((3, 2, 2))), ("4x2 N=5", prob, x0, l, L)]


def det_rollout(prob, x0, l):
    x = np.zeros((prob.N + 1, prob.n))
    x[0] = x0
    for k in range(prob.N):
        x[k + 1] = prob.A @ x[k] + prob.B @ l[k]
    return x


def lq_costs(prob, x, u):
    """J [K] of trajectories x [K, N+1, n], u [K, N, m] on an LQRiskSensitiveProblem with kappa = 0, plain NumPy"""
    tv = lambda tab, k: np.asarray(tab[k] if prob.cost_tv else tab, float)
    J = np.zeros(x.shape[0])
    for k in range(prob.N):
        Q, R, P, qv, rv, q0 = (tv(t, k) for t in (prob.Q, prob.R, prob.P, prob.qv, prob.rv, prob.q0))
        xk, uk = x[:, k], u[:, k]
        J += 0.5 * np.einsum("ki,ij,kj->k", xk, Q, xk) + 0.5 * np.einsum("ki,ij,kj->k", uk, R, uk) + np.einsum("ki,ij,kj->k", uk, P, xk)
        J += xk @ qv + uk @ rv + float(q0)
    xN = x[:, prob.N]
    return J + 0.5 * np.einsum("ki,ij,kj->k", xN, prob.Qf, xN) + xN @ prob.qvf + prob.q0f


def within_se(got, se, ref, label):
    """every entry of (mean_w, cov_w, cov_wz) [N, ...] within CF_NSE standard errors of the closed form.  A few hundred entries: a
    Gaussian tail at 6 is 2e-9 each, the union below 1e-6.  Where the exact value is a deterministic zero -- the covariance with x_0, with
    an open-loop control -- the estimate and its SE are both rounding: 1e-13 of sd(w) |z| is allowed on top, far below any SE."""
    worst = 0.0
    for g, s, r, name in zip(got, se, ref, ("mean_w", "cov_w", "cov_wz")):
        atol = 1e-13 * max(np.abs(r).max(), 1.0)
        ratio = np.max(np.maximum(np.abs(g - r) - atol, 0.0) / np.maximum(s, 1e-300))
        print(f"{label} {name}: worst {ratio:.2f} se over {g.size} entries")
        assert np.all(np.abs(g - r) <= CF_NSE * s + atol), (label, name, ratio)
        worst = max(worst, ratio)
    return worst


def host_pipeline(prob, x0, l, L):
    """generator model -> rollout -> costs: (w, x, u, J, x_det)"""
    z = rm.normals(CF_SEED, 0, CF_K, prob.N, prob.n)
    C = rm.chol_factors(prob)
    w = np.einsum("tij,ktj->kti", C, z)
    x_det = det_rollout(prob, x0, l)
    x, u, _ = rm.rollout(prob, x_det, l, L, z)
    return w, x, u, lq_costs(prob, x, u), x_det


@pytest.mark.parametrize("case", [0, 1])
def test_host_pipeline_against_the_closed_form(case):
    """theta = 0.3 / lambda_max(C'HC) and theta = 0, K = 2^16, seed 2026: generator model, rollout, costs, weights and `direct`, all on
    the host, against closed_form within 6 SE (the delta-method SE of the self-normalised estimate, from the same rollouts).  The
    condition ESS >= K / 4 is asserted: measured ESS / K = 0.698 (2 x 2, N = 3) and 0.25025 (4 x 2, N = 5: a margin of 1e-3, where costs
    that differ in their last digits move the ESS by 1e-12).  Worst entry: 2.98 SE."""
    label, prob, x0, l, L = closed_form_cases()[case]
    w, x, u, J, x_det = host_pipeline(prob, x0, l, L)
    lam = closed_form(prob, x0, l, L, x_det, 0.0)[4]
    theta = CF_FACTOR / lam
    y, dead = weights_from_rows(J, [theta, 0.0], [0, 0])
    ess = y.sum(axis=1) ** 2 / (y * y).sum(axis=1)
    print(f"{label}: theta {theta:.4g}, ESS / K = {ess[0] / CF_K:.3f}")
    assert ess[0] >= CF_K / 4 and ess[1] == CF_K
    mw, cw, cwz, se = direct(w, x, u, J, y, dead, want_se=True)
    for r, th in enumerate((theta, 0.0)):
        ref = closed_form(prob, x0, l, L, x_det, th)
        assert ref[3]
        within_se((mw[r], cw[r], cwz[r]), tuple(s[r] for s in se), ref[:3], f"{label} theta={th:.3g}")
    # theta = 0: cov_w is W(t) and the noise does not know the state it acts on
    ref0 = closed_form(prob, x0, l, L, x_det, 0.0)
    assert np.all(ref0[2] == 0.0) and np.all(ref0[0] == 0.0)
    assert np.allclose(ref0[1], [prob.W(t) for t in range(prob.N)], rtol=1e-12, atol=0)
    # theta > 0: the adversary's noise has a mean and depends on the state
    ref1 = closed_form(prob, x0, l, L, x_det, theta)
    assert np.abs(ref1[0]).max() > 0 and np.abs(ref1[2][1:, :, :prob.n]).max() > 0


def test_closed_form_is_the_tilt_of_leqg_exact():
    """What the closed form must share with leqg_exact.exact_value, which builds b and H on its own: the tilt exists up to
    1 / lambda_max(C'HC) and not beyond -- the same threshold there -- and its covariance grows with theta in the Loewner order from
    Sigma at theta = 0."""
    from leqg_exact import exact_value
    _, prob, x0, l, L = closed_form_cases()[1]
    x_det = det_rollout(prob, x0, l)
    lam = closed_form(prob, x0, l, L, x_det, 0.0)[4]
    c0, c1, c2 = (closed_form(prob, x0, l, L, x_det, f / lam)[1] for f in (0.0, 0.3, 0.6))
    for t in range(prob.N):
        assert np.linalg.eigvalsh(c1[t] - c0[t]).min() > -1e-15 and np.linalg.eigvalsh(c2[t] - c1[t]).min() > -1e-15
    assert closed_form(prob, x0, l, L, x_det, 0.99 / lam)[3] and not closed_form(prob, x0, l, L, x_det, 1.01 / lam)[3]
    assert exact_value(prob, x0, l, None, L, x_det, 0.99 / lam)[1] and not exact_value(prob, x0, l, None, L, x_det, 1.01 / lam)[1]


def test_the_entry_point_is_exported_and_mirrored():
    assert "rat_policy_worst_case_disturbance" in nv.EXPORTS and hasattr(nv.lib(), "rat_policy_worst_case_disturbance")
    assert callable(rat.Context.policy_worst_case_disturbance)
    rc = nv.lib().rat_policy_worst_case_disturbance(None, None, 0, None, 0, None, None, None, None)
    assert rc == 1 and b"rat_policy_worst_case_disturbance" in nv.lib().rat_last_error()
