"""The NumPy model of rat_policy_worst_case_trajectory's moment kernels (tests/wc_trajectory_model.py) against a direct np.longdouble
weighted mean and covariance, and the Python mirror of the entry point."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
from ratilqr.jl_amd import _native as nv
from wc_trajectory_model import centre, deviation, direct, moments, row_weights, split

# The deviation of the restated order from the extended-precision answer that test_model_against_longdouble measures (worst over its
# cases, each relative to its step's scale -- wc_trajectory_model.deviation): the GPU tests allow the device ten times this.
CPU_DEV_MEAN, CPU_DEV_COV = 1.2e-16, 3.3e-15


def sample(K, seed, n=3, m=2, N=2, nan_every=0):
    rng = np.random.default_rng(seed)
    x_nom, l = rng.standard_normal((N + 1, n)) * 3.0, rng.standard_normal((N, m))
    x = x_nom[None] + 0.3 * rng.standard_normal((K, N + 1, n))
    u = l[None] + 0.1 * rng.standard_normal((K, N, m))
    J = 5.0 + (x ** 2).sum(axis=(1, 2)) * 0.1 + rng.standard_normal(K)
    if nan_every:
        bad = np.arange(K) % nan_every == 1
        J[bad] = np.nan
        x[bad, 1:] = np.nan                                  # a DomainError rollout's trajectory holds NaN from the step it failed at
        u[bad, 1:] = np.nan
    return x, u, J, x_nom, l


@pytest.mark.parametrize("K,nan_every", [(K, e) for K in (1, 3, 4, 5, 257) for e in (0, 3)] + [(65536 + 5, 7)])
def test_model_against_longdouble(K, nan_every):
    """Rows: the nominal distribution (theta = 0), a tilt, a searched radius and a saturated one (d = +Inf).  K = 65536 + 5
    crosses a chunk, as the GPU tests do.  Measured here, worst over the eleven cases: mean 1.17e-16 (K = 5) and covariance 3.24e-15
    (K = 3 with one rollout selected out: two rollouts under a tilt) of the step's scale; at K = 257 and 65541 the covariance deviates
    by 3.0e-16 and 4.6e-16.  The covariance's subtraction S2 / S0 - mu mu' costs a few ulps of the second moment about the centre, which
    the centring keeps of the covariance's own size unless a tilt moves nearly all the weight onto one rollout.  CPU_DEV_* round these
    up; they are asserted, not only recorded."""
    x, u, J, x_nom, l = sample(K, 10 * K + nan_every, N=2 if K < 1000 else 1, nan_every=nan_every)
    c = centre(x_nom, l)
    y, dead, wc = row_weights(J, kl_bounds=(0.05, np.inf), thetas=(0.0, 0.7))
    assert wc["bounds"]["flag"][1] == 1 and not dead.any()
    mean, cov, ess = moments(x, u, J, c, y, dead)
    mean_d, cov_d = direct(x, u, J, y, dead)
    idx = list(range(3)) + [12, 13]
    dm, dc = deviation(mean, cov, mean_d, cov_d, c[:, idx], K=K)
    print(f"K={K} nan_every={nan_every}: mean {dm:.2e} cov {dc:.2e}")
    assert dm <= CPU_DEV_MEAN and dc <= CPU_DEV_COV
    assert np.all(mean[:, -1, 3:] == 0.0) and np.all(cov[:, -1, 3:, :] == 0.0) and np.all(cov[:, -1, :, 3:] == 0.0)   # u at step N
    assert np.array_equal(cov, cov.swapaxes(-1, -2))
    # the kernel's own effective sample size is the rows'
    ess_rows = np.concatenate([wc["bounds"]["ess"], wc["thetas"]["ess"]])
    assert np.allclose(ess, ess_rows, rtol=1e-12, atol=0.0)
    # the theta = 0 row is the plain sample mean and (population) covariance of the rollouts that have a cost
    ok = ~np.isnan(J)
    assert np.allclose(mean[2, :, :3], x[ok].mean(axis=0), rtol=0, atol=1e-14 * 10)
    # the saturated row is the rollout attaining the maximum
    k = int(np.nanargmax(J))
    assert np.allclose(mean[1, :, :3], x[k], rtol=0, atol=1e-14 * 10) and np.abs(cov[1]).max() < 1e-13


# The same with the centre far from the mean: under a policy the centre is the caller's x_nom, which need not be where the rollouts go (the
# pendulum policy of tests/user_noise_model.py sits seven standard deviations from its closed-loop mean).  There S2 / S0 and mu mu' are
# about fifty times the covariance each and their difference keeps that many fewer digits, in any summation order.
CPU_DEV_FAR_MEAN, CPU_DEV_FAR_COV = 2.2e-16, 4.4e-14


@pytest.mark.parametrize("K,seed", [(257, 1), (257, 2), (65536 + 5, 1), (65536 + 5, 2)])
def test_model_against_longdouble_with_the_centre_seven_standard_deviations_off(K, seed):
    """Trajectories of spread 0.05 about a nominal of size one, the centre 0.35 beside it in every component; one rollout in seven is
    selected out.  Measured: mean 1.7e-16 and covariance 4.3e-14 of the step's scale at K = 65541, seed 1 (seed 2: 2.2e-16 / 4.2e-14; 1.4e-16 / 2.8e-14
    at K = 257).  CPU_DEV_FAR_* round the worst up; asserted."""
    rng = np.random.default_rng(seed)
    n, m, N = 3, 2, 1
    x_nom, l = rng.standard_normal((N + 1, n)), rng.standard_normal((N, m))
    x = x_nom[None] + 0.05 * rng.standard_normal((K, N + 1, n))
    u = l[None] + 0.05 * rng.standard_normal((K, N, m))
    J = 5.0 + (x ** 2).sum(axis=(1, 2)) * 0.1 + rng.standard_normal(K)
    bad = np.arange(K) % 7 == 1
    J[bad], x[bad, 1:], u[bad, 1:] = np.nan, np.nan, np.nan
    c = centre(x_nom + 0.35, l + 0.35)
    y, dead, _ = row_weights(J, kl_bounds=(0.05, np.inf), thetas=(0.0, 0.7))
    mean, cov, _ = moments(x, u, J, c, y, dead)
    mean_d, cov_d = direct(x, u, J, y, dead)
    dm, dc = deviation(mean, cov, mean_d, cov_d, c[:, [0, 1, 2, 12, 13]], K=K)
    print(f"far centre K={K} seed={seed}: mean {dm:.2e} cov {dc:.2e}")
    assert dm <= CPU_DEV_FAR_MEAN and dc <= CPU_DEV_FAR_COV


def test_empty_sample_is_nan_and_nan_trajectories_do_not_leak():
    x, u, J, x_nom, l = sample(5, 1)
    c = centre(x_nom, l)
    y, dead, wc = row_weights(np.full(5, np.nan), kl_bounds=(0.1,), thetas=(0.0,))
    assert dead.all()
    mean, cov, _ = moments(x, u, np.full(5, np.nan), c, y, dead)
    assert np.isnan(mean).all() and np.isnan(cov).all()
    x, u, J, x_nom, l = sample(9, 2, nan_every=2)
    y, dead, _ = row_weights(J, thetas=(0.0, 1.5))
    mean, cov, _ = moments(x, u, J, centre(x_nom, l), y, dead)
    assert np.isfinite(mean).all() and np.isfinite(cov).all()
    # a centre that is not finite is replaced by zero, and any centre gives the same moments
    bad = x_nom.copy()
    bad[1, 0] = np.inf
    mean2, cov2, _ = moments(x, u, J, centre(bad, l), y, dead)
    assert np.allclose(mean2, mean, rtol=0, atol=1e-13) and np.allclose(cov2, cov, rtol=0, atol=1e-12)


def test_split_has_the_documented_shapes():
    x, u, J, x_nom, l = sample(6, 3)
    y, dead, _ = row_weights(J, thetas=(0.0,))
    mean, cov, _ = moments(x, u, J, centre(x_nom, l), y, dead)
    p = split(mean, cov, 3, 2)
    assert p["mean_x"].shape == (1, 3, 3) and p["cov_x"].shape == (1, 3, 3, 3) and p["mean_u"].shape == (1, 2, 2)
    assert p["cov_u"].shape == (1, 2, 2, 2) and p["cov_xu"].shape == (1, 2, 3, 2)


def test_the_entry_point_is_exported_and_mirrored():
    assert "rat_policy_worst_case_trajectory" in nv.EXPORTS and hasattr(nv.lib(), "rat_policy_worst_case_trajectory")
    assert callable(rat.Context.policy_worst_case_trajectory)
    rc = nv.lib().rat_policy_worst_case_trajectory(None, None, 0, None, 0, None, None, None)
    assert rc == 1 and b"rat_policy_worst_case_trajectory" in nv.lib().rat_last_error()
