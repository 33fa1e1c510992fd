"""NumPy model of rat_policy_tail_trajectory / _disturbance / _params (csrc/policy_mc.hip: tlt_levels, tlt_weights and the liveness
schedule of the moment kernels) -- test aid.

`tail_weights` restates the rule of the row weights: the OK costs sorted, the rank k = clamp(ceil(n alpha), 1, n), v = s_k, y = 1 above
v, the fractional atom ((n - k - c_gt) + (k - n alpha)) / c_eq on v, 0 below and at a NaN cost; a tail thinner than one rollout puts
y = 1 on the maxima; an empty sample or one that holds +-Inf is dead (flags 2, 3).  dtype = np.longdouble gives the same rule in extended
precision (the atom and the sums; the comparisons are exact either way).

The moments of given trajectories under those weights are the worst-case calls' models with y handed in: `moments` of
wc_trajectory_model / wc_disturbance_model / wc_params_model restate the device's summation order -- which the liveness schedule keeps:
a skipped term is 0 D, and adding it changes no bit where D is finite -- and their `direct` is np.longdouble straight from the
definition.  The difference the schedule makes on non-finite data: a rollout without weight in a row is left out of that row even where
its trajectory holds Inf (`select_out`).

`closed_form`: n = N = 1, f = x + u, c = 0, h = x[0] under Gaussian noise of standard deviation sigma: J = x_1 is normal, its tail above
the alpha-quantile is the upper tail of a normal."""
import math

import numpy as np

OK, SATURATED, EMPTY, NONFINITE = 0, 1, 2, 3
MARGIN = 8.0
# The restatement (float64, the device's order and its S2 / S0 - m m' about the centre) against np.longdouble, in the scales of
# wc_trajectory_model.deviation / wc_disturbance_model.deviation / wc_params_model.deviation: the worst over the shapes of
# tests/test_gpu_tail_scenarios.py, measured by tests/test_cpu_tail_scenarios.py::test_restatement_against_longdouble on the host.
CPU_DEV_MEAN = 2.1e-16       # 5 x 3, N = 4, K = 65541 (measured 2.10e-16)
CPU_DEV_COV = 7.4e-15        # 1 x 1, N = 1, K = 3: two rollouts in the tail, the covariance a difference of squares (measured 7.32e-15)


def tail_weights(costs, alphas, dtype=np.float64):
    """(y [R, K], dead [R], info): info holds per level v, tail, atom (the weight on v), cvar and flag"""
    J = np.asarray(costs, dtype=np.float64).ravel()
    al = np.atleast_1d(np.asarray(alphas, dtype=np.float64)).ravel()
    ok = ~np.isnan(J)
    s = np.sort(np.where(J[ok] == 0.0, 0.0, J[ok]))                    # (-0.0 counts as +0.0)
    n = s.size
    R = al.size
    y = np.zeros((R, J.size), dtype=dtype)
    info = dict(v=np.full(R, np.nan), tail=np.full(R, np.nan), atom=np.full(R, np.nan), cvar=np.full(R, np.nan), flag=np.zeros(R, dtype=np.int64))
    flag = EMPTY if n == 0 else (NONFINITE if not np.isfinite(s).all() else OK)
    if flag != OK:
        info["flag"][:] = flag
        return y, np.ones(R, dtype=bool), info
    for r in range(R):
        av = np.float64(n) * al[r]                                    # one rounded product
        tail = dtype(n) - dtype(av)
        k = int(min(max(math.ceil(av), 1), n))
        v = s[k - 1]
        gt, eq = ok & (J > v), ok & (J == v)
        if tail < 1:
            y[r] = np.where(eq, 1, 0)
            info["flag"][r] = SATURATED
            atom, cvar = dtype(1), dtype(v)
        else:
            atom = ((dtype(n) - k - int(gt.sum())) + (dtype(k) - dtype(av))) / int(eq.sum())
            y[r] = np.where(gt, dtype(1), np.where(eq, atom, dtype(0)))
            cvar = dtype(v) + (J[gt].astype(dtype) - dtype(v)).sum() / tail
        info["v"][r], info["tail"][r], info["atom"][r], info["cvar"][r] = v, float(tail), float(atom), float(cvar)
    return y, np.zeros(R, dtype=bool), info


def select_out(z, y_row):
    """what one row of the liveness schedule reads of per-rollout data z [K, ...]: a rollout without weight is left out whatever it holds"""
    keep = np.asarray(y_row) != 0
    return np.where(keep.reshape((-1,) + (1,) * (z.ndim - 1)), z, 0.0)


def phi(z):
    return math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def norm_ppf(p):
    """the standard normal quantile by bisection on erf (no SciPy): 200 halvings of [-10, 10], far past the last bit"""
    lo, hi = -10.0, 10.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 0.5 * (1.0 + math.erf(mid / math.sqrt(2.0))) < p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def closed_form(x0, u0, sigma, alpha):
    """(mean, variance) of x_1 = x0 + u0 + sigma z given z above its alpha-quantile: the upper tail of a normal"""
    if alpha == 0.0:
        return x0 + u0, sigma * sigma
    za = norm_ppf(alpha)
    lam = phi(za) / (1.0 - alpha)
    return x0 + u0 + sigma * lam, sigma * sigma * (1.0 + za * lam - lam * lam)


def closed_form_se(sigma, alpha, K):
    """standard errors of the tail's sample mean and sample variance, from the closed form's moments and the tail's size: the tail holds
    K (1 - alpha) rollouts, so sqrt(var / (K (1 - alpha))) for the mean and sqrt((m4 - var^2) / (K (1 - alpha))) for the variance, the
    fourth central moment by quadrature on the closed-form density.  (The threshold is itself a sample quantile, which adds to the
    estimator's variance; that term is left out, so these are the smaller figures and the bound in them the stricter one.)"""
    _, var = closed_form(0.0, 0.0, sigma, alpha)
    za = norm_ppf(alpha) if alpha > 0.0 else -10.0
    z = np.linspace(za, za + 12.0, 200001)
    w = np.exp(-0.5 * z * z)
    w /= w.sum()
    mu = (w * z).sum()
    m4 = sigma ** 4 * (w * (z - mu) ** 4).sum()
    n_tail = K * (1.0 - alpha)
    return math.sqrt(var / n_tail), math.sqrt(max(m4 - var * var, 0.0) / n_tail)
