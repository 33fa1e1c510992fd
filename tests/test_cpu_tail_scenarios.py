"""The host model of the tail calls (tests/tail_scenarios_model.py): the weights rule on hand-made costs, the restatement of the
moments against np.longdouble over the shapes of tests/test_gpu_tail_scenarios.py (the figures the device is then held to eight times
of), and the closed-form truncated normal on K = 2^16 NumPy draws."""
import numpy as np
import pytest

import tail_risk_model as tr
import tail_scenarios_model as ts
from wc_trajectory_model import centre, deviation, direct, moments

SHAPES = ((1, 1, 1), (5, 3, 4), (12, 4, 3))
KS = (1, 3, 4 * 4 * 8 + 1, (1 << 16) + 5)                            # 4 WT_WAVES WT_SLOTS + 1: one slot gets a second group; a second chunk of five
LEVELS = (0.0, 0.5, 0.9)
CLOSED_K, CLOSED_SEED, CLOSED_SIGMA, CLOSED_ALPHAS = 1 << 16, 11, 0.7, (0.5, 0.9, 0.99)


def levels(K):
    return LEVELS + (1.0 - 0.5 / K,)


def host_rollouts(n, m, N, K, seed=1):
    """closed-loop linear rollouts of that shape on the host: (x [K, N+1, n], u [K, N, m], costs [K], the noise-free x, l)"""
    r = np.random.default_rng(seed)
    A = 0.9 * np.linalg.qr(r.standard_normal((n, n)))[0]
    B = r.standard_normal((n, m)) / np.sqrt(n)
    L = 0.1 * r.standard_normal((N, m, n))
    l = 0.5 * r.standard_normal((N, m))
    x0 = r.standard_normal(n)
    xd = np.zeros((N + 1, n))
    xd[0] = x0
    for t in range(N):
        xd[t + 1] = A @ xd[t] + B @ l[t]
    x, u = np.zeros((K, N + 1, n)), np.zeros((K, N, m))
    x[:, 0] = x0
    for t in range(N):
        u[:, t] = l[t] + (x[:, t] - xd[t]) @ L[t].T
        x[:, t + 1] = x[:, t] @ A.T + u[:, t] @ B.T + 0.3 * r.standard_normal((K, n))
    costs = 0.5 * (x ** 2).sum(axis=(1, 2)) + 0.05 * (u ** 2).sum(axis=(1, 2))
    return x, u, costs, xd, l


# ---- the weights rule ----------------------------------------------------------------------------------------------------------------------
HAND = {
    "all distinct": (np.array([3.0, -1.0, 7.5, 2.0, 0.25, 11.0, 4.0, -6.0, 9.0, 1.0]), (0.0, 0.3, 0.5, 0.85, 0.9)),
    "ties straddling the rank": (np.array([1.0, 2.0, 5.0, 5.0, 5.0, 5.0, 5.0, 8.0, 9.0, 0.5, 5.0, 7.0]), (0.0, 0.3, 0.45, 0.5, 0.6)),
    "all equal": (np.full(9, 2.5), (0.0, 0.5, 0.8)),
    "NaNs mixed in": (np.array([np.nan, 3.0, 1.0, np.nan, 4.0, 4.0, 2.0, np.nan, 9.0]), (0.0, 0.5, 0.7)),
    "a tail thinner than one rollout": (np.array([1.0, 6.0, 2.0, 6.0, 3.0]), (0.85, 0.99)),
}


@pytest.mark.parametrize("name", list(HAND))
def test_weights_rule_on_hand_made_costs(name):
    J, alphas = HAND[name]
    y, dead, info = ts.tail_weights(J, alphas)
    yl, _, il = ts.tail_weights(J, alphas, dtype=np.longdouble)
    ok = ~np.isnan(J)
    n = ok.sum()
    assert not dead.any() and np.all(y[:, ~ok] == 0.0)
    for r, a in enumerate(alphas):
        w = y[r] / y[r].sum()
        assert abs(w.sum() - 1.0) <= 4e-16
        tail = n - n * a
        if tail < 1.0:
            assert info["flag"][r] == ts.SATURATED and np.array_equal(y[r] != 0, ok & (J == np.nanmax(J))) and info["cvar"][r] == np.nanmax(J)
        else:
            assert info["flag"][r] == ts.OK
            assert abs(y[r].sum() - tail) <= 1e-14 * n               # the weights are the tail's mass in rollouts
            v, P1 = info["v"][r], np.clip(J[ok] - info["v"][r], 0.0, None).sum()
            assert abs((w[ok] * J[ok]).sum() - (v + P1 / tail)) <= 1e-14 * np.abs(J[ok]).max()     # Rockafellar-Uryasev
            assert np.all(w <= 1.0 / tail * (1 + 1e-15))             # the CVaR dual's bound on the density
        assert np.allclose(y[r], yl[r].astype(float), rtol=1e-15, atol=0) and abs(info["cvar"][r] - il["cvar"][r]) <= 1e-15 * np.abs(J[ok]).max()
        # the existing model of rat_policy_tail_risk: the same quantile, CVaR and, normalised, the same weights
        ref = tr.tail_risk(J, [a], want_weights=True)
        assert ref["var"][0] == info["v"][r] and abs(ref["cvar"][0] - info["cvar"][r]) <= 1e-14 * np.abs(J[ok]).max()
        assert np.allclose(ref["weights"], w, rtol=1e-14, atol=0)
    if alphas[0] == 0.0:                                              # the whole sample: y = 1 wherever there is a cost
        assert np.array_equal(y[0], ok.astype(float))


def test_dead_samples():
    for J, flag in ((np.full(4, np.nan), ts.EMPTY), (np.array([1.0, np.inf, 2.0]), ts.NONFINITE)):
        y, dead, info = ts.tail_weights(J, (0.0, 0.9))
        assert dead.all() and not y.any() and np.all(info["flag"] == flag)


def test_select_out():
    z = np.array([[1.0, np.inf], [2.0, 3.0], [np.nan, 0.0]])
    assert np.array_equal(ts.select_out(z, np.array([0.0, 1.0, 0.0])), np.array([[0.0, 0.0], [2.0, 3.0], [0.0, 0.0]]))


# ---- the restatement against np.longdouble -------------------------------------------------------------------------------------------------
def test_restatement_against_longdouble():
    """the device's order and its S2 / S0 - m m' about the centre, in float64, against the definition in np.longdouble, under the tail
    weights of the GPU test's levels, over its shapes: the figures CPU_DEV_MEAN / CPU_DEV_COV record"""
    worst_m = worst_c = 0.0
    for (n, m, N) in SHAPES:
        for K in KS:
            x, u, costs, xd, l = host_rollouts(n, m, N, K)
            y, dead, _ = ts.tail_weights(costs, levels(K))
            c = centre(xd, l)
            mean, cov, _ = moments(x, u, costs, c, y, dead)
            mean_d, cov_d = direct(x, u, costs, y, dead)
            dm, dc = deviation(mean, cov, mean_d, cov_d, c[:, list(range(n)) + list(range(12, 12 + m))], K=K)
            print(f"{n} x {m}, N = {N}, K = {K}: mean {dm:.2e} cov {dc:.2e}")
            worst_m, worst_c = max(worst_m, dm), max(worst_c, dc)
    print(f"worst: mean {worst_m:.3e} cov {worst_c:.3e}")
    assert worst_m <= ts.CPU_DEV_MEAN and worst_c <= ts.CPU_DEV_COV
    assert worst_m >= 0.5 * ts.CPU_DEV_MEAN and worst_c >= 0.5 * ts.CPU_DEV_COV        # the recorded figures are the measured ones


# ---- the closed form -----------------------------------------------------------------------------------------------------------------------
def closed_form_check(x1, costs, mean, var, x0, u0, label):
    """mean [R], var [R] of x_1 per level of CLOSED_ALPHAS against the truncated normal, in standard errors; returns the worst"""
    worst = 0.0
    for r, a in enumerate(CLOSED_ALPHAS):
        cm, cv = ts.closed_form(x0, u0, CLOSED_SIGMA, a)
        se_m, se_v = ts.closed_form_se(CLOSED_SIGMA, a, costs.size)
        em, ev = abs(mean[r] - cm) / se_m, abs(var[r] - cv) / se_v
        print(f"{label} alpha = {a}: mean {em:.2f} se, variance {ev:.2f} se")
        worst = max(worst, em, ev)
    assert worst <= 5.0, (label, worst)
    return worst


def test_closed_form_on_numpy_draws():
    x0, u0 = 0.3, -0.1
    z = np.random.default_rng(CLOSED_SEED).standard_normal(CLOSED_K)
    x1 = x0 + u0 + CLOSED_SIGMA * z
    y, dead, _ = ts.tail_weights(x1, CLOSED_ALPHAS)
    w = y / y.sum(axis=1, keepdims=True)
    mean = (w * x1).sum(axis=1)
    var = (w * (x1[None] - mean[:, None]) ** 2).sum(axis=1)
    closed_form_check(x1, x1, mean, var, x0, u0, "numpy")
