"""NumPy model of rat_policy_tail_events / rat_policy_tail_events_user (csrc/policy_mc.hip: tlt_levels, tlt_weights, tle_sums, tle_final)
-- test aid.

The rows are tests/tail_risk_model.tail_risk's.  `level_weights` restates tlt_levels / tlt_weights from them: per level y = 1 above VAR,
the atom ((n - k - c_gt) + (k - a)) / c_eq on VAR, 0 below and at a NaN cost; a level thinner than one rollout puts y = 1 on the maxima;
an empty or non-finite sample is dead.  (The common factor 1 / TAIL_N of the tail distribution divides out of every slot.)

`reduce` restates tle_sums and tle_final on a given g [K, N+1, E]: tests/events_model's per-rollout margins, first steps and indicators,
its summation order (a term the liveness schedule passes over is a 0, and adding it changes no bit) and its slots, with the one
difference the schedule makes: a rollout without weight in a row is selected out of that row's y M, whatever its margin holds.
PROB_ROBUST is min(1, (N_VIOL / N_OK) / (TAIL_N / N_OK)) in double (PROB where rounding leaves that a last bit below it), EVENT_FLAG the
row's flag.  `tail_events` is `reduce` on the g of
quadratic events in the device's order of operations (events_model.g_device)."""
import numpy as np

import events_model as em
import tail_risk_model as tr

OK, SATURATED, EMPTY, NONFINITE = tr.OK, tr.SATURATED, tr.EMPTY, tr.NONFINITE
SLOT_NAMES = em.SLOT_NAMES + ("prob_robust",)


def level_weights(costs, rows):
    """(y [R, K], dead [R]) from the costs and tail_risk's rows (its var, c_gt, c_eq, flag and alpha)"""
    J = np.asarray(costs, dtype=np.float64).ravel()
    ok = ~np.isnan(J)
    al = np.atleast_1d(rows["alpha"])
    n = float(ok.sum())
    y = np.zeros((al.size, J.size))
    dead = np.isin(rows["flag"], (EMPTY, NONFINITE))
    for r in range(al.size):
        if dead[r]:
            continue
        v = rows["var"][r]
        with np.errstate(invalid="ignore"):
            gt, eq = ok & (J > v), ok & (J == v)
        if rows["flag"][r] == SATURATED:
            atom = 1.0
        else:
            a, k = tr.rank_of(n, al[r])
            atom = ((n - k - rows["c_gt"][r]) + (k - a)) / rows["c_eq"][r]
        y[r] = np.where(gt, 1.0, np.where(eq, atom, 0.0))
    return y, dead


def reduce(g, windows, costs, alphas):
    """the device's answer on g [K, N+1, E] with the windows [(Q, a, b, t_lo, t_hi)] * E (only t_lo, t_hi are read): a dict of the rows
    (tail_risk_model.SLOTS), SLOT_NAMES [R, E+1], event_flag [R, E+1], step [R, E+1, N+1], margins and tau [E+1, K], y [R, K]"""
    J = np.asarray(costs, dtype=np.float64).ravel()
    ok = ~np.isnan(J)
    rows = tr.tail_risk(J, alphas)
    y, dead = level_weights(J, rows)
    M, tau, viol = em.per_rollout(np.asarray(g, dtype=np.float64), windows, ok)
    R, E1 = y.shape[0], M.shape[0]
    A = tau >= 0
    S = np.zeros((R, E1, 6))
    with np.errstate(all="ignore"):
        for e in range(E1):
            for r in range(R):
                yr, y2 = y[r], y[r] * y[r]
                has = yr != 0.0                                       # (a rollout with weight has a cost)
                terms = np.stack([yr, np.where(A[e], yr, 0.0), np.where(A[e], y2, 0.0), np.where(A[e], 0.0, y2),
                                  np.where(has, yr * np.where(has, M[e], 0.0), 0.0), np.where(A[e], yr * tau[e], 0.0)], axis=1)
                S[r, e] = em.ordered_sum(terms)
        mmax = np.array([np.nanmax(M[e][ok]) if ok.any() and not np.isnan(M[e][ok]).all() else -np.inf for e in range(E1)])
    nviol = A.sum(axis=1).astype(np.float64)
    out = em._assemble(S, mmax[None, :], nviol[None, :], dead)
    n_ok = float(ok.sum())
    with np.errstate(all="ignore"):
        rob = (nviol[None, :] / n_ok) / (rows["tail_n"][:, None] / n_ok)
        rob = np.where(rob < 1.0, rob, 1.0)
        out["prob_robust"] = np.where(rob < out["prob"], out["prob"], rob)   # (never below PROB: the last bit of two roundings of one number)
    out["prob_robust"][dead] = np.nan
    step = np.zeros((R, E1, viol.shape[1]))
    for r in range(R):
        s = em.ordered_sum(np.where(viol, y[r][:, None, None], 0.0))              # [N+1, E+1]
        with np.errstate(all="ignore"):
            step[r] = (s / S[r, :, 0][None, :]).T
    step[dead] = np.nan
    out.update({k: rows[k] for k in tr.SLOTS})
    out.update(step=step, margins=M, tau=tau, y=y, event_flag=np.repeat(np.asarray(rows["flag"])[:, None], E1, axis=1))
    return out


def tail_events(x, u, costs, alphas, evs):
    """`reduce` for quadratic events (Q or None, a, b, t_lo, t_hi) on the trajectories x [K, N+1, n], u [K, N, m]"""
    return reduce(em.g_device(x, u, evs), evs, costs, alphas)


def deviation(got, ref, sc, N):
    """events_model.deviation with prob_robust among the probabilities"""
    dp, dm = em.deviation(got, ref, sc, N)
    a, b = np.asarray(got["prob_robust"], float), np.asarray(ref["prob_robust"], float)
    assert np.array_equal(np.isnan(a), np.isnan(b)), "prob_robust"
    if np.isfinite(b).any():
        dp = max(dp, float(np.nanmax(np.abs(a - b))))
    return dp, dm
