"""NumPy model of the device reduction of rat_policy_evaluate (csrc/policy_mc.hip) -- test aid.

Same two passes, same exclusions, same order of summation: lane g of the BLOCKS x THREADS grid sums elements g, g + T, g + 2 T, ... in
order, the THREADS lanes of a workgroup combine in a binary tree (lane i takes lane i + s for s = THREADS / 2 .. 1), and the BLOCKS
partials combine in the same tree.  NaN costs (DomainError rollouts) are counted and left out.  The exponentials are shifted by the
maximum (every exponent <= 0) and summed about y_ref = exp(theta (mean - max)), as the kernels do."""
import numpy as np

BLOCKS, THREADS = 256, 256


def _tree(v, op):
    v = np.array(v, dtype=np.float64)
    s = v.size // 2
    while s > 0:
        v[:s] = op(v[:s], v[s:2 * s])
        s //= 2
    return float(v[0])


def _fixed_order(vals, valid, op=np.add, neutral=0.0):
    """vals[k] over the valid k, reduced in the device's order."""
    T = BLOCKS * THREADS
    K = vals.size
    rows = -(-K // T)
    pad = np.full(rows * T, neutral)
    pad[:K] = np.where(valid, vals, neutral)
    lanes = np.full(T, neutral)
    for r in pad.reshape(rows, T):                       # element g + r T belongs to lane g: summed in order of r
        lanes = op(lanes, r)
    blocks = [_tree(b, op) for b in lanes.reshape(BLOCKS, THREADS)]
    return _tree(blocks, op)


def reduce_costs(costs, thetas=()):
    """The dict Context.policy_evaluate returns (without `costs`), from the K costs."""
    J = np.asarray(costs, dtype=np.float64)
    ok = ~np.isnan(J)
    nan = float("nan")
    with np.errstate(all="ignore"):
        n = _fixed_order(np.ones_like(J), ok)
        n_dom = _fixed_order(np.ones_like(J), ~ok)
        th = np.atleast_1d(np.asarray(thetas, dtype=np.float64))
        if n == 0:
            return dict(n_ok=0, n_domain=int(n_dom), mean=nan, var=nan, min=nan, max=nan, se_mean=nan, risk=np.full(th.size, nan),
                        risk_se=np.full(th.size, nan))
        mn = _fixed_order(J, ok, np.minimum, np.inf)
        mx = _fixed_order(J, ok, np.maximum, -np.inf)
        mean = _fixed_order(J, ok) / n
        s2 = _fixed_order((J - mean) ** 2, ok)
        var = s2 / (n - 1) if n >= 2 else nan
        se_mean = np.sqrt(var / n)
        risk, risk_se = np.zeros(th.size), np.zeros(th.size)
        for i, t in enumerate(th):
            if t == 0.0:
                risk[i], risk_se[i] = mean, se_mean
                continue
            yref = np.exp(t * (mean - mx))
            d = np.exp(t * (J - mx)) - yref
            s1, sq = _fixed_order(d, ok), _fixed_order(d * d, ok)
            ybar = yref + s1 / n
            vy = max((sq - s1 * s1 / n) / (n - 1), 0.0) if n >= 2 else nan
            risk[i] = mx + np.log(ybar) / t
            risk_se[i] = np.sqrt(vy) / (ybar * t * np.sqrt(n))
    return dict(n_ok=int(n), n_domain=int(n_dom), mean=mean, var=var, min=mn, max=mx, se_mean=se_mean, risk=risk, risk_se=risk_se)


def direct(costs, thetas=()):
    """The same quantities straight from their definitions in NumPy (what a user computes on the host from K costs today)."""
    J = np.asarray(costs, dtype=np.float64)
    J = J[~np.isnan(J)]
    n = J.size
    th = np.atleast_1d(np.asarray(thetas, dtype=np.float64))
    mean, var, mx = J.mean(), J.var(ddof=1), J.max()
    risk, risk_se = np.zeros(th.size), np.zeros(th.size)
    for i, t in enumerate(th):
        if t == 0.0:
            risk[i], risk_se[i] = mean, np.sqrt(var / n)
            continue
        y = np.exp(t * (J - mx))
        risk[i] = mx + np.log(y.mean()) / t
        risk_se[i] = y.std(ddof=1) / (y.mean() * t * np.sqrt(n))
    return dict(n_ok=n, mean=mean, var=var, min=J.min(), max=mx, se_mean=np.sqrt(var / n), risk=risk, risk_se=risk_se)
