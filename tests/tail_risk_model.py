"""NumPy model of rat_policy_tail_risk (csrc/policy_mc.hip) -- test aid.

`tail_risk` restates the device's schedule: pass 1 (n, min, max), the radix select over the costs' keys -- the bit pattern made monotone,
eight digits of eight bits, the leading digits that the keys of min and max share skipped, per level the walk of the digit's histogram to
the bin where the running count reaches the rank that is left -- then P1 = sum (J - v)^+, P2 = sum ((J - v)^+)^2, c_gt and c_eq in the
fixed order of tests/worst_case_model.py (lane g sums elements g, g + T, ... in order, the binary tree over a workgroup, the same tree
over the workgroups), and the rows.  A histogram is a count: it has no order to restate.

`direct` is an independent answer from the sorted sample: np.sort, the tail written as sum_{i > k} s_i + frac s_k in math.fsum, the tail
distribution's weights laid out element by element and ESS and KL taken from them by their definitions in np.longdouble."""
import math

import numpy as np

from worst_case_model import fixed_order

BITS, PASSES = 8, 8
OK, SATURATED, EMPTY, NONFINITE = 0, 1, 2, 3
SLOTS = ("alpha", "var", "cvar", "cvar_se", "tail_n", "ess", "kl", "flag")
TOP = np.uint64(1) << np.uint64(63)


def key_of(J):
    """ascending key order is ascending value order; -0.0 counts as +0.0"""
    J = np.array(J, dtype=np.float64).ravel()
    J[J == 0.0] = 0.0
    b = J.view(np.uint64)
    return np.where((b >> np.uint64(63)) != 0, ~b, b | TOP)


def value_of(key):
    key = np.uint64(key)
    b = key ^ TOP if (key >> np.uint64(63)) else ~key
    return float(np.array([b], dtype=np.uint64).view(np.float64)[0])


def rank_of(n, alpha):
    """a = n alpha (one rounded product), k = clamp(ceil(a), 1, n)"""
    a = float(np.float64(n) * np.float64(alpha))
    return a, int(min(max(math.ceil(a), 1), n))


def select(keys, ranks, kmin, kmax):
    """the key of rank ranks[l] (1-based) among keys, per level, digit by digit; also the passes that swept the keys"""
    x = int(kmin) ^ int(kmax)
    d0 = PASSES if x == 0 else (64 - x.bit_length()) // BITS
    pfx, left = [0] * len(ranks), [int(r) for r in ranks]
    swept = 0
    for p in range(PASSES):
        sd = 64 - BITS * (p + 1)
        if p < d0:                                          # every key shares this digit
            dg = (int(kmin) >> sd) & 255
            pfx = [(q << BITS) | dg for q in pfx]
            continue
        swept += 1
        digit = ((keys >> np.uint64(sd)) & np.uint64(255)).astype(np.int64)
        hi = keys >> np.uint64(sd + BITS) if p > 0 else np.zeros_like(keys)
        hists = {}
        for l in range(len(ranks)):
            if pfx[l] not in hists:                         # levels that share a prefix share a histogram
                hists[pfx[l]] = np.bincount(digit[hi == np.uint64(pfx[l])], minlength=256)
            cum = np.cumsum(hists[pfx[l]])
            b = int(np.searchsorted(cum, left[l], side="left"))          # the first bin where the running count reaches the rank
            left[l] -= int(cum[b - 1]) if b > 0 else 0
            pfx[l] = (pfx[l] << BITS) | b
    return pfx, swept


def tail_risk(costs, alphas, want_weights=False):
    """What Context.policy_tail_risk returns, from the costs; plus c_gt, c_eq and the sweeps of the select."""
    J = np.asarray(costs, dtype=np.float64).ravel()
    al = np.atleast_1d(np.asarray(alphas, dtype=np.float64))
    ok = ~np.isnan(J)
    nan = float("nan")
    with np.errstate(all="ignore"):
        n = float(fixed_order(np.ones_like(J), ok))
        mn = float(fixed_order(J, ok, np.minimum, np.inf))
        mx = float(fixed_order(J, ok, np.maximum, -np.inf))
    kind = EMPTY if not n > 0 else NONFINITE if not (mn > -np.inf and mx < np.inf) else OK
    out = {k: np.full(al.size, nan) for k in SLOTS}
    out["alpha"] = al.copy()
    out["c_gt"], out["c_eq"] = np.full(al.size, nan), np.full(al.size, nan)
    out["sweeps"] = 0
    w = None
    if kind != OK:
        out["flag"] = np.full(al.size, kind, dtype=np.int64)
        if want_weights:
            w = np.where(ok, nan, 0.0)
        out["weights"] = w
        return out
    keys = key_of(J)[ok]
    ak = [rank_of(n, a) for a in al]
    pfx, out["sweeps"] = select(keys, [k for _, k in ak], key_of([mn])[0], key_of([mx])[0])
    flag = np.zeros(al.size, dtype=np.int64)
    for l, (a, k) in enumerate(ak):
        v = value_of(pfx[l])
        with np.errstate(all="ignore"):
            gt = ok & (J > v)
            d = np.where(gt, J - v, 0.0)
            P1, P2 = float(fixed_order(d, ok)), float(fixed_order(d * d, ok))
            cgt, ceq = float(fixed_order(gt.astype(np.float64), ok)), float(fixed_order((J == v).astype(np.float64), ok))
        tail = n - a
        out["c_gt"][l], out["c_eq"][l], out["tail_n"][l] = cgt, ceq, tail
        if tail < 1.0:
            flag[l] = SATURATED
            out["var"][l] = out["cvar"][l] = v
            out["ess"][l], out["kl"][l] = ceq, math.log(n / ceq)
            w_gt, w_eq = 0.0, 1.0 / ceq
        else:
            frac = k - a
            r = (n - k - cgt) + frac
            wv = r / ceq
            s2 = max(P2 - P1 * P1 / n, 0.0)
            out["var"][l], out["cvar"][l] = v, v + P1 / tail
            out["cvar_se"][l] = math.sqrt(n * s2 / (n - 1.0)) / tail if n >= 2 else nan
            out["ess"][l] = tail * tail / (cgt + ceq * wv * wv)
            out["kl"][l] = (cgt * math.log(n / tail) + (r * math.log(n * wv / tail) if r > 0.0 else 0.0)) / tail
            w_gt, w_eq = 1.0 / tail, wv / tail
        if l == 0 and want_weights:
            with np.errstate(all="ignore"):
                w = np.where(ok & (J > v), w_gt, np.where(ok & (J == v), w_eq, 0.0))
    out["flag"] = flag
    out["weights"] = w
    return out


# ---- the independent answer ----------------------------------------------------------------------------------------------------------
def direct(costs, alpha):
    """var, cvar, cvar_se, tail_n, ess, kl, flag, c_gt, c_eq, k and the weights (aligned with costs) for one level, from the sorted sample."""
    J = np.asarray(costs, dtype=np.float64).ravel()
    ok = ~np.isnan(J)
    s = np.sort(J[ok])
    nan = float("nan")
    dead = dict(var=nan, cvar=nan, cvar_se=nan, tail_n=nan, ess=nan, kl=nan, c_gt=nan, c_eq=nan, k=0, weights=np.where(ok, nan, 0.0))
    if s.size == 0:
        return dict(dead, flag=EMPTY)
    if not np.all(np.isfinite(s)):
        return dict(dead, flag=NONFINITE)
    n = s.size
    a, k = rank_of(n, alpha)
    v = float(s[k - 1]) + 0.0                               # (-0.0 counts as +0.0)
    c_eq = int(np.searchsorted(s, v, side="right") - np.searchsorted(s, v, side="left"))
    c_gt = int(n - np.searchsorted(s, v, side="right"))
    tail = n - a
    L = np.longdouble
    if tail < 1.0:
        nmax = int((s == s[-1]).sum())
        return dict(var=float(s[-1]) + 0.0, cvar=float(s[-1]) + 0.0, cvar_se=nan, tail_n=tail, ess=float(nmax), kl=math.log(n / nmax), flag=SATURATED,
                    c_gt=0, c_eq=nmax, k=k, weights=np.where(ok & (J == s[-1]), 1.0 / nmax, 0.0))
    frac = L(k) - L(a)
    cvar = (L(math.fsum(s[k:])) + frac * L(s[k - 1])) / (L(n) - L(a))    # sum_{i > k} s_i + frac s_k
    x = np.maximum(s.astype(L) - L(v), L(0.0))
    se = float(np.sqrt(((x - x.mean()) ** 2).sum() / L(n - 1) * L(n)) / (L(n) - L(a))) if n >= 2 else nan
    # the tail distribution element by element: mass 1 above v, and what is left of n - a spread evenly over the ties at v
    ws = np.where(s > v, L(1.0), L(0.0))
    at = s == v
    ws[at] = ((L(n) - L(a)) - L(c_gt)) / L(c_eq)
    W = ws.sum()
    pos = ws > 0
    kl = float((ws[pos] / W * np.log(L(n) * ws[pos] / W)).sum())
    ess = float(W * W / (ws * ws).sum())
    with np.errstate(all="ignore"):
        w = np.where(ok & (J > v), 1.0, np.where(ok & (J == v), float(ws[at][0]), 0.0)) / float(W)
    return dict(var=v, cvar=float(cvar), cvar_se=se, tail_n=tail, ess=ess, kl=kl, flag=OK, c_gt=c_gt, c_eq=c_eq, k=k, weights=w)
