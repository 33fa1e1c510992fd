"""NumPy model of rat_policy_worst_case (csrc/policy_mc.hip) -- test aid.

`worst_case` restates the device's schedule and summation order: pass 1 and the variance pass, twelve search passes of 16 thetas per
bound (the geometric grid theta_0 4^(j - 7) around theta_0 = sqrt(2 d) / sd(J), then eleven 17-sections), the final sums at theta* = the
middle of the last bracket, the rows.  Every sum runs in the order of tests/policy_mc_model.py (lane g sums elements g, g + T, ... in
order, the binary tree over a workgroup, the same tree over the workgroups), centred the way the kernels centre it: about the mean with
y_ref = exp(theta (mean - Jmax)) and y - y_ref = y_ref expm1(theta (J - mean)) while theta (Jmax - mean) <= 32, about Jmax with
y_ref = 0 beyond.

`direct` is an independent answer: np.longdouble, plain sums, a bisection of KL(theta) = d to 1e-15 relative, no 16-section search."""
import numpy as np

from policy_mc_model import BLOCKS, THREADS

NPT, GEO_BELOW, LINEAR_PASSES, CENTRE_MAX, THETA_CAP = 16, 7, 11, 32.0, 1e300
PASSES = 1 + LINEAR_PASSES
OK, SATURATED, EMPTY, NONFINITE = 0, 1, 2, 3
SLOTS = ("theta", "kl", "bound", "bound_se", "tilt_mean", "tilt_var", "ess", "flag")


def _tree(v, op):
    """the binary tree over the last axis (lane i takes lane i + s, s = size / 2 .. 1)"""
    v = np.array(v, dtype=np.float64)
    s = v.shape[-1] // 2
    while s > 0:
        v[..., :s] = op(v[..., :s], v[..., s:2 * s])
        s //= 2
    return v[..., 0]


def fixed_order(vals, valid, op=np.add, neutral=0.0):
    """vals[..., k] over the valid k, reduced along the last axis in the device's order (any number of leading axes at once)."""
    vals = np.asarray(vals, dtype=np.float64)
    T = BLOCKS * THREADS
    K = vals.shape[-1]
    rows = -(-K // T)
    pad = np.full(vals.shape[:-1] + (rows * T,), neutral)
    pad[..., :K] = np.where(valid, vals, neutral)
    pad = pad.reshape(vals.shape[:-1] + (rows, T))
    lanes = np.full(vals.shape[:-1] + (T,), neutral)
    for r in range(rows):                                  # element g + r T belongs to lane g: summed in order of r
        lanes = op(lanes, pad[..., r, :])
    blocks = _tree(lanes.reshape(vals.shape[:-1] + (BLOCKS, THREADS)), op)
    return _tree(blocks, op)


class _Head:
    def __init__(self, costs):
        J = np.asarray(costs, dtype=np.float64).ravel()
        self.J, self.ok = J, ~np.isnan(J)
        with np.errstate(all="ignore"):
            self.n = float(fixed_order(np.ones_like(J), self.ok))
            self.mn = float(fixed_order(J, self.ok, np.minimum, np.inf))
            self.mx = float(fixed_order(J, self.ok, np.maximum, -np.inf))
            self.mean = float(fixed_order(J, self.ok)) / self.n if self.n > 0 else float("nan")
            self.s2 = float(fixed_order((J - self.mean) ** 2, self.ok))
            self.nmax = float(fixed_order((J == self.mx).astype(np.float64), self.ok))
            self.sd = float(np.sqrt(self.s2 / self.n)) if self.n > 0 else float("nan")
            self.klmax = float(np.log(self.n / self.nmax)) if self.n > 0 else float("nan")
        self.kind = EMPTY if not self.n > 0 else NONFINITE if not (self.mn > -np.inf and self.mx < np.inf) else OK

    def yref(self, th):
        """per theta: exp(theta (mean - Jmax)) where the sums are centred about the mean, 0 where about Jmax"""
        th = np.asarray(th, dtype=np.float64)
        with np.errstate(all="ignore"):
            return np.where(th * (self.mx - self.mean) <= CENTRE_MAX, np.exp(th * (self.mean - self.mx)), 0.0)

    def sums(self, th, squares=False):
        """A = sum (y - y_ref), B = sum y (J - c) [, A2 = sum (y - y_ref)^2, B2 = sum y (J - c)^2, B2x = sum y (J - Jmax)^2] per theta, in the device's order"""
        th = np.atleast_1d(np.asarray(th, dtype=np.float64))
        yr = self.yref(th)
        with np.errstate(all="ignore"):
            dm, dx = self.J - self.mean, self.J - self.mx
            cen = (yr != 0.0)[:, None]
            c = np.where(cen, dm[None, :], dx[None, :])
            e = np.where(cen, np.expm1(th[:, None] * dm[None, :]), np.exp(th[:, None] * dx[None, :]))
            dd = np.where(cen, yr[:, None] * e, e)              # y - y_ref: y_ref expm1(theta (J - mean)) where centred
            yc = np.where(cen, yr[:, None] + dd, e) * c
            A, B = fixed_order(dd, self.ok), fixed_order(yc, self.ok)
            if not squares:
                return yr, A, B
            y = np.where(cen, yr[:, None] + dd, e)
            return yr, A, B, fixed_order(dd * dd, self.ok), fixed_order(yc * c, self.ok), fixed_order(y * dx[None, :] * dx[None, :], self.ok)

    def kl(self, th, yr, A, B):
        with np.errstate(all="ignore"):
            sumy = np.where(yr != 0.0, self.n * yr + A, A)
            lz = np.where(yr != 0.0, np.log1p(A / (self.n * np.where(yr != 0.0, yr, 1.0))), np.log(np.abs(A) / self.n))
            return th * (B / sumy) - lz, sumy, lz


def _grid(p, lo, hi, theta0):
    j = np.arange(NPT)
    with np.errstate(all="ignore"):
        t = theta0 * 2.0 ** (2 * (j - GEO_BELOW)) if p == 0 else lo + (hi - lo) * ((j + 1) / (NPT + 1.0))
    return np.minimum(t, THETA_CAP)


def _search(h, d):
    """(theta*, state) of one bound: state OK (searched), 'zero', or SATURATED"""
    if h.kind != OK:
        return 0.0, h.kind
    if d == 0.0:
        return 0.0, "zero"
    if d >= h.klmax:
        return 0.0, SATURATED
    with np.errstate(all="ignore"):
        theta0 = float(np.sqrt(2.0 * d) / h.sd)
    if not (0.0 < theta0 < np.inf):
        return 0.0, SATURATED
    lo = hi = 0.0
    for p in range(PASSES):
        g = _grid(p, lo, hi, theta0)
        yr, A, B = h.sums(g)
        kl = h.kl(g, yr, A, B)[0]
        hit = np.nonzero(kl >= d)[0]
        if hit.size:
            j = int(hit[0])
            lo, hi = (float(g[j - 1]) if j > 0 else lo), float(g[j])
        elif p == 0:
            return 0.0, SATURATED                           # KL(theta_top) < d
        else:
            lo = float(g[-1])
    return 0.5 * (lo + hi), OK


def _row(h, th, state, d):
    nan = float("nan")
    if state in (EMPTY, NONFINITE):
        return [nan] * 7 + [float(state)], nan
    n = h.n
    if state == "zero":
        se = float(np.sqrt(h.s2 / (n - 1.0) / n)) if n >= 2 else nan
        return [0.0, 0.0, h.mean, se, h.mean, h.s2 / n, n, 0.0], n
    if state == SATURATED:
        return [float("inf"), h.klmax, h.mx, nan, h.mx, 0.0, h.nmax, 1.0], nan
    yr, A, B, A2, B2, B2x = (float(v[0]) for v in h.sums([th], squares=True))
    kl, sumy, lz = (float(v) for v in h.kl(th, np.float64(yr), np.float64(A), np.float64(B)))
    c = h.mean if yr != 0.0 else h.mx
    mc = B / sumy
    dd = kl if d is None else d
    with np.errstate(all="ignore"):
        mx = mc + (h.mean - h.mx) if yr != 0.0 else mc         # m - Jmax: the variance is taken about the nearer centre
        tvar = max(B2 / sumy - mc * mc if abs(mc) <= abs(mx) else B2x / sumy - mx * mx, 0.0)
        vy = max((A2 - A * A / n) / (n - 1.0), 0.0) if n >= 2 else nan
        se = float(np.sqrt(vy) / ((sumy / n) * th * np.sqrt(n)))
        ess = sumy * sumy / (A2 + 2.0 * yr * A + n * yr * yr)
    return [th, kl, c + (lz + dd) / th, se, c + mc, tvar, ess, 0.0], sumy


def worst_case(costs, kl_bounds=(), thetas=(), want_weights=False):
    """What Context.policy_worst_case returns, from the costs."""
    h = _Head(costs)
    rows_b, rows_t, first = [], [], None
    for d in np.atleast_1d(np.asarray(kl_bounds, dtype=np.float64)):
        th, st = _search(h, float(d))
        r, sumy = _row(h, th, st, float(d))
        rows_b.append(r)
        first = first or (th, st, sumy)
    for t in np.atleast_1d(np.asarray(thetas, dtype=np.float64)):
        st = h.kind if h.kind != OK else ("zero" if t == 0.0 else OK)
        r, sumy = _row(h, float(t), st, None)
        rows_t.append(r)
        first = first or (float(t), st, sumy)

    def pack(rows):
        o = np.array(rows, dtype=np.float64).reshape(len(rows), 8)
        r = {k: o[:, i].copy() for i, k in enumerate(SLOTS)}
        r["flag"] = r["flag"].astype(np.int64)
        return r
    w = None
    if want_weights:
        th, st, sumy = first
        with np.errstate(all="ignore"):
            if st == SATURATED:
                w = np.where(h.J == h.mx, 1.0 / h.nmax, 0.0)
            elif st in (EMPTY, NONFINITE):
                w = np.full(h.J.size, np.nan)
            else:
                w = np.exp(th * (h.J - h.mx)) / sumy
        w = np.where(h.ok, w, 0.0)
    return dict(bounds=pack(rows_b), thetas=pack(rows_t), weights=w)


# ---- the independent answer ----------------------------------------------------------------------------------------------------------
def _tilt(J, th):
    """(KL, m, log Z + theta Jmax ... ) in longdouble at one theta: returns KL, m, bound - d / theta, tilted variance, ESS"""
    mx = J.max()
    y = np.exp(th * (J - mx))
    sy = y.sum()
    m = (y * J).sum() / sy
    logz = np.log(sy / J.size)
    kl = th * (m - mx) - logz
    return kl, m, mx + logz / th, (y * (J - m) ** 2).sum() / sy, sy * sy / (y * y).sum()


def kl_of(costs, th):
    """KL(theta) of the sample, longdouble, straight from the definition"""
    J = np.asarray(costs, dtype=np.float64)
    J = J[~np.isnan(J)].astype(np.longdouble)
    return float(_tilt(J, np.longdouble(th))[0]) if th > 0 else 0.0


def direct(costs, d):
    """theta*, KL, bound, tilted mean / variance, ESS and flag for one radius d, by bisection in np.longdouble."""
    J = np.asarray(costs, dtype=np.float64)
    J = J[~np.isnan(J)]
    nan = float("nan")
    if J.size == 0:
        return dict(theta=nan, kl=nan, bound=nan, tilt_mean=nan, tilt_var=nan, ess=nan, flag=EMPTY)
    if not np.all(np.isfinite(J)):
        return dict(theta=nan, kl=nan, bound=nan, tilt_mean=nan, tilt_var=nan, ess=nan, flag=NONFINITE)
    n, nmax = J.size, int((J == J.max()).sum())
    if d == 0.0:
        return dict(theta=0.0, kl=0.0, bound=float(J.mean()), tilt_mean=float(J.mean()), tilt_var=float(J.var()), ess=float(n), flag=OK)
    sat = dict(theta=float("inf"), kl=float(np.log(n / nmax)), bound=float(J.max()), tilt_mean=float(J.max()), tilt_var=0.0, ess=float(nmax),
               flag=SATURATED)
    if d >= np.log(n / nmax):
        return sat
    Jl, dl = J.astype(np.longdouble), np.longdouble(d)
    lo, hi = np.longdouble(0.0), np.longdouble(1.0) / np.longdouble(J.std())
    for _ in range(4000):                                   # grow until KL(hi) >= d
        if _tilt(Jl, hi)[0] >= dl:
            break
        lo, hi = hi, hi * 2
    else:
        return sat
    while hi - lo > np.longdouble(1e-15) * hi:
        mid = (lo + hi) / 2
        if mid == lo or mid == hi:
            break
        if _tilt(Jl, mid)[0] >= dl:
            hi = mid
        else:
            lo = mid
    th = (lo + hi) / 2
    kl, m, risk, tv, ess = _tilt(Jl, th)
    return dict(theta=float(th), kl=float(kl), bound=float(risk + dl / th), tilt_mean=float(m), tilt_var=float(tv), ess=float(ess), flag=OK)
