"""NumPy model of rat_policy_events' kernels (csrc/policy_mc.hip: ev_eval, ev_sums, ev_final) -- test aid.

An event is (Q or None, a, b, t_lo, t_hi) over the d = n + m coordinates of z = (x_t, u_t), as Event.dense returns it.

`events` restates the device's order.  g of a (rollout, step, event) in the 12 + 4 tile: lane kq = 0 .. 3 of the rollout's column holds the
components kq, kq + 4, kq + 8, kq + 12, forms a[c] z[c] over them and, for the quadratic part, (Q z)[c] z[c] with (Q z)[c] summed over
k = 0 .. 15 in order (the four MFMAs); the four lanes are added as (p0 + p1) + (p2 + p3), b last.  The sums: the rollouts in chunks of
2^16; inside a chunk lane tid of slot s adds the rollouts s * 256 + tid, + 2048, ... in order, the 256 lanes combine in the binary LDS
tree, a slot's partial is added chunk after chunk and the eight slots in index order.  Weights come from the rows
(wc_trajectory_model.weights_from_rows); a rollout whose cost is NaN is selected out whatever its trajectory holds.

`direct` is an independent answer in np.longdouble, straight from the definitions, no tile, no grouping."""
import numpy as np

from wc_trajectory_model import tile

CHUNK, SLOTS, THREADS = 1 << 16, 8, 256
SLOT_NAMES = ("prob", "prob_se", "margin_mean", "margin_max", "first_mean", "n_viol")


def between(v, q):
    """a threshold inside the spread of the values v that is none of them: the middle of the two neighbours at the q-quantile (below a
    lone value), so that no rollout sits on the boundary it defines"""
    v = np.unique(np.asarray(v, float)[np.isfinite(v)])
    if v.size < 2:
        return float(v[0] - 0.1 * (abs(v[0]) + 1.0)) if v.size else 0.0
    i = min(int(q * v.size), v.size - 2)
    return float(0.5 * (v[i] + v[i + 1]))


def tile_index(n, m):
    return list(range(n)) + list(range(12, 12 + m))


def ordered_sum(v):
    """sum over axis 0 in the device's order"""
    v = np.asarray(v, dtype=np.float64)
    K, rest = v.shape[0], v.shape[1:]
    part = np.zeros((SLOTS,) + rest)
    for k0 in range(0, K, CHUNK):
        c = v[k0:k0 + CHUNK]
        it = -(-c.shape[0] // (SLOTS * THREADS))
        pad = np.zeros((it * SLOTS * THREADS,) + rest)
        pad[:c.shape[0]] = c
        pad = pad.reshape((it, SLOTS, THREADS) + rest)
        acc = np.zeros((SLOTS, THREADS) + rest)
        for i in range(it):
            acc = acc + pad[i]
        s = THREADS // 2
        while s:
            acc[:, :s] = acc[:, :s] + acc[:, s:2 * s]
            s //= 2
        part = acc[:, 0] if k0 == 0 else part + acc[:, 0]
    tot = part[0]
    for s in range(1, SLOTS):
        tot = tot + part[s]
    return tot


def g_device(x, u, evs):
    """g [K, N+1, E] in the device's order of operations (NaN trajectories give NaN)"""
    x, u = np.asarray(x, float), np.asarray(u, float)
    K, T, n = x.shape
    m = u.shape[2]
    idx = tile_index(n, m)
    z = tile(x, u)
    g = np.zeros((K, T, len(evs)))
    with np.errstate(all="ignore"):
        for e, (Q, a, b, lo, hi) in enumerate(evs):
            at = np.zeros(16)
            at[idx] = a
            p = np.zeros((4, K, T))
            for kq in range(4):
                for r in range(4):
                    p[kq] = p[kq] + at[kq + 4 * r] * z[:, :, kq + 4 * r]
            if Q is not None:
                Qt = np.zeros((16, 16))
                Qt[np.ix_(idx, idx)] = Q
                for kq in range(4):
                    qp = np.zeros((K, T))
                    for r in range(4):
                        c = np.zeros((K, T))
                        for k in range(16):
                            c = c + Qt[kq + 4 * r, k] * z[:, :, k]
                        qp = qp + c * z[:, :, kq + 4 * r]
                    p[kq] = p[kq] + qp
            g[:, :, e] = ((p[0] + p[1]) + (p[2] + p[3])) + b
    return g


def g_direct(x, u, evs):
    """g [K, N+1, E] in np.longdouble from the dense coordinates"""
    x, u = np.asarray(x, float), np.asarray(u, float)
    K, T, n = x.shape
    z = np.zeros((K, T, n + u.shape[2]), dtype=np.longdouble)
    z[:, :, :n] = x
    z[:, :T - 1, n:] = u
    g = np.zeros((K, T, len(evs)), dtype=np.longdouble)
    with np.errstate(all="ignore"):
        for e, (Q, a, b, lo, hi) in enumerate(evs):
            g[:, :, e] = (z * np.asarray(a, dtype=np.longdouble)).sum(axis=2) + np.longdouble(b)
            if Q is not None:
                g[:, :, e] += np.einsum("kti,ij,ktj->kt", z, np.asarray(Q, dtype=np.longdouble), z)
    return g


def per_rollout(g, evs, ok):
    """(M [E+1, K], tau [E+1, K] (-1: none), viol [K, N+1, E+1]) from g; the last event is "any"; rollouts that are not ok: NaN, -1, False"""
    K, T, E = g.shape
    M = np.full((E + 1, K), np.nan, dtype=g.dtype)
    tau = np.full((E + 1, K), -1, dtype=np.int64)
    viol = np.zeros((K, T, E + 1), dtype=bool)
    with np.errstate(all="ignore"):
        for e, (Q, a, b, lo, hi) in enumerate(evs):
            w = g[:, lo:hi + 1, e]
            allnan = np.isnan(w).all(axis=1)
            M[e] = np.where(allnan, np.nan, np.nanmax(np.where(allnan[:, None], 0.0, w), axis=1))
            viol[:, lo:hi + 1, e] = w > 0
    viol[~ok] = False
    viol[:, :, E] = viol[:, :, :E].any(axis=2)
    for e in range(E + 1):
        has = viol[:, :, e].any(axis=1)
        tau[e] = np.where(has, viol[:, :, e].argmax(axis=1), -1)
    with np.errstate(all="ignore"):
        allnan = np.isnan(M[:E]).all(axis=0)
        M[E] = np.where(allnan, np.nan, np.nanmax(np.where(allnan[None], 0.0, M[:E]), axis=0))
    M[:, ~ok] = np.nan
    return M, tau, viol


def _assemble(S, mmax, nviol, dead):
    """slots from the sums S [R, E+1, 6] = sum y, y A, y^2 A, y^2 (1 - A), y M, y A tau"""
    out = {}
    with np.errstate(all="ignore"):
        sy = S[..., 0]
        pr = S[..., 1] / sy
        out["prob"] = pr
        out["prob_se"] = np.sqrt((1 - pr) * (1 - pr) * S[..., 2] + pr * pr * S[..., 3]) / sy
        out["margin_mean"] = S[..., 4] / sy
        out["margin_max"] = np.broadcast_to(mmax, pr.shape).copy()
        out["first_mean"] = S[..., 5] / S[..., 1]
        out["n_viol"] = np.broadcast_to(nviol, pr.shape).astype(np.float64).copy()
    for k in out:
        out[k] = np.asarray(out[k], dtype=np.float64)
        out[k][dead] = np.nan
    return out


def events(x, u, costs, y, dead, evs):
    """the device's answer: dict of SLOT_NAMES [R, E+1], step [R, E+1, N+1], margins [E+1, K], tau [E+1, K]"""
    J = np.asarray(costs, float).ravel()
    ok = ~np.isnan(J)
    M, tau, viol = per_rollout(g_device(x, u, evs), evs, ok)
    y = np.where(ok[None, :], y, 0.0)
    R, E1 = y.shape[0], M.shape[0]
    A = tau >= 0
    S = np.zeros((R, E1, 6))
    for e in range(E1):
        Me = np.where(ok, M[e], 0.0)
        for r in range(R):
            yr, y2 = y[r], y[r] * y[r]
            terms = np.stack([yr, np.where(A[e], yr, 0.0), np.where(A[e], y2, 0.0), np.where(A[e], 0.0, y2), np.where(ok, yr * Me, 0.0),
                              np.where(A[e], yr * tau[e], 0.0)], axis=1)
            S[r, e] = ordered_sum(terms)
    with np.errstate(all="ignore"):
        mmax = np.array([np.nanmax(M[e][ok]) if ok.any() and not np.isnan(M[e][ok]).all() else -np.inf for e in range(E1)])
    out = _assemble(S, mmax[None, :], A.sum(axis=1)[None, :], dead)
    step = np.zeros((R, E1, viol.shape[1]))
    for r in range(R):
        s = ordered_sum(np.where(viol, y[r][:, None, None], 0.0))              # [N+1, E+1]
        with np.errstate(all="ignore"):
            step[r] = (s / S[r, :, 0][None, :]).T
    step[dead] = np.nan
    out.update(step=step, margins=M, tau=tau)
    return out


def direct(x, u, costs, y, dead, evs):
    """the same in np.longdouble: w = y / sum y, every slot from its definition"""
    J = np.asarray(costs, float).ravel()
    ok = ~np.isnan(J)
    M, tau, viol = per_rollout(g_direct(x, u, evs), evs, ok)
    R, E1, T = y.shape[0], M.shape[0], viol.shape[1]
    A = tau >= 0
    out = {k: np.full((R, E1), np.nan) for k in SLOT_NAMES}
    step = np.full((R, E1, T), np.nan)
    with np.errstate(all="ignore"):
        for r in range(R):
            if dead[r]:
                continue
            w = np.where(ok, y[r], 0.0).astype(np.longdouble)
            w = w / w.sum()
            for e in range(E1):
                p = w[A[e]].sum()
                out["prob"][r, e] = p
                out["prob_se"][r, e] = np.sqrt((w * w * (A[e] - p) ** 2).sum())
                out["margin_mean"][r, e] = (w[ok] * M[e][ok]).sum()
                out["margin_max"][r, e] = M[e][ok].max()
                out["first_mean"][r, e] = (w[A[e]] * tau[e][A[e]]).sum() / p if p > 0 else np.nan
                out["n_viol"][r, e] = A[e].sum()
                step[r, e] = (w[:, None] * viol[:, :, e]).sum(axis=0)
    out.update(step=step, margins=M, tau=tau)
    return out


def scales(x, u, costs, evs):
    """|b| + |a| |z| + |Q| |z|^2 per event ("any": the largest), |z| the largest norm of (x_t, u_t) among the rollouts that have a cost"""
    ok = ~np.isnan(np.asarray(costs, float).ravel())
    zn = 0.0
    if ok.any():
        x2 = (np.asarray(x, float)[ok] ** 2).sum(axis=2)
        x2[:, :-1] += (np.asarray(u, float)[ok] ** 2).sum(axis=2)
        zn = float(np.sqrt(x2.max()))
    sc = [abs(b) + np.linalg.norm(a) * zn + (np.linalg.norm(Q, 2) * zn * zn if Q is not None else 0.0) for Q, a, b, lo, hi in evs]
    sc = [max(s, np.finfo(float).tiny) for s in sc]
    return np.array(sc + [max(sc)])


def deviation(got, ref, sc, N):
    """(worst deviation of the probabilities -- prob, prob_se, step, first_mean / N -- and of margin_mean relative to the event's scale);
    NaN must meet NaN"""
    dp = dm = 0.0
    for k, div in (("prob", 1.0), ("prob_se", 1.0), ("step", 1.0), ("first_mean", float(max(N, 1)))):
        a, b = np.asarray(got[k], float), np.asarray(ref[k], float)
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        if np.isfinite(b).any():
            dp = max(dp, float(np.nanmax(np.abs(a - b))) / div)
    a, b = np.asarray(got["margin_mean"], float), np.asarray(ref["margin_mean"], float)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    if np.isfinite(b).any():
        dm = float(np.nanmax(np.abs(a - b) / sc[None, :]))
    return dp, dm
