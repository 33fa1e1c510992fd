"""NumPy model of rat_policy_rare_event (csrc/rare_event.hip, csrc/rare_event.h) -- test aid: the whole call on the host.

Keying, restated.  Pass p -- the final pass is p = 0, adaptation iteration j is p = j + 1 -- has seed_p = seed + 0xD1B54A32D192ED03 p
(mod 2^64).  Inside a pass the K rollouts are cut into chunks of min(K, 2^16); chunk c draws under the Philox4x32-10 key
seed_p + 0x9E3779B97F4A7C15 c (low word, high word), rollout k of the chunk with the counter (k, 0, t >> 1, component): the block's four
words give two 53-bit uniforms, one Box-Muller transform (csrc/rat_normal.h through oracle/normal_check.c) and from it the normals of
steps 2 (t >> 1) and 2 (t >> 1) + 1.  That is rat_policy_evaluate's keying at the seed seed_p.

Order, restated.  logw of a rollout: lane kq = 0 .. 3 adds -s z + s^2 / 2 over the steps in order and, within a step, over its components
kq, kq + 4, kq + 8; the four lanes are added as (l0 + l1) + (l2 + l3).  The elite sums: lane tid of slot s takes the rollouts s * 256 + tid,
+ 64 * 256, ... in order, the 256 lanes combine in the binary tree (lane i takes lane i + h, h = 128 .. 1), the 64 slots are added in index
order.  The final sums and the extremes: policy_mc_model._fixed_order.  g of a step: events_model.g_device.

The rollout itself is plain NumPy (matrix products, not the device's chains of fused multiply-adds): states agree to rounding, not bit for
bit.  DomainError of the power-law family: a negative state or control under a fractional exponent (every exponent of the family's test
problems is fractional)."""
import functools

import numpy as np

from events_model import g_device, per_rollout
from policy_mc_model import _fixed_order

PASS_STRIDE, CHUNK_STRIDE, MASK64 = 0xD1B54A32D192ED03, 0x9E3779B97F4A7C15, (1 << 64) - 1
CHUNK, SLOTS, THREADS = 1 << 16, 64, 256
OK, NOT_REACHED, EMPTY, NONFINITE = 0, 1, 2, 3


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of 32-bit words held in uint64 (csrc/rat_philox.h); the key may be an array too"""
    M = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(v, np.uint64) & M for v in (c0, c1, c2, c3))
    k0, k1 = np.asarray(k0, np.uint64) & M, np.asarray(k1, np.uint64) & M
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return c0, c1, c2, c3


@functools.lru_cache(maxsize=8)
def normals(seed, p, K, N, n):
    """xi [K, N, n] of pass p (read-only: a pass drawn again -- under another shift -- is served from the cache)"""
    from test_cpu_normal import parts
    seed_p = (int(seed) + PASS_STRIDE * int(p)) & MASK64
    chunk = min(K, CHUNK)
    i = np.arange(K)
    ci, k = i // chunk, i % chunk
    keys = np.array([(seed_p + CHUNK_STRIDE * int(c)) & MASK64 for c in range(int(ci.max()) + 1)], dtype=np.uint64)[ci]
    P2 = (N + 1) // 2
    kk, tp, c = np.meshgrid(k, np.arange(P2), np.arange(n), indexing="ij")
    key = np.broadcast_to(keys[:, None, None], kk.shape)
    r0, r1, r2, r3 = philox4x32_10(kk, 0 * kk, tp, c, key & np.uint64(0xFFFFFFFF), key >> np.uint64(32))
    u1 = (((r0 << np.uint64(32)) | r1) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    u2 = (((r2 << np.uint64(32)) | r3) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    out = parts(np.ascontiguousarray(u1.ravel()), np.ascontiguousarray(u2.ravel()))
    z0, z1 = out[4].reshape(u1.shape), out[5].reshape(u1.shape)
    xi = np.ascontiguousarray(np.stack([z0, z1], axis=2).reshape(K, 2 * P2, n)[:, :N])
    xi.setflags(write=False)
    return xi


def chol_factors(prob):
    W = np.asarray(prob.Wtab, dtype=np.float64)
    W = W if W.ndim == 3 else np.broadcast_to(W, (prob.N,) + W.shape)
    return np.stack([np.linalg.cholesky(W[t]) for t in range(prob.N)])


def rollout(prob, x_nom, l, L, z):
    """x [K, N+1, n], u [K, N, m], dom [K] of x' = f(x, u) + chol(W(t)) z_t under u = l + L (x - x_nom) (L None: open loop)"""
    K, N, n = z.shape
    m = prob.m
    C = chol_factors(prob)
    x_nom, l = np.asarray(x_nom, float), np.asarray(l, float)
    lq = hasattr(prob, "A")
    x, u, dom = np.zeros((K, N + 1, n)), np.zeros((K, N, m)), np.zeros(K, dtype=bool)
    x[:, 0] = x_nom if L is None else x_nom[0]
    with np.errstate(all="ignore"):
        for t in range(N):
            u[:, t] = l[t] if L is None else l[t] + (x[:, t] - x_nom[t]) @ np.asarray(L[t], float).T
            if lq:
                f = x[:, t] @ prob.A.T + u[:, t] @ prob.B.T + prob.kappa * x[:, t] ** 3
            else:
                dom |= (x[:, t] < 0).any(axis=1) | (u[:, t] < 0).any(axis=1)
                f = x[:, t] ** prob.a + u[:, t] ** prob.b
            x[:, t + 1] = f + z[:, t] @ C[t].T
    return x, u, dom


def logw_device(s, z):
    """logw [K] in the device's order; s [N, n], z [K, N, n] the shifted draws"""
    K, N, n = z.shape
    lane = np.zeros((4, K))
    for t in range(N):
        for kq in range(4):
            for c in range(kq, n, 4):
                lane[kq] = lane[kq] + (-s[t, c] * z[:, t, c] + 0.5 * s[t, c] * s[t, c])
    return (lane[0] + lane[1]) + (lane[2] + lane[3])


def elite_sum(v):
    """sum over axis 0 (the rollouts) in re_elite's order"""
    v = np.asarray(v, dtype=np.float64)
    K, rest = v.shape[0], v.shape[1:]
    it = -(-K // (SLOTS * THREADS))
    pad = np.zeros((it * SLOTS * THREADS,) + rest)
    pad[:K] = v
    pad = pad.reshape((it, SLOTS, THREADS) + rest)
    acc = np.zeros((SLOTS, THREADS) + rest)
    for i in range(it):
        acc = acc + pad[i]
    h = THREADS // 2
    while h:
        acc[:, :h] = acc[:, :h] + acc[:, h:2 * h]
        h //= 2
    tot = np.zeros(rest)
    for sl in range(SLOTS):
        tot = tot + acc[sl, 0]
    return tot


def one_pass(prob, x_nom, l, L, ev, seed, p, K, s):
    """(M [K] -- NaN for a DomainError rollout --, logw [K], dom [K], xi [K, N, n]) of pass p under the shift s"""
    xi = normals(seed, p, K, prob.N, prob.n)
    z = xi + s[None]
    x, u, dom = rollout(prob, x_nom, l, L, z)
    M = per_rollout(g_device(x, u, [ev]), [ev], ~dom)[0][0]
    return M, logw_device(s, z), dom, xi


def level(M, rho):
    """(gamma, code, the sorted margins, the rank): code 0 go on, 1 gamma == 0, 2 nothing to rank, 3 not finite"""
    v = np.sort(M[~np.isnan(M)])
    if v.size == 0:
        return np.nan, 2, v, 0
    if not np.all(np.isfinite(v)):
        return np.nan, 3, v, 0
    k = int(min(max(np.ceil(v.size * (1.0 - rho)), 1), v.size))
    val = v[k - 1]
    return (0.0, 1, v, k) if val >= 0 else (float(val), 0, v, k)


def adapt(M, logw, dom, xi, s, gamma):
    """(the new shift, elite count, elite effective sample size): s + sum_E w xi / sum_E w"""
    with np.errstate(invalid="ignore"):
        E = M >= gamma
    lmax = _fixed_order(logw, ~dom, np.maximum, -np.inf)
    w = np.where(E, np.exp(logw - lmax), 0.0)
    W, W2 = elite_sum(w), elite_sum(w * w)
    S = elite_sum(w[:, None, None] * np.where(E[:, None, None], xi, 0.0))
    return s + S / W, int(E.sum()), W * W / W2


def estimate(M, logw, dom):
    """the final pass's slots from its margins, log-weights and flags (without flag, n_iter, level)"""
    nan = float("nan")
    ok = ~dom
    n = _fixed_order(np.ones(M.size), ok)
    n_dom = _fixed_order(np.ones(M.size), dom)
    if n == 0:
        return dict(prob=nan, prob_se=nan, ess=nan, n_viol=0, n_ok=0, n_domain=int(n_dom), logw_max=nan, logw_min=nan)
    lmax, lmin = _fixed_order(logw, ok, np.maximum, -np.inf), _fixed_order(logw, ok, np.minimum, np.inf)
    with np.errstate(invalid="ignore"):
        A = M > 0
    wt = np.exp(logw - lmax)
    S1, S2, nv = _fixed_order(wt, A), _fixed_order(wt * wt, A), _fixed_order(np.ones(M.size), A)
    e = np.exp(lmax)
    with np.errstate(all="ignore"):
        se = e * np.sqrt(max(S2 - S1 * S1 / n, 0.0) / (n - 1) / n) if n >= 2 else nan
    return dict(prob=e * S1 / n, prob_se=se, ess=S1 * S1 / S2 if nv > 0 else 0.0, n_viol=int(nv), n_ok=int(n), n_domain=int(n_dom),
                logw_max=lmax, logw_min=lmin)


def rare_event(prob, x_nom, l, L, event, K, seed=0, shift=None, n_iter=8, rho=0.1):
    """The whole call.  event: an Event of the package.  Returns the slots as a dict, with shift [N, n], trace [n_iter, 4], margins, logw
    (the final pass) and `levels`: per iteration that ran (gamma, code, sorted margins, rank) for the callers' separation checks."""
    n, m, N = prob.n, prob.m, prob.N
    ev = event.dense(n, m, N)
    s = np.zeros((N, n)) if shift is None else np.array(shift, dtype=np.float64)
    trace, levels = np.full((n_iter, 4), np.nan), []
    reached, n_run, gamma, bad = False, 0, np.nan, False
    for j in range(n_iter):
        M, logw, dom, xi = one_pass(prob, x_nom, l, L, ev, seed, j + 1, K, s)
        gamma, code, v, k = level(M, rho)
        levels.append((gamma, code, v, k))
        trace[j, 0] = gamma
        n_run += 1
        reached |= code == 1
        bad |= code == 3
        if code != 0:
            break
        s_new, cnt, ess = adapt(M, logw, dom, xi, s, gamma)
        if np.all(np.isfinite(s_new)):
            s = s_new
        else:
            bad = True
        trace[j, 1:] = cnt, ess, np.sqrt((s * s).sum())
    M, logw, dom, _ = one_pass(prob, x_nom, l, L, ev, seed, 0, K, s)
    out = estimate(M, logw, dom)
    flag = OK if reached else NOT_REACHED
    if out["n_ok"] == 0:
        flag = EMPTY
    elif bad or not (np.isfinite(out["logw_max"]) and np.isfinite(out["logw_min"]) and out["prob"] < np.inf):
        flag = NONFINITE
    if flag >= EMPTY:
        out.update(prob=np.nan, prob_se=np.nan, ess=np.nan)
    out.update(flag=flag, n_iter=n_run, level=gamma if n_run else np.nan, shift=s, trace=trace, margins=M, logw=logw, levels=levels)
    return out


def linear_gaussian_event(prob, x_nom, l, L, a, t):
    """(mu, sigma) of a' (x_t, u_t) for an LQ problem with kappa = 0 under the affine policy: the host mean and covariance recursion"""
    n, m, N = prob.n, prob.m, prob.N
    W = np.asarray(prob.Wtab, float)
    W = W if W.ndim == 3 else np.broadcast_to(W, (N,) + W.shape)
    x_nom, l = np.asarray(x_nom, float), np.asarray(l, float)
    mu, S = (x_nom[0] if L is not None else x_nom).astype(float), np.zeros((n, n))
    for k in range(t + 1):
        Lk = np.asarray(L[k], float) if (L is not None and k < N) else np.zeros((m, n))
        uk = (l[k] + (Lk @ (mu - x_nom[k]) if L is not None else 0.0)) if k < N else np.zeros(m)
        if k == t:
            c = a[:n] + (Lk.T @ a[n:] if k < N else 0.0)
            return float(a[:n] @ mu + a[n:] @ uk), float(np.sqrt(c @ S @ c))
        Acl = prob.A + prob.B @ Lk
        mu, S = prob.A @ mu + prob.B @ uk, Acl @ S @ Acl.T + W[k]
