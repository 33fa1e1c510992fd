"""NumPy model of rat_policy_rare_event_noise (csrc/source_rare.h, re_elite_rng of csrc/rare_event.hip) -- test aid: the whole call on the
host, and the source models its tests share.

Keying, restated.  Pass p -- the final pass is p = 0, adaptation iteration j is p = j + 1 -- has seed_p = seed + 0xD1B54A32D192ED03 p
(mod 2^64).  Inside a pass the generator is rat_rng's (csrc/rat_rng.h), rollout g of the K counted globally: the normals of step t come
from the Philox4x32-10 blocks with counter (g lo, g hi, t, q), q = 0 .. ceil(P / 2) - 1, key (seed_p lo, seed_p hi): two 53-bit uniforms,
one Box-Muller transform (csrc/rat_normal.h through oracle/normal_check.c, tests/test_cpu_normal.parts), normal 2 q and normal 2 q + 1;
the uniforms from counter (g lo, g hi, t, 0x80000000 | q): uniform 2 q = u01(r0, r1), uniform 2 q + 1 = u01(r2, r3).  No chunks.

The sampler is a Python function noise(k, x, u, rng, p) on all K rollouts at once (x (K, n), u (K, m); it returns w (K, n)) that draws
from a counting rng: the i-th rng.normal() of a step returns s[t, i] + xi and adds -s z + s^2 / 2 to logw at the draw, in draw order; a
draw beyond the declared count returns NaN and is flagged.  The samplers here draw the same number of values on every rollout.
The elite sums, the level and the estimate are tests/rare_event_model.py's (elite_sum, level, adapt, estimate): the same orders."""
import functools

import numpy as np

import ratilqr.jl_amd as rat
import rare_event_model as rm
from events_model import g_device, per_rollout
from rare_event_model import MASK64, PASS_STRIDE, philox4x32_10
from user_noise_model import (LQ_GAUSS, PEND_DIAG, PEND_DIAG_DIMS, PEND_NAN, PEND_OVER, PEND_PLAIN, PEND_STATE,  # noqa: F401
                              PEND_STATE_DIMS, PEND_STATE_P, pend_c, pend_h)

# ---- tests/test_cpu_rare_event.linear_case() as a source model: p = A (row-major, 4) | B (2) | chol_lower(W) (l00, l10, l11) ----------
LIN_GAUSS = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) {
    xn[0] = p[0] * x[0] + p[1] * x[1] + p[4] * u[0];
    xn[1] = p[2] * x[0] + p[3] * x[1] + p[5] * u[0];
}
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) {
    return 0.5 * (x[0] * x[0] + x[1] * x[1]) + 0.5 * (u[0] * u[0]);
}
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return 0.5 * (x[0] * x[0] + x[1] * x[1]); }
#define RAT_USER_NOISE
template <class R> __device__ void rat_user_noise(int k, const double *x, const double *u, R &rng, double *w, const double *p) {
    const double z0 = rng.normal();
    const double z1 = rng.normal();
    w[0] = p[6] * z0;
    w[1] = p[7] * z0 + p[8] * z1;
}
"""
LIN_GAUSS_DIMS = dict(n=2, m=1, normals_per_step=2, uniforms_per_step=0)


def lin_params(prob):
    C = np.linalg.cholesky(np.asarray(prob.Wtab, float))
    return np.concatenate([np.asarray(prob.A, float).ravel(), np.asarray(prob.B, float).ravel(), [C[0, 0], C[1, 0], C[1, 1]]])


def lin_source_problem(prob):
    return rat.DeviceSourceProblem(LIN_GAUSS, 2, 1, prob.N, np.asarray(prob.Wtab, float), params=lin_params(prob))


def lin_f(x, u, p):
    return np.stack([p[0] * x[:, 0] + p[1] * x[:, 1] + p[4] * u[:, 0], p[2] * x[:, 0] + p[3] * x[:, 1] + p[5] * u[:, 0]], axis=1)


def lin_noise(k, x, u, rng, p):
    z0, z1 = rng.normal(), rng.normal()
    return np.stack([p[6] * z0, p[7] * z0 + p[8] * z1], axis=1)


# ---- the samplers of tests/user_noise_model.py on (K, n) states -----------------------------------------------------------------------
def pend_f(x, u, p):
    return np.stack([x[:, 0] + p[0] * x[:, 1], x[:, 1] + p[0] * (-np.sin(x[:, 0]) - 0.1 * x[:, 1] + u[:, 0])], axis=1)


def pend_state_noise(k, x, u, rng, p):
    z0, z1, z2 = rng.normal(), rng.normal(), rng.normal()
    return np.stack([p[1] * np.abs(x[:, 0]) * z0, p[1] * np.abs(x[:, 1]) * z1 + p[2] * z2], axis=1)


def pend_diag_noise(k, x, u, rng, p):
    return np.stack([p[1] * rng.normal(), p[2] * rng.normal()], axis=1)


def pend_nan_noise(k, x, u, rng, p):
    z = rng.normal()
    with np.errstate(invalid="ignore"):
        return np.stack([np.zeros_like(z), np.where(z > 3.0, np.nan, p[1] * z)], axis=1)


def lq_gauss_model(gp):
    """(f, noise) of LQ_GAUSS for the generative problem gp (tests/user_noise_model.lq_generative)"""
    lq, C = gp.lq, np.asarray(gp.nchol, float)

    def f(x, u, p):
        return x @ lq.A.T + u @ lq.B.T + lq.kappa * x ** 3

    def noise(k, x, u, rng, p):
        z = np.stack([rng.normal() for _ in range(gp.n)], axis=1)
        return z @ np.tril(C).T
    return f, noise


# ---- rat_rng's generator ----------------------------------------------------------------------------------------------------------------
def _u01(hi, lo):
    return (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


@functools.lru_cache(maxsize=8)
def normals(seed, p, K, N, P):
    """xi [K, N, P] of pass p (read-only)"""
    from test_cpu_normal import parts
    seed_p = (int(seed) + PASS_STRIDE * int(p)) & MASK64
    nq = (P + 1) // 2
    g, t, q = np.meshgrid(np.arange(K, dtype=np.uint64), np.arange(N, dtype=np.uint64), np.arange(nq, dtype=np.uint64), indexing="ij")
    r0, r1, r2, r3 = philox4x32_10(g, g >> np.uint64(32), t, q, seed_p & 0xFFFFFFFF, seed_p >> 32)
    u1, u2 = _u01(r0, r1), _u01(r2, r3)
    out = parts(np.ascontiguousarray(u1.ravel()), np.ascontiguousarray(u2.ravel()))
    xi = np.ascontiguousarray(np.stack([out[4].reshape(u1.shape), out[5].reshape(u1.shape)], axis=3).reshape(K, N, 2 * nq)[:, :, :P])
    xi.setflags(write=False)
    return xi


def uniforms(seed, p, K, N, U):
    """the uniforms [K, N, U] of pass p"""
    seed_p = (int(seed) + PASS_STRIDE * int(p)) & MASK64
    nq = (U + 1) // 2
    g, t, q = np.meshgrid(np.arange(K, dtype=np.uint64), np.arange(N, dtype=np.uint64), np.arange(nq, dtype=np.uint64), indexing="ij")
    r0, r1, r2, r3 = philox4x32_10(g, g >> np.uint64(32), t, np.uint64(0x80000000) | q, seed_p & 0xFFFFFFFF, seed_p >> 32)
    return np.stack([_u01(r0, r1), _u01(r2, r3)], axis=3).reshape(K, N, 2 * nq)[:, :, :U]


class ShiftRng:
    """the counting rng of one pass over K rollouts: the shifted normals, logw at the draw, the overdraw flag"""

    def __init__(self, xi, un, s):
        self.xi, self.un, self.s = xi, un, s
        self.logw = np.zeros(xi.shape[0])
        self.over, self.t, self.i, self.iu = 0, 0, 0, 0

    def at(self, t):
        self.t, self.i, self.iu = t, 0, 0

    def normal(self):
        i = self.i
        self.i += 1
        if i >= self.xi.shape[2]:
            self.over |= 1
            return np.full(self.xi.shape[0], np.nan)
        sv = self.s[self.t, i]
        z = sv + self.xi[:, self.t, i]
        self.logw = self.logw + (-sv * z + 0.5 * sv * sv)
        return z

    def uniform(self):
        i = self.iu
        self.iu += 1
        if self.un is None or i >= self.un.shape[2]:
            self.over |= 2
            return np.full(self.xi.shape[0], np.nan)
        return self.un[:, self.t, i]


class Model:
    """A source model on the host: f(x, u, p), noise(k, x, u, rng, p) on (K, .) arrays, optional c(k, x, u, p) and h(x, p) (the
    DomainError rule alone reads them), the parameters, the sizes and the declared draws."""

    def __init__(self, f, noise, p, n, m, N, P, U=0, c=None, h=None):
        self.f, self.noise, self.p, self.n, self.m, self.N, self.P, self.U, self.c, self.h = f, noise, np.asarray(p, float), n, m, N, P, U, c, h


def one_pass(mod, x_nom, l, L, ev, seed, p, K, s):
    """(M [K] -- NaN for a DomainError rollout --, logw [K], dom [K], xi [K, N, P]) of pass p under the shift s [N, P]"""
    n, m, N = mod.n, mod.m, mod.N
    xi = normals(seed, p, K, N, mod.P)
    rng = ShiftRng(xi, uniforms(seed, p, K, N, mod.U) if mod.U else None, s)
    x_nom, l = np.asarray(x_nom, float), np.asarray(l, float)
    x, u, dom = np.zeros((K, N + 1, n)), np.zeros((K, N, m)), np.zeros(K, dtype=bool)
    x[:, 0] = x_nom if L is None else x_nom[0]
    with np.errstate(all="ignore"):
        for t in range(N):
            u[:, t] = l[t] if L is None else l[t] + (x[:, t] - x_nom[t]) @ np.asarray(L[t], float).T
            inok = ~(np.isnan(x[:, t]).any(axis=1) | np.isnan(u[:, t]).any(axis=1))
            rng.at(t)
            w = mod.noise(t, x[:, t], u[:, t], rng, mod.p)
            xn = mod.f(x[:, t], u[:, t], mod.p)
            out = np.isnan(xn).any(axis=1) | np.isnan(w).any(axis=1)
            if mod.c is not None:
                out |= np.isnan(mod.c(t, x[:, t].T, u[:, t].T, mod.p))
            dom |= inok & out
            x[:, t + 1] = xn + w
        if mod.h is not None:
            dom |= ~np.isnan(x[:, N]).any(axis=1) & np.isnan(mod.h(x[:, N].T, mod.p))
    if rng.over:
        raise OverflowError(f"overdraw {rng.over}")
    M = per_rollout(g_device(x, u, [ev]), [ev], ~dom)[0][0]
    return M, rng.logw, dom, xi


def rare_event_noise(mod, x_nom, l, L, event, K, seed=0, shift=None, n_iter=8, rho=0.1):
    """The whole call; rare_event_model.rare_event's dict, with shift [N, P]."""
    ev = event.dense(mod.n, mod.m, mod.N)
    s = np.zeros((mod.N, mod.P)) if shift is None else np.array(shift, dtype=np.float64)
    trace, levels = np.full((n_iter, 4), np.nan), []
    reached, n_run, gamma, bad = False, 0, np.nan, False
    for j in range(n_iter):
        M, logw, dom, xi = one_pass(mod, x_nom, l, L, ev, seed, j + 1, K, s)
        gamma, code, v, k = rm.level(M, rho)
        levels.append((gamma, code, v, k))
        trace[j, 0] = gamma
        n_run += 1
        reached |= code == 1
        bad |= code == 3
        if code != 0:
            break
        s_new, cnt, ess = rm.adapt(M, logw, dom, xi, s, gamma)
        if np.all(np.isfinite(s_new)):
            s = s_new
        else:
            bad = True
        trace[j, 1:] = cnt, ess, np.sqrt((s * s).sum())
    M, logw, dom, _ = one_pass(mod, x_nom, l, L, ev, seed, 0, K, s)
    out = rm.estimate(M, logw, dom)
    flag = rm.OK if reached else rm.NOT_REACHED
    if out["n_ok"] == 0:
        flag = rm.EMPTY
    elif bad or not (np.isfinite(out["logw_max"]) and np.isfinite(out["logw_min"]) and out["prob"] < np.inf):
        flag = rm.NONFINITE
    if flag >= rm.EMPTY:
        out.update(prob=np.nan, prob_se=np.nan, ess=np.nan)
    out.update(flag=flag, n_iter=n_run, level=gamma if n_run else np.nan, shift=s, trace=trace, margins=M, logw=logw, levels=levels)
    return out
