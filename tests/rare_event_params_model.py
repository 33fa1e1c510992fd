"""NumPy model of rat_policy_rare_event_params (csrc/source_rare.h and csrc/source_params.h under RAT_PARAM_SHIFT, re_elite_rng and
re_update of csrc/rare_event.hip) -- test aid: the whole call on the host.  It is tests/rare_event_noise_model.py with a parameter vector
per rollout, drawn in front of step 0 by a Python restatement of the source's rat_user_params from the parameter stream of
tests/user_params_model.gen_draws -- here with the Box-Muller parts of the device (tests/test_cpu_normal.parts), as
rare_event_noise_model.normals takes them.

Keying, restated.  Pass p has seed_p = seed + 0xD1B54A32D192ED03 p (mod 2^64), the final pass is p = 0.  The i-th parameter normal of
rollout g comes from the Philox4x32-10 block with counter (g lo, g hi, 0xFFFFFFFF, i / 2), key seed_p; the i-th parameter uniform from
counter (g lo, g hi, 0xFFFFFFFF, 0x80000000 | i / 2).  The step draws keep rare_event_noise_model's counters.

The hook is a Python function hook(rng, p) on all K rollouts at once that returns q (K, n_params): the i-th rng.normal() returns
ps[i] + xi and adds -ps[i] z + ps[i]^2 / 2 to the rollout's logw at the draw; the step draws then add their terms to that sum in draw
order, so logw is the whole ratio.  f, the sampler and the event read the rollout's own parameters as P = q.T: P[i] is (K,), which the
(K, n) functions of rare_event_noise_model broadcast as they broadcast a scalar.

The event is an Event of the package (n_event == 0: events_model.g_device, as rare_event_noise_model.one_pass) or a Python function
uev(k, x, u, P) -> g (K,) or None (n_event > 0: rat_user_event's entry, None where the function leaves it alone; u is 0 at k == N).

The update of an iteration: both parts over the same elite with the same weights (rare_event_model.elite_sum's order), a part whose bit
of `adapt` is clear stays where it is, and one entry that is not finite in either moving part drops both."""
import functools

import numpy as np

import rare_event_model as rm
import rare_event_noise_model as nm
import user_noise_model as um
import user_params_model as pm
from events_model import g_device, per_rollout
from policy_mc_model import _fixed_order
from rare_event_model import MASK64, PASS_STRIDE, philox4x32_10

ADAPT = {"step": 1, "params": 2, "both": 3}


# ---- the parameter stream ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=16)
def param_normals(seed, p, K, PN):
    """xi^p [K, PN] of pass p (read-only)"""
    from test_cpu_normal import parts
    seed_p = (int(seed) + PASS_STRIDE * int(p)) & MASK64
    nq = (PN + 1) // 2
    g, q = np.meshgrid(np.arange(K, dtype=np.uint64), np.arange(nq, dtype=np.uint64), indexing="ij")
    r0, r1, r2, r3 = philox4x32_10(g, g >> np.uint64(32), np.full(g.shape, pm.STEP_WORD, dtype=np.uint64), q, seed_p & 0xFFFFFFFF, seed_p >> 32)
    u1, u2 = nm._u01(r0, r1), nm._u01(r2, r3)
    out = parts(np.ascontiguousarray(u1.ravel()), np.ascontiguousarray(u2.ravel()))
    xi = np.ascontiguousarray(np.stack([out[4].reshape(u1.shape), out[5].reshape(u1.shape)], axis=2).reshape(K, 2 * nq)[:, :PN])
    xi.setflags(write=False)
    return xi


def param_uniforms(seed, p, K, PU):
    seed_p = (int(seed) + PASS_STRIDE * int(p)) & MASK64
    return pm.gen_draws(seed_p, K, 0, PU)[1]


class ParamShiftRng:
    """the counting rng of rat_user_params over K rollouts: the shifted normals, logw at the draw, the overdraw flag"""

    def __init__(self, xi, un, ps):
        self.xi, self.un, self.ps = xi, un, ps
        self.logw = np.zeros(xi.shape[0])
        self.over, self.i, self.iu = 0, 0, 0

    def normal(self):
        i = self.i
        self.i += 1
        if i >= self.xi.shape[1]:
            self.over |= 1
            return np.full(self.xi.shape[0], np.nan)
        sv = self.ps[i]
        z = sv + self.xi[:, i]
        self.logw = self.logw + (-sv * z + 0.5 * sv * sv)
        return z

    def uniform(self):
        i = self.iu
        self.iu += 1
        if self.un is None or i >= self.un.shape[1]:
            self.over |= 2
            return np.full(self.xi.shape[0], np.nan)
        return self.un[:, i]


class Model(nm.Model):
    """rare_event_noise_model.Model with the hook, its declared draws and, for the user-event variant, the event's function"""

    def __init__(self, f, noise, hook, p, n, m, N, P, PN, U=0, PU=0, uev=None):
        super().__init__(f, noise, p, n, m, N, P, U)
        self.hook, self.PN, self.PU, self.uev = hook, PN, PU, uev


def one_pass(mod, x_nom, l, L, ev, seed, p, K, s, ps):
    """(M [K] -- NaN for a DomainError rollout --, logw [K], dom [K], xi [K, N, P], xi^p [K, PN]) of pass p under the shifts s [N, P], ps [PN]"""
    n, m, N = mod.n, mod.m, mod.N
    xip = param_normals(seed, p, K, mod.PN)
    prng = ParamShiftRng(xip, param_uniforms(seed, p, K, mod.PU) if mod.PU else None, ps)
    with np.errstate(all="ignore"):
        q = mod.hook(prng, mod.p)
    if prng.over:
        raise OverflowError(f"parameter overdraw {prng.over}")
    P = q.T
    dom = np.isnan(q).any(axis=1) & ~np.isnan(mod.p).any()
    xi = nm.normals(seed, p, K, N, mod.P)
    rng = nm.ShiftRng(xi, nm.uniforms(seed, p, K, N, mod.U) if mod.U else None, s)
    rng.logw = prng.logw                                              # the lane's logw starts from the parameter part
    x_nom, l = np.asarray(x_nom, float), np.asarray(l, float)
    x, u = np.zeros((K, N + 1, n)), np.zeros((K, N, m))
    x[:, 0] = x_nom if L is None else x_nom[0]
    with np.errstate(all="ignore"):
        for t in range(N):
            u[:, t] = l[t] if L is None else l[t] + (x[:, t] - x_nom[t]) @ np.asarray(L[t], float).T
            inok = ~(np.isnan(x[:, t]).any(axis=1) | np.isnan(u[:, t]).any(axis=1))
            rng.at(t)
            w = mod.noise(t, x[:, t], u[:, t], rng, P)
            xn = mod.f(x[:, t], u[:, t], P)
            dom |= inok & (np.isnan(xn).any(axis=1) | np.isnan(w).any(axis=1))
            x[:, t + 1] = xn + w
    if rng.over:
        raise OverflowError(f"overdraw {rng.over}")
    if mod.uev is None:
        M = per_rollout(g_device(x, u, [ev]), [ev], ~dom)[0][0]
    else:
        M = np.full(K, np.nan)
        with np.errstate(invalid="ignore"):
            for t in range(N + 1):
                g = mod.uev(t, x[:, t], u[:, t] if t < N else np.zeros((K, m)), P)
                if g is not None:
                    M = np.where((g > M) | np.isnan(M), g, M)
        M[dom] = np.nan
    return M, rng.logw, dom, xi, xip


def adapt(M, logw, dom, xi, xip, s, ps, gamma):
    """(s + sum_E w xi / sum_E w, ps + sum_E w xi^p / sum_E w, elite count, elite effective sample size)"""
    with np.errstate(invalid="ignore"):
        E = M >= gamma
    lmax = _fixed_order(logw, ~dom, np.maximum, -np.inf)
    w = np.where(E, np.exp(logw - lmax), 0.0)
    W, W2 = rm.elite_sum(w), rm.elite_sum(w * w)
    S = rm.elite_sum(w[:, None, None] * np.where(E[:, None, None], xi, 0.0))
    Sp = rm.elite_sum(w[:, None] * np.where(E[:, None], xip, 0.0))
    with np.errstate(all="ignore"):
        return s + S / W, ps + Sp / W, int(E.sum()), W * W / W2


def rare_event_params(mod, x_nom, l, L, event, K, seed=0, shift=None, param_shift=None, adapt_mode="both", n_iter=8, rho=0.1):
    """The whole call; rare_event_noise_model.rare_event_noise's dict with param_shift [PN] and param_trace [n_iter].  event: an Event
    (mod.uev None) or ignored."""
    ev = event.dense(mod.n, mod.m, mod.N) if mod.uev is None else None
    bits = ADAPT[adapt_mode]
    s = np.zeros((mod.N, mod.P)) if shift is None else np.array(shift, dtype=np.float64)
    ps = np.zeros(mod.PN) if param_shift is None else np.array(param_shift, dtype=np.float64)
    trace, ptrace, levels = np.full((n_iter, 4), np.nan), np.full(n_iter, np.nan), []
    reached, n_run, gamma, bad = False, 0, np.nan, False
    for j in range(n_iter):
        M, logw, dom, xi, xip = one_pass(mod, x_nom, l, L, ev, seed, j + 1, K, s, ps)
        gamma, code, v, k = rm.level(M, rho)
        levels.append((gamma, code, v, k))
        trace[j, 0] = gamma
        n_run += 1
        reached |= code == 1
        bad |= code == 3
        if code != 0:
            break
        s_new, ps_new, cnt, ess = adapt(M, logw, dom, xi, xip, s, ps, gamma)
        ok = (not bits & 1 or np.all(np.isfinite(s_new))) and (not bits & 2 or np.all(np.isfinite(ps_new)))
        if ok:
            s = s_new if bits & 1 else s
            ps = ps_new if bits & 2 else ps
        else:
            bad = True
        trace[j, 1:] = cnt, ess, np.sqrt((s * s).sum())
        ptrace[j] = np.sqrt((ps * ps).sum())
    M, logw, dom, _, _ = one_pass(mod, x_nom, l, L, ev, seed, 0, K, s, ps)
    out = rm.estimate(M, logw, dom)
    flag = rm.OK if reached else rm.NOT_REACHED
    if out["n_ok"] == 0:
        flag = rm.EMPTY
    elif bad or not (np.isfinite(out["logw_max"]) and np.isfinite(out["logw_min"]) and out["prob"] < np.inf):
        flag = rm.NONFINITE
    if flag >= rm.EMPTY:
        out.update(prob=np.nan, prob_se=np.nan, ess=np.nan)
    out.update(flag=flag, n_iter=n_run, level=gamma if n_run else np.nan, shift=s, param_shift=ps, trace=trace, param_trace=ptrace,
               margins=M, logw=logw, levels=levels)
    return out


# ---- the closed forms: n = m = 1, N = 1, x0 = 1, one parameter normal, one step normal ----------------------------------------------------------
# p = a0 | s | c (the event's threshold) | sigma.  x1 = (a0 + s z_p) x0 + w, the event x1 > c watched at step 1 alone.
# (a) user_params_model.SCALAR, w = 0 z: P = Phi(-beta), beta = (c / x0 - a0) / s.  (b) w = sigma z: x1 ~ N(a0 x0, s^2 x0^2 + sigma^2).
SCALAR_EVENT = r"""
#define RAT_USER_EVENT
__device__ void rat_user_event(int k, const double *x, const double *u, double *g, const double *p) {
    if (k >= 1) g[0] = x[0] - p[2];
}
"""
SCALAR_A = pm.SCALAR + SCALAR_EVENT
SCALAR_B = pm.SCALAR.replace("0.0 * rng.normal()", "p[3] * rng.normal()") + SCALAR_EVENT
assert SCALAR_B != SCALAR_A
BETA, A0, S_A, X0 = 6.0, 0.9, 0.05, 1.0
K_CLOSED, N_ITER_CLOSED, RHO_CLOSED = 1 << 14, 8, 0.1
SEED_A, SEED_B = 1234, 4321                                           # the seeds tests/test_cpu_rare_event_params.py confirms the cap at


def closed_case(which):
    """(source, params, NumPy model, exact probability) of closed form "a" or "b" """
    from math import erfc, sqrt
    sigma = 0.0 if which == "a" else 0.03
    c = A0 * X0 + BETA * sqrt(S_A * S_A * X0 * X0 + sigma * sigma)
    p = np.array([A0, S_A, c, sigma])

    def hook(rng, p):
        q = np.repeat(p[None], rng.xi.shape[0], axis=0)
        q[:, 0] = p[0] + p[1] * rng.normal()
        return q

    f = lambda x, u, P: (P[0] * x[:, 0])[:, None]
    noise = lambda k, x, u, rng, P: ((0.0 if which == "a" else P[3]) * rng.normal())[:, None]
    uev = lambda k, x, u, P: x[:, 0] - P[2] if k >= 1 else None
    mod = Model(f, noise, hook, p, 1, 1, 1, 1, 1, uev=uev)
    return (SCALAR_A if which == "a" else SCALAR_B), p, mod, 0.5 * erfc(BETA / sqrt(2.0))


def closed_policy():
    return np.array([X0]), np.zeros((1, 1)), None


# ---- the cases of the parity tests: user_params_model's pendulum and 12 x 4 source, the hook "scale" on the obstacle's radius ----------------
def lqc_f(x, u, P):
    n, m = x.shape[1], u.shape[1]
    i = np.arange(n)
    c = lambda v: np.asarray(v)[:, None] if np.ndim(v) else v
    return c(P[0]) * x + c(P[1]) * (np.roll(x, -1, axis=1) - np.roll(x, 1, axis=1)) + c(P[2]) * (u[:, i % m] - 0.5 * u[:, (i + 1) % m]) + c(P[3]) * x ** 3


def lqc_noise(k, x, u, rng, P):
    c = lambda v: np.asarray(v)[:, None] if np.ndim(v) else v
    second = rng.uniform() < P[8]
    z = np.stack([rng.normal() for _ in range(x.shape[1])], axis=1)
    return np.where(second[:, None], c(P[9]) + c(P[10]) * z, c(P[11]) * (z + 0.5 * np.roll(z, -1, axis=1)))


class ParityCase:
    """pend (2, 1, N = 5, three step normals) or lq12 (12, 4, N = 3, twelve normals and a uniform): the source with the hook "scale" on
    (the obstacle's radius p[EVP], a scale of the sampler, a dynamics coefficient) and user_params_model.EVENT, whose margin
    p[EVP] - |x[0]| reads the drawn radius"""

    def __init__(self, name):
        c = pm.case(name)
        self.name, self.n, self.m = name, c.n, c.m
        self.N = 5 if name == "pend" else 3
        self.npn, self.npu, self.evp = c.npn, c.npu, c.evp
        self.idx = dict(pi0=c.evp, pi1=c.idx["pi1"], pi2=c.idx["pi2"], psh=c.idx["psh"])
        self.source = pm.source(c.base, "scale", **self.idx) + f"#define EVP {c.evp}\n" + pm.EVENT
        self.p, self.W = c.p.copy(), c.W
        if name == "pend":
            self.policy = um.pend_policy(self.N)
            self.f, self.noise = nm.pend_f, nm.pend_state_noise
        else:
            x, l, L = c.policy
            self.policy = (x[:self.N + 1], l[:self.N], L[:self.N])
            self.f, self.noise = lqc_f, lqc_noise

    def hook(self, rng, p):
        i = self.idx
        q = np.repeat(np.asarray(p, float)[None], rng.xi.shape[0], axis=0)
        z0, z1, v = rng.normal(), rng.normal(), rng.uniform()
        q[:, i["pi0"]] = p[i["pi0"]] * (1.0 + 0.2 * z0)
        q[:, i["pi1"]] = p[i["pi1"]] * (1.0 + 0.2 * z1)
        q[:, i["pi2"]] = p[i["pi2"]] + i["psh"] * v
        return q

    def model(self, p=None):
        evp = self.evp
        uev = lambda k, x, u, P: P[evp] - np.abs(x[:, 0])
        return Model(self.f, self.noise, self.hook, self.p if p is None else p, self.n, self.m, self.N, self.npn, pm.PARAM_NORMALS, U=self.npu,
                     PU=pm.PARAM_UNIFORMS, uev=uev)

    def rarefied(self, K, seed, q=0.998):
        """the parameters with the nominal radius moved so that about 1 - q of the plain rollouts of pass 0 enter their own obstacle: between
        two neighbouring rollouts' thresholds, never on one (tests/test_gpu_rare_event_noise.rarefy for a margin r c_j - d_j)"""
        mod = self.model()
        M = one_pass(mod, *self.policy, None, seed, 0, K, np.zeros((self.N, self.npn)), np.zeros(pm.PARAM_NORMALS))[0]
        c = 1.0 + 0.2 * param_normals(seed, 0, K, pm.PARAM_NORMALS)[:, 0]
        d = self.p[self.evp] * c - M                                  # min_t |x_t[0]| of every rollout
        assert np.all(c > 0)
        r = np.sort(d / c)                                            # rollout j violates where the radius is above d_j / c_j
        i = max(int((1.0 - q) * K), 1)
        p = self.p.copy()
        p[self.evp] = 0.5 * (r[i - 1] + r[i])
        return p
