"""Safety events the user writes (rat_user_event, include/ratilqr.h "source models") -- test aid shared by tests/test_cpu_user_event.py,
tests/test_gpu_user_event.py and tools/policy_events_user_bench.py: the test events as HIP text and in NumPy, two source models to hang
them on, and the reduction of their values.

Every test event is built from single IEEE operations -- one subtraction, fmin / fmax / fabs, a comparison, a look-up in p -- so the
compiler has nothing to contract and NumPy gives the device's bits: no tolerance on g, M, tau or the masks.  An event reads its own
parameters at q = p + EVOFF, behind the model's.

`g_user` evaluates an event on trajectories: g [K, N+1, E], NaN where the function writes nothing (u is 0 at k = N).  M, tau, the
indicators and "any" follow by tests/events_model.per_rollout's rules -- a NaN g is passed over exactly as a quadratic event's is, every
step is in the window -- and the weighted sums by tests/events_model.events: `reduce` hands that model the g it would otherwise form from
Q, a, b and restates none of it."""
from unittest import mock

import numpy as np

import events_model as em
import ratilqr.jl_amd as rat
import user_noise_model as um

# ---- two sources with a plain Gaussian sampler ------------------------------------------------------------------------------------------
# the double integrator (2, 1): p = dt | s0 | s1
DI = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) {
    xn[0] = x[0] + p[0] * x[1];
    xn[1] = x[1] + p[0] * u[0];
}
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) {
    return 0.5 * (x[0] * x[0] + x[1] * x[1]) + 0.05 * (u[0] * u[0]);
}
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return x[0] * x[0] + x[1] * x[1]; }
#define RAT_USER_NOISE
template <class R> __device__ void rat_user_noise(int k, const double *x, const double *u, R &rng, double *w, const double *p) {
    w[0] = p[1] * rng.normal();
    w[1] = p[2] * rng.normal();
}
"""
DI_P = [0.1, 0.05, 0.1]
# a random walk (1, 1), x_{k+1} = x_k + p[0] u_k + p[1] z_k: x_N is Gaussian about its noise-free value with variance N p[1]^2
WALK = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) { xn[0] = x[0] + p[0] * u[0]; }
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) { return 0.5 * (x[0] * x[0]) + 0.5 * (u[0] * u[0]); }
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return 0.5 * (x[0] * x[0]); }
#define RAT_USER_NOISE
template <class R> __device__ void rat_user_noise(int k, const double *x, const double *u, R &rng, double *w, const double *p) {
    w[0] = p[1] * rng.normal();
}
"""
WALK_P = [0.0, 0.25]

# ---- the events: (HIP body of rat_user_event, n_event) -------------------------------------------------------------------------------------
EVENT_HEAD = r"""
#define RAT_USER_EVENT
__device__ void rat_user_event(int k, const double *x, const double *u, double *g, const double *p) {
    const double *q = p + EVOFF;
"""
BODIES = {
    "half": ("    g[0] = x[0] - q[0];\n", 1),
    "box": ("    g[0] = fmin(fmin(x[0] - q[0], q[1] - x[0]), fmin(x[1] - q[2], q[3] - x[1]));\n", 1),
    "moving": ("    const double cx = q[1 + 2 * k], cy = q[2 + 2 * k];\n    g[0] = q[0] - fmax(fabs(x[0] - cx), fabs(x[1] - cy));\n", 1),
    "window": ("    if (k >= 3 && k <= 5) g[0] = x[0] - q[0];\n", 1),
    # fourteen half-spaces on the state components in turn, one on u[0] (watched at k = N with u = 0), and one that is never written
    "16": ("    for (int i = 0; i < 14; ++i) g[i] = x[i % RAT_N] - q[i];\n    g[14] = u[0] - q[14];\n", 16),
    # the half-space at one step alone, the step a parameter
    "half_at": ("    if (k == (int)q[1]) g[0] = x[0] - q[0];\n", 1),
}
SYNTAX_ERROR = "    g[0] = x[0] - q[0]\n"                              # (no semicolon: the compiler names this line of model.hip)


def source(base, name, evoff, body=None):
    """the base source with the event `name` behind it, its parameters at p + evoff"""
    return base + f"#define EVOFF {int(evoff)}\n" + EVENT_HEAD + (BODIES[name][0] if body is None else body) + "}\n"


def n_params(name, N):
    return {"half": 1, "box": 4, "moving": 3 + 2 * N, "window": 1, "16": 15, "half_at": 2}[name]


def g_user(name, x, u, q):
    """g [K, N+1, E] of the event `name` with parameters q on trajectories x [K, N+1, n], u [K, N, m]"""
    x, u, q = np.asarray(x, float), np.asarray(u, float), np.asarray(q, float)
    K, T, n = x.shape
    uu = np.zeros((K, T, u.shape[2]))
    uu[:, :T - 1] = u                                                 # u_N = 0
    g = np.full((K, T, BODIES[name][1]), np.nan)
    with np.errstate(invalid="ignore"):
        if name == "half":
            g[:, :, 0] = x[:, :, 0] - q[0]
        elif name == "box":
            g[:, :, 0] = np.fmin(np.fmin(x[:, :, 0] - q[0], q[1] - x[:, :, 0]), np.fmin(x[:, :, 1] - q[2], q[3] - x[:, :, 1]))
        elif name == "moving":
            k = np.arange(T)
            g[:, :, 0] = q[0] - np.fmax(np.abs(x[:, :, 0] - q[1 + 2 * k][None]), np.abs(x[:, :, 1] - q[2 + 2 * k][None]))
        elif name == "window":
            g[:, 3:6, 0] = x[:, 3:6, 0] - q[0]
        elif name == "16":
            for i in range(14):
                g[:, :, i] = x[:, :, i % n] - q[i]
            g[:, :, 14] = uu[:, :, 0] - q[14]
        elif name == "half_at":
            k = int(q[1])
            g[:, k, 0] = x[:, k, 0] - q[0]
        else:
            raise KeyError(name)
    return g


def windows(g):
    """the events of a g as tests/events_model takes them: no Q, a, b to read, every step in the window"""
    return [(None, None, None, 0, g.shape[1] - 1)] * g.shape[2]


def per_rollout(g, costs):
    """(M [E+1, K], tau [E+1, K], viol [K, N+1, E+1]) by events_model.per_rollout: the last event is "any"; a rollout whose cost is NaN is
    selected out (NaN, -1, False)"""
    return em.per_rollout(np.asarray(g, float), windows(g), ~np.isnan(np.asarray(costs, float).ravel()))


def reduce(g, costs, y, dead):
    """events_model.events on the user's g: its dict of slots [R, E+1], step [R, E+1, N+1], margins and tau [E+1, K]"""
    K, T, _ = g.shape
    with mock.patch.object(em, "g_device", lambda x, u, evs: np.asarray(g, float)):
        return em.events(np.zeros((K, T, 1)), np.zeros((K, T - 1, 1)), costs, y, dead, windows(g))


# ---- the problems of the GPU tests and the benchmark --------------------------------------------------------------------------------------
def di_case(name, N, q=None):
    """(problem, x_nom, l, L, evoff) of the double integrator with the event `name`; q: the event's parameters (zeros when None)"""
    r = np.random.default_rng(3)
    x_nom = np.array([0.5, -0.2]) + 0.05 * r.standard_normal((N + 1, 2))
    l, L = 0.2 * r.standard_normal((N, 1)), -0.3 * np.abs(r.standard_normal((N, 1, 2)))
    q = np.zeros(n_params(name, N)) if q is None else np.asarray(q, float)
    prob = rat.DeviceSourceProblem(source(DI, name, len(DI_P)), 2, 1, N, 1e-3 * np.eye(2), params=np.concatenate([DI_P, q]))
    return prob, x_nom, l, L, len(DI_P)


def lq_case(name, N, q=None):
    """the same for the 12 x 4 linear source: LQ_GAUSS of tests/user_noise_model.py with kappa = 0"""
    gp = um.lq_generative(Nh=N, kappa=0.0)
    base = um.lq_source_problem(gp, source=um.LQ_GAUSS, mean=False)
    r = np.random.default_rng(21)
    x_nom = 0.3 * r.standard_normal((N + 1, 12))
    l, L = 0.1 * r.standard_normal((N, 4)), 0.1 * r.standard_normal((N, 4, 12))
    q = np.zeros(n_params(name, N)) if q is None else np.asarray(q, float)
    off = base.params.size
    prob = rat.DeviceSourceProblem(source(um.LQ_GAUSS, name, off), 12, 4, N, base.Wtab, params=np.concatenate([base.params, q]))
    return prob, x_nom, l, L, off


CASES = {"di": (di_case, 2), "lq": (lq_case, 12)}


def thresholds(name, x, u, costs):
    """parameters of the event `name` sized from the spread of the rollouts that have a cost, each threshold between two neighbouring
    values (events_model.between), never on one: a share of the rollouts violates, not none and not all"""
    ok = ~np.isnan(np.asarray(costs, float).ravel())
    K, T, n = x.shape
    xs, us = (x[ok], u[ok]) if ok.any() else (np.zeros((1, T, n)), np.zeros((1, T - 1, u.shape[2])))
    x0, x1 = xs[:, :, 0], xs[:, :, 1]
    if name in ("half", "window"):
        seen = x0[:, 3:6] if name == "window" and T > 5 else x0      # (a horizon the window never opens in: any number will do)
        return np.array([em.between(seen.max(axis=1), 0.6)])
    if name == "box":
        return np.array([em.between(x0.ravel(), 0.3), em.between(x0.ravel(), 0.9), em.between(x1.ravel(), 0.2), em.between(x1.ravel(), 0.95)])
    if name == "moving":
        cx, cy = np.median(x0, axis=0), np.median(x1, axis=0)         # the centre follows the bulk of the rollouts, step by step ...
        cx[0], cy[0] = cx[0] + 10.0, cy[0] + 10.0                     # ... from far away: x_0 is the same point on every rollout
        half = em.between(np.fmax(np.abs(x0 - cx), np.abs(x1 - cy))[:, 1:].min(axis=1), 0.4)
        return np.concatenate([[half], np.stack([cx, cy], axis=1).ravel()])
    if name == "16":
        q = [em.between(xs[:, :, i % n].max(axis=1), 0.1 + 0.06 * i) for i in range(14)]
        return np.array(q + [em.between(np.append(us[:, :, 0].max(axis=1), 0.0), 0.5)])
    raise KeyError(name)
