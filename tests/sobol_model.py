"""Sobol indices of a policy's Monte-Carlo cost (rat_policy_sobol, include/ratilqr.h "which uncertainty drives the cost") -- test aid shared
by tests/test_cpu_sobol.py, tests/test_gpu_sobol.py and tools/policy_sobol_bench.py: a NumPy restatement of the whole call.  Both streams
are generated under their seeds (the step draws with tests/rare_event_noise_model.normals / uniforms, the parameter draws with
tests/user_params_model.gen_draws), mixed draw by draw as a variant's masks say, rolled out with user_params_model.np_rollouts, and the
estimator is formed with math.fsum.

A draw of the generator is a function of (seed, rollout, step, index) alone, so "draw i of stream B" is entry i of the array generated
under seed_b: mixing whole arrays column by column is the device's rule, the Box-Muller pairing included (normal 2q + 1 of a stream is the
second output of that stream's block q whatever its neighbour 2q was taken from).

The two closed forms of the tests (n = m = 1, N = 4, x_0 = 0, c = 0, h = x, two parameter normals z0, z1, one step normal xi):
  additive     f = x + q0 + q1, q0 = 0.3 z0, q1 = 0.4 z1, w = 0.5 xi:  J = 4 (q0 + q1) + 0.5 sum xi, Var J = 1.44 + 2.56 + 1 = 5,
               S = T = (0.288, 0.512, 0.2) for the groups {z0}, {z1}, {xi}
  interaction  f = x + q0 q1, q0 = z0, q1 = z1, w = xi:  J = 4 z0 z1 + sum xi, Var J = 16 + 4 = 20, S = (0, 0, 0.2), T = (0.8, 0.8, 0.2)
are rolled out for all K base samples at once (closed_costs), in the device's order of operations."""
import math

import numpy as np

import rare_event_noise_model as rn
import ratilqr.jl_amd as rat
import user_noise_model as um
import user_params_model as pm

DEGENERATE = 16
ALL = (1 << 64) - 1


def variants(groups):
    """the masks (param normals, param uniforms, step normals, step uniforms) of rows A, B and the groups' AB_i"""
    return [(0, 0, 0, 0), (ALL, ALL, ALL, ALL)] + [tuple(g.words) for g in groups]


def pick(a, b, mask):
    """column i of b where bit i of mask is set, of a elsewhere (the last axis counts draws)"""
    out = a.copy()
    for i in range(a.shape[-1]):
        if (mask >> i) & 1:
            out[..., i] = b[..., i]
    return out


def streams(seed, K, N, npn, npu, ppn, ppu):
    """what the generator yields under `seed` for base samples 0 .. K - 1: step normals [K, N, npn], step uniforms [K, N, npu], parameter
    normals [K, ppn], parameter uniforms [K, ppu]"""
    zpn, zpu = pm.gen_draws(seed, K, ppn, ppu)
    return dict(sn=np.array(rn.normals(seed, 0, K, N, npn)), su=np.array(rn.uniforms(seed, 0, K, N, npu)), pn=zpn, pu=zpu)


def mixed(A, B, words):
    return dict(pn=pick(A["pn"], B["pn"], words[0]), pu=pick(A["pu"], B["pu"], words[1]),
                sn=pick(A["sn"], B["sn"], words[2]), su=pick(A["su"], B["su"], words[3]))


def case_costs(c, hook, closed, groups, K, seed_a, seed_b, p=None):
    """Y [d + 2, K] of the case c (user_params_model.Case) under the hook `hook` (None: parameter sampling off)"""
    ppn, ppu = (pm.PARAM_NORMALS, pm.PARAM_UNIFORMS) if hook is not None else (0, 0)
    A, B = (streams(s, K, c.N, c.npn, c.npu, ppn, ppu) for s in (seed_a, seed_b))
    p = c.p if p is None else p
    rows = []
    for words in variants(groups):
        z = mixed(A, B, words)
        q = np.repeat(np.asarray(p, float)[None], K, axis=0) if hook is None else pm.np_params(hook, p, z["pn"], z["pu"], **c.idx)
        zu = z["su"].ravel() if c.npu else None
        rows.append(pm.np_rollouts(*c.fns, q, *c.args(closed), K, z["sn"].ravel(), zu, c.npn, c.npu)[0])
    return np.array(rows)


def estimator(Y):
    """the header's estimator on Y [d + 2, K] with math.fsum: dict(S, S_se, T, T_se, n_ok, mean, var, var_se, flag)"""
    Y = np.asarray(Y, float)
    d = Y.shape[0] - 2
    ok = ~np.isnan(Y).any(axis=0)
    n = int(ok.sum())
    nan = float("nan")
    out = dict(S=np.full(d, nan), S_se=np.full(d, nan), T=np.full(d, nan), T_se=np.full(d, nan), n_ok=n, mean=nan, var=nan, var_se=nan,
               flag=DEGENERATE)
    if n == 0:
        return out
    ya, yb = Y[0, ok], Y[1, ok]
    mu = math.fsum(np.concatenate([ya, yb])) / (2 * n)
    ap, bp = ya - mu, yb - mu
    s = 0.5 * (ap * ap + bp * bp)
    V = math.fsum(s) / n
    out.update(mean=mu, var=V)
    if n < 2:
        return out
    out["var_se"] = math.sqrt(max(math.fsum((s - V) ** 2), 0.0) / (n - 1) / n)
    if not (V > 0.0 and math.isfinite(V)):
        return out
    out["flag"] = 0
    for i in range(d):
        D = Y[2 + i, ok] - ya
        for key, a in (("S", bp * D), ("T", 0.5 * D * D)):
            R = (math.fsum(a) / n) / V
            e = a - R * s
            out[key][i] = R
            out[key + "_se"][i] = math.sqrt(math.fsum(e * e) / (n - 1) / n) / V
    return out


# ---- the closed forms ----------------------------------------------------------------------------------------------------------------------
CLOSED_N = 4
CLOSED_K = 1 << 14
_FCH = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) { xn[0] = x[0] + DRIFT; }
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) { return 0.0 * x[0]; }
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return x[0]; }
""" + um.NOISE_HEAD + "    w[0] = WSCALE * rng.normal();\n}\n" + r"""
#define RAT_USER_PARAMS
template <class R> __device__ void rat_user_params(R &rng, const double *p, double *q) {
    const double z0 = rng.normal();
    const double z1 = rng.normal();
    q[0] = Q0 * z0;
    q[1] = Q1 * z1;
}
"""
CLOSED = {
    "additive": dict(source="#define DRIFT (p[0] + p[1])\n#define WSCALE 0.5\n#define Q0 0.3\n#define Q1 0.4\n" + _FCH, q=(0.3, 0.4), w=0.5,
                     drift=lambda q0, q1: q0 + q1, var=5.0, S=(0.288, 0.512, 0.2), T=(0.288, 0.512, 0.2)),
    "interaction": dict(source="#define DRIFT (p[0] * p[1])\n#define WSCALE 1.0\n#define Q0 1.0\n#define Q1 1.0\n" + _FCH, q=(1.0, 1.0), w=1.0,
                        drift=lambda q0, q1: q0 * q1, var=20.0, S=(0.0, 0.0, 0.2), T=(0.8, 0.8, 0.2)),
}


def closed_groups():
    return [rat.SobolGroup(param_normals=(0,), name="z0"), rat.SobolGroup(param_normals=(1,), name="z1"),
            rat.SobolGroup(step_normals=(0,), name="xi")]


def closed_problem(which):
    return rat.DeviceSourceProblem(CLOSED[which]["source"], 1, 1, CLOSED_N, 1e-2 * np.eye(1), params=[0.0, 0.0])


def closed_policy():
    return np.zeros(1), np.zeros((CLOSED_N, 1)), None


def closed_costs(which, K, seed_a, seed_b):
    """Y [5, K] of a closed form, all base samples at once: x_{t+1} = (x_t + drift) + w_t from x_0 = 0, J = 0 + ... + 0 + x_N"""
    m = CLOSED[which]
    A, B = (streams(s, K, CLOSED_N, 1, 0, 2, 0) for s in (seed_a, seed_b))
    rows = []
    for words in variants(closed_groups()):
        z = mixed(A, B, words)
        drift = m["drift"](m["q"][0] * z["pn"][:, 0], m["q"][1] * z["pn"][:, 1])
        x = np.zeros(K)
        for t in range(CLOSED_N):
            x = (x + drift) + m["w"] * z["sn"][:, t, 0]
        rows.append(x)
    return np.array(rows)
