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
are rolled out for all K base samples at once (closed_costs), in the device's order of operations.

OFFSET is the additive form with h = x + p[2]: J = p[2] + 4 (q0 + q1) + 0.5 sum xi, the same variance and indices about a mean of p[2].
The offset is a parameter the hook leaves alone, so one compiled module serves every offset (Context.set_params).

The wide closed form (WIDE_*; n = m = 1, N = 2, x_0 = 0, c = 0, h = x, open loop, 32 parameters) declares WD = 64 draws of each of the
four kinds and is linear in every one.  With the coefficient of draw i of a kind k(i) = scale (1 + i / 64), an exact binary fraction,
  rat_user_params  q[j] = 0; q[i % 32] += PN k(i) z_i for i = 0 .. 63, then q[i % 32] += PU k(i) (v_i - 0.5) for i = 0 .. 63
  rat_user_f       x+ = x + (q[0] + ... + q[31])
  rat_user_noise   w = sum_i SN k(i) xi_i, then + sum_i SU k(i) (u_i - 0.5)
so J = 2 sum_j q[j] + w_0 + w_1 and Var J = sum_i k(i)^2 (4 PN^2 + 4 PU^2 / 12 + 2 SN^2 + 2 SU^2 / 12): a group's S = T is the sum of
its own terms over Var J (wide_exact).  "#define WD 40" in front of the source (wide_source(40)) gives the 40-draw instantiation of the refusal test."""
import functools
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


# ---- the additive form about a mean: h = x + p[2] -----------------------------------------------------------------------------------------
OFFSET_SOURCE = CLOSED["additive"]["source"].replace("return x[0]; }", "return x[0] + p[2]; }")
assert OFFSET_SOURCE != CLOSED["additive"]["source"]


def offset_problem():
    return rat.DeviceSourceProblem(OFFSET_SOURCE, 1, 1, CLOSED_N, 1e-2 * np.eye(1), params=[0.0, 0.0, 0.0])


def offset_costs(offset, K, seed_a, seed_b):
    """Y [5, K] of OFFSET: the additive form's x_N, then 0 + (x_N + offset), one rounded addition"""
    return closed_costs("additive", K, seed_a, seed_b) + float(offset)


def plain_estimator(Y, centred):
    """S, S_se of estimator() in plain float64 sums (no fsum), every base sample OK.  centred=False forms the numerator from the costs
    themselves, mean(y_B (y_i - y_A)), and the residuals about it -- the estimator the comment above sb_pass1 warns of: the same mean, a
    spread that carries mu^2 T."""
    Y = np.asarray(Y, float)
    n = Y.shape[1]
    ya, yb = Y[0], Y[1]
    mu = (ya.sum() + yb.sum()) / (2 * n)
    ap, bp = ya - mu, yb - mu
    s = 0.5 * (ap * ap + bp * bp)
    V = s.sum() / n
    S, S_se = [], []
    for i in range(Y.shape[0] - 2):
        a = (bp if centred else yb) * (Y[2 + i] - ya)
        R = (a.sum() / n) / V
        e = a - R * s
        S.append(R)
        S_se.append(math.sqrt((e * e).sum() / (n - 1) / n) / V)
    return dict(S=np.array(S), S_se=np.array(S_se))


# ---- the wide closed form: 64 draws of every kind, 32 parameters --------------------------------------------------------------------------
WIDE_N, WIDE_D, WIDE_NPAR = 2, 64, 32
WIDE_SCALE = dict(pn=0.5, pu=2.0, sn=1.0, su=2.0)                     # PN, PU, SN, SU
WIDE_SOURCE = r"""
#ifndef WD
#define WD 64
#endif
#define PN 0.5
#define PU 2.0
#define SN 1.0
#define SU 2.0
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) {
    T s = 0.0;
    for (int j = 0; j < 32; ++j) s += p[j];
    xn[0] = x[0] + s;
}
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) { return 0.0 * x[0]; }
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return x[0]; }
""" + um.NOISE_HEAD + r"""#pragma clang fp contract(off)
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < WD; ++i) a += (SN * (1.0 + i / 64.0)) * rng.normal();
#pragma unroll
    for (int i = 0; i < WD; ++i) a += (SU * (1.0 + i / 64.0)) * (rng.uniform() - 0.5);
    w[0] = a;
}
#define RAT_USER_PARAMS
template <class R> __device__ void rat_user_params(R &rng, const double *p, double *q) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 32; ++j) q[j] = 0.0;
#pragma unroll
    for (int i = 0; i < WD; ++i) q[i % 32] += (PN * (1.0 + i / 64.0)) * rng.normal();
#pragma unroll
    for (int i = 0; i < WD; ++i) q[i % 32] += (PU * (1.0 + i / 64.0)) * (rng.uniform() - 0.5);
}
"""


def wide_source(nd=WIDE_D):
    return WIDE_SOURCE if nd == WIDE_D else f"#define WD {int(nd)}\n" + WIDE_SOURCE


def wide_problem(nd=WIDE_D):
    return rat.DeviceSourceProblem(wide_source(nd), 1, 1, WIDE_N, 1e-2 * np.eye(1), params=np.zeros(WIDE_NPAR))


def wide_policy():
    return np.zeros(1), np.zeros((WIDE_N, 1)), None


def wide_coef(kind, i):
    return WIDE_SCALE[kind] * (1.0 + i / 64.0)


def wide_streams(K, seed_a, seed_b, nd=WIDE_D):
    return tuple(streams(s, K, WIDE_N, nd, nd, nd, nd) for s in (seed_a, seed_b))


def wide_row(A, B, words, nd=WIDE_D):
    """the costs [K] of one variant, in the device's order of additions"""
    z = mixed(A, B, words)
    K = z["pn"].shape[0]
    q = np.zeros((K, WIDE_NPAR))
    for i in range(nd):
        q[:, i % 32] += wide_coef("pn", i) * z["pn"][:, i]
    for i in range(nd):
        q[:, i % 32] += wide_coef("pu", i) * (z["pu"][:, i] - 0.5)
    s = np.zeros(K)
    for j in range(WIDE_NPAR):
        s += q[:, j]
    x = np.zeros(K)
    for t in range(WIDE_N):
        a = np.zeros(K)
        for i in range(nd):
            a += wide_coef("sn", i) * z["sn"][:, t, i]
        for i in range(nd):
            a += wide_coef("su", i) * (z["su"][:, t, i] - 0.5)
        x = (x + s) + a
    return x


def wide_costs(groups, K, seed_a, seed_b, nd=WIDE_D):
    """Y [d + 2, K] of the wide closed form, all base samples at once"""
    A, B = wide_streams(K, seed_a, seed_b, nd)
    return np.array([wide_row(A, B, words, nd) for words in variants(groups)])


@functools.lru_cache(maxsize=2)
def wide_model(K, seed_a, seed_b):
    """wide_costs of wide_groups(), computed once and left unchanged"""
    Y = wide_costs(wide_groups(), K, seed_a, seed_b)
    Y.setflags(write=False)
    return Y


def wide_share(words, nd=WIDE_D):
    """the variance the draws of the masks carry: sum of squared coefficients, 1/12 for a uniform, N^2 for a parameter draw (it enters every
    step), N for a step draw (one independent draw a step)"""
    weight = (("pn", WIDE_N ** 2), ("pu", WIDE_N ** 2 / 12.0), ("sn", WIDE_N), ("su", WIDE_N / 12.0))
    return math.fsum(w * wide_coef(kind, i) ** 2 for (kind, w), mask in zip(weight, words) for i in range(nd) if (mask >> i) & 1)


def wide_exact(groups, nd=WIDE_D):
    """(Var J, the exact S_g = T_g of every group)"""
    full = (1 << nd) - 1
    var = wide_share((full,) * 4, nd)
    return var, np.array([wide_share(g.words, nd) / var for g in groups])


def wide_groups():
    """the sixteen groups of the wide tests: in each of the four words bits 31, 32 and 63 alone (the last bit of the low half, the first and
    the last of the high half); step normal 33 and parameter normal 33 alone, so that Box-Muller block 16 of a step and of the parameters
    gives its two outputs (32, 33) to different groups; step uniforms 24 .. 30 and 33 .. 36, one mask with bits in both halves (31 and 32
    are taken); the empty group last"""
    G, kinds, out = rat.SobolGroup, ("param_normals", "param_uniforms", "step_normals", "step_uniforms"), []
    for kind, short in zip(kinds, ("pn", "pu", "sn", "su")):
        out += [G(**{kind: (b,)}, name=f"{short}{b}") for b in (31, 32, 63)]
    out += [G(step_normals=(33,), name="sn33"), G(param_normals=(33,), name="pn33"),
            G(step_uniforms=tuple(range(24, 31)) + tuple(range(33, 37)), name="su24-30,33-36"), G(name="empty")]
    return out


# ---- the pendulum of user_params_model on all base samples at once ------------------------------------------------------------------------
def pend_costs(c, hook, groups, K, seed_a, seed_b, p=None):
    """case_costs(c = user_params_model.case("pend"), hook, closed=True, ...) with every base sample of a row rolled out at once: the same
    operations in the same order on [K] arrays (the feedback product is NumPy's matmul, as there)"""
    A, B = (streams(s, K, c.N, c.npn, 0, pm.PARAM_NORMALS, pm.PARAM_UNIFORMS) for s in (seed_a, seed_b))
    p = c.p if p is None else p
    x_nom, l, L = c.args(True)
    rows = []
    with np.errstate(invalid="ignore"):
        for words in variants(groups):
            z = mixed(A, B, words)
            q = pm.np_params(hook, p, z["pn"], z["pu"], **c.idx)
            pv = q.T                                                  # pv[i]: parameter i of every base sample
            x, tot = np.repeat(x_nom[0][None], K, axis=0), np.zeros(K)
            for t in range(c.N):
                u = l[t] + (x - x_nom[t]) @ L[t].T
                tot = tot + um.pend_c(t, x.T, u.T, pv)
                x = rn.pend_f(x, u, pv) + rn.pend_state_noise(t, x, u, _Draws(z["sn"][:, t]), pv)
            cost = tot + um.pend_h(x.T, pv)
            cost[np.isnan(q).any(axis=1)] = np.nan
            rows.append(cost)
    return np.array(rows)


class _Draws:
    """rng.normal() over the columns of one step's normals [K, P]"""

    def __init__(self, z):
        self.z, self.i = z, 0

    def normal(self):
        self.i += 1
        return self.z[:, self.i - 1]


def nan_thresholds(c, K, seed_a, seed_b):
    """the larger first parameter normal of the two streams per base sample: under the "nan" hook with a group that holds parameter normal
    0, base sample k survives in every row where this is at most the threshold p[pnan]"""
    return np.maximum(pm.gen_draws(seed_a, K, pm.PARAM_NORMALS, 0)[0][:, 0], pm.gen_draws(seed_b, K, pm.PARAM_NORMALS, 0)[0][:, 0])
