"""Model parameters drawn per rollout (rat_user_params, include/ratilqr.h "source models"; csrc/source_params.h) -- test aid shared by
tests/test_cpu_user_params.py, tests/test_gpu_user_params.py and tools/policy_user_params_bench.py: the test hooks as HIP text and in
NumPy, the sources they hang on, the parameter-draw keying (injected rows, or Philox4x32-10 under the step word 0xFFFFFFFF, with the
Python Philox of tests/rare_event_model.py), and a NumPy restatement of rat_src_user_noisy_rollout with a parameter vector per rollout,
after tests/user_noise_model.np_rollouts.

A source model whose rollouts draw parameters has at most 32 of them, so the 12 x 4 and 5 x 3 cases are an LQ + cubic source of their
own, LQC, with structured matrices (a ring coupling, a two-tap input map) behind fourteen parameters, twelve (RAT_N) normals and a
uniform per step like tests/user_noise_model.LQ_MIX, whose several hundred tabulated parameters are beyond that limit.

The hooks of the cases scale two parameters by 1 + 0.2 z and shift one by a uniform, under `#pragma clang fp contract(off)`, so that a
parameter is one rounded product, sum and product: NumPy gives the device's bits.

The functions of the sources that read p are under the same pragma.  A sum of two products, such as the pendulum sampler's
p[1] |x[1]| z1 + p[2] z2, can be contracted into a fused multiply-add around either product, and which one the compiler takes depends on
whether p sits in scalar registers (one p for the wavefront: sampling off) or in vector registers (a q per lane: sampling on) -- read in
the ISA of both compiles.  The language leaves those bits open, so "a hook that leaves q alone returns the sampling-off bits" can only be
asked of a source whose bits are defined; with contraction off in the user's functions they are."""
import numpy as np

import ratilqr.jl_amd as rat
import user_noise_model as um
from rare_event_model import philox4x32_10
from source_pets_models import SlotRng

# ---- the hooks ------------------------------------------------------------------------------------------------------------------------------
HOOK_HEAD = r"""
#define RAT_USER_PARAMS
template <class R> __device__ void rat_user_params(R &rng, const double *p, double *q) {
#pragma clang fp contract(off)
"""
DRAW3 = "    const double z0 = rng.normal();\n    const double z1 = rng.normal();\n    const double v = rng.uniform();\n"
BODIES = {
    "identity": "",
    "scale": DRAW3 + "    q[PI0] = p[PI0] * (1.0 + 0.2 * z0);\n    q[PI1] = p[PI1] * (1.0 + 0.2 * z1);\n    q[PI2] = p[PI2] + PSH * v;\n",
    # the same, and a NaN where the first normal is beyond p[PNAN]: a DomainError of the hook
    "nan": DRAW3 + "    q[PI0] = p[PI0] * (1.0 + 0.2 * z0);\n    q[PI1] = p[PI1] * (1.0 + 0.2 * z1);\n    q[PI2] = p[PI2] + PSH * v;\n"
           "    if (z0 > p[PNAN]) q[PI0] = sqrt(p[PNAN] - z0);\n",
    # one normal more than the cases declare
    "over": DRAW3 + "    q[PI0] = p[PI0] * (1.0 + 0.2 * z0) + 0.0 * rng.normal();\n",
}
PARAM_NORMALS, PARAM_UNIFORMS = 2, 1


def source(base, name, pi0, pi1, pi2, psh, pnan=0):
    """the base source with the hook `name` behind it: entries pi0, pi1 are scaled, pi2 is shifted by psh v, p[pnan] is the NaN threshold"""
    defs = f"#define PI0 {pi0}\n#define PI1 {pi1}\n#define PI2 {pi2}\n#define PSH ({psh!r})\n#define PNAN {pnan}\n"
    return base + defs + HOOK_HEAD + BODIES[name] + "}\n"


def np_params(name, p, zpn, zpu, pi0, pi1, pi2, psh, pnan=0):
    """q [K, n_params] of the hook `name` on the parameter draws zpn [K, 2], zpu [K, 1]: the device's bits"""
    p = np.asarray(p, float)
    q = np.repeat(p[None], zpn.shape[0], axis=0)
    if name == "identity":
        return q
    q[:, pi0] = p[pi0] * (1.0 + 0.2 * zpn[:, 0])
    q[:, pi1] = p[pi1] * (1.0 + 0.2 * zpn[:, 1])
    q[:, pi2] = p[pi2] + psh * zpu[:, 0]
    if name == "nan":
        q[zpn[:, 0] > p[pnan], pi0] = np.nan
    return q


# ---- the keying of the generator ------------------------------------------------------------------------------------------------------------
STEP_WORD = 0xFFFFFFFF                                                # the step word of the parameter draws: no step t < N uses it


def _u01(hi, lo):
    return ((hi.astype(np.uint64) << np.uint64(32) | lo.astype(np.uint64)) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def gen_draws(seed, K, pn, pu, j0=0):
    """(zpn [K, pn], zpu [K, pu]) of rollouts j0 .. j0 + K - 1 as csrc/source_params.h draws them under `seed`: Philox4x32-10, key (seed
    lo, seed hi), counter (g lo, g hi, 0xFFFFFFFF, i / 2) for normals (Box-Muller on (u01(r0, r1), u01(r2, r3)): normal 2q, 2q + 1) and
    (g lo, g hi, 0xFFFFFFFF, 0x80000000 | i / 2) for uniforms (u01(r0, r1), u01(r2, r3))"""
    g = np.arange(j0, j0 + K, dtype=np.uint64)
    lo, hi = g & np.uint64(0xFFFFFFFF), g >> np.uint64(32)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    t = np.full(K, STEP_WORD, dtype=np.uint64)
    zn, zu = np.zeros((K, pn)), np.zeros((K, pu))
    for b in range((pn + 1) // 2):
        r0, r1, r2, r3 = philox4x32_10(lo, hi, t, np.full(K, b, dtype=np.uint64), k0, k1)
        u1, u2 = _u01(r0, r1), _u01(r2, r3)
        rad = np.sqrt(-2.0 * np.log(1.0 - u1))
        pair = (rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2))
        for s in range(2):
            if 2 * b + s < pn:
                zn[:, 2 * b + s] = pair[s]
    for b in range((pu + 1) // 2):
        r0, r1, r2, r3 = philox4x32_10(lo, hi, t, np.full(K, 0x80000000 | b, dtype=np.uint64), k0, k1)
        pair = (_u01(r0, r1), _u01(r2, r3))
        for s in range(2):
            if 2 * b + s < pu:
                zu[:, 2 * b + s] = pair[s]
    return zn, zu


# ---- the LQ + cubic source with fourteen parameters -----------------------------------------------------------------------------------------
# p: 0 a | 1 b (ring coupling) | 2 g (input gain) | 3 kappa | 4 qx | 5 ru | 6 l1u | 7 qf | 8 weight of the second component | 9 its mean |
#    10 its scale | 11 the first component's scale | 12 an obstacle's radius (EVENT) | 13 the NaN threshold of the "nan" hook
CONTRACT_OFF = "#pragma clang fp contract(off)\n"
LQC = r"""
constexpr int NX = RAT_N, NU = RAT_M;
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) {
#pragma clang fp contract(off)
    for (int i = 0; i < NX; ++i)
        xn[i] = p[0] * x[i] + p[1] * (x[(i + 1) % NX] - x[(i + NX - 1) % NX]) + p[2] * (u[i % NU] - 0.5 * u[(i + 1) % NU]) + p[3] * (x[i] * x[i] * x[i]);
}
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) {
#pragma clang fp contract(off)
    T sx = 0.0, su = 0.0, s1 = 0.0;
    for (int i = 0; i < NX; ++i) sx += x[i] * x[i];
    for (int i = 0; i < NU; ++i) { su += u[i] * u[i]; s1 += fabs(u[i]); }
    return 0.5 * p[4] * sx + 0.5 * p[5] * su + p[6] * s1 + 0.1 * (x[0] * u[0]);
}
template <class T> __device__ T rat_user_h(const T *x, const double *p) {
#pragma clang fp contract(off)
    T sx = 0.0;
    for (int i = 0; i < NX; ++i) sx += x[i] * x[i];
    return 0.5 * p[7] * sx;
}
""" + um.NOISE_HEAD + CONTRACT_OFF + r"""
    const bool second = rng.uniform() < p[8];
    double z[NX];
    for (int i = 0; i < NX; ++i) z[i] = rng.normal();
    for (int i = 0; i < NX; ++i) w[i] = second ? p[9] + p[10] * z[i] : p[11] * (z[i] + 0.5 * z[(i + 1) % NX]);
}
"""
LQC_P = np.array([0.8, 0.15, 0.4, -0.01, 1.0, 0.1, 0.2, 2.0, 0.3, 0.2, 0.25, 0.15, 0.6, 1e300])


def lqc_f(x, u, p):
    n, m = x.size, u.size
    i = np.arange(n)
    return p[0] * x + p[1] * (np.roll(x, -1) - np.roll(x, 1)) + p[2] * (u[i % m] - 0.5 * u[(i + 1) % m]) + p[3] * x ** 3


lqc_c = lambda k, x, u, p: 0.5 * p[4] * (x @ x) + 0.5 * p[5] * (u @ u) + p[6] * np.abs(u).sum() + 0.1 * (x[0] * u[0])
lqc_h = lambda x, p: 0.5 * p[7] * (x @ x)


def lqc_noise(k, x, u, rng, p):
    second = rng.uniform() < p[8]
    z = np.array([rng.normal() for _ in range(x.size)])
    return p[9] + p[10] * z if second else p[11] * (z + 0.5 * np.roll(z, -1))


# the pendulum of tests/user_noise_model.PEND_STATE, its sampler with contraction off: p = dt | s (state-dependent scale) | floor | an
# obstacle's radius | the NaN threshold
_body = um.PEND_STATE[len(um.PEND_FCH + um.NOISE_HEAD):]
assert um.PEND_STATE.startswith(um.PEND_FCH + um.NOISE_HEAD)
PEND = um.PEND_FCH + um.NOISE_HEAD + CONTRACT_OFF + _body
PEND_P = np.array([0.1, 0.3, 0.05, 0.9, 1e300])

# rat_user_event of the replay and rare-event tests: inside an obstacle about the origin of the first coordinate whose radius is p[EVP]
EVENT = r"""
#define RAT_USER_EVENT
__device__ void rat_user_event(int k, const double *x, const double *u, double *g, const double *p) {
    g[0] = p[EVP] - fabs(x[0]);
}
"""


# ---- the rollouts in NumPy ------------------------------------------------------------------------------------------------------------------
def np_rollouts(f, c, h, noise, q, x_nom, l, L, K, zn, zu, npn, npu, j0=0):
    """user_noise_model.np_rollouts with the parameters q[j] of rollout j0 + j in place of one p: (cost (K,), x (K, N+1, n), u (K, N, m)) of
    rollouts j0 .. j0 + K - 1 on the injected step draws zn / zu (flat, rollout j0 first).  A NaN in q[j] is that rollout's DomainError:
    a NaN cost (the trajectory is whatever the NaN left of it)."""
    l = np.asarray(l, float)
    N, m = l.shape
    x_nom = np.asarray(x_nom, float)
    x0 = x_nom if L is None else x_nom[0]
    rng = SlotRng(zn, zu, npn, npu)
    cost, xs, us = np.zeros(K), np.zeros((K, N + 1, x0.size)), np.zeros((K, N, m))
    with np.errstate(invalid="ignore"):
        for j in range(K):
            p = q[j0 + j]
            x, tot = x0.copy(), 0.0
            for t in range(N):
                u = l[t] if L is None else l[t] + L[t] @ (x - x_nom[t])
                xs[j, t], us[j, t] = x, u
                tot += c(t, x, u, p)
                rng.at(j, t, N)
                x = f(x, u, p) + noise(t, x, u, rng, p)
            xs[j, N] = x
            cost[j] = np.nan if np.isnan(p).any() else tot + h(x, p)
    return cost, xs, us


# ---- the cases of the tests -----------------------------------------------------------------------------------------------------------------
class Case:
    """A source with a sampler, its NumPy functions, a policy, injected step draws and injected parameter draws for K rollouts.  The hook
    scales the sampler's two scales (the pendulum: s and the floor; LQC: the two components') and shifts a dynamics coefficient (dt; a)."""

    def __init__(self, name):
        r = np.random.default_rng(11)
        self.name = name
        if name == "pend":
            self.n, self.m, self.N, self.K, self.npn, self.npu = 2, 1, 8, 256, 3, 0
            self.base, self.p = PEND, PEND_P.copy()
            self.idx = dict(pi0=1, pi1=2, pi2=0, psh=0.02, pnan=4)
            self.evp = 3
            self.W = 1e-2 * np.eye(2)
            self.fns = (um.pend_f, um.pend_c, um.pend_h, um.pend_state_noise)
            x_nom, l, L = um.pend_policy(self.N)
            self.policy = (x_nom, l, 4.0 * L)
        else:
            self.n, self.m = (12, 4) if name == "lq12" else (5, 3)
            self.N, self.K, self.npn, self.npu = 4, (128 if name == "lq12" else 65), self.n, 1
            self.base, self.p = LQC, LQC_P.copy()
            self.idx = dict(pi0=10, pi1=11, pi2=0, psh=0.1, pnan=13)
            self.evp = 12
            self.W = 0.02 * np.eye(self.n)
            self.fns = (lqc_f, lqc_c, lqc_h, lqc_noise)
            self.policy = (0.5 * r.standard_normal((self.N + 1, self.n)), 0.8 * r.standard_normal((self.N, self.m)),
                           0.1 * r.standard_normal((self.N, self.m, self.n)))
        self.zn = r.standard_normal((self.K, self.N, self.npn))
        self.zu = r.random((self.K, self.N, self.npu)) if self.npu else None
        self.zpn = r.standard_normal((self.K, PARAM_NORMALS))
        self.zpu = r.random((self.K, PARAM_UNIFORMS))

    def source(self, hook, event=False):
        """the case's source with the hook `hook` (None: without RAT_USER_PARAMS), and with EVENT"""
        src = self.base if hook is None else source(self.base, hook, **self.idx)
        return src + (f"#define EVP {self.evp}\n" + EVENT if event else "")

    def problem(self, hook, p=None, event=False, N=None):
        return rat.DeviceSourceProblem(self.source(hook, event), self.n, self.m, self.N if N is None else N, self.W,
                                       params=self.p if p is None else p)

    def args(self, closed):
        x_nom, l, L = self.policy
        return (x_nom, l, L) if closed else (x_nom[0], l, None)

    def q(self, hook, p=None, zpn=None, zpu=None):
        """the parameters of the K rollouts (of as many as the draws hold) under the hook"""
        return np_params(hook, self.p if p is None else p, self.zpn if zpn is None else zpn, self.zpu if zpu is None else zpu, **self.idx)

    def model(self, hook, closed, p=None, K=None, j0=0):
        """the NumPy rollouts j0 .. j0 + K - 1 on zn / zu under the parameters of the hook (None: the nominal ones)"""
        K = self.K - j0 if K is None else K
        q = self.q("identity" if hook is None else hook, p)
        zn = self.zn[j0:j0 + K].ravel()
        zu = None if self.zu is None else self.zu[j0:j0 + K].ravel()
        return np_rollouts(*self.fns, q, *self.args(closed), K, zn, zu, self.npn, self.npu, j0=j0)

    def user_noise(self, **kw):
        return rat.UserNoise(self.npn, self.npu, **kw)

    def sampling(self, injected=True):
        return rat.ParamSampling(PARAM_NORMALS, PARAM_UNIFORMS, zpn=self.zpn, zpu=self.zpu) if injected else \
            rat.ParamSampling(PARAM_NORMALS, PARAM_UNIFORMS)


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


CASE_NAMES = ("pend", "lq12", "lq5")

# ---- the closed form of tests/test_cpu_user_params.py: x+ = a x + w without process noise, cost sum_t x_t^2 (h = x_N^2), a ~ N(a0, s^2) ---
SCALAR = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) { xn[0] = p[0] * x[0]; }
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) { return x[0] * x[0]; }
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return x[0] * x[0]; }
""" + um.NOISE_HEAD + "    w[0] = 0.0 * rng.normal();\n}\n" + r"""
#define RAT_USER_PARAMS
template <class R> __device__ void rat_user_params(R &rng, const double *p, double *q) { q[0] = p[0] + p[1] * rng.normal(); }
"""


def normal_moment(mu, s, k):
    """E a^k of a ~ N(mu, s^2)"""
    m = [1.0, mu]
    for i in range(2, k + 1):
        m.append(mu * m[i - 1] + (i - 1) * s * s * m[i - 2])
    return m[k]


def scalar_mean_cost(a0, s, x0, N):
    """E sum_{t=0}^{N} x_t^2 with x_t = a^t x_0"""
    return x0 * x0 * sum(normal_moment(a0, s, 2 * t) for t in range(N + 1))
