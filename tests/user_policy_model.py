"""The controller the user writes (rat_user_policy, include/ratilqr.h "source models") -- test aid shared by tests/test_cpu_user_policy.py,
tests/test_gpu_user_policy.py and tools/policy_user_policy_bench.py: the test hooks as HIP text and in NumPy, the sources they hang on,
and a NumPy restatement of the two Monte-Carlo rollouts of a source model with the hook in place (rat_src_user_noisy_rollout of
csrc/source_user_noise.h on injected draws, rat_src_noisy_rollout of csrc/source_noisy.h on injected normals), after
tests/user_noise_model.np_rollouts: the affine law, then the hook, then everything that reads u.

Every hook is built from single IEEE operations -- fmin / fmax, one subtraction, one addition, a comparison, a look-up in p -- so the
compiler has nothing to contract and NumPy applies the device's bits to the u it is given.  A hook reads its own parameters at
q = p + POFF, behind the model's: q[0] the clamp, q[1] the rate limit, q[2] the state threshold of the NaN hook."""
import numpy as np

import ratilqr.jl_amd as rat
import user_event_model as ue
import user_noise_model as um
from source_pets_models import SlotRng, lq_params

HOOK_HEAD = r"""
#define RAT_USER_POLICY
__device__ void rat_user_policy(int k, const double *x, const double *u_prev, double *u, const double *p) {
    const double *q = p + POFF;
"""
BODIES = {
    "identity": "",
    "clamp": "    for (int i = 0; i < RAT_M; ++i) u[i] = fmin(fmax(u[i], -q[0]), q[0]);\n",
    "rate": "    for (int i = 0; i < RAT_M; ++i) {\n"
            "        const double d = fmin(fmax(u[i] - u_prev[i], -q[1]), q[1]);\n"
            "        u[i] = fmin(fmax(u_prev[i] + d, -q[0]), q[0]);\n"
            "    }\n",
    # the clamp, and a NaN where the first state is beyond q[2]: a DomainError of the hook
    "nan": "    for (int i = 0; i < RAT_M; ++i) u[i] = fmin(fmax(u[i], -q[0]), q[0]);\n"
           "    if (x[0] > q[2]) u[0] = sqrt(q[2] - x[0]);\n",
}
WRONG_SIGNATURE = HOOK_HEAD.replace("const double *u_prev, ", "")       # (four parameters: the kernels' call does not match)
N_HOOK_PARAMS = 3


def source(base, poff, name):
    """the base source with the hook `name` behind it, its parameters at p + poff (a number, or an expression of the source's constants)"""
    return base + f"#define POFF ({poff})\n" + HOOK_HEAD + BODIES[name] + "}\n"


def np_hook(name):
    """rat_user_policy of BODIES[name] in NumPy: (k, x, u_prev, u, q) -> the applied u"""
    def hook(k, x, u_prev, u, q):
        if name == "identity":
            return u
        if name == "rate":
            d = np.fmin(np.fmax(u - u_prev, -q[1]), q[1])
            return np.fmin(np.fmax(u_prev + d, -q[0]), q[0])
        v = np.fmin(np.fmax(u, -q[0]), q[0])
        if name == "nan" and x[0] > q[2]:
            v = v.copy()
            v[0] = np.nan
        return v
    return hook


# ---- the rollouts in NumPy ---------------------------------------------------------------------------------------------------------------
def np_rollouts(f, c, h, noise, p, x_nom, l, L, K, zn=None, zu=None, npn=0, npu=0, hook=None, q=None, Wchol=None, z=None):
    """(cost (K,), x (K, N+1, n), u (K, N, m)): user_noise_model.np_rollouts with the hook between the affine law and everything that
    reads u -- the stored control, c, the sampler, f.  noise a sampler of user_noise_model on the injected draws zn / zu, or None: the
    disturbance is Wchol z[j, t] (rat_src_noisy_rollout; Wchol (n, n) or (N, n, n)).  hook None: the hookless source."""
    l = np.asarray(l, float)
    N, m = l.shape
    x_nom = np.asarray(x_nom, float)
    x0 = x_nom if L is None else x_nom[0]
    rng = SlotRng(zn, zu, npn, npu) if noise is not None else None
    cost, xs, us = np.zeros(K), np.zeros((K, N + 1, x0.size)), np.zeros((K, N, m))
    with np.errstate(invalid="ignore"):
        for j in range(K):
            x, tot, u_prev = x0.copy(), 0.0, np.zeros(m)
            for t in range(N):
                u = l[t] if L is None else l[t] + L[t] @ (x - x_nom[t])
                if hook is not None:
                    u = hook(t, x, u_prev, u, q)
                u_prev = u
                xs[j, t], us[j, t] = x, u
                tot += c(t, x, u, p)
                if noise is not None:
                    rng.at(j, t, N)
                    w = noise(t, x, u, rng, p)
                else:
                    w = (Wchol[t] if Wchol.ndim == 3 else Wchol) @ z[j, t]
                x = f(x, u, p) + w
            xs[j, N] = x
            cost[j] = tot + h(x, p)
    return cost, xs, us


def beyond(us, limit):
    """the share of the (rollout, step) pairs at which some control lies outside [-limit, limit]"""
    return float((np.abs(us) > limit).any(axis=2).mean())


# ---- the cases of the tests: name -> everything a test needs ---------------------------------------------------------------------------
class Case:
    """A source with a sampler, its NumPy functions, a closed-loop policy, injected draws for K rollouts and the hook's parameters
    q = (clamp, rate limit, NaN threshold).  The clamp is the median over (rollout, step) of the largest |u_i| the hookless NumPy model
    applies under the closed-loop policy -- the smaller of the two medians, under the sampler and under chol(W) z -- so the hookless
    policy leaves the limits in at least half of the pairs under either disturbance; the rate limit is half
    the clamp; the NaN threshold is out of reach (set_nan_rollout moves it)."""

    def __init__(self, name):
        r = np.random.default_rng(5)
        self.name = name
        if name == "pend":
            self.n, self.m, self.N, self.K, self.npn, self.npu = 2, 1, 8, 256, 3, 0
            self.base, self.poff = um.PEND_STATE, 3
            self.p_model = np.array([0.1, 0.3, 0.05])              # (a sampler strong enough for the feedback term to move u)
            self.W = 1e-2 * np.eye(2)
            self.fns = (um.pend_f, um.pend_c, um.pend_h, um.pend_state_noise)
            x_nom, l, L = um.pend_policy(self.N)
            self.policy = (x_nom, l, 4.0 * L)
        else:
            self.n, self.m = (12, 4) if name == "lq12" else (5, 3)
            self.N, self.K, self.npn, self.npu = 4, (128 if name == "lq12" else 65), self.n, 1
            self.gp = um.lq_generative(n=self.n, m=self.m, Nh=self.N)
            self.base, self.poff = um.LQ_MIX, "ohi + 1"
            self.p_model = lq_params(self.gp)
            self.W = self.gp.nchol @ self.gp.nchol.T
            mdl = um.LqNumpy(self.gp)
            self.fns = (mdl.f, mdl.c, mdl.h, mdl.noise)
            self.policy = (r.standard_normal((self.N + 1, self.n)), 0.8 * r.standard_normal((self.N, self.m)),
                           0.1 * r.standard_normal((self.N, self.m, self.n)))
        self.zn = r.standard_normal((self.K, self.N, self.npn))
        self.zu = r.random((self.K, self.N, self.npu)) if self.npu else None
        self.z = r.standard_normal((self.K, self.N, self.n))         # rat_policy_evaluate's injected normals
        self.Wchol = np.linalg.cholesky(self.W)
        self.q = np.array([0.0, 0.0, 1e300])
        _, _, us = self.model(None, True)
        _, _, ug = self.model(None, True, gaussian=True)
        clamp = float(min(np.median(np.abs(us).max(axis=2)), np.median(np.abs(ug).max(axis=2))))
        self.q = np.array([clamp, 0.5 * clamp, 1e300])
        self.hookless_u = us

    def params(self, q=None):
        return np.concatenate([self.p_model, self.q if q is None else q])

    def problem(self, hook, q=None, base=None):
        """the DeviceSourceProblem of the case with the hook `hook` (None: the same source without RAT_USER_POLICY; the parameters keep
        their places)"""
        base = self.base if base is None else base
        src = base if hook is None else source(base, self.poff, hook)
        return rat.DeviceSourceProblem(src, self.n, self.m, self.N, self.W, params=self.params(q))

    def args(self, closed):
        x_nom, l, L = self.policy
        return (x_nom, l, L) if closed else (x_nom[0], l, None)

    def model(self, hook, closed, gaussian=False, q=None):
        """the NumPy rollouts under the user's sampler on zn / zu, or (gaussian) under chol(W) z"""
        f, c, h, noise = self.fns
        x_nom, l, L = self.args(closed)
        q = self.q if q is None else q
        hk = None if hook is None else np_hook(hook)
        p = self.params(q)
        if gaussian:
            return np_rollouts(f, c, h, None, p, x_nom, l, L, self.K, hook=hk, q=q, Wchol=self.Wchol, z=self.z)
        return np_rollouts(f, c, h, noise, p, x_nom, l, L, self.K, self.zn.ravel(), None if self.zu is None else self.zu.ravel(),
                           self.npn, self.npu, hook=hk, q=q)

    def user_noise(self, **kw):
        return rat.UserNoise(self.npn, self.npu, **kw)


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


CASE_NAMES = ("pend", "lq12", "lq5")


# ---- a sampler that reads u, and an event on u ---------------------------------------------------------------------------------------------
# the pendulum with a disturbance that grows with the control: what rat_user_noise is handed shows in w
PEND_UDEP = um.PEND_FCH + um.NOISE_HEAD + r"""
    const double z0 = rng.normal();
    const double z1 = rng.normal();
    w[0] = p[1] * z0;
    w[1] = p[2] * (1.0 + fabs(u[0])) * z1;
}
"""


def udep_noise(k, x, u, rng, p):
    """PEND_UDEP's sampler on (K, .) arrays (tests/test_gpu_wc_disturbance.source_w's calling convention)"""
    z0, z1 = rng.normal(), rng.normal()
    return np.stack([p[1] * z0, p[2] * (1.0 + np.abs(u[:, 0])) * z1], axis=1)


U_EVENT = "    g[0] = u[0] - q[0];\n"                                  # rat_user_event: the first control above q[0] (p + EVOFF)


def with_u_event(src, evoff):
    return ue.source(src, "half", evoff, body=U_EVENT)
