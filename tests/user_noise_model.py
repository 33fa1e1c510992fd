"""Source models with a noise sampler of their own (rat_user_noise, include/ratilqr.h "source models") shared by
tests/test_cpu_user_noise.py, tests/test_gpu_user_noise.py and tools/policy_noise_bench.py, and a NumPy restatement of
rat_src_user_noisy_rollout (csrc/source_user_noise.h): the feedback law, c(0) .. c(N-1) then h, x_{t+1} = f(x_t, u_t) + w_t, the draws
read by the slot layout of include/ratilqr.h (SlotRng of tests/source_pets_models.py) or taken from a NumPy generator."""
import numpy as np

import ratilqr.jl_amd as rat
from source_pets_models import LQ, SlotRng, lq_params

# ---- the pendulum of tests/test_gpu_source_model.py; p[0] = dt, the rest belongs to the sampler -------------------------------------
PEND_FCH = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) {
    const double dt = p[0];
    xn[0] = x[0] + dt * x[1];
    xn[1] = x[1] + dt * (-sin(x[0]) - 0.1 * x[1] + u[0]);
}
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) {
    return 0.5 * (x[0] * x[0] + x[1] * x[1]) + 0.05 * (u[0] * u[0]) + 0.01 * k * x[0];
}
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return 2.0 * (x[0] * x[0] + x[1] * x[1]); }
"""
NOISE_HEAD = r"""
#define RAT_USER_NOISE
template <class R> __device__ void rat_user_noise(int k, const double *x, const double *u, R &rng, double *w, const double *p) {
"""
# state-dependent: w = p |x| z, and a floor on the velocity from a third normal (an odd count: the generator's spare Box-Muller output)
PEND_STATE = PEND_FCH + NOISE_HEAD + r"""
    const double z0 = rng.normal();
    const double z1 = rng.normal();
    const double z2 = rng.normal();
    w[0] = p[1] * fabs(x[0]) * z0;
    w[1] = p[1] * fabs(x[1]) * z1 + p[2] * z2;
}
"""
PEND_STATE_DIMS = dict(n=2, m=1, normals_per_step=3, uniforms_per_step=0)
PEND_STATE_P = [0.1, 0.2, 0.02]
# the Gaussian special case with a diagonal W: w_i = s_i z_i
PEND_DIAG = PEND_FCH + NOISE_HEAD + r"""
    for (int i = 0; i < 2; ++i) w[i] = p[1 + i] * rng.normal();
}
"""
PEND_DIAG_DIMS = dict(n=2, m=1, normals_per_step=2, uniforms_per_step=0)
# NaN beyond three standard deviations: a DomainError of the sampler
PEND_NAN = PEND_FCH + NOISE_HEAD + r"""
    const double z = rng.normal();
    w[1] = (z > 3.0) ? sqrt(3.0 - z) : p[1] * z;
}
"""
# one normal more than PEND_DIAG_DIMS declares
PEND_OVER = PEND_FCH + NOISE_HEAD + r"""
    for (int i = 0; i < 2; ++i) w[i] = p[1 + i] * rng.normal();
    w[0] += 0.0 * rng.normal();
}
"""
# a two-component mixture chosen by one uniform: N(0, diag(p1, p2)^2), or with probability p[3] a kick N(p[4], (3 p2)^2) on the velocity
PEND_MIX = PEND_FCH + NOISE_HEAD + r"""
    const bool kick = rng.uniform() < p[3];
    const double z0 = rng.normal();
    const double z1 = rng.normal();
    w[0] = p[1] * z0;
    w[1] = kick ? p[4] + 3.0 * p[2] * z1 : p[2] * z1;
}
"""
PEND_MIX_DIMS = dict(n=2, m=1, normals_per_step=2, uniforms_per_step=1)
# the pendulum without a sampler
PEND_PLAIN = PEND_FCH


def pend_f(x, u, p):
    return np.array([x[0] + p[0] * x[1], x[1] + p[0] * (-np.sin(x[0]) - 0.1 * x[1] + u[0])])


pend_c = lambda k, x, u, p: 0.5 * (x[0] * x[0] + x[1] * x[1]) + 0.05 * (u[0] * u[0]) + 0.01 * k * x[0]
pend_h = lambda x, p: 2.0 * (x[0] * x[0] + x[1] * x[1])


def pend_policy(N):
    """A fixed closed-loop policy for the pendulum: a nominal trajectory that is not the rollout of l, so the feedback term works."""
    rng = np.random.default_rng(17)
    x_nom = np.array([1.0, 0.0]) + 0.05 * rng.standard_normal((N + 1, 2))
    return x_nom, 0.2 * rng.standard_normal((N, 1)), -0.3 * np.abs(rng.standard_normal((N, 1, 2)))


def pend_state_noise(k, x, u, rng, p):
    z0, z1, z2 = rng.normal(), rng.normal(), rng.normal()
    return np.array([p[1] * np.abs(x[0]) * z0, p[1] * np.abs(x[1]) * z1 + p[2] * z2])


def pend_nan_noise(k, x, u, rng, p):
    z = rng.normal()
    return np.array([0.0, np.nan if z > 3.0 else p[1] * z])


# ---- the LQ + cubic family of tests/source_pets_models.py as an iLEQG source: its offsets, c and h, a deterministic f and the true-model
# mixture (one selector uniform, then n normals) as the sampler -------------------------------------------------------------------------
_cut0, _cut1 = LQ.index("__device__ void rat_user_f_stochastic"), LQ.index("template <class T> __device__ T rat_user_c")
LQ_F = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) {
    for (int i = 0; i < NX; ++i) {
        T a = 0.0;
        for (int j = 0; j < NX; ++j) a += p[oA + i * NX + j] * x[j];
        for (int b = 0; b < NU; ++b) a += p[oB + i * NU + b] * u[b];
        xn[i] = a + p[okap] * (x[i] * x[i] * x[i]);
    }
}
"""
LQ_FCH = LQ[:_cut0] + LQ_F + LQ[_cut1:]
LQ_MIX = LQ_FCH + NOISE_HEAD + r"""
    const bool second = rng.uniform() < p[otw];
    double z[NX];
    for (int i = 0; i < NX; ++i) z[i] = rng.normal();
    const double *mean = p + (second ? otm : onm), *L = p + (second ? otc : onc);
    for (int i = 0; i < NX; ++i) {
        double a = 0.0;
        for (int j = 0; j <= i; ++j) a += L[i * NX + j] * z[j];
        w[i] = mean[i] + a;
    }
}
"""
# the Gaussian chol(W) z: the model component alone, no mean
LQ_GAUSS = LQ_FCH + NOISE_HEAD + r"""
    double z[NX];
    for (int i = 0; i < NX; ++i) z[i] = rng.normal();
    for (int i = 0; i < NX; ++i) {
        double a = 0.0;
        for (int j = 0; j <= i; ++j) a += p[onc + i * NX + j] * z[j];
        w[i] = a;
    }
}
"""


def lq_generative(n=12, m=4, Nh=3, kappa=-0.01):
    """rich_problem of tests/test_gpu_pets.py at horizon Nh: the tables lq_params packs."""
    r = np.random.default_rng(8)
    A = 0.9 * np.linalg.qr(r.standard_normal((n, n)))[0]
    cov = 0.02 * np.eye(n) + 0.01 * np.outer(np.ones(n), np.ones(n)) / n
    return rat.LQGenerativeProblem(A, r.standard_normal((n, m)) / np.sqrt(n), Nh, ("gaussian", 0.05 * r.standard_normal(n), cov),
                                   Q=np.eye(n), R=0.1 * np.eye(m), P=0.02 * r.standard_normal((m, n)), qv=0.1 * r.standard_normal(n),
                                   rv=0.1 * r.standard_normal(m), q0=0.5, Qf=2 * np.eye(n), qvf=0.1 * r.standard_normal(n), q0f=1.0,
                                   kappa=kappa, l1u=0.2, true_noise=(0.3, 0.2 * np.ones(n), 0.05 * np.eye(n)))


def lq_source_problem(gp, source=LQ_MIX, mean=True):
    """DeviceSourceProblem of the LQ source for the generative problem gp; W = the model component's covariance (what rat_policy_evaluate
    draws from).  mean=False zeroes the model component's mean, so that chol(W) z is the whole model noise."""
    p = lq_params(gp)
    if not mean:
        n, m = gp.n, gp.m
        onm = 3 * n * n + 2 * n * m + m * m + 2 * n + m + 5
        assert np.array_equal(p[onm:onm + n], gp.nmean)
        p[onm:onm + n] = 0.0
    return rat.DeviceSourceProblem(source, gp.n, gp.m, gp.N, gp.nchol @ gp.nchol.T, params=p)


class LqNumpy:
    """f, c, h and the mixture sampler of LQ_MIX in NumPy, from the generative problem's tables."""

    def __init__(self, gp):
        self.gp, self.lq = gp, gp.lq
        self.q0 = float(np.asarray(gp.lq.q0).ravel()[0])

    def f(self, x, u, p):
        lq = self.lq
        return lq.A @ x + lq.B @ u + lq.kappa * x ** 3

    def c(self, k, x, u, p):
        lq = self.lq
        return x @ (0.5 * (lq.Q @ x) + lq.qv) + u @ ((0.5 * (lq.R @ u) + lq.P @ x) + lq.rv) + self.q0 + self.gp.l1u * np.abs(u).sum()

    def h(self, x, p):
        lq = self.lq
        return x @ (0.5 * (lq.Qf @ x) + lq.qvf) + lq.q0f

    def noise(self, k, x, u, rng, p):
        gp = self.gp
        second = rng.uniform() < gp.tw2
        z = np.array([rng.normal() for _ in range(gp.n)])
        return (gp.tmean2 + gp.tchol2 @ z) if second else (gp.nmean + gp.nchol @ z)


# ---- the rollout in NumPy ------------------------------------------------------------------------------------------------------------
def np_rollouts(f, c, h, noise, p, x_nom, l, L, K, zn, zu, npn, npu):
    """rat_src_user_noisy_rollout on injected draws: (cost (K,), x (K, N+1, n), u (K, N, m)).  Open loop (L None, x_nom = x_0) or under
    u_t = l_t + L_t (x_t - x_nom_t).  A NaN cost marks a rollout whose sampler, f or cost returned NaN (DomainError)."""
    l = np.asarray(l, float)
    N, m = l.shape
    x_nom = np.asarray(x_nom, float)
    x0 = x_nom if L is None else x_nom[0]
    rng = SlotRng(zn, zu, npn, npu)
    cost, xs, us = np.zeros(K), np.zeros((K, N + 1, x0.size)), np.zeros((K, N, m))
    with np.errstate(invalid="ignore"):
        for j in range(K):
            x, tot = x0.copy(), 0.0
            for t in range(N):
                u = l[t] if L is None else l[t] + L[t] @ (x - x_nom[t])
                xs[j, t], us[j, t] = x, u
                tot += c(t, x, u, p)
                rng.at(j, t, N)
                x = f(x, u, p) + noise(t, x, u, rng, p)
            xs[j, N] = x
            cost[j] = tot + h(x, p)
    return cost, xs, us


class GenRng:
    """rat_rng's interface over a NumPy generator, K rollouts at a time (the statistical check: other streams, the same distribution)."""

    def __init__(self, seed, K):
        self.g, self.K = np.random.default_rng(seed), K

    def normal(self):
        return self.g.standard_normal(self.K)

    def uniform(self):
        return self.g.random(self.K)


def np_pend_state_costs(p, x_nom, l, L, K, seed):
    """The K costs of PEND_STATE under a policy with NumPy's generator, all rollouts at once (states as (2, K) arrays)."""
    l = np.asarray(l, float)
    N = l.shape[0]
    rng = GenRng(seed, K)
    x = np.repeat(np.asarray(x_nom[0], float)[:, None], K, axis=1)
    tot = np.zeros(K)
    for t in range(N):
        u = l[t][:, None] + L[t] @ (x - np.asarray(x_nom[t], float)[:, None])
        tot += pend_c(t, x, u, p)
        x = pend_f(x, u, p) + pend_state_noise(t, x, u, rng, p)
    return tot + pend_h(x, p)
