"""Generative source models (PETS, rat_pets_problem_set_source) shared by tests/test_cpu_source_pets.py and tests/test_gpu_source_pets.py,
and a NumPy restatement of compute_cost_worker (pets.jl:76-98) that reads injected draws by the slot layout of include/ratilqr.h."""
import numpy as np

# the documentation example of FiniteHorizonGenerativeOptimalControlProblem (optimal_control_problems.jl:102-123): a 2-D single
# integrator, x + u + rand(rng, d) with d = N(0, 0.5 I), or under use_true_model the mixture 0.5 N(0, 0.5 I) + 0.5 N(1, I) -- the
# mixture's component is the uniform (< 0.5: the first); c(k, x, u) = k/2 x'x + k/2 u'u; h(x) = N/2 x'x with N = p[0]
DOCS = r"""
__device__ void rat_user_f_stochastic(const double *x, const double *u, rat_rng &rng, int use_true_model, double *xn, const double *p) {
    if (use_true_model && rng.uniform() >= 0.5) {
        for (int i = 0; i < 2; ++i) xn[i] = x[i] + u[i] + (1.0 + rng.normal());
    } else {
        const double s = sqrt(0.5);
        for (int i = 0; i < 2; ++i) xn[i] = x[i] + u[i] + s * rng.normal();
    }
}
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) {
    return k / 2.0 * (x[0] * x[0] + x[1] * x[1]) + k / 2.0 * (u[0] * u[0] + u[1] * u[1]);
}
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return p[0] / 2.0 * (x[0] * x[0] + x[1] * x[1]); }
"""
DOCS_DIMS = dict(n=2, m=2, normals_per_step=2, uniforms_per_step=1)


def docs_f(x, u, rng, use_true, p):
    if use_true and rng.uniform() >= 0.5:
        return x + u + (1.0 + np.array([rng.normal(), rng.normal()]))
    return x + u + np.sqrt(0.5) * np.array([rng.normal(), rng.normal()])


docs_c = lambda k, x, u, p: k / 2.0 * (x @ x) + k / 2.0 * (u @ u)
docs_h = lambda x, p: p[0] / 2.0 * (x @ x)

# a damped pendulum with additive process noise on the velocity; p = (dt, damping, noise scale)
PENDULUM = r"""
__device__ void rat_user_f_stochastic(const double *x, const double *u, rat_rng &rng, int use_true_model, double *xn, const double *p) {
    const double dt = p[0];
    xn[0] = x[0] + dt * x[1];
    xn[1] = x[1] + dt * (-sin(x[0]) - p[1] * x[1] + u[0]) + p[2] * rng.normal();
}
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) {
    return 0.5 * (x[0] * x[0] + x[1] * x[1]) + 0.05 * (u[0] * u[0]) + 0.01 * k * x[0];
}
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return 2.0 * (x[0] * x[0] + x[1] * x[1]); }
"""
PENDULUM_DIMS = dict(n=2, m=1, normals_per_step=1, uniforms_per_step=0)
PENDULUM_P = [0.1, 0.1, 0.05]


def pendulum_f(x, u, rng, use_true, p):
    dt = p[0]
    return np.array([x[0] + dt * x[1], x[1] + dt * (-np.sin(x[0]) - p[1] * x[1] + u[0]) + p[2] * rng.normal()])


pendulum_c = lambda k, x, u, p: 0.5 * (x @ x) + 0.05 * (u @ u) + 0.01 * k * x[0]
pendulum_h = lambda x, p: 2.0 * (x @ x)

# test/pets_test.jl:15-20: x + u + rand(rng, 2), c = sum(abs.(u)), h = 1
REF_TEST = r"""
__device__ void rat_user_f_stochastic(const double *x, const double *u, rat_rng &rng, int use_true_model, double *xn, const double *p) {
    for (int i = 0; i < 2; ++i) xn[i] = x[i] + u[i] + rng.uniform();
}
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) { return fabs(u[0]) + fabs(u[1]); }
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return T(1.0); }
"""
REF_TEST_DIMS = dict(n=2, m=2, normals_per_step=0, uniforms_per_step=2)

# the LQ + cubic generative family (LQGenerativeProblem) written as source, its tables in p (lq_params); p[okind] = 0 Gaussian noise with
# the optional true-model mixture (one selector uniform, then n normals), 1 uniform noise (n uniforms)
LQ = r"""
constexpr int NX = RAT_N, NU = RAT_M;
constexpr int oA = 0, oB = oA + NX * NX, oQ = oB + NX * NU, oR = oQ + NX * NX, oP = oR + NU * NU, oqv = oP + NU * NX, orv = oqv + NX,
              oq0 = orv + NU, oQf = oq0 + 1, oqvf = oQf + NX * NX, oq0f = oqvf + NX, okap = oq0f + 1, ol1u = okap + 1, okind = ol1u + 1,
              onm = okind + 1, onc = onm + NX, otw = onc + NX * NX, otm = otw + 1, otc = otm + NX, olo = otc + NX * NX, ohi = olo + 1;

__device__ void rat_user_f_stochastic(const double *x, const double *u, rat_rng &rng, int use_true_model, double *xn, const double *p) {
    double y[NX];
    for (int i = 0; i < NX; ++i) {
        double a = 0.0;
        for (int j = 0; j < NX; ++j) a += p[oA + i * NX + j] * x[j];
        for (int b = 0; b < NU; ++b) a += p[oB + i * NU + b] * u[b];
        y[i] = a + p[okap] * (x[i] * x[i] * x[i]);
    }
    if (p[okind] == 0.0) {
        bool second = false;
        if (use_true_model && p[otw] > 0.0) second = rng.uniform() < p[otw];
        double z[NX];
        for (int i = 0; i < NX; ++i) z[i] = rng.normal();
        const double *mean = p + (second ? otm : onm), *L = p + (second ? otc : onc);
        for (int i = 0; i < NX; ++i) {
            double w = 0.0;
            for (int j = 0; j <= i; ++j) w += L[i * NX + j] * z[j];
            xn[i] = y[i] + (mean[i] + w);
        }
    } else {
        for (int i = 0; i < NX; ++i) xn[i] = y[i] + (p[olo] + (p[ohi] - p[olo]) * rng.uniform());
    }
}
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) {
    T c = 0.0;
    for (int i = 0; i < NX; ++i) {
        T a = 0.0;
        for (int j = 0; j < NX; ++j) a += p[oQ + i * NX + j] * x[j];
        c += x[i] * (0.5 * a + p[oqv + i]);
    }
    for (int q = 0; q < NU; ++q) {
        T a = 0.0, px = 0.0;
        for (int b = 0; b < NU; ++b) a += p[oR + q * NU + b] * u[b];
        for (int j = 0; j < NX; ++j) px += p[oP + q * NX + j] * x[j];
        c += u[q] * ((0.5 * a + px) + p[orv + q]);
    }
    T l1 = 0.0;
    for (int q = 0; q < NU; ++q) l1 += fabs(u[q]);
    return c + p[oq0] + p[ol1u] * l1;
}
template <class T> __device__ T rat_user_h(const T *x, const double *p) {
    T c = 0.0;
    for (int i = 0; i < NX; ++i) {
        T a = 0.0;
        for (int j = 0; j < NX; ++j) a += p[oQf + i * NX + j] * x[j];
        c += x[i] * (0.5 * a + p[oqvf + i]);
    }
    return c + p[oq0f];
}
"""


def lq_params(prob):
    """p of the LQ source for an LQGenerativeProblem with time-invariant cost tables (matrices row-major)."""
    lq = prob.lq
    n, m = prob.n, prob.m
    q0 = float(np.asarray(lq.q0).ravel()[0])
    parts = [lq.A, lq.B, lq.Q, lq.R, lq.P, lq.qv, lq.rv, [q0], lq.Qf, lq.qvf, [lq.q0f], [lq.kappa], [prob.l1u], [float(prob.noise_kind)],
             prob.nmean, prob.nchol, [prob.tw2], prob.tmean2, prob.tchol2, [prob.nlo], [prob.nhi]]
    p = np.concatenate([np.asarray(a, float).ravel() for a in parts])
    assert p.size == 5 * n * n + 2 * n * m + m * m + 4 * n + m + 8
    return p


class SlotRng:
    """rat_rng on injected streams: the i-th normal / uniform of (trajectory j, step t) is zn[(j N + t) npn + i] / zu[(j N + t) npu + i]."""

    def __init__(self, zn, zu, npn, npu):
        self.zn, self.zu, self.npn, self.npu = zn, zu, npn, npu

    def at(self, j, t, N):
        self.bn, self.bu, self.i, self.k = (j * N + t) * self.npn, (j * N + t) * self.npu, 0, 0

    def normal(self):
        assert self.i < self.npn
        self.i += 1
        return self.zn[self.bn + self.i - 1]

    def uniform(self):
        assert self.k < self.npu
        self.k += 1
        return self.zu[self.bu + self.k - 1]


def np_compute_cost(f, c, h, p, x0, ctrl, K, zn, zu, npn, npu, use_true=False):
    """compute_cost_serial (pets.jl:128-157) in NumPy: cost[ii] = mean over kk of sum_t c(t, x_t, u_t) + h(x_N), trajectory j = ii K + kk."""
    S, N = ctrl.shape[0], ctrl.shape[1]
    rng = SlotRng(zn, zu, npn, npu)
    out = np.zeros(S)
    for ii in range(S):
        tot = np.zeros(K)
        for kk in range(K):
            x, cost = np.asarray(x0, float), 0.0
            for t in range(N):
                cost += c(t, x, ctrl[ii, t], p)
                rng.at(ii * K + kk, t, N)
                x = f(x, ctrl[ii, t], rng, use_true, p)
            tot[kk] = cost + h(x, p)
        out[ii] = tot.mean()
    return out
