"""NumPy model of rat_policy_param_gradient / rat_policy_tail_param_gradient (csrc/source_adjoint_params.h, ppg_moments and ppg_final of
csrc/policy_mc.hip) -- test aid, shared by tests/test_cpu_param_gradient.py, tests/test_gpu_param_gradient.py and
tools/policy_param_gradient_bench.py.

On top of tests/policy_gradient_model.py: its draws, its policy, its row weights and (through the same case interface f, c, h, fx, fu,
cx, cu, hx, noise) its adjoint.  What is new here is the parameters: a case holds P (1 or K, n_params) in any float dtype, which f, c
and h read, beside Pn, which the sampler reads -- the noise is frozen, so a finite difference moves P alone, and with parameter
sampling both are the rollouts' drawn q.  The recursion is the header's,
    lambda_N = h_x(x_N),  gp = h_p(x_N);   gp += c_p + f_p' lambda_{t+1},  lambda_t = (x part of g_t) + L_t' gu_t,   t = N - 1 .. 0
with f_p, c_p, h_p written out by hand per case; lambda_0 is dJ_k / dx_0 with the law centred on x_nom_0 (the rollout may start at
x_nom_0 + delta).  A rollout with a cost but a NaN or Inf in h_x, some g_t, h_p or some parameter term is left out of every sum and of
the denominator.  dtype=np.longdouble runs everything in extended precision on the same draws and the same weight rule."""
import numpy as np

import policy_gradient_model as pgm

AD = "#define RAT_USER_PARAMS_AD\n"
F_SIG = "template <class T, class P> __device__ void rat_user_f(const T *x, const T *u, T *xn, const P *p)"
C_SIG = "template <class T, class P> __device__ T rat_user_c(int k, const T *x, const T *u, const P *p)"
H_SIG = "template <class T, class P> __device__ T rat_user_h(const T *x, const P *p)"
NOISE_SIG = "#define RAT_USER_NOISE\ntemplate <class R> __device__ void rat_user_noise(int k, const double *x, const double *u, R &rng, double *w, const double *p)"


class PCase:
    """A source model with differentiable parameters on (K, .) arrays: pgm.Case's interface at the parameters P, and f_p (K, n, np),
    c_p (K, np), h_p (K, np)."""
    source, n, m, npn, p = None, 0, 0, 0, None

    def __init__(self, p=None):
        self.p = np.asarray(self.p if p is None else p, float)
        self.P = self.Pn = self.p[None, :]

    @property
    def n_params(self):
        return self.p.size

    def dims(self):
        return dict(n=self.n, m=self.m, normals_per_step=self.npn, uniforms_per_step=0)

    def at(self, P, noise=None):
        """a copy whose f, c, h read P (n_params,) or (K, n_params) in P's dtype; noise: what the sampler reads (default: as before)"""
        o = object.__new__(type(self))
        o.__dict__.update(self.__dict__)
        o.P = np.atleast_2d(np.asarray(P))
        if noise is not None:
            o.Pn = np.atleast_2d(np.asarray(noise))
        return o

    def q(self, i, like):
        """parameter i as a (1 or K,) array in like's dtype"""
        return self.P[:, i].astype(like.dtype)

    def zeros_p(self, x, *shape):
        return np.zeros((x.shape[0],) + shape + (self.n_params,), dtype=x.dtype)


# ---- the scalar LQ source of pgm.SCALAR_LQ with its six parameters opened --------------------------------------------------------------
SCALAR_AD = AD + F_SIG + " { xn[0] = p[0] * x[0] + p[1] * u[0]; }\n" + C_SIG + r""" {
    return 0.5 * p[2] * (x[0] * x[0]) + 0.5 * p[3] * (u[0] * u[0]);
}
""" + H_SIG + " { return 0.5 * p[4] * (x[0] * x[0]); }\n" + NOISE_SIG + " { w[0] = p[5] * rng.normal(); }\n"


class ScalarLQ(PCase):
    source, n, m, npn, p = SCALAR_AD, 1, 1, 1, pgm.SCALAR_P

    def f(self, x, u): return self.q(0, x)[:, None] * x + self.q(1, x)[:, None] * u
    def c(self, t, x, u): return 0.5 * self.q(2, x) * x[:, 0] ** 2 + 0.5 * self.q(3, x) * u[:, 0] ** 2
    def h(self, x): return 0.5 * self.q(4, x) * x[:, 0] ** 2
    def fx(self, x, u): return np.broadcast_to(self.q(0, x)[:, None, None], (x.shape[0], 1, 1))
    def fu(self, x, u): return np.broadcast_to(self.q(1, x)[:, None, None], (x.shape[0], 1, 1))
    def cx(self, t, x, u): return self.q(2, x)[:, None] * x
    def cu(self, t, x, u): return self.q(3, x)[:, None] * u
    def hx(self, x): return self.q(4, x)[:, None] * x
    def noise(self, z): return self.Pn[:, 5].astype(z.dtype)[:, None] * z

    def fp(self, x, u):
        o = self.zeros_p(x, 1)
        o[:, 0, 0], o[:, 0, 1] = x[:, 0], u[:, 0]
        return o

    def cp(self, t, x, u):
        o = self.zeros_p(x)
        o[:, 2], o[:, 3] = 0.5 * x[:, 0] ** 2, 0.5 * u[:, 0] ** 2
        return o

    def hp(self, x):
        o = self.zeros_p(x)
        o[:, 4] = 0.5 * x[:, 0] ** 2
        return o


# the scalar source with h = sqrt(|p4 (x - 1/2)|) and a rectified sampler: where x_N == 1/2 exactly, h is 0 with slope Inf, so h_x is Inf
# and h_p is Inf times the zero tangent, NaN
SQRT_PARAM = AD + F_SIG + " { xn[0] = p[0] * x[0] + p[1] * u[0]; }\n" + C_SIG + r""" {
    return 0.5 * p[2] * (x[0] * x[0]) + 0.5 * p[3] * (u[0] * u[0]);
}
""" + H_SIG + " { return sqrt(fabs(p[4] * (x[0] - 0.5))); }\n" + NOISE_SIG + r""" {
    const double z = rng.normal();
    w[0] = (z > 0.0) ? p[5] * z : 0.0;
}
"""


class SqrtParam(ScalarLQ):
    source, p = SQRT_PARAM, [0.5, 0.5, 1.0, 0.2, 1.0, 0.3]

    def _s(self, x): return self.q(4, x) * (x[:, 0] - 0.5)
    def h(self, x): return np.sqrt(np.abs(self._s(x)))

    def _slope(self, x):
        s = self._s(x)
        with np.errstate(all="ignore"):
            return np.where(s < 0, -1.0, 1.0) * (0.5 / np.sqrt(np.abs(s)))

    def hx(self, x):
        with np.errstate(all="ignore"):
            return (self._slope(x) * self.q(4, x))[:, None]

    def hp(self, x):
        o = self.zeros_p(x)
        with np.errstate(all="ignore"):
            o[:, 4] = self._slope(x) * (x[:, 0] - 0.5)
        return o

    def noise(self, z): return np.where(z > 0.0, self.Pn[:, 5].astype(z.dtype)[:, None] * z, 0.0)


# ---- linear 2 x 1: an additive drift p0 on x_0' and a weight p1 on the running state cost: J is at most quadratic in each of p0, p1, x_0 --
LIN2_AD = AD + F_SIG + r""" {
    xn[0] = 0.95 * x[0] + 0.1 * x[1] + p[0];
    xn[1] = -0.05 * x[0] + 0.9 * x[1] + 0.3 * u[0];
}
""" + C_SIG + " { return 0.5 * p[1] * (x[0] * x[0] + x[1] * x[1]) + 0.5 * (u[0] * u[0]); }\n" + H_SIG + r""" {
    return 0.5 * (x[0] * x[0] + x[1] * x[1]);
}
""" + NOISE_SIG + r""" {
    const double z0 = rng.normal(), z1 = rng.normal();
    w[0] = 0.2 * z0;
    w[1] = 0.05 * z0 + 0.15 * z1;
}
"""


class Lin2(PCase):
    source, n, m, npn, p = LIN2_AD, 2, 1, 2, [0.05, 1.5]
    A, B, C = np.array([[0.95, 0.1], [-0.05, 0.9]]), np.array([[0.0], [0.3]]), np.array([[0.2, 0.0], [0.05, 0.15]])

    def f(self, x, u):
        o = x @ self.A.T.astype(x.dtype) + u @ self.B.T.astype(x.dtype)
        o[:, 0] = o[:, 0] + self.q(0, x)
        return o

    def c(self, t, x, u): return 0.5 * self.q(1, x) * (x[:, 0] ** 2 + x[:, 1] ** 2) + 0.5 * u[:, 0] ** 2
    def h(self, x): return 0.5 * (x[:, 0] ** 2 + x[:, 1] ** 2)
    def fx(self, x, u): return np.broadcast_to(self.A.astype(x.dtype), (x.shape[0], 2, 2))
    def fu(self, x, u): return np.broadcast_to(self.B.astype(x.dtype), (x.shape[0], 2, 1))
    def cx(self, t, x, u): return self.q(1, x)[:, None] * x
    def cu(self, t, x, u): return u
    def hx(self, x): return x
    def noise(self, z): return z @ self.C.T.astype(z.dtype)

    def fp(self, x, u):
        o = self.zeros_p(x, 2)
        o[:, 0, 0] = 1.0
        return o

    def cp(self, t, x, u):
        o = self.zeros_p(x)
        o[:, 1] = 0.5 * (x[:, 0] ** 2 + x[:, 1] ** 2)
        return o

    def hp(self, x): return self.zeros_p(x)


# ---- the pendulum with its length p0, its damping p1 and a cost weight p2 ------------------------------------------------------------------
_PEND_REST = C_SIG + r""" {
    return 0.5 * p[2] * (x[0] * x[0] + x[1] * x[1]) + 0.05 * (u[0] * u[0]) + 0.01 * k * x[0];
}
""" + H_SIG + " { return 2.0 * (x[0] * x[0] + x[1] * x[1]); }\n" + NOISE_SIG + r""" {
    w[0] = 0.05 * rng.normal();
    w[1] = 0.1 * rng.normal();
}
"""
PEND_AD = AD + F_SIG + r""" {
    xn[0] = x[0] + 0.1 * x[1];
    xn[1] = x[1] + 0.1 * (u[0] - sin(x[0]) / p[0] - p[1] * x[1]);
}
""" + _PEND_REST
PEND_AD_JAC = PEND_AD + r"""
#define RAT_USER_F_JACOBIAN
__device__ void rat_user_f_jacobian(const double *x, const double *u, double *xn, double *A, double *B, const double *p) {
    xn[0] = x[0] + 0.1 * x[1];
    xn[1] = x[1] + 0.1 * (u[0] - sin(x[0]) / p[0] - p[1] * x[1]);
    A[0] = 1.0; A[1] = -0.1 * cos(x[0]) / p[0]; A[2] = 0.1; A[3] = 1.0 - 0.1 * p[1];
    B[0] = 0.0; B[1] = 0.1;
}
"""
# rat_user_params for the sampling test: every parameter scaled by a draw of its own
PEND_AD_JAC_SAMPLED = PEND_AD_JAC + r"""
#define RAT_USER_PARAMS
template <class R> __device__ void rat_user_params(R &rng, const double *p, double *q) {
    q[0] = p[0] * (1.0 + 0.1 * rng.normal());
    q[1] = p[1] * (1.0 + 0.2 * rng.normal());
    q[2] = p[2] * (1.0 + 0.5 * rng.uniform());
}
"""


class Pendulum(PCase):
    source, n, m, npn, p = PEND_AD, 2, 1, 2, [1.3, 0.1, 0.8]

    def __init__(self, p=None, source=None):
        super().__init__(p)
        if source is not None:
            self.source = source

    def f(self, x, u):
        return np.stack([x[:, 0] + 0.1 * x[:, 1], x[:, 1] + 0.1 * (u[:, 0] - np.sin(x[:, 0]) / self.q(0, x) - self.q(1, x) * x[:, 1])], axis=1)

    def c(self, t, x, u): return 0.5 * self.q(2, x) * (x[:, 0] ** 2 + x[:, 1] ** 2) + 0.05 * u[:, 0] ** 2 + 0.01 * t * x[:, 0]
    def h(self, x): return 2.0 * (x[:, 0] ** 2 + x[:, 1] ** 2)

    def fx(self, x, u):
        one = np.ones(x.shape[0], dtype=x.dtype)
        return np.stack([np.stack([one, 0.1 * one], axis=1),
                         np.stack([-0.1 * np.cos(x[:, 0]) / self.q(0, x), (1.0 - 0.1 * self.q(1, x)) * one], axis=1)], axis=1)

    def fu(self, x, u):
        o = np.zeros((x.shape[0], 2, 1), dtype=x.dtype)
        o[:, 1, 0] = 0.1
        return o

    def cx(self, t, x, u): return np.stack([self.q(2, x) * x[:, 0] + 0.01 * t, self.q(2, x) * x[:, 1]], axis=1)
    def cu(self, t, x, u): return 0.1 * u
    def hx(self, x): return 4.0 * x
    def noise(self, z): return z * np.array([0.05, 0.1]).astype(z.dtype)

    def fp(self, x, u):
        o = self.zeros_p(x, 2)
        o[:, 1, 0] = 0.1 * np.sin(x[:, 0]) / self.q(0, x) ** 2
        o[:, 1, 1] = -0.1 * x[:, 1]
        return o

    def cp(self, t, x, u):
        o = self.zeros_p(x)
        o[:, 2] = 0.5 * (x[:, 0] ** 2 + x[:, 1] ** 2)
        return o

    def hp(self, x): return self.zeros_p(x)


# ---- LQ + cubic at n x m with NP parameters: parameter i acts on state j = i % n in role (i / n) % 3 ----------------------------------------
#   role 0: x_j' += p_i x_j^3       role 1: c += p_i x_j^2 / 2       role 2: h += p_i x_j^2 / 2 and x_j' += p_i / 10
# behind x_j' = 0.9 x_j + 0.05 x_{(j + 1) % n} + 0.3 u_{j % m}, c = sum u^2 / 20 + sum x / 10, h = 0; w = z / 10
def lq_cubic_source(NP):
    return AD + f"#define NP {NP}\n" + F_SIG + r""" {
    for (int j = 0; j < RAT_N; ++j) xn[j] = 0.9 * x[j] + 0.05 * x[(j + 1) % RAT_N] + 0.3 * u[j % RAT_M];
    for (int i = 0; i < NP; ++i) {
        const int j = i % RAT_N, role = (i / RAT_N) % 3;
        if (role == 0) xn[j] = xn[j] + p[i] * (x[j] * x[j] * x[j]);
        if (role == 2) xn[j] = xn[j] + 0.1 * p[i];
    }
}
""" + C_SIG + r""" {
    T s = 0.1 * x[0];
    for (int j = 1; j < RAT_N; ++j) s = s + 0.1 * x[j];
    for (int j = 0; j < RAT_M; ++j) s = s + 0.05 * (u[j] * u[j]);
    for (int i = 0; i < NP; ++i)
        if ((i / RAT_N) % 3 == 1) s = s + 0.5 * p[i] * (x[i % RAT_N] * x[i % RAT_N]);
    return s;
}
""" + H_SIG + r""" {
    T s = 0.0 * x[0];
    for (int i = 0; i < NP; ++i)
        if ((i / RAT_N) % 3 == 2) s = s + 0.5 * p[i] * (x[i % RAT_N] * x[i % RAT_N]);
    return s;
}
""" + NOISE_SIG + r""" {
    for (int j = 0; j < RAT_N; ++j) w[j] = 0.1 * rng.normal();
}
"""


class LqCubic(PCase):
    def __init__(self, n, m, NP):
        self.n, self.m, self.npn, self.source = n, m, n, lq_cubic_source(NP)
        i = np.arange(NP)
        self.j, self.role = i % n, (i // n) % 3
        super().__init__(np.where(self.role == 0, -0.05, 1.0) * (1.0 + 0.1 * np.cos(1.0 + i)))

    def f(self, x, u):
        n, m = self.n, self.m
        o = 0.9 * x + 0.05 * x[:, (np.arange(n) + 1) % n] + 0.3 * u[:, np.arange(n) % m]
        for i, (j, r) in enumerate(zip(self.j, self.role)):
            if r == 0:
                o[:, j] = o[:, j] + self.q(i, x) * x[:, j] ** 3
            if r == 2:
                o[:, j] = o[:, j] + 0.1 * self.q(i, x)
        return o

    def c(self, t, x, u):
        s = 0.1 * x.sum(axis=1) + 0.05 * (u * u).sum(axis=1)
        for i, (j, r) in enumerate(zip(self.j, self.role)):
            if r == 1:
                s = s + 0.5 * self.q(i, x) * x[:, j] ** 2
        return s

    def h(self, x):
        s = np.zeros(x.shape[0], dtype=x.dtype)
        for i, (j, r) in enumerate(zip(self.j, self.role)):
            if r == 2:
                s = s + 0.5 * self.q(i, x) * x[:, j] ** 2
        return s

    def fx(self, x, u):
        n = self.n
        A = 0.9 * np.eye(n) + 0.05 * np.eye(n)[(np.arange(n) + 1) % n]
        o = np.broadcast_to(A.astype(x.dtype), (x.shape[0], n, n)).copy()
        for i, (j, r) in enumerate(zip(self.j, self.role)):
            if r == 0:
                o[:, j, j] += 3.0 * self.q(i, x) * x[:, j] ** 2
        return o

    def fu(self, x, u):
        B = np.zeros((self.n, self.m))
        B[np.arange(self.n), np.arange(self.n) % self.m] = 0.3
        return np.broadcast_to(B.astype(x.dtype), (x.shape[0], self.n, self.m))

    def _quad_x(self, x, role):
        o = np.zeros_like(x)
        for i, (j, r) in enumerate(zip(self.j, self.role)):
            if r == role:
                o[:, j] = o[:, j] + self.q(i, x) * x[:, j]
        return o

    def cx(self, t, x, u): return 0.1 + self._quad_x(x, 1)
    def cu(self, t, x, u): return 0.1 * u
    def hx(self, x): return self._quad_x(x, 2)
    def noise(self, z): return 0.1 * z

    def fp(self, x, u):
        o = self.zeros_p(x, self.n)
        for i, (j, r) in enumerate(zip(self.j, self.role)):
            if r == 0:
                o[:, j, i] = x[:, j] ** 3
            if r == 2:
                o[:, j, i] = 0.1
        return o

    def _quad_p(self, x, role):
        o = self.zeros_p(x)
        for i, (j, r) in enumerate(zip(self.j, self.role)):
            if r == role:
                o[:, i] = 0.5 * x[:, j] ** 2
        return o

    def cp(self, t, x, u): return self._quad_p(x, 1)
    def hp(self, x): return self._quad_p(x, 2)


# ---- 3 x 2 with c and f reading v = u + p: dJ / dp_j = sum_t dJ / du_t[j] -------------------------------------------------------------------
U_PLUS_P = AD + F_SIG + r""" {
    for (int j = 0; j < 3; ++j) xn[j] = 0.9 * x[j] + 0.05 * x[(j + 1) % 3] + 0.3 * (u[j % 2] + p[j % 2]) + 0.1 * sin(x[j]);
}
""" + C_SIG + r""" {
    return 0.5 * (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) + 0.1 * ((u[0] + p[0]) * (u[0] + p[0]) + (u[1] + p[1]) * (u[1] + p[1]))
           + 0.05 * (u[0] + p[0]) * x[0];
}
""" + H_SIG + " { return 0.5 * (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]); }\n" + NOISE_SIG + r""" {
    for (int j = 0; j < 3; ++j) w[j] = 0.1 * rng.normal();
}
"""


class UPlusP(PCase):
    source, n, m, npn, p = U_PLUS_P, 3, 2, 3, [0.2, -0.1]

    def v(self, u): return u + np.stack([self.q(0, u), self.q(1, u)], axis=1)

    def f(self, x, u):
        v = self.v(u)
        return 0.9 * x + 0.05 * x[:, [1, 2, 0]] + 0.3 * v[:, [0, 1, 0]] + 0.1 * np.sin(x)

    def c(self, t, x, u):
        v = self.v(u)
        return 0.5 * (x * x).sum(axis=1) + 0.1 * (v * v).sum(axis=1) + 0.05 * v[:, 0] * x[:, 0]

    def h(self, x): return 0.5 * (x * x).sum(axis=1)

    def fx(self, x, u):
        A = 0.9 * np.eye(3) + 0.05 * np.eye(3)[[1, 2, 0]]
        o = np.broadcast_to(A.astype(x.dtype), (x.shape[0], 3, 3)).copy()
        i = np.arange(3)
        o[:, i, i] += 0.1 * np.cos(x)
        return o

    def fu(self, x, u):
        B = np.zeros((3, 2))
        B[[0, 1, 2], [0, 1, 0]] = 0.3
        return np.broadcast_to(B.astype(x.dtype), (x.shape[0], 3, 2))

    def cx(self, t, x, u):
        o = x.copy()
        o[:, 0] = o[:, 0] + 0.05 * self.v(u)[:, 0]
        return o

    def cu(self, t, x, u):
        o = 0.2 * self.v(u)
        o[:, 0] = o[:, 0] + 0.05 * x[:, 0]
        return o

    def hx(self, x): return x
    def noise(self, z): return 0.1 * z
    def fp(self, x, u): return self.fu(x, u)
    def cp(self, t, x, u): return self.cu(t, x, u)
    def hp(self, x): return self.zeros_p(x)


def rollout(case, x_nom, l, L, z, dtype=np.float64, dx0=None):
    """pgm.rollout with the initial state off the nominal one by dx0 (n,): the law stays centred on x_nom"""
    l = np.asarray(l, float).astype(dtype)
    N, K = l.shape[0], z.shape[0]
    x_nom = np.asarray(x_nom, float).astype(dtype)
    Lq = None if L is None else np.asarray(L, float).astype(dtype)
    z = np.asarray(z).astype(dtype)
    xs, us = np.zeros((K, N + 1, case.n), dtype=dtype), np.zeros((K, N, case.m), dtype=dtype)
    xs[:, 0] = (x_nom if L is None else x_nom[0]) + (0 if dx0 is None else np.asarray(dx0).astype(dtype))
    J = np.zeros(K, dtype=dtype)
    with np.errstate(all="ignore"):
        for t in range(N):
            x = xs[:, t]
            u = np.broadcast_to(l[t], (K, case.m)) if L is None else l[t] + (x - x_nom[t]) @ Lq[t].T
            us[:, t] = u
            J = J + case.c(t, x, u)
            xs[:, t + 1] = case.f(x, u) + case.noise(z[:, t])
        J = J + case.h(xs[:, N])
    return J, xs, us


def adjoint(case, xs, us, L):
    """(gp (K, np), lam0 (K, n), finite (K,)): dJ_k / dp and dJ_k / dx_0, and whether h_x, every g_t, h_p and every parameter term are
    finite"""
    K, N = us.shape[0], us.shape[1]
    Lq = None if L is None else np.asarray(L, float).astype(xs.dtype)
    with np.errstate(all="ignore"):
        lam = case.hx(xs[:, N])
        gp = case.hp(xs[:, N]).copy()
        fin = np.isfinite(lam).all(axis=1) & np.isfinite(gp).all(axis=1)
        for t in range(N - 1, -1, -1):
            x, u = xs[:, t], us[:, t]
            term = case.cp(t, x, u) + (case.fp(x, u) * lam[:, :, None]).sum(axis=1)
            gx = case.cx(t, x, u) + (case.fx(x, u) * lam[:, :, None]).sum(axis=1)
            g_u = case.cu(t, x, u) + (case.fu(x, u) * lam[:, :, None]).sum(axis=1)
            fin &= np.isfinite(term).all(axis=1) & np.isfinite(gx).all(axis=1) & np.isfinite(g_u).all(axis=1)
            gp = gp + term
            lam = gx if L is None else gx + g_u @ Lq[t]
    return gp, lam, fin


def sums(v, fin, y, dead, J):
    """(mean (R, d), se (R, d), n_nonfinite, sum p^2 v^2 (R, d)) of the per-rollout sensitivities v (K, d) under the row weights y (R, K):
    pgm.gradient's sums"""
    dtype = v.dtype
    ok = ~np.isnan(np.asarray(J, float))
    use = ok & fin
    R, d = y.shape[0], v.shape[1]
    V = np.where(use[:, None], v, 0)
    mean, se, sc = (np.full((R, d), np.nan, dtype=dtype) for _ in range(3))
    with np.errstate(all="ignore"):
        for r in range(R):
            if dead[r]:
                continue
            w = np.where(use, y[r].astype(dtype), 0)
            sf, sf2 = w.sum(), (w * w).sum()
            mean[r] = (w[:, None] * V).sum(axis=0) / sf
            s2, s22 = ((w * w)[:, None] * V).sum(axis=0), ((w * w)[:, None] * V * V).sum(axis=0)
            var = ((s22 - 2.0 * mean[r] * s2) + mean[r] * mean[r] * sf2) / (sf * sf)
            sc[r] = s22 / (sf * sf)
            se[r] = np.where(var > 0, np.sqrt(np.where(var > 0, var, 0)), np.where(np.isnan(var), np.nan, 0))
    return mean, se, int((ok & ~fin).sum()), sc


def model(case, x_nom, l, L, K, seed, kl_bounds=(), thetas=(), alphas=None, dtype=np.float64, q=None):
    """The whole call: dict(J, x, u, gp, lam0, fin, y, dead, rows, grad_p, grad_p_se, grad_x0, grad_x0_se, n_nonfinite, p_scale,
    x0_scale).  q (K, n_params): the rollouts' own drawn parameters (parameter sampling on), read by f, c, h and the sampler."""
    N = np.asarray(l).shape[0]
    z = pgm.draws(case, seed, K, N)
    if q is not None:
        case = case.at(np.asarray(q).astype(dtype), noise=np.asarray(q).astype(dtype))
    J, xs, us = rollout(case, x_nom, l, L, z, dtype)
    gp, lam0, fin = adjoint(case, xs, us, L)
    y, dead, rows = pgm.weights(J, kl_bounds, thetas, alphas, dtype)
    P = case.n_params
    mean, se, nf, sc = sums(np.concatenate([gp, lam0], axis=1), fin, y, dead, J)
    return dict(J=J, x=xs, u=us, gp=gp, lam0=lam0, fin=fin, y=y, dead=dead, rows=rows, grad_p=mean[:, :P], grad_p_se=se[:, :P],
                grad_x0=mean[:, P:], grad_x0_se=se[:, P:], n_nonfinite=nf, p_scale=sc[:, :P], x0_scale=sc[:, P:])
