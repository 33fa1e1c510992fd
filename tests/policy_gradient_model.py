"""NumPy model of rat_policy_gradient / rat_policy_tail_gradient (csrc/source_adjoint.h, pg_moments and pg_final of csrc/policy_mc.hip) --
test aid, shared by tests/test_cpu_policy_gradient.py, tests/test_gpu_policy_gradient.py and tools/policy_gradient_bench.py.

The rollout is rat_src_user_noisy_rollout's on the device generator's draws (rat_rng's normals of tests/rare_event_noise_model.py at
pass 0: the Philox key is the caller's seed, the counter the global rollout index), all K rollouts at once.  The adjoint is the header's:
    lambda_N = h_x(x_N);  g_t = c_z + f_z' lambda_{t+1};  gu_t = the u part;  lambda_t = the x part + L_t' gu_t
with Jacobians written out by hand per case.  The row weights are the existing models' (wc_trajectory_model.row_weights on the costs,
tail_scenarios_model.tail_weights), and a rollout with a cost but a NaN or Inf anywhere in h_x or some g_t is left out of every sum and
of the denominator.  dtype=np.longdouble runs rollout, adjoint and sums in extended precision on the same draws and the same weight
rule (theta and the tail's cut come from the float64 costs, so the two runs put the weight on the same rollouts)."""
import numpy as np

import rare_event_noise_model as rn
import user_noise_model as un
from source_pets_models import lq_params
from tail_scenarios_model import tail_weights
from wc_trajectory_model import row_weights

# ---- the scalar LQ source: x+ = a x + b u + w, c = (q x^2 + r u^2) / 2, h = qf x^2 / 2, w = sigma z; p = a, b, q, r, qf, sigma -----------
SCALAR_LQ = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) { xn[0] = p[0] * x[0] + p[1] * u[0]; }
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) {
    return 0.5 * p[2] * (x[0] * x[0]) + 0.5 * p[3] * (u[0] * u[0]);
}
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return 0.5 * p[4] * (x[0] * x[0]); }
#define RAT_USER_NOISE
template <class R> __device__ void rat_user_noise(int k, const double *x, const double *u, R &rng, double *w, const double *p) {
    w[0] = p[5] * rng.normal();
}
"""
SCALAR_P = [0.9, 0.5, 1.0, 0.2, 2.0, 0.3]

# ---- a 2 x 1 linear source (quadratic cost): every functional of the mean is quadratic in the policy ------------------------------------
LIN2 = rn.LIN_GAUSS
LIN2_P = [0.95, 0.1, -0.05, 0.9, 0.0, 0.3, 0.2, 0.05, 0.15]

# the pendulum with rat_user_f_jacobian (A, B column-major): the same f, so the same gradient
PEND_JAC = un.PEND_DIAG + r"""
#define RAT_USER_F_JACOBIAN
__device__ void rat_user_f_jacobian(const double *x, const double *u, double *xn, double *A, double *B, const double *p) {
    const double dt = p[0];
    xn[0] = x[0] + dt * x[1];
    xn[1] = x[1] + dt * (-sin(x[0]) - 0.1 * x[1] + u[0]);
    A[0] = 1.0; A[1] = -dt * cos(x[0]); A[2] = dt; A[3] = 1.0 - 0.1 * dt;
    B[0] = 0.0; B[1] = dt;
}
"""

# the scalar source with a cost whose derivative is infinite at u == 0: c = sqrt(|u|) + x^2 / 2 (fabs has slope +1 at 0, sqrt slope Inf)
SQRT_COST = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) { xn[0] = p[0] * x[0] + p[1] * u[0]; }
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) { return sqrt(fabs(u[0])) + 0.5 * (x[0] * x[0]); }
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return 0.5 * p[4] * (x[0] * x[0]); }
#define RAT_USER_NOISE
template <class R> __device__ void rat_user_noise(int k, const double *x, const double *u, R &rng, double *w, const double *p) {
    const double z = rng.normal();
    w[0] = (z > 0.0) ? p[5] * z : 0.0;
}
"""


class Case:
    """A source model on (K, .) arrays in any float dtype: f, c, h, their hand-written Jacobians and the sampler as a function of the
    step's normals z (K, npn)."""
    source, n, m, npn, p = None, 0, 0, 0, None

    def dims(self):
        return dict(n=self.n, m=self.m, normals_per_step=self.npn, uniforms_per_step=0)


class ScalarLQ(Case):
    source, n, m, npn = SCALAR_LQ, 1, 1, 1

    def __init__(self, p=SCALAR_P):
        self.p = np.asarray(p, float)

    def f(self, x, u): return self.p[0] * x + self.p[1] * u
    def c(self, t, x, u): return 0.5 * self.p[2] * x[:, 0] ** 2 + 0.5 * self.p[3] * u[:, 0] ** 2
    def h(self, x): return 0.5 * self.p[4] * x[:, 0] ** 2
    def fx(self, x, u): return np.full((x.shape[0], 1, 1), self.p[0], dtype=x.dtype)
    def fu(self, x, u): return np.full((x.shape[0], 1, 1), self.p[1], dtype=x.dtype)
    def cx(self, t, x, u): return self.p[2] * x
    def cu(self, t, x, u): return self.p[3] * u
    def hx(self, x): return self.p[4] * x
    def noise(self, z): return self.p[5] * z


class SqrtCost(ScalarLQ):
    source = SQRT_COST

    def c(self, t, x, u): return np.sqrt(np.abs(u[:, 0])) + 0.5 * x[:, 0] ** 2
    def cx(self, t, x, u): return x

    def cu(self, t, x, u):
        with np.errstate(all="ignore"):
            return np.where(np.signbit(u), -1.0, 1.0) * (0.5 / np.sqrt(np.abs(u)))

    def noise(self, z): return np.where(z > 0.0, self.p[5] * z, 0.0)


class Lin2(Case):
    source, n, m, npn = LIN2, 2, 1, 2

    def __init__(self, p=LIN2_P):
        self.p = np.asarray(p, float)
        self.A, self.B = self.p[:4].reshape(2, 2), self.p[4:6].reshape(2, 1)
        self.C = np.array([[self.p[6], 0.0], [self.p[7], self.p[8]]])

    def f(self, x, u): return x @ self.A.T.astype(x.dtype) + u @ self.B.T.astype(x.dtype)
    def c(self, t, x, u): return 0.5 * (x[:, 0] ** 2 + x[:, 1] ** 2) + 0.5 * u[:, 0] ** 2
    def h(self, x): return 0.5 * (x[:, 0] ** 2 + x[:, 1] ** 2)
    def fx(self, x, u): return np.broadcast_to(self.A.astype(x.dtype), (x.shape[0], 2, 2))
    def fu(self, x, u): return np.broadcast_to(self.B.astype(x.dtype), (x.shape[0], 2, 1))
    def cx(self, t, x, u): return x
    def cu(self, t, x, u): return u
    def hx(self, x): return x
    def noise(self, z): return z @ self.C.T.astype(z.dtype)


class Pendulum(Case):
    source, n, m, npn = un.PEND_DIAG, 2, 1, 2

    def __init__(self, p=(0.1, 0.05, 0.1), source=None):
        self.p = np.asarray(p, float)
        if source is not None:
            self.source = source

    def f(self, x, u):
        dt = self.p[0]
        return np.stack([x[:, 0] + dt * x[:, 1], x[:, 1] + dt * (-np.sin(x[:, 0]) - 0.1 * x[:, 1] + u[:, 0])], axis=1)

    def c(self, t, x, u): return 0.5 * (x[:, 0] ** 2 + x[:, 1] ** 2) + 0.05 * u[:, 0] ** 2 + 0.01 * t * x[:, 0]
    def h(self, x): return 2.0 * (x[:, 0] ** 2 + x[:, 1] ** 2)

    def fx(self, x, u):
        dt, one = self.p[0], np.ones(x.shape[0], dtype=x.dtype)
        return np.stack([np.stack([one, dt * one], axis=1), np.stack([-dt * np.cos(x[:, 0]), (1.0 - 0.1 * dt) * one], axis=1)], axis=1)

    def fu(self, x, u):
        out = np.zeros((x.shape[0], 2, 1), dtype=x.dtype)
        out[:, 1, 0] = self.p[0]
        return out

    def cx(self, t, x, u): return np.stack([x[:, 0] + 0.01 * t, x[:, 1]], axis=1)
    def cu(self, t, x, u): return 0.1 * u
    def hx(self, x): return 4.0 * x
    def noise(self, z): return z * self.p[1:3].astype(z.dtype)


class LqCubic(Case):
    """LQ_GAUSS of tests/user_noise_model.py (linear plus cubic dynamics, quadratic cost with an |u| term, w = chol z) at n x m"""
    source = un.LQ_GAUSS

    def __init__(self, n, m, N):
        self.gp = gp = un.lq_generative(n, m, N)
        self.n, self.m, self.npn = n, m, n
        self.p = lq_params(gp)
        onm = 3 * n * n + 2 * n * m + m * m + 2 * n + m + 5
        self.lq, self.q0 = gp.lq, float(np.asarray(gp.lq.q0).ravel()[0])
        assert np.array_equal(self.p[onm:onm + n], gp.nmean)

    def _t(self, a, like): return np.asarray(a, float).astype(like.dtype)

    def f(self, x, u):
        lq = self.lq
        return x @ self._t(lq.A, x).T + u @ self._t(lq.B, x).T + lq.kappa * x ** 3

    def c(self, t, x, u):
        lq = self.lq
        cx = (x * (0.5 * (x @ self._t(lq.Q, x).T) + self._t(lq.qv, x))).sum(axis=1)
        cu = (u * ((0.5 * (u @ self._t(lq.R, x).T) + x @ self._t(lq.P, x).T) + self._t(lq.rv, x))).sum(axis=1)
        return cx + cu + self.q0 + self.gp.l1u * np.abs(u).sum(axis=1)

    def h(self, x):
        lq = self.lq
        return (x * (0.5 * (x @ self._t(lq.Qf, x).T) + self._t(lq.qvf, x))).sum(axis=1) + lq.q0f

    def fx(self, x, u):
        out = np.broadcast_to(self._t(self.lq.A, x), (x.shape[0], self.n, self.n)).copy()
        i = np.arange(self.n)
        out[:, i, i] += 3.0 * self.lq.kappa * x ** 2
        return out

    def fu(self, x, u): return np.broadcast_to(self._t(self.lq.B, x), (x.shape[0], self.n, self.m))

    def cx(self, t, x, u):
        lq = self.lq
        Q = self._t(lq.Q, x)
        return x @ (0.5 * (Q + Q.T)).T + self._t(lq.qv, x) + u @ self._t(lq.P, x)

    def cu(self, t, x, u):
        lq = self.lq
        R = self._t(lq.R, x)
        return u @ (0.5 * (R + R.T)).T + x @ self._t(lq.P, x).T + self._t(lq.rv, x) + self.gp.l1u * np.where(np.signbit(u), -1.0, 1.0)

    def hx(self, x):
        Qf = self._t(self.lq.Qf, x)
        return x @ (0.5 * (Qf + Qf.T)).T + self._t(self.lq.qvf, x)

    def noise(self, z): return z @ np.tril(self._t(self.gp.nchol, z)).T


def policy(case, N, closed=True, seed=5):
    """A fixed policy: a nominal trajectory that is not the rollout of l, so the feedback term works; open loop: (x_0, l, None)"""
    r = np.random.default_rng(seed)
    x_nom = 0.5 + 0.1 * r.standard_normal((N + 1, case.n))
    l = 0.2 * r.standard_normal((N, case.m))
    L = -0.2 * np.abs(r.standard_normal((N, case.m, case.n)))
    return (x_nom, l, L) if closed else (x_nom[0].copy(), l, None)


def draws(case, seed, K, N):
    """the device generator's normals [K, N, npn] under `seed`"""
    return rn.normals(int(seed), 0, int(K), int(N), case.npn)


def rollout(case, x_nom, l, L, z, dtype=np.float64):
    """(J (K,), x (K, N+1, n), u (K, N, m)) on the draws z (K, N, npn): c(0) .. c(N-1) then h, in that order"""
    l = np.asarray(l, float).astype(dtype)
    N, K = l.shape[0], z.shape[0]
    x_nom = np.asarray(x_nom, float).astype(dtype)
    Lq = None if L is None else np.asarray(L, float).astype(dtype)
    z = np.asarray(z).astype(dtype)
    xs, us = np.zeros((K, N + 1, case.n), dtype=dtype), np.zeros((K, N, case.m), dtype=dtype)
    xs[:, 0] = x_nom if L is None else x_nom[0]
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
    """(gu (K, N, m), finite (K,)): dJ_k / du_t with the loop closed downstream, and whether h_x and every g_t are finite"""
    K, N = us.shape[0], us.shape[1]
    Lq = None if L is None else np.asarray(L, float).astype(xs.dtype)
    gu = np.zeros((K, N, case.m), dtype=xs.dtype)
    with np.errstate(all="ignore"):
        lam = case.hx(xs[:, N])
        fin = np.isfinite(lam).all(axis=1)
        for t in range(N - 1, -1, -1):
            x, u = xs[:, t], us[:, t]
            gx = case.cx(t, x, u) + (case.fx(x, u) * lam[:, :, None]).sum(axis=1)
            g_u = case.cu(t, x, u) + (case.fu(x, u) * lam[:, :, None]).sum(axis=1)
            fin &= np.isfinite(gx).all(axis=1) & np.isfinite(g_u).all(axis=1)
            gu[:, t] = g_u
            lam = gx if L is None else gx + g_u @ Lq[t]
    return gu, fin


def gradient(gu, fin, xs, x_nom, L, y, dead, J):
    """(grad_l (R, N, m), grad_L (R, N, m, n) or None, grad_l_se (R, N, m), n_nonfinite, sum p^2 gu^2 (R, N, m)) under the row weights
    y (R, K); the last is the size of the terms the standard error's uncentred form subtracts"""
    dtype = gu.dtype
    ok = ~np.isnan(np.asarray(J, float))
    use = ok & fin
    R, (K, N, m) = y.shape[0], gu.shape
    G = np.where(use[:, None, None], gu, 0)
    gl, se, sc = (np.full((R, N, m), np.nan, dtype=dtype) for _ in range(3))
    gL = None
    if L is not None:
        dx = np.where(use[:, None, None], xs[:, :N] - np.asarray(x_nom, float).astype(dtype)[None, :N], 0)
        gL = np.full((R, N, m, xs.shape[2]), np.nan, dtype=dtype)
    with np.errstate(all="ignore"):
        for r in range(R):
            if dead[r]:
                continue
            w = np.where(use, y[r].astype(dtype), 0)
            sf, sf2 = w.sum(), (w * w).sum()
            mean = (w[:, None, None] * G).sum(axis=0) / sf
            gl[r] = mean
            s2g, s2g2 = ((w * w)[:, None, None] * G).sum(axis=0), ((w * w)[:, None, None] * G * G).sum(axis=0)
            var = ((s2g2 - 2.0 * mean * s2g) + mean * mean * sf2) / (sf * sf)
            sc[r] = s2g2 / (sf * sf)
            se[r] = np.where(var > 0, np.sqrt(np.where(var > 0, var, 0)), np.where(np.isnan(var), np.nan, 0))
            if gL is not None:
                gL[r] = (w[:, None, None, None] * G[:, :, :, None] * dx[:, :, None, :]).sum(axis=0) / sf
    return gl, gL, se, int((ok & ~fin).sum()), sc


def weights(J, kl_bounds=(), thetas=(), alphas=None, dtype=np.float64):
    """(y (R, K) in dtype, dead (R,), rows): the worst-case rows (bounds, then thetas) or, with alphas, the tail levels -- theta, the
    saturated set and the tail's cut from the float64 costs, the exponentials in dtype from the costs J as given"""
    J64 = np.asarray(J).astype(np.float64)
    if alphas is not None:
        y, dead, info = tail_weights(J64, alphas, dtype=dtype)
        return y, dead, info
    y64, dead, wc = row_weights(J64, kl_bounds, thetas)
    th = np.concatenate([wc["bounds"]["theta"], wc["thetas"]["theta"]])
    ok = ~np.isnan(J64)
    y = y64.astype(dtype)
    if dtype != np.float64 and ok.any():
        Jd = np.asarray(J).astype(dtype)
        Jmax = Jd[ok].max()
        for r in range(y.shape[0]):
            smooth = (y64[r][ok] > 0).all() and th[r] != 0.0 and np.isfinite(th[r]) and not dead[r]        # (a searched or tilted row, not a saturated one)
            if smooth:
                d = np.where(ok, Jd, Jmax) - Jmax                        # (0 at the maximum: weight 1 whatever theta is)
                y[r] = np.where(ok, np.where(d == 0, 1, np.exp(dtype(th[r]) * np.where(d == 0, -1, d))), 0)
    return y, dead, wc


def model(case, x_nom, l, L, K, seed, kl_bounds=(), thetas=(), alphas=None, dtype=np.float64, drop_nonfinite=True):
    """The whole call: dict(J, x, u, gu, fin, y, dead, rows, grad_l, grad_L, grad_l_se, n_nonfinite)"""
    N = np.asarray(l).shape[0]
    z = draws(case, seed, K, N)
    J, xs, us = rollout(case, x_nom, l, L, z, dtype)
    gu, fin = adjoint(case, xs, us, L)
    y, dead, rows = weights(J, kl_bounds, thetas, alphas, dtype)
    gl, gL, se, nf, sc = gradient(gu, fin, xs, x_nom, L, y, dead, J)
    return dict(J=J, x=xs, u=us, gu=gu, fin=fin, y=y, dead=dead, rows=rows, grad_l=gl, grad_L=gL, grad_l_se=se, n_nonfinite=nf, se_scale=sc)
