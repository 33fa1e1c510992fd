"""One source-model family for any (n, m) <= (12, 4), with its derivatives in closed form (tests/test_cpu_source_shapes.py,
tests/test_gpu_source_shapes.py).

Everything is a scalar function of a linear form of z = (x, u), so gradients and Hessians are sums of outer products at any size:

    c(k, x, u) = (1 + 0.05 k) F_c(z)        h(x) = F_h(x)
    F(z)   = 1/2 z'Hz + g'z + sum_j a_j phi_j(w_j'z + b_j) + (v1'z)(v2'z) / (3 + (v3'z)^2)
    f_i    = (A x + B u)_i + kappa psi_i(r_i'z)

phi_j runs through every elementary function of csrc/rat_ad.h (PHI below), psi_i cycles sin, tanh, atan and a cube.  H is dense with a
full x-u block, every w_j, v_i and r_i is dense over x and u, A = 0.9 * orthogonal.  The NumPy side is evaluated in np.longdouble and
rounded once to double; the device source gets its derivatives from the AD header: two independent derivations of the same numbers."""
import numpy as np

LD = np.longdouble
ALPHA, BETA = 0.5, 3.0                                                    # the second atan2 argument is ALPHA s + BETA

# (name, device expression in s, offset b_j, weight scale of a_j)
PHI = (("sin", "sin(s)", 0.3, 1.0), ("cos", "cos(s)", 0.5, 1.0), ("tan", "tan(s)", 0.2, 0.5), ("exp", "exp(s)", 0.1, 0.5),
       ("log", "log(s)", 3.0, 1.0), ("sqrt", "sqrt(s)", 3.0, 1.0), ("tanh", "tanh(s)", 0.4, 1.0), ("atan", "atan(s)", -0.6, 1.0),
       ("pow_Td", "pow(s, 2.5)", 2.5, 0.2), ("pow_TT", "pow(s, s)", 1.6, 0.2), ("pow_dT", "pow(1.7, s)", 0.5, 0.5),
       ("atan2_lo", "atan2(s, 0.5 * s + 3.0)", 0.7, 1.0),                # |y| < |x|: the derivatives of atan(y / x)
       ("atan2_hi", "atan2(0.5 * s + 3.0, s)", -0.8, 1.0),               # |y| > |x|, second quadrant: those of -atan(x / y)
       ("fabs", "fabs(s)", -2.5, 1.0), ("fmin", "fmin(s * s, 3.0 * s)", 1.2, 1.0), ("fmax", "fmax(s * s, 3.0 * s)", 1.2, 1.0))
NPHI = len(PHI)


def phi(j, s):
    """phi_j, phi_j', phi_j'' at s (longdouble)."""
    name = PHI[j][0]
    one = LD(1)
    if name == "sin":
        return np.sin(s), np.cos(s), -np.sin(s)
    if name == "cos":
        return np.cos(s), -np.sin(s), -np.cos(s)
    if name == "tan":
        t = np.tan(s)
        return t, one + t * t, 2 * t * (one + t * t)
    if name == "exp":
        return np.exp(s), np.exp(s), np.exp(s)
    if name == "log":
        return np.log(s), one / s, -one / (s * s)
    if name == "sqrt":
        r = np.sqrt(s)
        return r, one / (2 * r), -one / (4 * s * r)
    if name == "tanh":
        t = np.tanh(s)
        return t, one - t * t, -2 * t * (one - t * t)
    if name == "atan":
        d = one + s * s
        return np.arctan(s), one / d, -2 * s / (d * d)
    if name == "pow_Td":
        e = LD(5) / 2
        return s ** e, e * s ** (e - 1), e * (e - 1) * s ** (e - 2)
    if name == "pow_TT":
        v, ls = s ** s, np.log(s) + one
        return v, v * ls, v * (ls * ls + one / s)
    if name == "pow_dT":
        a = LD(17) / 10
        v = a ** s
        return v, v * np.log(a), v * np.log(a) ** 2
    al, be = LD(ALPHA), LD(BETA)
    if name == "atan2_lo":                                                # y = s, x = al s + be
        x, y = al * s + be, s
        r2 = x * x + y * y
        return np.arctan2(y, x), be / r2, -be * (2 * x * al + 2 * y) / (r2 * r2)
    if name == "atan2_hi":                                                # y = al s + be, x = s
        x, y = s, al * s + be
        r2 = x * x + y * y
        return np.arctan2(y, x), -be / r2, be * (2 * x + 2 * y * al) / (r2 * r2)
    if name == "fabs":
        return (s, one, 0 * s) if s > 0 else (-s, -one, 0 * s)
    lo = s * s < 3 * s
    if (name == "fmin") == bool(lo):
        return s * s, 2 * s, 2 * one
    return 3 * s, 3 * one, 0 * s


def phi_margin(j, s):
    """Distance of s from the edge of phi_j's domain, from its kink or from the |y| = |x| switch of atan2 (inf where there is none)."""
    name, s = PHI[j][0], float(s)
    if name == "tan":
        return np.pi / 2 - abs(s)
    if name in ("log", "sqrt", "pow_Td", "pow_TT"):
        return s
    if name in ("atan2_lo", "atan2_hi"):                                  # one argument is s, the other ALPHA s + BETA, the larger
        return abs(ALPHA * s + BETA) - abs(s)
    if name == "fabs":
        return abs(s)
    if name in ("fmin", "fmax"):
        return min(abs(s), abs(3.0 - s))                                  # s^2 = 3 s at s = 0 and s = 3
    return np.inf


SOURCE = r"""
// F(z) = 1/2 z'Hz + g'z + sum_j a_j phi_j(w_j'z + b_j) + (v1'z)(v2'z) / (3 + (v3'z)^2) over d variables.  q: H (d x d), g, a, b, w (NPHI x d), v (3 x d)
#define SHP_NPHI %(nphi)d
#define SHP_NZ (RAT_N + RAT_M)
#define SHP_BLOCK(d) ((d) * (d) + (d) + 2 * SHP_NPHI + SHP_NPHI * (d) + 3 * (d))
template <class T> __device__ T shp_phi(int j, const T &s) {
    switch (j) {
%(cases)s
    }
    return s;
}
template <class T> __device__ T shp_form(const T *z, int d, const double *q) {
    const double *H = q, *g = H + d * d, *a = g + d, *b = a + SHP_NPHI, *w = b + SHP_NPHI, *v = w + SHP_NPHI * d;
    T acc = 0.0;
    for (int i = 0; i < d; ++i) {
        T row = 0.0;
        for (int j = 0; j < d; ++j) row += H[i * d + j] * z[j];
        acc += z[i] * row;
    }
    acc *= 0.5;
    for (int i = 0; i < d; ++i) acc += g[i] * z[i];
    for (int j = 0; j < SHP_NPHI; ++j) {
        T s = b[j];
        for (int i = 0; i < d; ++i) s += w[j * d + i] * z[i];
        acc += a[j] * shp_phi<T>(j, s);
    }
    T l1 = 0.0, l2 = 0.0, l3 = 0.0;
    for (int i = 0; i < d; ++i) { l1 += v[i] * z[i]; l2 += v[d + i] * z[i]; l3 += v[2 * d + i] * z[i]; }
    T den = l3;
    den *= l3;
    den += 3.0;
    l1 *= l2;
    l1 /= den;
    return acc + l1;
}
// p: A (n x n, row-major), B (n x m), kappa, r (n x nz), the block of c over z, the block of h over x%(extra_doc)s
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) {
    const double *A = p, *B = A + RAT_N * RAT_N, kap = B[RAT_N * RAT_M], *r = B + RAT_N * RAT_M + 1;
    for (int i = 0; i < RAT_N; ++i) {
        T lin = 0.0, s = 0.0;
        for (int j = 0; j < RAT_N; ++j) { lin += A[i * RAT_N + j] * x[j]; s += r[i * SHP_NZ + j] * x[j]; }
        for (int g = 0; g < RAT_M; ++g) { lin += B[i * RAT_M + g] * u[g]; s += r[i * SHP_NZ + RAT_N + g] * u[g]; }
        T psi;
        switch (i %% 4) {
        case 0: psi = sin(s); break;
        case 1: psi = tanh(s); break;
        case 2: psi = atan(s); break;
        default: psi = s * s * s; break;
        }
        xn[i] = lin + kap * psi;
    }
}
#define SHP_PC (RAT_N * RAT_N + RAT_N * RAT_M + 1 + RAT_N * SHP_NZ)
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) {
    T z[SHP_NZ];
    for (int i = 0; i < RAT_N; ++i) z[i] = x[i];
    for (int g = 0; g < RAT_M; ++g) z[RAT_N + g] = u[g];
    T c = (1.0 + 0.05 * k) * shp_form<T>(z, SHP_NZ, p + SHP_PC);%(extra_c)s
    return c;
}
template <class T> __device__ T rat_user_h(const T *x, const double *p) {
    T c = shp_form<T>(x, RAT_N, p + SHP_PC + SHP_BLOCK(SHP_NZ));%(extra_h)s
    return c;
}
"""

# the domain variant: log(x_0 - threshold) in c at k = 2 and in h, each with a threshold of its own after the two blocks
_EXTRA = dict(
    extra_doc=", thr_c, thr_h",
    extra_c="\n    c += (k == 2 ? 1.0 : 0.0) * log(x[0] - p[SHP_PC + SHP_BLOCK(SHP_NZ) + SHP_BLOCK(RAT_N)]);",
    extra_h="\n    c += log(x[0] - p[SHP_PC + SHP_BLOCK(SHP_NZ) + SHP_BLOCK(RAT_N) + 1]);")


def source(domain_variant=False):
    cases = "\n".join(f"    case {j}: return {expr};" for j, (_, expr, _, _) in enumerate(PHI))
    extra = _EXTRA if domain_variant else dict(extra_doc="", extra_c="", extra_h="")
    return SOURCE % dict(nphi=NPHI, cases=cases, **extra)


class Block:
    """The parameters of one F over d variables."""

    def __init__(self, rng, d):
        M = rng.standard_normal((d, d))
        self.d = d
        self.H = M @ M.T / d + 3.0 * np.eye(d)                            # dense, symmetric, positive definite
        self.g = 0.3 * rng.standard_normal(d)
        self.a = np.array([sc for (_, _, _, sc) in PHI]) * rng.choice([-1.0, 1.0], NPHI) * rng.uniform(0.5, 1.5, NPHI)
        self.b = np.array([b for (_, _, b, _) in PHI])
        self.w = 0.35 * rng.standard_normal((NPHI, d)) / np.sqrt(d)
        self.v = rng.standard_normal((3, d)) / np.sqrt(d)

    def pack(self):
        return np.concatenate([self.H.ravel(), self.g, self.a, self.b, self.w.ravel(), self.v.ravel()])

    def eval(self, z):
        """F, grad F, hess F at z, in longdouble."""
        z = np.asarray(z, LD)
        H, g, w, v = (np.asarray(t, LD) for t in (self.H, self.g, self.w, self.v))
        val = z @ H @ z / 2 + g @ z
        grad = H @ z + g
        hess = H.copy()
        for j in range(NPHI):
            p0, p1, p2 = phi(j, w[j] @ z + LD(self.b[j]))
            a = LD(self.a[j])
            val = val + a * p0
            grad = grad + a * p1 * w[j]
            hess = hess + a * p2 * np.outer(w[j], w[j])
        l1, l2, l3 = v @ z
        D = 3 + l3 * l3
        val = val + l1 * l2 / D
        s12 = l2 * v[0] + l1 * v[1]
        grad = grad + s12 / D - 2 * l1 * l2 * l3 / (D * D) * v[2]
        hess = hess + (np.outer(v[0], v[1]) + np.outer(v[1], v[0])) / D - 2 * l3 / (D * D) * (np.outer(s12, v[2]) + np.outer(v[2], s12)) \
            - l1 * l2 * (2 / (D * D) - 8 * l3 * l3 / (D * D * D)) * np.outer(v[2], v[2])
        return val, grad, hess

    def margin(self, z):
        return min(phi_margin(j, self.w[j] @ np.asarray(z, float) + self.b[j]) for j in range(NPHI))


class Model:
    """model(n, m, seed): device source, packed p and the NumPy closed forms of f, c, h and of their derivatives."""

    def __init__(self, n, m, seed, kappa=0.05, domain_thresholds=None):
        rng = np.random.default_rng(seed)
        self.n, self.m, self.nz, self.kappa = n, m, n + m, float(kappa)
        Qo, _ = np.linalg.qr(rng.standard_normal((n, n)))
        self.A = 0.9 * Qo
        self.B = rng.standard_normal((n, m)) / np.sqrt(n)
        self.r = rng.standard_normal((n, self.nz)) / np.sqrt(self.nz)
        self.bc, self.bh = Block(rng, self.nz), Block(rng, n)
        self.thr = domain_thresholds
        self.source = source(domain_variant=domain_thresholds is not None)
        self.p = np.concatenate([self.A.ravel(), self.B.ravel(), [self.kappa], self.r.ravel(), self.bc.pack(), self.bh.pack(),
                                 [] if domain_thresholds is None else list(domain_thresholds)])

    # ---- closed forms, longdouble inside, rounded once ---------------------------------------------------------------------------
    def _f(self, x, u):
        z = np.concatenate([np.asarray(x, LD), np.asarray(u, LD)])
        A, B, r, kap = np.asarray(self.A, LD), np.asarray(self.B, LD), np.asarray(self.r, LD), LD(self.kappa)
        s = r @ z
        psi, dpsi = np.zeros(self.n, LD), np.zeros(self.n, LD)
        for i in range(self.n):
            if i % 4 == 0:
                psi[i], dpsi[i] = np.sin(s[i]), np.cos(s[i])
            elif i % 4 == 1:
                psi[i] = np.tanh(s[i]); dpsi[i] = 1 - psi[i] ** 2
            elif i % 4 == 2:
                psi[i], dpsi[i] = np.arctan(s[i]), 1 / (1 + s[i] ** 2)
            else:
                psi[i], dpsi[i] = s[i] ** 3, 3 * s[i] ** 2
        xn = A @ z[:self.n] + B @ z[self.n:] + kap * psi
        J = np.hstack([A, B]) + kap * dpsi[:, None] * r
        return xn, J

    def f(self, x, u, f_returns_jacobian=False):
        xn, J = self._f(x, u)
        if not f_returns_jacobian:
            return xn.astype(np.float64)
        return xn.astype(np.float64), J[:, :self.n].astype(np.float64), J[:, self.n:].astype(np.float64)

    def jac(self, x, u):
        return self.f(x, u, True)[1:]

    def c_all(self, k, x, u):
        """c and (q_vec, Q, r_vec, R, P) of the reference's cost_derivs; P is m x n (c_ux)."""
        n = self.n
        val, g, Hs = self.bc.eval(np.concatenate([x, u]))
        sc = 1 + LD(5) / 100 * k
        val, g, Hs = (np.asarray(sc * t).astype(np.float64) for t in (val, g, Hs))
        return float(val), (g[:n], Hs[:n, :n], g[n:], Hs[n:, n:], Hs[n:, :n])

    def c(self, k, x, u):
        return self.c_all(k, x, u)[0]

    def c_derivatives(self, k, x, u):
        return self.c_all(k, x, u)[1]

    def h_all(self, x):
        val, g, Hs = self.bh.eval(x)
        return float(val), (g.astype(np.float64), Hs.astype(np.float64))

    def h(self, x):
        return self.h_all(x)[0]

    def h_derivatives(self, x):
        return self.h_all(x)[1]

    def margin(self, x, u):
        """The smallest distance, over a trajectory, of any phi argument from a domain edge, a kink or the atan2 switch."""
        x, u = np.atleast_2d(x), np.atleast_2d(u)
        mc = min(self.bc.margin(np.concatenate([x[t], u[t]])) for t in range(len(u)))
        return min(mc, min(self.bh.margin(xx) for xx in x))

    # ---- whole-trajectory references ---------------------------------------------------------------------------------------------
    def rollout(self, x0, u, xbar=None, L=None):
        """Open loop from x0, or closed loop u_t = l_t + L_t (x_t - xbar_t) from xbar_0 (then `u` is l)."""
        N = len(u)
        x, uo = np.zeros((N + 1, self.n)), np.zeros((N, self.m))
        x[0] = x0 if xbar is None else xbar[0]
        for t in range(N):
            uo[t] = u[t] if L is None else u[t] + L[t] @ (x[t] - xbar[t])
            x[t + 1] = self.f(x[t], uo[t])
        return x, uo

    def approximation(self, u, x, W):
        """The ApproximationResult arrays of approximate_model(problem, u, x) as a dict of reference values."""
        N, n, m = len(u), self.n, self.m
        o = dict(q_array=np.zeros(N + 1), q_vec_array=np.zeros((N + 1, n)), Q_array=np.zeros((N + 1, n, n)), r_array=np.zeros((N, m)),
                 R_array=np.zeros((N, m, m)), P_array=np.zeros((N, m, n)), A_array=np.zeros((N, n, n)), B_array=np.zeros((N, n, m)),
                 W_array=np.stack([np.asarray(W(k), float) for k in range(N)]))
        for k in range(N):
            o["q_array"][k], (o["q_vec_array"][k], o["Q_array"][k], o["r_array"][k], o["R_array"][k], o["P_array"][k]) = self.c_all(k, x[k], u[k])
            o["A_array"][k], o["B_array"][k] = self.jac(x[k], u[k])
        o["q_array"][N], (o["q_vec_array"][N], o["Q_array"][N]) = self.h_all(x[N])
        return o


def model(n, m, seed, kappa=0.05, domain_thresholds=None):
    return Model(n, m, seed, kappa, domain_thresholds)


def noise(n):
    """A time-varying W(k)."""
    return lambda k: (1e-3 + 1e-4 * k) * np.eye(n)


# ---- the shapes and the solve cases of the two test files ---------------------------------------------------------------------------
SHAPES = ((12, 4), (11, 4), (12, 3), (10, 1), (7, 3), (3, 2), (1, 4), (1, 1))
SEED = {s: 100 + 16 * s[0] + s[1] for s in SHAPES}
SOLVE_SHAPES = ((12, 4), (10, 1), (7, 3), (1, 4))
SOLVE_N, SOLVE_THETAS = 9, (0.0, 0.5, 1.5)
# kappa and the scale of x_0, chosen on the oracle (tests/test_cpu_source_shapes.py asserts what they are chosen for): every solve ends
# with status 0 after at least two iterations, and at (10, 1), theta = 1.5 the line search rejects candidates
SOLVE_KAPPA = {(12, 4): (0.35, 1.0), (10, 1): (0.35, 1.0), (7, 3): (0.3, 0.5), (1, 4): (0.3, 0.5)}


def solve_case(n, m):
    """(model, x_0, u_array) of the solve tests at (n, m): N = SOLVE_N, W = noise(n)."""
    kappa, scale = SOLVE_KAPPA[(n, m)]
    mdl = model(n, m, SEED[(n, m)], kappa)
    rng = np.random.default_rng(SEED[(n, m)] + 1)
    return mdl, scale * rng.standard_normal(n), np.zeros((SOLVE_N, m))


LIN_CASES = tuple((s, N) for s in ((12, 4), (10, 1)) for N in (1, 3, 4, 8, 9)) + tuple((s, 4) for s in SHAPES if s not in ((12, 4), (10, 1)))


def lin_case(n, m, N):
    """(model, x trajectory, u trajectory) of the linearisation test at (n, m, N): a random trajectory, not a rollout."""
    mdl = model(n, m, SEED[(n, m)])
    rng = np.random.default_rng(1000 * N + SEED[(n, m)])
    return mdl, 0.7 * rng.standard_normal((N + 1, n)), 0.7 * rng.standard_normal((N, m))


DOMAIN_SHAPE, DOMAIN_N, DOMAIN_OFF = (3, 2), 4, -1e3                      # DOMAIN_OFF: a threshold no trajectory reaches


def domain_case(which):
    """The (3, 2) model with log(x_0 - thr) in c at k = 2 (which = "c") or in h (which = "h"), a start (x_0, u_array) whose open-loop
    rollout takes x_0's first component below the threshold at that step only, and that rollout.  Returns (model, x_0, u, x)."""
    n, m = DOMAIN_SHAPE
    base = model(n, m, SEED[DOMAIN_SHAPE])
    rng = np.random.default_rng(77)
    x0, u = 0.2 * rng.standard_normal(n), np.zeros((DOMAIN_N, m))
    t = 2 if which == "c" else DOMAIN_N
    u[t - 1] = -2.0 * base.B[0] / (base.B[0] @ base.B[0])                 # moves (x_t)_0 by about -2
    x, _ = base.rollout(x0, u)
    others = np.delete(x[:, 0], t)
    assert x[t, 0] < others.min() - 0.5
    thr = x[t, 0] + 0.25
    return model(n, m, SEED[DOMAIN_SHAPE], domain_thresholds=(thr, DOMAIN_OFF) if which == "c" else (DOMAIN_OFF, thr)), x0, u, x
