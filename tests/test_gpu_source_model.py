"""Source models (RAT_MODEL_SOURCE): f, c, h written as device code, compiled at run time, rollouts and linearisations on the GPU
(csrc/source_kernels.h), everything after them on the family's round-based machinery.  Checked against NumPy closed forms, the
oracle's closure path, the LQ family and the host-closure path (tests/test_gpu_generic.py's problems, copied here)."""
import ctypes as C

import numpy as np
import pytest

import ratilqr.jl_amd as rat
from ratilqr.jl_amd import cross_entropy as ce
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---- the pendulum of test_gpu_generic.py: closures, oracle closure problem and the same model as device source -------------------
N_P, DT = 25, 0.1
W_P = lambda k: (1e-3 + 1e-4 * k) * np.eye(2)                                              # time-varying noise

PENDULUM = r"""
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
PENDULUM_JAC = PENDULUM + r"""
#define RAT_USER_F_JACOBIAN
__device__ void rat_user_f_jacobian(const double *x, const double *u, double *xn, double *A, double *B, const double *p) {
    const double dt = p[0];
    rat_user_f<double>(x, u, xn, p);
    A[0] = 1.0; A[1] = -dt * cos(x[0]); A[2] = dt; A[3] = 1.0 - 0.1 * dt;
    B[0] = 0.0; B[1] = dt;
}
"""


def pendulum():
    n, m, N, dt = 2, 1, N_P, DT

    def f(x, u, f_returns_jacobian=False):
        xn = np.array([x[0] + dt * x[1], x[1] + dt * (-np.sin(x[0]) - 0.1 * x[1] + u[0])])
        if not f_returns_jacobian:
            return xn
        return xn, np.array([[1.0, dt], [-dt * np.cos(x[0]), 1.0 - 0.1 * dt]]), np.array([[0.0], [dt]])

    c = lambda k, x, u: 0.5 * (x @ x) + 0.05 * (u @ u) + 0.01 * k * x[0]
    cd = lambda k, x, u: (x + np.array([0.01 * k, 0.0]), np.eye(2), 0.1 * u, 0.1 * np.eye(1), np.zeros((1, 2)))
    h = lambda x: 2.0 * (x @ x)
    hd = lambda x: (4.0 * x, 4.0 * np.eye(2))
    gen = rat.GenericRiskSensitiveProblem(f, c, h, W_P, N, n, m, f_returns_jacobian=True, c_derivatives=cd, h_derivatives=hd)
    cp = orc.ClosureProblem(lambda x, u: f(x, u), c, h, W_P, N, n, m, lambda x, u: f(x, u, True)[1:], cd, hd)
    return gen, cp, np.array([1.0, 0.0]), np.zeros((N, m))


def source_pendulum(src=PENDULUM, dt=DT):
    return rat.DeviceSourceProblem(src, 2, 1, N_P, W_P, params=[dt])


def check_against_oracle(r, s, x, l, L, v, hist, vt=1e-9):
    assert r["status"] == 0 and r["iters"] == s.iter_current and r["ls_evals"] == len(hist)
    assert [e[0] for e in hist] == [e[0] for e in r["eps_history"]]
    assert abs(v - r["value"]) <= vt * abs(r["value"])
    assert rel(x, r["x"]) < 1e-9 and rel(l, r["l"]) < 1e-9 and rel(L, r["L"]) < 1e-9


def test_operators_against_closed_forms():
    """The pendulum (2, 1): the m x m block of R and the n x n block of Q.  The full-tile shapes, every pair-loop regime up to (12, 4), are in
    tests/test_gpu_source_shapes.py."""
    prob = source_pendulum()
    rng = np.random.default_rng(7)
    x0, u = rng.standard_normal(2), 0.3 * rng.standard_normal((N_P, 1))
    # simulate_dynamics, open loop
    xr = np.zeros((N_P + 1, 2)); xr[0] = x0
    for t in range(N_P):
        xr[t + 1] = [xr[t, 0] + DT * xr[t, 1], xr[t, 1] + DT * (-np.sin(xr[t, 0]) - 0.1 * xr[t, 1] + u[t, 0])]
    xs = rat.simulate_dynamics(prob, x0, u)
    assert rel(xs, xr) < 1e-12
    # closed loop under l + L (x - xbar): a nominal trajectory that is not the rollout of l, so x_t - xbar_t != 0 from t = 1 on
    L = 0.2 * rng.standard_normal((N_P, 1, 2))
    xbar = xr + np.vstack([np.zeros((1, 2)), 0.05 * rng.standard_normal((N_P, 2))])
    xc, uc = np.zeros_like(xr), np.zeros_like(u)
    xc[0] = xbar[0]
    for t in range(N_P):
        uc[t] = u[t] + L[t] @ (xc[t] - xbar[t])
        xc[t + 1] = [xc[t, 0] + DT * xc[t, 1], xc[t, 1] + DT * (-np.sin(xc[t, 0]) - 0.1 * xc[t, 1] + uc[t, 0])]
    xn, un = rat.simulate_dynamics(prob, xbar, u, L)
    assert rel(xn, xc) < 1e-12 and rel(un, uc) < 1e-12
    assert rel(un, u) > 1e-3                                           # the feedback term is exercised
    # approximate_model and integrate_cost at a random trajectory
    xt, ut = rng.standard_normal((N_P + 1, 2)), rng.standard_normal((N_P, 1))
    ap = rat.approximate_model(prob, ut, xt)
    k = np.arange(N_P)
    q = 0.5 * (xt[:N_P] ** 2).sum(1) + 0.05 * ut[:, 0] ** 2 + 0.01 * k * xt[:N_P, 0]
    want = dict(
        q_array=np.append(q, 2.0 * xt[N_P] @ xt[N_P]),
        q_vec_array=np.vstack([xt[:N_P] + np.c_[0.01 * k, np.zeros(N_P)], 4.0 * xt[N_P]]),
        Q_array=np.concatenate([np.repeat(np.eye(2)[None], N_P, 0), 4.0 * np.eye(2)[None]]),
        r_array=0.1 * ut, R_array=np.full((N_P, 1, 1), 0.1), P_array=np.zeros((N_P, 1, 2)),
        A_array=np.array([[[1.0, DT], [-DT * np.cos(a), 1.0 - 0.1 * DT]] for a in xt[:N_P, 0]]),
        B_array=np.repeat(np.array([[0.0], [DT]])[None], N_P, 0),
        W_array=np.array([W_P(kk) for kk in range(N_P)]))
    for name, w in want.items():
        got = getattr(ap, name)
        assert got.shape == w.shape and np.abs(got - w).max() <= 1e-12 * max(1.0, np.abs(w).max()), name
    assert abs(rat.integrate_cost(prob, xt, ut) - want["q_array"].sum()) <= 1e-12 * abs(want["q_array"].sum())


@pytest.mark.parametrize("theta", [0.0, 0.5, 1.5])
def test_solve_against_the_oracle_closure_path(theta):
    _, cp, x0, u0 = pendulum()
    prob = source_pendulum()
    s = rat.ILEQGSolver(prob)
    x, l, L, v, hist = rat.solve_(s, prob, x0, u0, theta=theta)
    check_against_oracle(orc.closure_solve(cp, x0, u0, theta), s, x, l, L, v, hist)
    if theta == 1.5:
        assert orc.closure_solve(cp, x0, u0, 3.0)["status"] == 1
        with pytest.raises(AssertionError):
            rat.solve_(rat.ILEQGSolver(prob), prob, x0, u0, theta=3.0)


LQ_SOURCE = r"""
// LQ + cubic drift, every cost term scaled by (1 + 0.05 k).  p: A, B (column-major), Q, R, P, qv, rv, q0, kappa, Qf
#define NN (RAT_N * RAT_N)
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) {
    const double *A = p, *B = p + NN, kap = p[2 * NN + RAT_N * RAT_M + RAT_M * RAT_M + RAT_M * RAT_N + RAT_N + RAT_M + 1];
    for (int i = 0; i < RAT_N; ++i) {
        T acc = 0.0;
        for (int j = 0; j < RAT_N; ++j) acc += A[i + RAT_N * j] * x[j];
        for (int g = 0; g < RAT_M; ++g) acc += B[i + RAT_N * g] * u[g];
        xn[i] = acc + kap * (x[i] * x[i] * x[i]);
    }
}
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) {
    const double *Q = p + NN + RAT_N * RAT_M, *R = Q + NN, *P = R + RAT_M * RAT_M, *qv = P + RAT_M * RAT_N, *rv = qv + RAT_N, *q0 = rv + RAT_M;
    T c = q0[0];
    for (int i = 0; i < RAT_N; ++i) {
        c += qv[i] * x[i];
        for (int j = 0; j < RAT_N; ++j) c += 0.5 * Q[i + RAT_N * j] * (x[i] * x[j]);
    }
    for (int g = 0; g < RAT_M; ++g) {
        c += rv[g] * u[g];
        for (int g2 = 0; g2 < RAT_M; ++g2) c += 0.5 * R[g + RAT_M * g2] * (u[g] * u[g2]);
        for (int j = 0; j < RAT_N; ++j) c += P[g + RAT_M * j] * (u[g] * x[j]);
    }
    return (1.0 + 0.05 * k) * c;
}
template <class T> __device__ T rat_user_h(const T *x, const double *p) {
    const double *Qf = p + 2 * NN + RAT_N * RAT_M + RAT_M * RAT_M + RAT_M * RAT_N + RAT_N + RAT_M + 2;
    T c = 0.0;
    for (int i = 0; i < RAT_N; ++i)
        for (int j = 0; j < RAT_N; ++j) c += 0.5 * Qf[i + RAT_N * j] * (x[i] * x[j]);
    return c;
}
"""


def lq_pair():
    rng = np.random.default_rng(2)
    n, m, N = 4, 2, 12
    Qo, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A, B = 0.9 * Qo, rng.standard_normal((n, m)) / np.sqrt(n)
    Q, R, P = np.eye(n), 0.3 * np.eye(m), 0.05 * rng.standard_normal((m, n))
    qv, rv, q0, kap, W, Qf = 0.1 * rng.standard_normal(n), 0.1 * rng.standard_normal(m), 0.2, 0.02, 1e-3 * np.eye(n), np.eye(n)
    s = 1.0 + 0.05 * np.arange(N)
    fam = rat.LQRiskSensitiveProblem(A, B, Q=s[:, None, None] * Q, R=s[:, None, None] * R, P=s[:, None, None] * P, qv=s[:, None] * qv,
                                     rv=s[:, None] * rv, q0=s * q0, N=N, W=W, Qf=Qf, kappa=kap)
    params = np.concatenate([A.T.ravel(), B.T.ravel(), Q.T.ravel(), R.T.ravel(), P.T.ravel(), qv, rv, [q0, kap], Qf.T.ravel()])
    src = rat.DeviceSourceProblem(LQ_SOURCE, n, m, N, W, params=params)
    return fam, src, 0.5 * rng.standard_normal(n), np.zeros((N, m))


def test_lq_source_against_the_family():
    fam, src, x0, u = lq_pair()
    for theta in (0.0, 1.5, 6.0):
        s1, s2 = rat.ILEQGSolver(fam, adaptive_eps_init=True), rat.ILEQGSolver(src, adaptive_eps_init=True)
        x1, l1, L1, v1, h1 = rat.solve_(s1, fam, x0, u, theta=theta)
        x2, l2, L2, v2, h2 = rat.solve_(s2, src, x0, u, theta=theta)
        assert s1.iter_current == s2.iter_current and [e[0] for e in h1] == [e[0] for e in h2], theta
        assert abs(v1 - v2) <= 1e-10 * abs(v1) and rel(x2, x1) < 1e-10 and rel(L2, L1) < 1e-9, theta


def test_batch_of_1024_against_closure_batch_and_per_sample_solves():
    gen, cp, x0, u0 = pendulum()
    prob = source_pendulum()
    theta = np.concatenate([np.linspace(0.0, 2.0, 1020), [0.25, 1e4, 3.0, 0.75]])
    ctx = rat.Context(prob, max_batch=1024)
    val, st, it, ls = ctx.solve_batch(x0, u0, theta)
    assert ctx.get_path(1024) == "rounds"
    sub = np.arange(0, 1024, 32)
    vg, sg, ig, lg = rat.solve_closure_batch(gen, x0, u0, theta[sub])
    assert np.array_equal(st[sub], sg) and np.array_equal(it[sub], ig) and np.array_equal(ls[sub], lg)
    ok = sg == 0
    assert np.all(np.abs(val[sub][ok] - vg[ok]) <= 1e-9 * np.abs(vg[ok]))
    assert st[1021] != 0 and np.isposinf(val[1021])
    for b in (0, 500, 1000, 1023):
        r = rat.Context(prob).solve(x0, u0, theta[b])
        assert r["status"] == st[b] and r["iters"] == it[b]
        if st[b] == 0:
            assert abs(r["value"] - val[b]) <= 1e-12 * abs(val[b])
    # speculative line search (spec_eps = 4, forced) gives the same counts
    ctx4 = rat.Context(prob, max_batch=1024, spec_eps=4)
    ctx4.debug_set("spec_force", 1)
    assert ctx4.debug_get("spec_width") == 4
    v4, s4, i4, l4 = ctx4.solve_batch(x0, u0, theta)
    assert np.array_equal(s4, st) and np.array_equal(i4, it) and np.array_equal(l4, ls)
    fin = np.isfinite(val)
    assert np.array_equal(fin, np.isfinite(v4)) and np.all(np.abs(v4[fin] - val[fin]) <= 1e-12 * np.abs(val[fin]))


def closure_ce(gen, x0, u0, z, kl, **kw):
    """The Cross-Entropy loop of rat_ce_solve (cross_entropy_bilevel_optimization.jl:252-335, :364-382) driven from here over the
    host-closure problem: draws from the stream z, costs from solve_closure_batch.  Returns theta_opt and the elite set of every step."""
    L = rat.native.lib()
    g = rat.CrossEntropyBilevelOptimizationSolver(**kw)
    c = g.c
    L.rat_ce_initialize(C.byref(c))
    zc = np.ascontiguousarray(z, dtype=np.float64)
    pos, redraw, elites = C.c_int64(0), C.c_int32(0), []
    B = int(c.num_samples)
    while c.iter_current < c.iter_max:
        L.rat_ce_begin_step(C.byref(c))
        while True:
            th = np.zeros(B)
            rat.native.check(L.rat_ce_draw_stream(C.byref(c), rat.native.P(zc), C.c_int64(zc.size), C.byref(pos), rat.native.P(th)))
            cost = rat.compute_cost(g, gen, x0, u0, th, kl)
            rat.native.check(L.rat_ce_update(C.byref(c), rat.native.P(th), rat.native.P(cost), C.byref(redraw)))
            if not redraw.value:
                break
        elites.append(np.sort(th[np.argsort(cost, kind="stable")[: int(c.num_elite)]]))
    return c.mu, elites


def test_cross_entropy_against_the_host_closure_problem():
    gen, _, x0, u0 = pendulum()
    prob = source_pendulum()
    z = np.random.default_rng(12344).standard_normal(20000)
    kl, kw = 0.5, dict(num_samples=16, num_elite=4, iter_max=3)
    th_ref, elites_ref = closure_ce(gen, x0, u0, z, kl, **kw)
    # rat_ce_solve on the source problem, same stream: theta_opt agrees with the closure problem's CE
    a = rat.CrossEntropyBilevelOptimizationSolver(**kw)
    ra = ce.solve_(a, prob, x0, u0, z, kl_bound=kl)
    assert a.c.n_final_retries == 0 and np.isfinite(ra[4])
    assert abs(ra[0] - th_ref) <= 1e-9 * abs(th_ref), (ra[0], th_ref)
    # the Python-driven loop (step_) on the source problem: the same elite sets, step by step, and costs equal to the closure problem's
    c = rat.CrossEntropyBilevelOptimizationSolver(**kw)
    g = rat.CrossEntropyBilevelOptimizationSolver(**kw)
    ce.initialize_(c)
    for it in range(3):
        th, cost = ce.step_(c, prob, x0, u0, kl, z)
        assert np.array_equal(np.sort(th[np.argsort(cost, kind="stable")[:4]]), elites_ref[it]), it
        cg = rat.compute_cost(g, gen, x0, u0, th, kl)
        assert np.array_equal(np.isinf(cost), np.isinf(cg))
        f = np.isfinite(cg)
        assert np.all(np.abs(cost[f] - cg[f]) <= 1e-9 * np.abs(cg[f]))
    assert abs(c.mu - th_ref) <= 1e-9 * abs(th_ref)


def test_set_params_equals_a_fresh_source_with_that_constant():
    _, _, x0, u0 = pendulum()
    prob = source_pendulum()
    ctx = rat.Context(prob)
    ctx.set_params([0.05])
    r1 = ctx.solve(x0, u0, 0.5)
    fixed = rat.DeviceSourceProblem(PENDULUM.replace("const double dt = p[0];", "const double dt = 0.05;"), 2, 1, N_P, W_P)
    r2 = rat.Context(fixed).solve(x0, u0, 0.5)
    assert r1["iters"] == r2["iters"] and r1["value"] == r2["value"] and np.array_equal(r1["x"], r2["x"])
    # the parameters belong to the handle: the problem object and the other handles bound to it keep theirs
    assert np.array_equal(prob.params, [DT]) and np.array_equal(ctx.params, [0.05])
    r0 = rat.Context(prob).solve(x0, u0, 0.5)
    assert r0["value"] == rat.Context(source_pendulum()).solve(x0, u0, 0.5)["value"] != r1["value"]
    ctx.set_problem(prob)                                              # setting the problem again uploads its own parameters
    assert ctx.solve(x0, u0, 0.5)["value"] == r0["value"]
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG"):
        ctx.set_params([0.05, 1.0])


def test_domain_error_of_a_sqrt_model():
    src = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) { xn[0] = sqrt(x[0]) + u[0]; }
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) { return x[0] * x[0] + u[0] * u[0]; }
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return x[0] * x[0]; }
"""
    prob = rat.DeviceSourceProblem(src, 1, 1, 10, np.eye(1) * 1e-2)
    ctx = rat.Context(prob, max_batch=2)
    val, st, it, ls = ctx.solve_batch(np.array([0.5]), -np.ones((10, 1)), np.array([0.0, 0.5]))
    assert np.all(st == rat.native.ST_DOMAIN) and np.all(np.isposinf(val))
    with pytest.raises(ArithmeticError):
        ctx.rollout_open(np.array([0.5]), -np.ones((10, 1)))


def test_exact_jacobian_agrees_with_ad():
    rng = np.random.default_rng(3)
    xt, ut = rng.standard_normal((N_P + 1, 2)), rng.standard_normal((N_P, 1))
    a1 = rat.approximate_model(source_pendulum(), ut, xt)
    a2 = rat.approximate_model(source_pendulum(PENDULUM_JAC), ut, xt)
    assert np.abs(a1.A_array - a2.A_array).max() <= 1e-12 and np.abs(a1.B_array - a2.B_array).max() <= 1e-12
    _, _, x0, u0 = pendulum()
    r1, r2 = rat.Context(source_pendulum()).solve(x0, u0, 0.5), rat.Context(source_pendulum(PENDULUM_JAC)).solve(x0, u0, 0.5)
    assert r1["iters"] == r2["iters"] and abs(r1["value"] - r2["value"]) <= 1e-12 * abs(r1["value"])


def test_refusals_and_a_failed_recompile_keeps_the_problem():
    _, _, x0, u0 = pendulum()
    prob = source_pendulum()
    ctx = rat.Context(prob)
    for path in ("fused", "block"):
        with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED"):
            ctx.set_path(path)
    ctx.set_path("rounds")
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED"):
        ctx.rollout_noisy(np.zeros((N_P + 1, 2)), np.zeros((N_P, 1)), K=4)
    before = ctx.solve(x0, u0, 0.5)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG") as e:
        ctx.set_problem(rat.DeviceSourceProblem(PENDULUM.replace("sin(", "sine("), 2, 1, N_P, W_P, params=[DT]))
    assert "sine" in str(e.value)
    after = ctx.solve(x0, u0, 0.5)
    assert after["iters"] == before["iters"] and after["value"] == before["value"]
