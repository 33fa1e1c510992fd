"""Generative source models on the GPU (rat_pets_problem_set_source, csrc/source_pets.h): PETS over f_stochastic, c, h written as device
code.  Checked against the oracle (the LQ family written as source), the reference's pets_test.jl, NumPy restatements of
compute_cost_worker on the same injected draws, the host loop (device-resident solve!), and a host restatement of the generator."""
import ctypes as C

import numpy as np
import pytest

import ratilqr.jl_amd as rat
from ratilqr.jl_amd import _native as nv
from ratilqr.jl_amd import pets
from oracle import oracle as orc
from source_pets_models import (DOCS, DOCS_DIMS, LQ, PENDULUM, PENDULUM_DIMS, PENDULUM_P, REF_TEST, REF_TEST_DIMS, docs_c, docs_f,
                                docs_h, lq_params, np_compute_cost, pendulum_c, pendulum_f, pendulum_h)
from test_gpu_pets import _philox4x32_10, rich_problem

pytestmark = pytest.mark.gpu


def gsp(src, d, N, params=None, **kw):
    a = dict(normals_per_step=d["normals_per_step"], uniforms_per_step=d["uniforms_per_step"])
    a.update(kw)
    return rat.DeviceGenerativeSourceProblem(src, d["n"], d["m"], N, params=params, **a)


def solver(N, m, S, K, **kw):
    return rat.CrossEntropyDirectOptimizationSolver(np.zeros((N, m)), np.stack([np.eye(m)] * N), num_control_samples=S,
                                                    num_trajectory_samples=K, **kw)


def cost_on(h, x0, ctrl, K, use_true=False, zn=None, zu=None, seed=0):
    """rat_pets_compute_cost on a raw handle: (rc, cost)."""
    ctrl = nv.f64(ctrl)
    cost = np.zeros(ctrl.shape[0])
    zn = None if zn is None else nv.f64(zn)
    zu = None if zu is None else nv.f64(zu)
    rc = nv.lib().rat_pets_compute_cost(h, nv.P(nv.f64(x0)), nv.P(ctrl), C.c_int64(ctrl.shape[0]), C.c_int64(K), int(use_true), nv.P(zn),
                                        nv.P(zu), C.c_uint64(seed), nv.P(cost))
    return rc, cost


def close(got, ref, tol):
    return np.all(np.isfinite(ref)) and np.all(np.abs(got - ref) <= tol * np.abs(ref))


# ---- 1. the LQ family written as source, against the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["gaussian", "gaussian_true_model", "uniform"])
def test_lq_family_as_source_matches_the_oracle(noise):
    prob, r = rich_problem()
    if noise == "uniform":
        lq = prob.lq
        prob = rat.LQGenerativeProblem(lq.A, lq.B, 30, ("uniform", -0.1, 0.2), Q=lq.Q, R=lq.R, P=lq.P, qv=lq.qv, rv=lq.rv, q0=0.5,
                                       Qf=lq.Qf, qvf=lq.qvf, q0f=1.0, kappa=lq.kappa, l1u=0.2)
    use_true = noise == "gaussian_true_model"
    npn, npu = (0, 12) if noise == "uniform" else (12, 1)
    src = rat.DeviceGenerativeSourceProblem(LQ, 12, 4, 30, params=lq_params(prob), normals_per_step=npn, uniforms_per_step=npu)
    S, K = 24, 50
    ds = solver(30, 4, S, K)
    ctrl = 0.3 * r.standard_normal((S, 30, 4))
    x0 = r.standard_normal(12)
    if noise == "uniform":                                             # the family's zn holds the uniforms: the source reads them as zu
        zn = r.random(S * K * 30 * 12)
        got = pets.compute_cost_serial(ds, src, x0, ctrl, None, use_true, streams=(None, zn))
        ref = orc.pets_compute_cost(orc.GenProblem(prob), x0, ctrl, K, use_true, zn, None)
    else:
        zn, zu = r.standard_normal(S * K * 30 * 12), r.random(S * K * 30)
        got = pets.compute_cost_serial(ds, src, x0, ctrl, None, use_true, streams=(zn, zu))
        ref = orc.pets_compute_cost(orc.GenProblem(prob), x0, ctrl, K, use_true, zn, zu if use_true else None)
    assert close(got, ref, 1e-11)


# ---- 2. the reference's pets_test.jl with its model as source ------------------------------------------------------------------
def test_reference_pets_test_as_source():                          # pets_test.jl:22-94
    N = 20
    prob = gsp(REF_TEST, REF_TEST_DIMS, N)
    mu0, Sig0 = np.zeros((N, 2)), np.stack([np.eye(2)] * N)
    ds = rat.CrossEntropyDirectOptimizationSolver(mu0, Sig0, num_control_samples=20, num_trajectory_samples=100, num_elite=5,
                                                  iter_max=20, smoothing_factor=0.1)
    rng = np.random.default_rng(1234)
    ctrl = rng.random((20, N, 2))
    x_init = np.zeros(2)
    zn, zu = pets.draw_noise(prob, rng, 20, 100)
    assert zn is None and zu.size == 20 * 100 * N * 2
    cost = pets.compute_cost_serial(ds, prob, x_init, ctrl, None, streams=(None, zu))
    cost2 = pets.compute_cost(ds, prob, x_init, ctrl, None, streams=(None, zu))
    assert np.all(cost == cost2) and cost.size == 20                                                              # :47-53
    for ii in range(20):                                                                                          # :54-63
        x, c = x_init, 0.0
        for t in range(N):
            c += np.sum(np.abs(ctrl[ii, t]))
            x = x + ctrl[ii, t] + zu[(ii * 100 * N + t) * 2:(ii * 100 * N + t) * 2 + 2]
        c += 1.0
        assert np.isclose(c, cost[ii], rtol=1e-12)
    per = N * 2 * 100                                                                                             # compute_cost_worker
    for ii in range(3):
        assert pets.compute_cost_worker(ds, prob, x_init, ctrl[ii], None, streams=(None, zu[ii * per:(ii + 1) * per])) == cost[ii]
    elite = pets.get_elite_samples(ds, ctrl, cost)                                                                # :66-70
    assert len(elite) == 5 and np.array_equal(elite, ctrl[np.argsort(cost, kind="stable")[:5]])
    pets.step_(ds, prob, x_init, np.random.default_rng(1234))                                                     # :87-89
    assert ds.iter_current == 1
    mu, Sig = pets.solve_(ds, prob, x_init, rng)                                                                  # :92-94
    assert ds.iter_current == ds.iter_max
    assert np.abs(mu).mean() < 0.25 and Sig.max() < 0.5       # c = sum|u|: the CE distribution contracts towards u = 0


# ---- 3. the documentation example and a noisy pendulum against NumPy ----------------------------------------------------------
@pytest.mark.parametrize("use_true", [False, True])
def test_docs_example_against_numpy(use_true):
    N, S, K = 10, 6, 40
    prob = gsp(DOCS, DOCS_DIMS, N, [10.0])
    ds = solver(N, 2, S, K)
    rng = np.random.default_rng(11)
    ctrl = 0.5 * rng.standard_normal((S, N, 2))
    x0 = np.array([0.5, -1.0])
    zn, zu = pets.draw_noise(prob, rng, S, K, use_true)
    got = pets.compute_cost_serial(ds, prob, x0, ctrl, None, use_true, streams=(zn, zu))
    ref = np_compute_cost(docs_f, docs_c, docs_h, [10.0], x0, ctrl, K, zn, zu, 2, 1, use_true)
    assert close(got, ref, 1e-10)


def test_noisy_pendulum_with_parameters_against_numpy():
    N, S, K = 25, 5, 30
    prob = gsp(PENDULUM, PENDULUM_DIMS, N, PENDULUM_P)
    ds = solver(N, 1, S, K)
    rng = np.random.default_rng(12)
    ctrl = rng.standard_normal((S, N, 1))
    x0 = np.array([1.0, 0.0])
    zn, zu = pets.draw_noise(prob, rng, S, K)
    assert zu is None
    got = pets.compute_cost_serial(ds, prob, x0, ctrl, None, streams=(zn, None))
    ref = np_compute_cost(pendulum_f, pendulum_c, pendulum_h, PENDULUM_P, x0, ctrl, K, zn, None, 1, 0)
    assert close(got, ref, 1e-10)
    assert pets.compute_cost_worker(ds, prob, x0, ctrl[2], None, streams=(zn[2 * K * N:3 * K * N], None)) == got[2]


# ---- 4. the device-resident loop of rat_pets_solve against the host loop ----------------------------------------------------------
@pytest.mark.parametrize("S,K,Nh", [(8, 16, 10), (30, 7, 25), (1024, 4, 5)])
def test_device_resident_solve_equals_the_host_loop(S, K, Nh):
    prob = gsp(PENDULUM, PENDULUM_DIMS, Nh, PENDULUM_P)
    kw = dict(num_control_samples=S, num_trajectory_samples=K, num_elite=max(2, S // 8), iter_max=4, smoothing_factor=0.2)
    mu0, Sig0 = 0.1 * np.ones((Nh, 1)), np.stack([0.5 * np.eye(1)] * Nh)
    dev = rat.CrossEntropyDirectOptimizationSolver(mu0, Sig0, **kw)
    host = rat.CrossEntropyDirectOptimizationSolver(mu0, Sig0, **kw)
    x0 = np.array([1.0, 0.0])
    assert dev.context(prob).debug_get("pets_device") == 1
    mu_d, Sig_d = pets.solve_(dev, prob, x0, np.random.default_rng(5), seed=77)
    assert dev.iter_current == 4
    pets.initialize_(host)
    rng = np.random.default_rng(5)
    while host.iter_current < host.iter_max:                          # the same control normals, rollout noise keyed by seed + iteration
        pets.step_(host, prob, x0, rng, seed=77 + host.iter_current)
    assert np.array_equal(mu_d, host.mu_array) and np.array_equal(Sig_d, host.Sigma_array)
    assert not np.array_equal(mu_d, mu0)


# ---- 5. the generator ------------------------------------------------------------------------------------------------------------
GEN = r"""
__device__ void rat_user_f_stochastic(const double *x, const double *u, rat_rng &rng, int use_true_model, double *xn, const double *p) {
    const double z0 = rng.normal();
    const double z1 = rng.normal();
    const double z2 = rng.normal();
    const double v0 = rng.uniform();
    const double v1 = rng.uniform();
    const double v2 = rng.uniform();
    xn[0] = z0 + 0.5 * z1 + 0.25 * z2;
    xn[1] = v0 + 0.5 * v1 + 0.25 * v2;
}
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) { return x[0] * x[0] + (1.0 + 0.1 * k) * x[1]; }
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return x[0] * x[0] + x[1]; }
"""


def test_generator_against_a_host_restatement():
    """Philox4x32-10 keyed by the seed; normals: counter (trajectory, t, pair), Box-Muller of csrc/rat_normal.h (oracle/normal_check.c),
    normal 2q the first output, 2q + 1 the second; uniforms: counter (trajectory, t, 0x80000000 | pair), both 53-bit uniforms.  Three of
    each per step leave half a pair unused."""
    from test_cpu_normal import parts
    S, K, N, seed = 5, 7, 7, 0x1234567890ABCDEF
    prob = rat.DeviceGenerativeSourceProblem(GEN, 2, 1, N, normals_per_step=3, uniforms_per_step=3)
    ds = solver(N, 1, S, K)
    x0 = np.array([0.3, 0.2])
    got = pets.compute_cost_serial(ds, prob, x0, np.zeros((S, N, 1)), None, seed=seed)
    g, t, q = np.meshgrid(np.arange(S * K), np.arange(N), np.arange(2), indexing="ij")
    u01 = lambda hi, lo: (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    r0, r1, r2, r3 = _philox4x32_10(g, 0 * g, t, q, seed & 0xFFFFFFFF, seed >> 32)
    u1, u2 = u01(r0, r1), u01(r2, r3)
    _, _, _, _, z0, z1 = parts(np.ascontiguousarray(u1.ravel()), np.ascontiguousarray(u2.ravel()))
    z = np.stack([z0.reshape(u1.shape), z1.reshape(u1.shape)], axis=3).reshape(S * K, N, 4)[:, :, :3]
    r0, r1, r2, r3 = _philox4x32_10(g, 0 * g, t, q | 0x80000000, seed & 0xFFFFFFFF, seed >> 32)
    v = np.stack([u01(r0, r1), u01(r2, r3)], axis=3).reshape(S * K, N, 4)[:, :, :3]
    xa = z[:, :, 0] + 0.5 * z[:, :, 1] + 0.25 * z[:, :, 2]            # x_{t+1}
    xb = v[:, :, 0] + 0.5 * v[:, :, 1] + 0.25 * v[:, :, 2]
    cost = np.full(S * K, x0[0] * x0[0] + x0[1])                        # c(0, x_0)
    for tt in range(1, N):
        cost += xa[:, tt - 1] ** 2 + (1.0 + 0.1 * tt) * xb[:, tt - 1]
    cost += xa[:, N - 1] ** 2 + xb[:, N - 1]
    ref = cost.reshape(S, K).mean(axis=1)
    assert np.all(np.abs(got - ref) <= 1e-12 * ref)


def test_generator_is_statistically_sane_against_the_family():
    """BASELINE config 5's shape: the LQ source's seeded costs against the family's seeded costs (other streams, the same distribution):
    per control sample the difference of two K-rollout means, within a few standard errors; reproducible per seed, different across seeds."""
    prob, r = rich_problem()
    src = rat.DeviceGenerativeSourceProblem(LQ, 12, 4, 30, params=lq_params(prob), normals_per_step=12, uniforms_per_step=1)
    S, K = 100, 100
    ds_s, ds_f = solver(30, 4, S, K), solver(30, 4, S, K)
    ctrl = 0.2 * r.standard_normal((S, 30, 4))
    x0 = r.standard_normal(12)
    c1 = pets.compute_cost_serial(ds_s, src, x0, ctrl, None, seed=42)
    c1b = pets.compute_cost_serial(ds_s, src, x0, ctrl, None, seed=42)
    c2 = pets.compute_cost_serial(ds_s, src, x0, ctrl, None, seed=43)
    cf = pets.compute_cost_serial(ds_f, prob, x0, ctrl, None, seed=42)
    assert np.array_equal(c1, c1b) and not np.array_equal(c1, c2)
    d = c1 - cf
    assert abs(d.mean()) < 5 * d.std() / np.sqrt(S) + 1e-9
    assert abs(np.mean(c1) / np.mean(cf) - 1) < 0.02


# ---- 6. parameters and handle state -------------------------------------------------------------------------------------------
def _pendulum_case(S=4, K=20, N=15, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((S, N, 1)), np.array([1.0, 0.0]), rng.standard_normal(S * K * N), S, K, N


def test_set_params_equals_a_fresh_source():
    ctrl, x0, zn, S, K, N = _pendulum_case()
    prob = gsp(PENDULUM, PENDULUM_DIMS, N, PENDULUM_P)
    ds = solver(N, 1, S, K)
    c0 = pets.compute_cost_serial(ds, prob, x0, ctrl, None, streams=(zn, None))
    ds.set_params(prob, [0.05, 0.2, 0.1])
    c1 = pets.compute_cost_serial(ds, prob, x0, ctrl, None, streams=(zn, None))
    g1 = pets.compute_cost_serial(ds, prob, x0, ctrl, None, seed=5)
    fresh = gsp(PENDULUM, PENDULUM_DIMS, N, [0.05, 0.2, 0.1])
    ds2 = solver(N, 1, S, K)
    assert np.array_equal(c1, pets.compute_cost_serial(ds2, fresh, x0, ctrl, None, streams=(zn, None)))
    assert np.array_equal(g1, pets.compute_cost_serial(ds2, fresh, x0, ctrl, None, seed=5))
    assert not np.array_equal(c0, c1) and np.array_equal(prob.params, PENDULUM_P)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG"):
        ds.set_params(prob, [0.05, 0.2])


OVER = PENDULUM.replace("+ p[2] * rng.normal();", "+ p[2] * rng.normal() + (use_true_model ? rng.normal() : 0.0);")


def test_an_overdraw_is_an_error_and_the_handle_goes_on():
    ctrl, x0, zn, S, K, N = _pendulum_case()
    prob = gsp(OVER, PENDULUM_DIMS, N, PENDULUM_P)
    ds = solver(N, 1, S, K, num_elite=2, iter_max=2)
    ok = pets.compute_cost_serial(ds, prob, x0, ctrl, None, streams=(zn, None))
    for kw in (dict(streams=(zn, None)), dict(seed=9)):
        with pytest.raises(rat.RatError, match=r"RAT_ERR_ARG.*normals_per_step = 1"):
            pets.compute_cost_serial(ds, prob, x0, ctrl, None, True, **kw)
    with pytest.raises(rat.RatError, match=r"RAT_ERR_ARG.*normals_per_step = 1"):
        pets.solve_(ds, prob, x0, np.random.default_rng(1), use_true_model=True, seed=4)         # the device-resident loop
    assert np.array_equal(ok, pets.compute_cost_serial(ds, prob, x0, ctrl, None, streams=(zn, None)))
    # injected draws need every declared stream
    docs = gsp(DOCS, DOCS_DIMS, N, [10.0])
    ds2 = solver(N, 2, S, K)
    zn2 = np.zeros(S * K * N * 2)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG"):
        pets.compute_cost_serial(ds2, docs, x0, np.zeros((S, N, 2)), None, streams=(zn2, None))


def test_a_failed_recompile_keeps_the_previous_generative_problem():
    ctrl, x0, zn, S, K, N = _pendulum_case()
    prob = gsp(PENDULUM, PENDULUM_DIMS, N, PENDULUM_P)
    ds = solver(N, 1, S, K)
    c0 = pets.compute_cost_serial(ds, prob, x0, ctrl, None, streams=(zn, None))
    L = nv.lib()
    h = ds.context(prob).h
    p = nv.f64(PENDULUM_P)
    assert L.rat_pets_problem_set_source(h, PENDULUM.replace("sin(", "sine(").encode(), 2, 1, N, 1, 0, nv.P(p), 3) == 1
    assert "model.hip:" in L.rat_last_error().decode()
    assert L.rat_pets_problem_set_source(h, PENDULUM.encode(), 13, 1, N, 1, 0, nv.P(p), 3) == 2
    assert L.rat_pets_problem_set_source(h, PENDULUM.encode(), 2, 1, N, -1, 0, nv.P(p), 3) == 1
    assert np.array_equal(c0, pets.compute_cost_serial(ds, prob, x0, ctrl, None, streams=(zn, None)))


def test_one_handle_runs_an_ileqg_source_problem_and_a_generative_one_interleaved():
    from test_gpu_source_model import pendulum, source_pendulum
    _, _, x0i, u0i = pendulum()
    ictx = rat.Context(source_pendulum())
    r0 = ictx.solve(x0i, u0i, 0.5)
    ctrl, x0, zn, S, K, N = _pendulum_case()
    ref = pets.compute_cost_serial(solver(N, 1, S, K), gsp(PENDULUM, PENDULUM_DIMS, N, PENDULUM_P), x0, ctrl, None, streams=(zn, None))
    L = nv.lib()
    p = nv.f64(PENDULUM_P)
    assert L.rat_pets_problem_set_source(ictx.h, PENDULUM.encode(), 2, 1, N, 1, 0, nv.P(p), 3) == 0
    for _ in range(2):
        rc, c = cost_on(ictx.h, x0, ctrl, K, zn=zn)
        assert rc == 0 and np.array_equal(c, ref)
        r = ictx.solve(x0i, u0i, 0.5)
        assert r["value"] == r0["value"] and r["iters"] == r0["iters"] and np.array_equal(r["x"], r0["x"])
    # rat_pets_problem_set switches the handle back to the family
    prob, rr = rich_problem()
    Sf, Kf = 6, 10
    ctrl_f, x0_f = 0.3 * rr.standard_normal((Sf, 30, 4)), rr.standard_normal(12)
    zn_f = rr.standard_normal(Sf * Kf * 30 * 12)
    fam = pets.compute_cost_serial(solver(30, 4, Sf, Kf), prob, x0_f, ctrl_f, None, streams=(zn_f, None))
    g, keep = pets.make_gen_desc(prob)
    nv.check(L.rat_pets_problem_set(ictx.h, C.byref(g)))
    rc, c = cost_on(ictx.h, x0_f, ctrl_f, Kf, zn=zn_f)
    assert rc == 0 and np.array_equal(c, fam)
    assert L.rat_pets_set_params(ictx.h, nv.P(p), 3) == 4                # RAT_ERR_NO_PROBLEM: the family has no source parameters
    assert ictx.solve(x0i, u0i, 0.5)["value"] == r0["value"]
