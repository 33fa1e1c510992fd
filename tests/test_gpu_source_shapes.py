"""Source models at every regime of rat_src_linearize's pair loop and rat_src_rollout's lane layout (csrc/source_kernels.h), against the
closed forms of tests/source_shapes_model.py, which tests/test_cpu_source_shapes.py pins on the host.

    (n, m)    pairs running / terminal
    (12, 4)   136 / 78   three turns of the pair loop, the last masked; terminal two turns; full tile, no padded R row
    (11, 4)   120 / 66   terminal crosses 64 by two pairs
    (12, 3)   120 / 78   one padded R row beside a full x block
    (10, 1)    66 / 55   running loop crosses 64 by two pairs; three padded R rows
    (7, 3)     55 / 28   the largest single-turn shape
    (3, 2)     15 / 6    small, padded both ways
    (1, 4)     15 / 1    one state, every control
    (1, 1)      3 / 1    the smallest

One hiprtc module per shape and process: the library caches code objects on (source text, n, m), and the model's numbers travel in p."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
from oracle import oracle as orc

import source_shapes_model as ssm
from test_gpu_source_model import check_against_oracle, rel

pytestmark = pytest.mark.gpu

ARRAYS = ("q_array", "q_vec_array", "Q_array", "r_array", "R_array", "P_array", "A_array", "B_array", "W_array")
_PROB = {}


def problem(mdl, N):
    """The DeviceSourceProblem of a model at horizon N, one per (shape, kappa, thresholds, N) for the whole module."""
    key = (mdl.n, mdl.m, mdl.kappa, mdl.thr, N)
    if key not in _PROB:
        _PROB[key] = rat.DeviceSourceProblem(mdl.source, mdl.n, mdl.m, N, ssm.noise(mdl.n), params=mdl.p)
    return _PROB[key]


def compare(ap, want, label, skip_step=None):
    """Every array of an ApproximationResult against the reference: shape, and values at 1e-12 max(1, max|want|)."""
    worst = {}
    for name in ARRAYS:
        got, w = getattr(ap, name), want[name]
        assert got.shape == w.shape, name
        if skip_step is not None:
            keep = np.arange(len(w)) != skip_step
            got, w = got[keep], w[keep]
        worst[name] = float(np.abs(got - w).max() / max(1.0, np.abs(w).max()))
    print(label, " ".join(f"{k[:-6]} {v:.1e}" for k, v in worst.items()))
    for name, e in worst.items():
        assert e <= 1e-12, (label, name, e)


# ---- (a) linearisation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,N", ssm.LIN_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_linearisation_against_closed_forms(shape, N):
    """approximate_model at a random trajectory, every array, every entry.  The public entry linearises slot 0 of a one-sample state whatever
    max_batch the handle has (the batch handle below returns the same bits), so the tiles of the other samples of a batch are covered
    through the batched solves of test_batch_of_16_against_per_sample_solves and test_rollout_lanes_do_not_depend_on_their_wavefront."""
    n, m = shape
    mdl, xt, ut = ssm.lin_case(n, m, N)
    assert mdl.margin(xt, ut) > 0.1                                    # inside every domain, off every kink
    want = mdl.approximation(ut, xt, ssm.noise(n))
    # the reference is not degenerate: a transposition, a dropped pair or a misplaced row cannot hide behind a zero or a symmetry
    off = lambda a: a[:, ~np.eye(a.shape[1], dtype=bool)]
    assert np.all(want["P_array"] != 0) and np.all(want["A_array"] != 0) and np.all(want["B_array"] != 0)
    assert np.all(off(want["Q_array"]) != 0) and np.all(off(want["R_array"]) != 0)
    if n == m and n > 1:
        assert np.all(np.abs(want["P_array"] - want["P_array"].transpose(0, 2, 1)).max(axis=(1, 2)) > 1e-3)
    prob = problem(mdl, N)
    ap = rat.approximate_model(prob, ut, xt)
    compare(ap, want, f"({n}, {m}) N={N}:")
    total = want["q_array"].sum()
    assert abs(rat.integrate_cost(prob, xt, ut) - total) <= 1e-12 * abs(total)
    if N == 4:
        ap5 = rat.Context(prob, max_batch=5).approximate_model(ut, xt)
        for name in ARRAYS:
            assert np.array_equal(getattr(ap5, name), getattr(ap, name)), name


# ---- (b) rollouts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(12, 4), (7, 3), (1, 4)])
def test_rollouts_against_numpy(n, m):
    N = ssm.SOLVE_N
    mdl = ssm.model(n, m, ssm.SEED[(n, m)])
    prob = problem(mdl, N)
    rng = np.random.default_rng(7)
    x0, u = 0.5 * rng.standard_normal(n), 0.3 * rng.standard_normal((N, m))
    xr, _ = mdl.rollout(x0, u)
    assert rel(rat.simulate_dynamics(prob, x0, u), xr) < 1e-12
    # closed loop under l + L (x - xbar): a nominal trajectory that is not the rollout of l
    L = 0.2 * rng.standard_normal((N, m, n))
    xbar = xr + np.vstack([np.zeros((1, n)), 0.05 * rng.standard_normal((N, n))])
    xc, uc = mdl.rollout(None, u, xbar, L)
    xn, un = rat.simulate_dynamics(prob, xbar, u, L)
    assert rel(xn, xc) < 1e-12 and rel(un, uc) < 1e-12
    assert rel(un, u) > 1e-3                                           # the feedback term moved the controls


@pytest.mark.parametrize("n,m", [(12, 4), (7, 3), (1, 4)])
def test_rollout_lanes_do_not_depend_on_their_wavefront(n, m):
    """A batch of 17 samples under src_tpw = 16, 32, 64: 17 candidates with the sequential line search, 68 with four speculative step
    sizes -- no multiple of any of the three, and more than one workgroup even at 64.  The same bits whichever wavefront holds a lane."""
    mdl, x0, u0 = ssm.solve_case(n, m)
    prob = problem(mdl, ssm.SOLVE_N)
    theta = np.linspace(0.0, 1.5, 17)
    for E in (1, 4):
        out = []
        for v in (16, 32, 64):
            ctx = rat.Context(prob, max_batch=17, spec_eps=E)
            if E > 1:
                ctx.debug_set("spec_force", 1)
                assert ctx.debug_get("spec_width") == E
            ctx.debug_set("src_tpw", v)
            assert ctx.debug_get("src_tpw") == v
            out.append(ctx.solve_batch(x0, u0, theta))
        assert np.all(out[0][1] == 0) and np.all(out[0][2] >= 2)
        for o in out[1:]:
            for a, b in zip(out[0], o):
                assert np.array_equal(a, b), E


# ---- (c) domain errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["c", "h"])
def test_domain_error_that_only_the_cost_produces(which):
    """log(x_0 - thr) in c at k = 2 alone, or in h alone: f never produces a NaN, one step's cost does."""
    mdl, x0, u, x = ssm.domain_case(which)
    assert mdl.margin(x, u) > 0.1                                      # the model's own terms are inside their domains: the log is the only NaN
    prob = problem(mdl, ssm.DOMAIN_N)
    assert np.allclose(rat.simulate_dynamics(prob, x0, u), x, rtol=0, atol=1e-12)
    with pytest.raises(ArithmeticError):
        rat.approximate_model(prob, u, x)
    r = rat.Context(prob).solve(x0, u, 0.5)
    assert r["status"] == rat.native.ST_DOMAIN and np.isposinf(r["value"])
    # with both thresholds out of reach the same source is fine on the same trajectory
    clean = ssm.model(mdl.n, mdl.m, ssm.SEED[ssm.DOMAIN_SHAPE], domain_thresholds=(ssm.DOMAIN_OFF, ssm.DOMAIN_OFF))
    pc = problem(clean, ssm.DOMAIN_N)
    assert np.all(np.isfinite(rat.approximate_model(pc, u, x).q_array))


def test_nan_in_the_input_trajectory_is_no_domain_error():
    n, m = ssm.DOMAIN_SHAPE
    mdl, xt, ut = ssm.lin_case(n, m, ssm.DOMAIN_N)
    want = mdl.approximation(ut, xt, ssm.noise(n))
    xt = xt.copy()
    xt[2, 1] = np.nan
    ap = rat.approximate_model(problem(mdl, ssm.DOMAIN_N), ut, xt)   # does not raise: the NaN was in the input, no function made it
    for name in ARRAYS[:-1]:
        assert np.all(np.isnan(getattr(ap, name)[2])), name
    compare(ap, want, "NaN planted at step 2, the other steps:", skip_step=2)


# ---- (d) solves -------------------------------------------------------------------------------------------------------------------------
def closures(mdl):
    n, m, N, W = mdl.n, mdl.m, ssm.SOLVE_N, ssm.noise(mdl.n)
    cp = orc.ClosureProblem(mdl.f, mdl.c, mdl.h, W, N, n, m, mdl.jac, mdl.c_derivatives, mdl.h_derivatives)
    gen = rat.GenericRiskSensitiveProblem(mdl.f, mdl.c, mdl.h, W, N, n, m, f_returns_jacobian=True, c_derivatives=mdl.c_derivatives,
                                          h_derivatives=mdl.h_derivatives)
    return cp, gen


@pytest.mark.parametrize("theta", ssm.SOLVE_THETAS)
@pytest.mark.parametrize("n,m", ssm.SOLVE_SHAPES)
def test_solve_against_the_oracle_closure_path(n, m, theta):
    mdl, x0, u0 = ssm.solve_case(n, m)
    prob = problem(mdl, ssm.SOLVE_N)
    s = rat.ILEQGSolver(prob)
    x, l, L, v, hist = rat.solve_(s, prob, x0, u0, theta=theta)
    r = orc.closure_solve(closures(mdl)[0], x0, u0, theta)
    assert r["iters"] >= 2
    check_against_oracle(r, s, x, l, L, v, hist)


def test_batch_of_16_against_per_sample_solves():
    mdl, x0, u0 = ssm.solve_case(12, 4)
    prob = problem(mdl, ssm.SOLVE_N)
    theta = np.linspace(0.0, 1.5, 16)
    val, st, it, ls = rat.Context(prob, max_batch=16).solve_batch(x0, u0, theta)
    one = rat.Context(prob)
    for b in range(16):
        r = one.solve(x0, u0, theta[b])
        assert r["status"] == st[b] == 0 and r["iters"] == it[b], b
        assert abs(r["value"] - val[b]) <= 1e-12 * abs(val[b]), b
    r = orc.closure_solve(closures(mdl)[0], x0, u0, theta[11])
    assert r["iters"] == it[11] and r["ls_evals"] == ls[11] and abs(r["value"] - val[11]) <= 1e-9 * abs(val[11])


def test_source_against_the_host_closure_path():
    """The same closures through GenericRiskSensitiveProblem: host rollouts and linearisations, device sweeps -- the other route to the tiles."""
    mdl, x0, u0 = ssm.solve_case(12, 4)
    prob = problem(mdl, ssm.SOLVE_N)
    gen = closures(mdl)[1]
    s1, s2 = rat.ILEQGSolver(prob), rat.ILEQGSolver(gen, f_returns_jacobian=True)
    x1, l1, L1, v1, h1 = rat.solve_(s1, prob, x0, u0, theta=0.5)
    x2, l2, L2, v2, h2 = rat.solve_(s2, gen, x0, u0, theta=0.5)
    assert s1.iter_current == s2.iter_current and [a[0] for a in h1] == [a[0] for a in h2]
    assert abs(v1 - v2) <= 1e-10 * abs(v1) and rel(x2, x1) < 1e-10 and rel(l2, l1) < 1e-9 and rel(L2, L1) < 1e-9
