"""Phase-local kernel arguments in solve_fused_kernel (kernels.hip: phase_args, rollout_view).

Every phase of the one-wavefront-per-sample solve reads the bases and strides it needs from the argument segment at its own start, and the
rollouts take the batch description from the sweeps' copy (FusedArgs.sw); only x0, u0 and the record switches are their own.  No
floating-point instruction changes, so a wrong base, stride or offset is the only way this can go wrong -- and it shows as different bits
at small shapes.  Everything here is compared with array_equal: the workloads of tests/stacked_operands_cases.py against what the tree
before the stacked operands computed (tests/golden/stacked_operands_parent.npz) and against the round-based path, and one case per
instantiation of the kernel those workloads do not reach, fused path against round-based path, 8 samples at N = 5 and N = 7."""
import os

import numpy as np
import pytest

import ratilqr.jl_amd as rat
import stacked_operands_cases as cases
from test_gpu_lq_replay import _draw_theta

pytestmark = pytest.mark.gpu

_cache = {}


def _fused_env():
    os.environ["RATILQR_BLOCK"] = "0"                          # (what the other fused-path tests set: no workgroup-per-sample kernel)


def results(path):
    """The stacked-operands workloads on one execution path, computed once per session."""
    if path not in _cache:
        _fused_env()
        try:
            _cache[path] = cases.run({}, path)
        finally:
            del os.environ["RATILQR_BLOCK"]
    return _cache[path]


def test_workloads_are_the_recorded_parents_bit_for_bit():
    """value, status, iterations, line-search counts, x, u, L, eps history and the replay counters of every workload"""
    got = results("fused")
    with np.load(os.path.join(os.path.dirname(__file__), "golden", "stacked_operands_parent.npz")) as z:
        want = {k: z[k] for k in z.files}
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert np.array_equal(got[k], want[k], equal_nan=True), k


def test_workloads_agree_with_the_round_based_path():
    got, rounds = results("fused"), results("rounds")
    assert sorted(got) == sorted(rounds)
    for k in sorted(got):
        if k.endswith("/counts"):                              # (the round-based path keeps no record: its counters stay 0)
            assert not rounds[k].any(), k
            continue
        assert np.array_equal(got[k], rounds[k], equal_nan=True), k


def _lq(N, seed, **kw):
    """The headline problem's construction at horizon N with the tables of one variant replaced (12 states, 4 controls)."""
    base, x0, u = rat.synthetic_lq_problem(N=N, seed=seed)
    args = dict(Q=np.eye(12), R=0.1 * np.eye(4), N=N, W=1e-3 * np.eye(12), Qf=np.eye(12))
    args.update(kw)
    return rat.LQRiskSensitiveProblem(base.A, base.B, **args), x0, u


def _variant(name, N):
    """(problem, x0, u, switches) of one instantiation of solve_fused_kernel at horizon N"""
    rng = np.random.default_rng(40 + N)
    k = np.arange(N, dtype=float)[:, None, None]
    if name == "kappa":
        return (*rat.synthetic_lq_problem(N=N, seed=5, kappa=0.05), {})
    if name == "cost_tv":                                      # c(k, x, u): Q, R, the linear terms and q0 by step
        return (*_lq(N, 6, Q=(0.5 + 0.1 * k) * np.eye(12), R=(0.2 + 0.05 * k) * np.eye(4), P=0.05 * rng.standard_normal((N, 4, 12)),
                     qv=0.1 * rng.standard_normal((N, 12)), rv=0.1 * rng.standard_normal((N, 4)), q0=k.ravel()), {})
    if name == "w_tv":                                         # W(k), not diagonal
        Wk = np.stack([1e-3 * (1 + 0.5 * np.sin(t)) * np.eye(12) + 1e-4 * np.outer(v, v) for t, v in zip(range(N), rng.standard_normal((N, 12)))])
        return (*_lq(N, 7, W=Wk), {})
    if name == "w_full":                                       # one W, not diagonal
        v = rng.standard_normal(12)
        return (*_lq(N, 8, W=1e-3 * np.eye(12) + 1e-4 * np.outer(v, v)), {})
    if name == "powerlaw":
        return rat.PowerLawRiskSensitiveProblem(2, N, 0.01 * np.eye(2), a=1.3, b=1.5, p=2.5, hconst=1.0), np.zeros(2), 0.1 * np.ones((N, 2)), {}
    switch = {"occ2": {"fused_occ2": 1}, "materialize": {"materialize": 1}, "own_init": {"init_share": 0}, "no_record": {"lq_replay": 0}}[name]
    return (*rat.synthetic_lq_problem(N=N), switch)


def _solve(prob, x0, u, theta, switches, path):
    ctx = rat.Context(prob, max_batch=theta.size)
    ctx.set_path(path)
    if path == "fused":
        for key, v in switches.items():
            ctx.debug_set(key, v)
    assert ctx.get_path(theta.size) == path
    return ctx, ctx.solve_batch(x0, u, theta)


@pytest.mark.parametrize("N", [5, 7])
@pytest.mark.parametrize("name", ["kappa", "cost_tv", "w_tv", "w_full", "powerlaw", "occ2", "materialize", "own_init", "no_record"])
def test_other_instantiations_agree_with_the_round_based_path(name, N, monkeypatch):
    monkeypatch.setenv("RATILQR_BLOCK", "0")
    prob, x0, u, switches = _variant(name, N)
    theta = np.array([0.0, 0.1, 0.2, 0.3, 0.35, 0.4, 0.43, 0.5]) if name == "powerlaw" else _draw_theta(8, seed=1000)
    ctx, fused = _solve(prob, x0, u, theta, switches, "fused")
    _, rounds = _solve(prob, x0, u, theta, {}, "rounds")
    for key, a, b in zip(("value", "status", "iters", "ls"), fused, rounds):
        assert np.array_equal(a, b, equal_nan=True), (name, N, key, a, b)
    assert np.isfinite(fused[0]).any() and (fused[2] > 0).any(), (name, N, fused)     # (solves that iterate, not eight failures)
    if name in ("no_record", "occ2", "materialize", "kappa", "cost_tv", "w_tv", "w_full", "powerlaw"):
        assert ctx.debug_get("lq_replay_count") == 0           # none of them is the recording instantiation
    else:
        assert ctx.debug_get("lq_replay_count") > 0


def test_initial_point_set_again_between_two_batches(monkeypatch):
    """x0 / u0 are the rollout's own arguments: a second batch on the same handle from another initial point must read the new one, with
    the shared initial trajectory (init_share, the default) and with every sample rolling out for itself."""
    monkeypatch.setenv("RATILQR_BLOCK", "0")
    theta = _draw_theta(8, seed=1000)
    prob, x0a, ua = rat.synthetic_lq_problem(N=7)
    rng = np.random.default_rng(77)
    x0b, ub = rng.standard_normal(12), 0.05 * rng.standard_normal((7, 4))
    ref = {}
    for tag, x0, u in (("a", x0a, ua), ("b", x0b, ub)):
        _, ref[tag] = _solve(prob, x0, u, theta, {}, "rounds")
    assert not np.array_equal(ref["a"][0], ref["b"][0])
    for share in (1, 0):
        ctx = rat.Context(prob, max_batch=theta.size)
        ctx.set_path("fused")
        ctx.debug_set("init_share", share)
        for tag, x0, u in (("a", x0a, ua), ("b", x0b, ub), ("a", x0a, ua)):
            got = ctx.solve_batch(x0, u, theta)
            for key, a, b in zip(("value", "status", "iters", "ls"), got, ref[tag]):
                assert np.array_equal(a, b, equal_nan=True), (share, tag, key)


def test_replay_counters_on_the_headline_problem(monkeypatch):
    """8 samples of the headline problem: every sample replays one pair (two sweeps) and the evaluation that ends its solve."""
    monkeypatch.setenv("RATILQR_BLOCK", "0")
    prob, x0, u = rat.synthetic_lq_problem()
    ctx, out = _solve(prob, x0, u, _draw_theta(8, seed=1000), {}, "fused")
    assert np.all(out[1] == 0)
    assert [ctx.debug_get("lq_replay_count"), ctx.debug_get("lq_replay_last_count")] == [16, 8]
