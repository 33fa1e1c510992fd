"""Stacked MFMA operands in the replayed pair of solve_fused_kernel (switch lq_replay_stack).

The replayed pair forms row 12 of T for both recursions in one mm3 (column 12 of recursion B's V rides in column 4 of recursion A's).  An
MFMA element reads its own row of A, column of B and element of C only, so no bit moves: every output here is compared with array_equal
-- switch on against switch off, against the round-based path, against the solve that never replays, and against what the commit before
the switch computed (tests/golden/stacked_operands_parent.npz, recorded from that commit's build by
tests/golden/make_stacked_operands_golden.py).  Workloads: tests/stacked_operands_cases.py."""
import os

import numpy as np
import pytest

import ratilqr.jl_amd as rat
import stacked_operands_cases as cases
from test_gpu_lq_replay import _draw_theta

pytestmark = pytest.mark.gpu

CONFIGS = {"on": {}, "off": {"lq_replay_stack": 0}, "no_record": {"lq_replay": 0}}
_cache = {}


def results(name):
    """Every workload under one configuration, computed once per session ("rounds": the round-based path, switches at their defaults)."""
    if name not in _cache:
        os.environ["RATILQR_BLOCK"] = "0"                      # (what the other fused-path tests set: no workgroup-per-sample kernel)
        try:
            _cache[name] = cases.run({}, "rounds") if name == "rounds" else cases.run(CONFIGS[name], "fused")
        finally:
            del os.environ["RATILQR_BLOCK"]
    return _cache[name]


def parent():
    with np.load(os.path.join(os.path.dirname(__file__), "golden", "stacked_operands_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def same(a, b, skip_counts=False):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        if skip_counts and k.endswith("/counts"):
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_switch_default_on_and_reported():
    prob, x0, u = rat.synthetic_lq_problem()
    ctx = rat.Context(prob, max_batch=8)
    assert ctx.debug_get("lq_replay_stack") == 1
    ctx.debug_set("lq_replay_stack", 0)
    assert ctx.debug_get("lq_replay_stack") == 0
    ctx.debug_set("lq_replay_stack", 1)
    assert ctx.debug_get("lq_replay_stack") == 1


def test_on_and_off_are_bit_identical():
    """value, status, iterations, line-search counts, x, u, L, eps history AND the replay counters, on every workload"""
    same(results("on"), results("off"))


def test_round_based_path_agrees():
    same(results("on"), results("rounds"), skip_counts=True)     # (the round-based path keeps no record: its counters stay 0)
    assert all(not v.any() for k, v in results("rounds").items() if k.endswith("/counts"))


@pytest.mark.parametrize("cfg", ["off", "on"])
def test_values_and_counters_are_the_parent_commits(cfg):
    """The switch off selects the code of the commit before it -- its recorded values and counters -- and the switch on gives the same."""
    same(results(cfg), parent())


def test_workloads_reach_what_they_are_there_for():
    on = results("on")
    for N in (5, 7, 1, 50):                                      # replayed pairs ran (stack on) at every horizon; nothing failed
        assert on[f"lq_N{N}/counts"][0] > 0 and np.all(on[f"lq_N{N}/status"] == 0), N
    assert on["lq_n3m2/counts"][0] > 0
    assert np.all(on["mu_restart/status"] == 3)                  # mu restarts keep the stress problem at iter_max
    assert (on["backtrack/ls"] > on["backtrack/iters"]).any()    # rejected line-search candidates
    assert len(on["backtrack/eps_history"]) > on["backtrack/scalars"][2]
    assert not np.isfinite(on["overflow/value"]).all() or (on["overflow/status"] != 0).any()


def test_non_finite_trajectory_matches_the_full_sweeps():
    """The overflowing trajectory with the switch on: status and values are those of the solve that never replays (lq_replay = 0)."""
    on, full = results("on"), results("no_record")
    for key in ("value", "status", "iters", "ls"):
        assert np.array_equal(on[f"overflow/{key}"], full[f"overflow/{key}"], equal_nan=True), key
    same(on, full, skip_counts=True)                             # ... and so is every other workload


def test_counters_on_the_headline_batch():
    """B = 1024: every sample replays one pair and its last evaluation, with the stack on and off; identical outputs."""
    prob, x0, u = rat.synthetic_lq_problem()
    theta = _draw_theta(1024, seed=1000)
    res = {}
    os.environ["RATILQR_BLOCK"] = "0"
    try:
        for name in ("on", "off"):
            ctx = rat.Context(prob, max_batch=theta.size)
            for k, v in CONFIGS[name].items():
                ctx.debug_set(k, v)
            assert ctx.get_path(theta.size) == "fused"
            res[name] = ctx.solve_batch(x0, u, theta)
            assert ctx.debug_get("lq_replay_count") == 2 * theta.size and ctx.debug_get("lq_replay_last_count") == theta.size
    finally:
        del os.environ["RATILQR_BLOCK"]
    for a, b in zip(res["on"], res["off"]):
        assert np.array_equal(a, b)
