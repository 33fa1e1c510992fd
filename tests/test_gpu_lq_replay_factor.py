"""The replayed pair of solve_fused_kernel takes the LDL' factor of H from the record (switch lq_replay_factor, csrc/sweep_dual.h).

The recording pass stores the factor of every step in the lanes of the record's -M^-1 words that hold no matrix data (csrc/layout.h:
REC_FACT_*), and replay_body<true, .., FACT> solves its columns from it instead of factoring the recorded H again.  H + mu I is matrix
data and both places round the factorisation alike (device_utils.h: ldl4_factor), so no bit may move: everything here is array_equal --
fused path against round-based path, switch on against off, against what the tree before the stacked operands computed
(tests/golden/stacked_operands_parent.npz: values AND replay counters), on the workloads of tests/stacked_operands_cases.py, which reach
every way out of a replay: theta = 0, a raised mu, a line search that backtracks, a trajectory that overflows.
The gains: a single solve returns L and the controls l, into which dl went (l + eps dl): both are compared, with x and the eps history."""
import os

import numpy as np
import pytest

import ratilqr.jl_amd as rat
import stacked_operands_cases as cases
import test_gpu_sgpr_diet as diet
from test_gpu_lq_replay import _draw_theta

pytestmark = pytest.mark.gpu

_cache = {}


def results(name):
    """Every workload of stacked_operands_cases: "on" (the default; shared with test_gpu_sgpr_diet), "off", "no_record", "rounds"."""
    if name == "on":
        return diet.results("fused")
    if name == "rounds":
        return diet.results("rounds")
    if name not in _cache:
        os.environ["RATILQR_BLOCK"] = "0"                      # (what the other fused-path tests set: no workgroup-per-sample kernel)
        try:
            _cache[name] = cases.run({"off": {"lq_replay_factor": 0}, "no_record": {"lq_replay": 0}}[name], "fused")
        finally:
            del os.environ["RATILQR_BLOCK"]
    return _cache[name]


def parent():
    with np.load(os.path.join(os.path.dirname(__file__), "golden", "stacked_operands_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def same(a, b, skip_counts=False, only=None):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        if (skip_counts and k.endswith("/counts")) or (only and not k.startswith(only)):
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _headline(N, switches, path):
    """8 samples of the headline problem at horizon N and one single solve: outputs, gains and the two replay counters"""
    prob, x0, u = rat.synthetic_lq_problem(N=N)
    theta = _draw_theta(8, seed=1000)                            # bench.draw_theta: positive samples of N(1, 2)
    out = {}
    for B, th in ((8, theta), (1, None)):
        ctx = rat.Context(prob, max_batch=B)
        ctx.set_path(path)
        for k, v in switches.items():
            ctx.debug_set(k, v)
        assert ctx.get_path(B) == path
        if th is not None:
            out["value"], out["status"], out["iters"], out["ls"] = ctx.solve_batch(x0, u, th)
            out["counts"] = [ctx.debug_get("lq_replay_count"), ctx.debug_get("lq_replay_last_count")]
        else:
            r = ctx.solve(x0, u, 3.0)
            out["x"], out["l"], out["L"], out["eps"] = r["x"], r["l"], r["L"], np.asarray(r["eps_history"], dtype=float)
            out["scalars"] = np.array([r["value"], r["status"], r["iters"]])
    return out


def test_switch_default_on_and_reported():
    prob, x0, u = rat.synthetic_lq_problem()
    ctx = rat.Context(prob, max_batch=8)
    assert ctx.debug_get("lq_replay_factor") == 1
    ctx.debug_set("lq_replay_factor", 0)
    assert ctx.debug_get("lq_replay_factor") == 0
    ctx.debug_set("lq_replay_factor", 1)
    assert ctx.debug_get("lq_replay_factor") == 1


@pytest.mark.parametrize("N", [3, 5, 7])
def test_fused_against_round_based_path_and_switch_off(N, monkeypatch):
    """N = 3, 5, 7: the three remainders of the replay's loop, which is unrolled by three steps.  The parent's counters: one replayed pair
    (two sweeps) and one replayed last evaluation per sample (the golden file's lq_N5 / lq_N7 / lq_N1 / lq_N50 rows: [16, 8])."""
    monkeypatch.setenv("RATILQR_BLOCK", "0")
    on, off, rounds = _headline(N, {}, "fused"), _headline(N, {"lq_replay_factor": 0}, "fused"), _headline(N, {}, "rounds")
    for k in ("value", "status", "iters", "ls", "x", "l", "L", "eps", "scalars"):
        assert np.array_equal(on[k], rounds[k], equal_nan=True), (N, "rounds", k)
        assert np.array_equal(on[k], off[k], equal_nan=True), (N, "off", k)
    assert np.all(on["status"] == 0) and (on["iters"] > 0).all()
    assert on["counts"] == [16, 8] and off["counts"] == on["counts"] and rounds["counts"] == [0, 0]
    if N in (5, 7):
        assert on["counts"] == parent()[f"lq_N{N}/counts"].tolist()


def test_on_and_off_are_bit_identical():
    """value, status, iterations, line-search counts, x, l, L, eps history AND the replay counters, on every workload"""
    same(results("on"), results("off"))


@pytest.mark.parametrize("cfg", ["on", "off"])
def test_values_and_counters_are_the_recorded_parents(cfg):
    """No array moved: the factor helper keeps the order the compiler's contraction gave every place before (profiles/lq_replay_factor.md)."""
    same(results(cfg), parent())


def test_round_based_path_agrees():
    same(results("on"), results("rounds"), skip_counts=True)
    assert all(not v.any() for k, v in results("rounds").items() if k.endswith("/counts"))


def test_replay_refusals_are_still_refused():
    """theta = 0 (sample 0 of both stress batches), a raised mu and a backtracking line search: no pair replays, as in the parent; and
    nothing replays under lq_replay = 0, with the outputs of the replaying solve."""
    on, want, full = results("on"), parent(), results("no_record")
    for name in ("mu_restart", "backtrack", "overflow"):
        assert not on[f"{name}/counts"].any() and np.array_equal(on[f"{name}/counts"], want[f"{name}/counts"]), name
        same(on, want, only=name)
    assert np.all(on["mu_restart/status"] == 3)                  # mu restarts keep the stress problem at iter_max
    assert (on["backtrack/ls"] > on["backtrack/iters"]).any()    # rejected line-search candidates
    assert all(not v.any() for k, v in full.items() if k.endswith("/counts"))
    same(on, full, skip_counts=True)


def test_non_finite_data_falls_back_to_the_full_pair():
    """The overflowing trajectory: non-finite H in the recording pass, so no record is valid (a non-finite factor invalidates it like a
    non-finite M^-1), nothing replays and the full pairs give the round-based path's outputs."""
    on, rounds = results("on"), results("rounds")
    assert not np.isfinite(on["overflow/value"]).all() or (on["overflow/status"] != 0).any()
    assert not on["overflow/counts"].any()
    for key in ("value", "status", "iters", "ls"):
        assert np.array_equal(on[f"overflow/{key}"], rounds[f"overflow/{key}"], equal_nan=True), key


def test_three_batches_on_one_handle_from_two_initial_points(monkeypatch):
    """The record of a batch must not leak into the next one on the handle: a, b, a against the round-based path."""
    monkeypatch.setenv("RATILQR_BLOCK", "0")
    theta = _draw_theta(8, seed=1000)
    prob, x0a, ua = rat.synthetic_lq_problem(N=7)
    rng = np.random.default_rng(77)
    x0b, ub = rng.standard_normal(12), 0.05 * rng.standard_normal((7, 4))
    ref = {}
    for tag, x0, u in (("a", x0a, ua), ("b", x0b, ub)):
        ctx = rat.Context(prob, max_batch=theta.size)
        ctx.set_path("rounds")
        ref[tag] = ctx.solve_batch(x0, u, theta)
    assert not np.array_equal(ref["a"][0], ref["b"][0])
    ctx = rat.Context(prob, max_batch=theta.size)
    ctx.set_path("fused")
    assert ctx.debug_get("lq_replay_factor") == 1
    for turn, (tag, x0, u) in enumerate((("a", x0a, ua), ("b", x0b, ub), ("a", x0a, ua))):
        got = ctx.solve_batch(x0, u, theta)
        for key, a, b in zip(("value", "status", "iters", "ls"), got, ref[tag]):
            assert np.array_equal(a, b, equal_nan=True), (turn, tag, key)
    assert ctx.debug_get("lq_replay_count") == 3 * 2 * theta.size
