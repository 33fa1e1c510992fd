"""Closed-loop rollouts of solve_fused_kernel on 4 x 4 x 4 f64 MFMAs (rollin_body<.., M4>, build constant RAT_ROLLOUT_MFMA4).

The seven MFMAs on the rollout's recursion chain are a matrix times one vector; the 4 x 4 x 4 form computes the same element from the same
operand registers in the same K order (tools/ubench/mfma_f64_shapes.hip), and x_{t+1} reaches B-form through DPP row rotations.  Only the
fused solve takes the form: the round-based path keeps the 16 x 16 x 4 sequence, so array_equal against it -- and against what the commit
before the stacked operands recorded (tests/golden/stacked_operands_parent.npz) -- holds the new form to the old, bit for bit.
Workloads: tests/stacked_operands_cases.py (computed once per session, shared with tests/test_gpu_stacked_operands.py), plus the horizons
that file does not have (the rollout runs groups of five steps and a tail: N mod 5 in {0, 1, 2}, and N = 1, 2: tails only) and a batch
that mixes theta = 0 samples, which replay nothing but roll out in the new form, with theta > 0 samples, and a cubic drift
(kappa != 0: the rollout then adds kappa x^3 on the one element a lane carries instead of on its three B-form registers).
The first five tests restate the issue's checklist for this change on the cached results of tests/test_gpu_stacked_operands.py (they cost no
GPU time of their own); the horizon, partial-tile, mixed-theta and cubic-drift tests are the new coverage.  The replays' row 12 of T stays
on 16 x 16 x 4 MFMAs, so there is no lq_replay_mfma4 switch to compare."""
import os

import numpy as np
import pytest

import ratilqr.jl_amd as rat
import test_gpu_stacked_operands as so
from test_gpu_lq_replay import _draw_theta

pytestmark = pytest.mark.gpu

KEYS = ("value", "status", "iters", "ls")


def _solve(prob, x0, u, theta, path, switches=()):
    os.environ["RATILQR_BLOCK"] = "0"
    try:
        ctx = rat.Context(prob, max_batch=theta.size)
        ctx.set_path(path)
        for k, v in switches:
            ctx.debug_set(k, v)
        assert ctx.get_path(theta.size) == path
        out = ctx.solve_batch(x0, u, theta)
        single = rat.Context(prob, max_batch=1)
        single.set_path(path)
        r = single.solve(x0, u, float(theta[-1]))
        return out, (ctx.debug_get("lq_replay_count"), ctx.debug_get("lq_replay_last_count")), r
    finally:
        del os.environ["RATILQR_BLOCK"]


def test_fused_equals_the_recorded_parent_counters_included():
    so.same(so.results("on"), so.parent())


def test_fused_equals_the_round_based_path():
    so.same(so.results("on"), so.results("rounds"), skip_counts=True)


def test_replay_stack_off_is_identical():
    so.same(so.results("on"), so.results("off"))


def test_refused_and_stopped_replays_keep_their_counters():
    on = so.results("on")
    for name in ("mu_restart", "backtrack", "overflow"):
        assert np.array_equal(on[f"{name}/counts"], [0, 0]), name


def test_counters_on_the_headline_problem_at_8_samples():
    assert np.array_equal(so.results("on")["lq_N50/counts"], [16, 8])


@pytest.mark.parametrize("N", [1, 2, 5, 6, 7, 50])
def test_horizons_against_the_round_based_path(N):
    prob, x0, u = rat.synthetic_lq_problem(N=N)
    th = _draw_theta(8, seed=1000)
    f, _, rf = _solve(prob, x0, u, th, "fused")
    r, _, rr = _solve(prob, x0, u, th, "rounds")
    for key, a, b in zip(KEYS, f, r):
        assert np.array_equal(a, b, equal_nan=True), (N, key)
    for key in ("x", "l", "L"):                                   # the trajectory the rollout produced, the controls, the gains
        assert np.array_equal(rf[key], rr[key], equal_nan=True), (N, key)


def test_partial_tile_against_the_round_based_path():
    """n = 3, m = 2 at a horizon with a tail of the group of five: rows and K entries beyond n, m stay zero through the block form."""
    prob, x0, u = rat.synthetic_lq_problem(n=3, m=2, N=7, seed=5)
    th = _draw_theta(8, seed=1000)
    f, _, rf = _solve(prob, x0, u, th, "fused")
    r, _, rr = _solve(prob, x0, u, th, "rounds")
    for key, a, b in zip(KEYS, f, r):
        assert np.array_equal(a, b, equal_nan=True), key
    for key in ("x", "l", "L"):
        assert np.array_equal(rf[key], rr[key], equal_nan=True), key


def test_mixed_theta_batch():
    """theta = 0 samples (risk-neutral: nothing replays) beside theta > 0 samples in one launch; every sample as in the round-based path,
    and the theta > 0 samples as in a batch of their own."""
    prob, x0, u = rat.synthetic_lq_problem()
    th = np.array([0.0, 3.0, 0.0, 0.5, 1.5, 0.0, 2.0, 0.0])
    f, counts, _ = _solve(prob, x0, u, th, "fused")
    r, _, _ = _solve(prob, x0, u, th, "rounds")
    for key, a, b in zip(KEYS, f, r):
        assert np.array_equal(a, b, equal_nan=True), key
    pos = th > 0
    g, counts_pos, _ = _solve(prob, x0, u, th[pos], "fused")
    for key, a, b in zip(KEYS, f, g):
        assert np.array_equal(a[pos], b, equal_nan=True), key
    assert counts == counts_pos                                   # the theta = 0 samples add no replay
    assert np.all(f[1] == 0)


@pytest.mark.parametrize("N", [7, 50])
def test_cubic_drift_against_the_round_based_path(N):
    """kappa = 0.05: x_{t+1} = [A|B][x; u] + kappa x^3 in the new form must round as the 16 x 16 x 4 form's per-register expression."""
    prob, x0, u = rat.synthetic_lq_problem(N=N, seed=5, kappa=0.05)
    th = _draw_theta(8, seed=1000)
    f, _, rf = _solve(prob, x0, u, th, "fused")
    r, _, rr = _solve(prob, x0, u, th, "rounds")
    for key, a, b in zip(KEYS, f, r):
        assert np.array_equal(a, b, equal_nan=True), (N, key)
    for key in ("x", "l", "L"):
        assert np.array_equal(rf[key], rr[key], equal_nan=True), (N, key)
    assert np.all(f[2] > 0)                                       # iterations ran: closed-loop rollouts with the cubic term
