"""Workloads of tests/test_gpu_stacked_operands.py, shared with tests/golden/make_stacked_operands_golden.py (which records what the tree
BEFORE the stacked operands computed on them: tests/golden/stacked_operands_parent.npz).

run(switches, path) solves every workload on one execution path and returns {name: array}: per batch value / status / iterations /
line-search counts, per single solve x, l (the controls: l + eps dl applied), L and the line search's eps history, and per handle the two
replay counters.  switches: {debug key: value} set on every handle before it solves (keys the library does not know are the caller's
business: the recorder passes none)."""
import numpy as np

import ratilqr.jl_amd as rat
from test_gpu_lq_replay import _draw_theta, _overflow_problem
from test_gpu_parity import stress_problem


def workloads():
    """(name, problem, x0, u, opts, thetas, theta of the single solve or None)"""
    it8 = rat.ileqg.make_opts(iter_max=8)
    th8 = _draw_theta(8, seed=1000)                              # the headline's draw: positive samples of N(1, 2)
    out = []
    # the headline problem at horizons around the replay's loop, which is unrolled by three steps: 5 and 7 leave it after its second and
    # first step of a turn, 1 after the only step, and the headline's own 50
    for N in (5, 7, 1, 50):
        prob, x0, u = rat.synthetic_lq_problem(N=N)
        out.append((f"lq_N{N}", prob, x0, u, None, th8, 3.0))
    # n = 3, m = 2: rows / columns 3..11 of V are padding, so the column the stack borrows (4) is zero in recursion A's own V
    prob, x0, u = rat.synthetic_lq_problem(n=3, m=2, N=12, seed=5)
    out.append(("lq_n3m2", prob, x0, u, None, th8, 1.5))
    # indefinite Q: H not PD, mu restarts, solves that run to iter_max (pairs the replay refuses at a raised mu)
    prob, x0, u = stress_problem(1, kappa=0.0)
    out.append(("mu_restart", prob, x0, u, it8, np.array([0.0, 0.3, 1.0, 4.0]), 1.0))
    # more indefinite: line searches that reject up to ~150 candidates per solve
    prob, x0, u = stress_problem(2, kappa=0.0, qs=-1.0)
    out.append(("backtrack", prob, x0, u, it8, np.array([0.0, 1.0, 4.0, 8.0]), 4.0))
    # a trajectory that overflows (non-finite operands: the replay must stop before its stores and the full sweep take over)
    prob, x0, u = _overflow_problem()
    out.append(("overflow", prob, x0, u, None, np.array([0.0, 0.5, 2.0, 5.0]), None))
    return out


def run(switches, path="fused"):
    res = {}

    def ctx(prob, opts, B):
        c = rat.Context(prob, opts, max_batch=B)
        c.set_path(path)
        for k, v in switches.items():
            c.debug_set(k, v)
        assert c.get_path(B) == path
        return c

    for name, prob, x0, u, opts, th, th1 in workloads():
        c = ctx(prob, opts, th.size)
        for key, a in zip(("value", "status", "iters", "ls"), c.solve_batch(x0, u, th)):
            res[f"{name}/{key}"] = a
        res[f"{name}/counts"] = np.array([c.debug_get("lq_replay_count"), c.debug_get("lq_replay_last_count")])
        if th1 is not None:
            r = ctx(prob, opts, 1).solve(x0, u, th1)
            res[f"{name}/x"], res[f"{name}/l"], res[f"{name}/L"] = r["x"], r["l"], r["L"]
            res[f"{name}/scalars"] = np.array([r["value"], r["status"], r["iters"]])
            res[f"{name}/eps_history"] = np.asarray(r["eps_history"], dtype=float)
    return res
