"""Device path of the theta-sharding layer on one GPU (world size 1; N > 1 ranks are covered by the gloo test on CPU and
run by the driver's multi-GPU bench): theta and values stay in HBM, CE result equals the single-call C-ABI solve."""
import os

import numpy as np
import pytest
import torch

import ratilqr.jl_amd as rat
from ratilqr.jl_amd import cross_entropy as ce
from ratilqr.jl_amd import distributed as rd

pytestmark = pytest.mark.gpu


def test_gpu_evaluator_and_sharded_ce_equal_rat_ce_solve():
    prob, x0, u = rat.synthetic_lq_problem()
    z = np.random.default_rng(11).standard_normal(20000)
    B = 96
    ref_solver = rat.CrossEntropyBilevelOptimizationSolver(num_samples=B, num_elite=12)
    ref = ce.solve_(ref_solver, prob, x0, u, z, kl_bound=0.1)

    solver = rat.CrossEntropyBilevelOptimizationSolver(num_samples=B, num_elite=12)
    ctx = rat.Context(prob, solver.ileqg_opts, max_batch=B)
    ctx.set_initial(x0, u)
    ev = rd.gpu_evaluator(ctx)
    th = torch.linspace(0.1, 30.0, 40, dtype=torch.float64, device="cuda")
    val = ev(th)
    vh, st, _, _ = ctx.solve_batch(x0, u, th.cpu().numpy())
    assert np.array_equal(val.cpu().numpy(), vh) and np.isinf(vh[-1]) and st[-1] == 1

    def final(theta):
        r = ctx.solve(x0, u, theta)
        return r["status"] in (0, 3), r["x"], r["l"], r["L"], r["value"]

    got = rd.solve_sharded(solver, 0.1, z, ev, final, device="cuda")
    assert got[0] == ref[0] and got[4] == ref[4] and got[5] == ref[5] and got[6] == ref[6]
    assert np.array_equal(got[3], ref[3])
    assert solver.c.mu_init == ref_solver.c.mu_init and solver.c.n_solves == ref_solver.c.n_solves


def test_pets_sharded_cost_equals_the_single_call():
    """BASELINE config 5 (PETS rollouts, control samples sharded): the device evaluator of a shard addresses the injected noise by
    global sample index, so the world-size-1 result is the single-call result bit for bit, and an arbitrary block evaluated alone
    reproduces its slice (what a rank of a larger world computes; N > 1 ranks: gloo test on CPU)."""
    from ratilqr.jl_amd import pets
    rng = np.random.default_rng(5)
    Nh, n, m, S, K = 30, 12, 4, 40, 25
    Qo, _ = np.linalg.qr(rng.standard_normal((n, n)))
    prob = rat.LQGenerativeProblem(0.9 * Qo, rng.standard_normal((n, m)) / np.sqrt(n), Nh, ("gaussian", np.zeros(n), 0.05 * np.eye(n)),
                                   Q=np.eye(n), R=0.1 * np.eye(m), Qf=np.eye(n))
    ds = rat.CrossEntropyDirectOptimizationSolver(np.zeros((Nh, m)), np.stack([np.eye(m)] * Nh), num_control_samples=S, num_trajectory_samples=K)
    ctrl, x0 = 0.3 * rng.standard_normal((S, Nh, m)), rng.standard_normal(n)
    zn, zu = pets.draw_noise(prob, rng, S, K)
    ref = pets.compute_cost_serial(ds, prob, x0, ctrl, None, streams=(zn, zu))
    ev = rd.pets_gpu_evaluator(ds, prob, x0, streams=(zn, zu))
    got = rd.pets_compute_cost_sharded(ctrl, ev)
    assert np.array_equal(got, ref)
    lo, hi = rd.shard_bounds(S, 3, 1)
    assert np.array_equal(ev(ctrl[lo:hi], lo).numpy(), ref[lo:hi])
    # device generator: finite, reproducible, and different blocks get different noise
    ev2 = rd.pets_gpu_evaluator(ds, prob, x0, seed=3)
    a, b = ev2(ctrl[:8], 0).numpy(), ev2(ctrl[:8], 0).numpy()
    c = ev2(ctrl[:8], 8).numpy()
    assert np.all(np.isfinite(a)) and np.array_equal(a, b) and not np.array_equal(a, c)


def test_compute_cost_dev_is_value_plus_kl_over_theta(monkeypatch):
    """rat_ce_compute_cost_dev (theta and costs stay in HBM; on the fused path the sample's own wave writes its cost: one launch per
    batch) equals value + kl/theta of the host-pointer entry point bit for bit, Inf for infeasible samples, on every execution path."""
    prob, x0, u = rat.synthetic_lq_problem()
    theta_h = np.concatenate([np.abs(1.0 + 2.0 * np.random.default_rng(3).standard_normal(200)), [30.0, 50.0]])
    theta = torch.as_tensor(theta_h, dtype=torch.float64, device="cuda")
    for env in ({}, {"RATILQR_FUSED_DUAL": "0"}, {"RATILQR_FUSED": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for E in (1, 4):
            ctx = rat.Context(prob, max_batch=theta_h.size, spec_eps=E)
            ctx.set_initial(x0, u)
            cost = torch.empty_like(theta)
            ctx.compute_cost_dev(theta.data_ptr(), theta_h.size, 0.1, cost.data_ptr())
            v, st, _, _ = ctx.solve_batch(x0, u, theta_h)
            assert np.array_equal(cost.cpu().numpy(), v + 0.1 / theta_h)
            assert np.isposinf(cost.cpu().numpy()[-1]) and st[-1] == 1
            # stream-ordered form: three batches chained on the handle's stream without a host wait, consumed by torch work
            # ordered on the same stream
            hs = torch.cuda.ExternalStream(ctx.stream)
            costs = [torch.zeros_like(theta) for _ in range(3)]
            for c in costs:
                ctx.compute_cost_enqueue(theta.data_ptr(), theta_h.size, 0.1, c.data_ptr())
            with torch.cuda.stream(hs):
                stacked = torch.stack(costs)
            hs.synchronize()
            assert all(np.array_equal(row, v + 0.1 / theta_h) for row in stacked.cpu().numpy())
        for k in env:
            monkeypatch.delenv(k)


def _run_bench(nproc, extra_env, *args, launcher=True):
    """bench.py under torch.distributed.run (the driver's command) or, launcher=False, started plainly: it then launches its ranks itself."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(MASTER_ADDR="127.0.0.1", **extra_env)
    if launcher:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.join(root, "bench.py"), *args]
    else:
        cmd = [sys.executable, os.path.join(root, "bench.py"), *args]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def test_bench_collective_path_over_rccl_on_the_solver_stream():
    """The N > 1 step of bench.py -- batch enqueued on the handle's HIP stream, RCCL all-gather ordered behind it on that stream, next
    batch ordered behind the gather -- run with a one-rank RCCL communicator (test hook), costs checked by bench.py itself."""
    d = _run_bench(1, {"RATILQR_BENCH_FORCE_DIST": "1"}, "--gpus", "1", "--steps", "4", "--warmup", "2", "--full", "--no-cpu", "--no-second",
                   "--batch", "512")
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["value"] > 0 and d["roofline"]["launches"] == 4
    assert d["rccl_ranks"] == 1 and d["collective_backend"].startswith("rccl")


def test_bench_self_launches_two_ranks():
    """`python bench.py --gpus 2` with NO launcher around it: bench.py starts its two ranks itself (before touching the GPU), they shard
    the ONE global CE batch (strong scaling, `value`), run the barrier-bracketed timing with the max over ranks and the cost gather, and
    rank 0 prints the JSON line with `weak` and `strong_spec_eps8` beside it.  Two ranks share this box's single GPU and the collective
    is host-staged (test hooks of bench.py; on a multi-GPU node the same flow runs one rank per GPU over RCCL)."""
    d = _run_bench(2, {"RATILQR_BENCH_BACKEND": "gloo", "RATILQR_BENCH_ONE_DEVICE": "1"}, "--gpus", "2", "--steps", "3", "--warmup", "1",
                   "--full", "--no-cpu", "--batch", "256", launcher=False)
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 2 and d["self_launched"] is True and d["scaling"] == "strong" and d["steps"] == 3
    assert d["config"]["global_batch"] == 256 and d["strong"]["solves_per_gpu"] == [128, 128]
    assert d["value"] == d["strong"]["value"] > 0 and abs(d["value"] - 256 * 3 / (d["ms_per_step"] * 3e-3)) < 1e-6 * d["value"]
    assert d["config"]["feasible_fraction"] == 1.0 and d["roofline"]["launches"] == 3 and d["roofline"]["trajectories_per_launch"] == 128
    assert d["weak"]["global_batch"] == 512 and d["weak"]["value"] > 0
    assert d["strong_spec_eps8"]["costs_match_primary_1e-12"] is True and d["strong_spec_eps8"]["value"] > 0


def test_bench_runs_as_two_ranks_under_the_drivers_launcher():
    d = _run_bench(2, {"RATILQR_BENCH_BACKEND": "gloo", "RATILQR_BENCH_ONE_DEVICE": "1"}, "--gpus", "2", "--steps", "2", "--warmup", "1",
                   "--no-cpu", "--no-second", "--batch", "64")
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 2 and d["self_launched"] is False and d["strong"]["solves_per_gpu"] == [32, 32]


def test_bench_plain_run_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """A plain `bench.py --gpus 1` run: the headline alone (no roofline, CPU baseline or secondary in the line), exactly --steps timed
    steps, and with --dump-outputs the last timed step's per-sample cost and counters of the whole batch, as float64 .npy files that
    equal a direct solve of the same seeded batch."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    d = _run_bench(1, {}, "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path), launcher=False)
    assert d["steps"] == 3 and d["value"] > 0 and abs(d["value"] - 1024 * 3 / (d["ms_per_step"] * 3e-3)) < 1e-6 * d["value"]
    assert not {"roofline", "kernel_ms_per_step", "cpu_baseline", "steady_state", "secondary_contract"} & set(d)
    out = {k: np.load(tmp_path / f"{k}.npy") for k in ("cost", "status", "iters", "ls_evals")}
    assert all(v.dtype == np.float64 and v.shape == (1024,) for v in out.values())
    theta = bench.draw_theta(1024, seed=1000)
    prob, x0, u0 = rat.synthetic_lq_problem(n=12, m=4, N=50, seed=0)
    val, st, it, ls = rat.Context(prob, max_batch=1024, device=0).solve_batch(x0, u0, theta)
    assert np.array_equal(out["status"], st) and np.array_equal(out["iters"], it) and np.array_equal(out["ls_evals"], ls)
    assert np.allclose(out["cost"], val + 0.1 / theta, rtol=1e-12, atol=0.0)
    assert d["config"]["feasible_fraction"] == float(np.mean((st == 0) | (st == 3)))
