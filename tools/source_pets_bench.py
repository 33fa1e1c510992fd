"""PETS on generative source models (rat_pets_problem_set_source, csrc/source_pets.h) against the LQ generative family at BASELINE config 5's
shape (N = 30, n = 12, m = 4, cubic drift, Gaussian noise, device generator), the documentation example, one device-resident rat_pets_solve,
and the compile times.  Prints one JSON line; profiles/source_pets.md records a run.  Run on an MI355X under a timeout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ratilqr.jl_amd as rat  # noqa: E402
from ratilqr.jl_amd import pets  # noqa: E402
from source_pets_models import DOCS, LQ, lq_params  # noqa: E402

n, m, Nh = 12, 4, 30


def config5():
    r = np.random.default_rng(8)
    A = 0.9 * np.linalg.qr(r.standard_normal((n, n)))[0]
    B = r.standard_normal((n, m)) / np.sqrt(n)
    fam = rat.LQGenerativeProblem(A, B, Nh, ("gaussian", np.zeros(n), 0.03 * np.eye(n)), Q=np.eye(n), R=0.1 * np.eye(m), Qf=np.eye(n),
                                  kappa=-0.01)
    src = rat.DeviceGenerativeSourceProblem(LQ, n, m, Nh, params=lq_params(fam), normals_per_step=n, uniforms_per_step=1)
    return fam, src, r.standard_normal(n), r


def per_call(ds, prob, x0, ctrl, reps):
    for i in range(3):
        c = pets.compute_cost_serial(ds, prob, x0, ctrl, None, False, seed=11 + i)      # warm-up (compile cache, buffers)
    t0 = time.perf_counter()
    for i in range(reps):
        c = pets.compute_cost_serial(ds, prob, x0, ctrl, None, False, seed=11 + i)
    dt = (time.perf_counter() - t0) / reps
    assert np.all(np.isfinite(c))
    return dt, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    out = {}
    # sources unique to this run (the compiler's on-disk cache must not serve them): first compile, a second with the compiler loaded,
    # the library's cache hit
    tag = f"// {time.time_ns()} {os.getpid()}\n"
    for key, src in (("compile_first_ms", LQ + tag), ("compile_second_ms", LQ + tag + "//\n"), ("compile_cached_ms", LQ + tag)):
        t = time.perf_counter(); rat.native.pets_source_check(src, n, m, n, 1); out[key] = (time.perf_counter() - t) * 1e3
    fam, src, x0, r = config5()
    for S, K in ((100, 100), (1000, 1000)):
        ctrl = 0.3 * r.standard_normal((S, Nh, m))
        res = {}
        for name, prob in (("family", fam), ("lq_source", src)):
            ds = rat.CrossEntropyDirectOptimizationSolver(np.zeros((Nh, m)), np.stack([np.eye(m)] * Nh), num_control_samples=S,
                                                          num_trajectory_samples=K)
            dt, c = per_call(ds, prob, x0, ctrl, a.reps)
            res[name] = c
            out[f"{name}_{S}x{K}_ms"] = dt * 1e3
            out[f"{name}_{S}x{K}_traj_per_s"] = S * K / dt
            if name == "lq_source":
                for tpw in (16, 32):                                   # trajectories per wavefront (switch src_pets_tpw, default 64)
                    ds.context(prob).debug_set("src_pets_tpw", tpw)
                    out[f"{name}_{S}x{K}_tpw{tpw}_traj_per_s"] = S * K / per_call(ds, prob, x0, ctrl, a.reps)[0]
                ds.context(prob).debug_set("src_pets_tpw", 64)
        out[f"mean_cost_ratio_{S}x{K}"] = float(np.mean(res["lq_source"]) / np.mean(res["family"]))
        out[f"source_vs_family_{S}x{K}"] = out[f"family_{S}x{K}_ms"] / out[f"lq_source_{S}x{K}_ms"]
    docs = rat.DeviceGenerativeSourceProblem(DOCS, 2, 2, 10, params=[10.0], normals_per_step=2, uniforms_per_step=1)
    for S, K in ((100, 100), (1000, 1000)):
        ds = rat.CrossEntropyDirectOptimizationSolver(np.zeros((10, 2)), np.stack([np.eye(2)] * 10), num_control_samples=S,
                                                      num_trajectory_samples=K)
        ctrl = r.standard_normal((S, 10, 2))
        for _ in range(3):
            pets.compute_cost_serial(ds, docs, np.zeros(2), ctrl, None, True, seed=1)
        t0 = time.perf_counter()
        for i in range(a.reps):
            pets.compute_cost_serial(ds, docs, np.zeros(2), ctrl, None, True, seed=1 + i)
        out[f"docs_true_model_{S}x{K}_traj_per_s"] = S * K * a.reps / (time.perf_counter() - t0)
    for name, prob in (("family", fam), ("lq_source", src)):       # solve!: 5 iterations x 100 control samples x 100 rollouts, one host wait
        ds = rat.CrossEntropyDirectOptimizationSolver(np.zeros((Nh, m)), np.stack([0.3 * np.eye(m)] * Nh), num_control_samples=100,
                                                      num_trajectory_samples=100, num_elite=10, iter_max=5)
        for _ in range(2):
            pets.solve_(ds, prob, x0, None, seed=3)
        t0 = time.perf_counter()
        for i in range(a.reps):
            pets.solve_(ds, prob, x0, None, seed=3 + i)
        out[f"{name}_solve_5x100x100_ms"] = (time.perf_counter() - t0) / a.reps * 1e3
    print(json.dumps({k: round(v, 4) for k, v in out.items()}))


if __name__ == "__main__":
    main()
