"""Solves per second of runtime-compiled source models (RAT_MODEL_SOURCE) against the host-closure path and the LQ family, plus
compile times.  Prints one JSON line; profiles/source_model.md records a run."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import ratilqr.jl_amd as rat  # noqa: E402
from test_gpu_source_model import PENDULUM, lq_pair, pendulum, source_pendulum  # noqa: E402


def rate(fn, B, reps):
    fn()                                                   # warm-up (first batch: compile cache, allocation)
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return B * reps / (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tpw", type=int, default=0, help="trajectories per wavefront of the rollout kernel (0: the library's default)")
    a = ap.parse_args()
    out = {}
    # sources unique to this run (the compiler's own on-disk cache must not serve them): the first compile of the process, a second one
    # with the compiler loaded, and the library's cache hit
    tag = f"// {time.time_ns()} {os.getpid()}\n"
    for key, src in (("compile_first_ms", PENDULUM + tag), ("compile_second_ms", PENDULUM + tag + "//\n"), ("compile_cached_ms", PENDULUM + tag)):
        t = time.perf_counter(); rat.native.source_check(src, 2, 1); out[key] = (time.perf_counter() - t) * 1e3
    gen, _, x0, u0 = pendulum()
    prob = source_pendulum()
    for B in (1, 128, 1024):
        ctx = rat.Context(prob, max_batch=B)
        if a.tpw:
            ctx.debug_set("src_tpw", a.tpw)
        th = np.linspace(0.0, 1.5, B)
        out[f"pendulum_B{B}_solves_per_s"] = rate(lambda: ctx.solve_batch(x0, u0, th), B, a.reps)
    th = np.linspace(0.0, 1.5, 128)
    gctx = rat.GenericContext(gen, max_batch=128)
    out["pendulum_closure_B128_solves_per_s"] = rate(lambda: rat.solve_closure_batch(gen, x0, u0, th, ctx=gctx), 128, 1)
    out["speedup_B128_vs_closure"] = out["pendulum_B128_solves_per_s"] / out["pendulum_closure_B128_solves_per_s"]
    fam, src, lx0, lu = lq_pair()
    th = np.linspace(0.0, 6.0, 1024)
    for name, p in (("lq_source", src), ("lq_family", fam)):
        for path in ("rounds", "auto"):
            ctx = rat.Context(p, max_batch=1024)
            ctx.set_path(path)
            out[f"{name}_{path}_B1024_solves_per_s"] = rate(lambda: ctx.solve_batch(lx0, lu, th), 1024, a.reps)
    print(json.dumps({k: round(v, 3) for k, v in out.items()}))


if __name__ == "__main__":
    main()
