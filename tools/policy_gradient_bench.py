"""What rat_policy_gradient costs beside the replay it rides on; profiles/policy_gradient.md records what was run.

  resources  no device: rat_src_adjoint (source_adjoint.h) compiled offline for gfx950 from the translation unit csrc/source_model.cpp
             builds, at every size the tests use (1 x 1, 2 x 1 with and without the Jacobian hook, 5 x 3, 12 x 4): registers, spills,
             scratch, occupancy.
  measure    one MI355X, one process: the LQ + cubic source at 12 x 4, N = 50, a fixed closed-loop policy, four rows (theta = 0, 0.2 and
             two KL radii).  Per K: rat_policy_gradient against (a) rat_policy_worst_case_trajectory of the same rows -- the same replay
             with a cheaper payload: the floor, and the difference is the adjoint's price -- and, with --host-route, (b) x_out / u_out
             fetched and the NumPy adjoint of tests/policy_gradient_model.py; --runs alternating runs of each behind one warm-up of
             each, the median and the spread (max - min) per side.  (c), finite differences, is arithmetic: 2 x 2600 evaluations at
             the measured time of one.  The entry points are synchronous."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 50


def load():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import policy_gradient_model as pg
    import ratilqr.jl_amd as rat
    return rat, pg


def resources(a):
    _, pg = load()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    shapes = [("1 x 1 scalar LQ", pg.ScalarLQ()), ("2 x 1 pendulum", pg.Pendulum()), ("2 x 1 pendulum, Jacobian hook", pg.Pendulum(source=pg.PEND_JAC)),
              ("5 x 3 LQ + cubic", pg.LqCubic(5, 3, 2)), ("12 x 4 LQ + cubic", pg.LqCubic(12, 4, 3))]
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for label, case in shapes:
            tu = ('#include <hip/hip_runtime.h>\n#include "source_args.h"\n#include "rat_ad.h"\n#include "rat_rng.h"\n'
                  '#line 1 "model.hip"\n' + case.source + '\n#line 1 "source_adjoint.h"\n#include "source_adjoint.h"\n')
            path = os.path.join(tmp, "tu.hip")
            open(path, "w").write(tu)
            cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-I", a.csrc, f"-DRAT_N={case.n}", f"-DRAT_M={case.m}",
                   f"-DRAT_PETS_NORMALS={case.npn}", "-DRAT_PETS_UNIFORMS=0", "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o",
                   os.path.join(tmp, "tu.o")]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode:
                sys.exit(p.stderr[-3000:])
            block = p.stderr[p.stderr.index("Function Name: rat_src_adjoint"):]
            get = lambda key: int(re.search(key + r": (\d+)", block).group(1))
            rows.append(dict(shape=label, vgprs=get("VGPRs"), agprs=get("AGPRs"), sgprs=get("SGPRs"), vgpr_spill=get("VGPRs Spill"),
                             sgpr_spill=get("SGPRs Spill"), scratch=get(r"ScratchSize \[bytes/lane\]"), occupancy=get(r"Occupancy \[waves/SIMD\]"),
                             lds=get(r"LDS Size \[bytes/block\]")))
    for r in rows:
        print(json.dumps(r))


def measure(a):
    import numpy as np
    rat, pg = load()
    case = pg.LqCubic(12, 4, N)
    prob = rat.DeviceSourceProblem(case.source, case.n, case.m, N, np.eye(case.n), params=case.p)
    ctx = rat.Context(prob, max_batch=1, device=0)
    pol = pg.policy(case, N)
    rows = dict(kl_bounds=[0.05, 0.2], thetas=[0.0, 0.2])

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3
    for K in a.K:
        noise = rat.UserNoise(case.npn, 0, seed=3)
        t_eval = statistics.median(timed(lambda: ctx.policy_evaluate_noise(*pol, noise=noise, K=K)) for _ in range(3))
        sides = dict(gradient=lambda: ctx.policy_gradient(**rows), trajectory=lambda: ctx.policy_worst_case_trajectory(**rows))
        if a.host_route and K <= a.host_route:
            def host():
                ev = ctx.policy_evaluate_noise(*pol, noise=noise, K=K, want_costs=True, want_trajectories=True)
                gu, fin = pg.adjoint(case, ev["x"], ev["u"], pol[2])
                y, dead, _ = pg.weights(ev["costs"], **rows)
                pg.gradient(gu, fin, ev["x"], pol[0], pol[2], y, dead, ev["costs"])
            sides["host_route"] = host
        for fn in sides.values():
            fn()                                                      # one warm-up of each (the first gradient call compiles the adjoint kernel)
        t = {k: [] for k in sides}
        for _ in range(a.runs):
            for k, fn in sides.items():                               # alternating
                t[k].append(timed(fn))
        out = dict(K=K, evaluate_ms=t_eval, finite_differences_ms=2 * (N * case.m + N * case.m * case.n) * t_eval)
        for k, v in t.items():
            out[k + "_ms"], out[k + "_spread_ms"] = statistics.median(v), max(v) - min(v)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("resources", "measure"))
    ap.add_argument("--csrc", default=os.path.join(ROOT, "ratilqr.jl_amd", "csrc"))
    ap.add_argument("--K", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--host-route", type=int, default=0, help="largest K the host route is timed at (0: never)")
    a = ap.parse_args()
    dict(resources=resources, measure=measure)[a.mode](a)
