"""What rat_policy_margin_gradient costs beside the calls it is built from; profiles/policy_margin_gradient.md records what was run.

  resources  no device: rat_src_margin_adjoint (source_margin_adjoint.h) compiled offline for gfx950 from the translation unit
             csrc/source_model.cpp builds, with 1, 2 and 4 events at 12 x 4 and at the other sizes the tests use: registers, spills,
             scratch, LDS, occupancy.
  measure    one MI355X, one process: the LQ + cubic source at 12 x 4, N = 50, a fixed closed-loop policy.  Per K and for 1 and 4 events
             x 2 levels: rat_policy_margin_gradient against (a) rat_policy_tail_gradient with the same number of rows on the same handle
             -- the same replay and moments but one sweep and one pass -- and (b) one rat_policy_events call with the same events, pass
             A's floor; --runs alternating runs of each behind one warm-up of each, the median and the spread (max - min) per side.
             The ratio asked for, four events in one call against four single-event calls, is printed per K.  The entry points are
             synchronous.
  trace      one call of each kind at --K for a kernel trace (run under rocprofv3 --kernel-trace --stats -- python tools/... trace)."""
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
    import margin_gradient_model as mg
    import policy_gradient_model as pg
    import ratilqr.jl_amd as rat
    return rat, pg, mg


def resources(a):
    _, pg, _ = load()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    big = pg.LqCubic(12, 4, 3)
    shapes = [("12 x 4 LQ + cubic", big, 1), ("12 x 4 LQ + cubic", big, 2), ("12 x 4 LQ + cubic", big, 4), ("1 x 1 scalar LQ", pg.ScalarLQ(), 4),
              ("2 x 1 pendulum", pg.Pendulum(), 4), ("2 x 1 pendulum, Jacobian hook", pg.Pendulum(source=pg.PEND_JAC), 4),
              ("5 x 3 LQ + cubic", pg.LqCubic(5, 3, 2), 4)]
    with tempfile.TemporaryDirectory() as tmp:
        for label, case, E in shapes:
            tu = ('#include <hip/hip_runtime.h>\n#include "source_args.h"\n#include "rat_ad.h"\n#include "rat_rng.h"\n'
                  '#line 1 "model.hip"\n' + case.source + '\n#line 1 "source_margin_adjoint.h"\n#include "source_margin_adjoint.h"\n')
            path = os.path.join(tmp, "tu.hip")
            open(path, "w").write(tu)
            cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-I", a.csrc, f"-DRAT_N={case.n}", f"-DRAT_M={case.m}",
                   f"-DRAT_PETS_NORMALS={case.npn}", "-DRAT_PETS_UNIFORMS=0", f"-DRAT_N_MARGIN={E}", "-Rpass-analysis=kernel-resource-usage", "-c",
                   path, "-o", os.path.join(tmp, "tu.o")]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode:
                sys.exit(p.stderr[-3000:])
            block = p.stderr[p.stderr.index("Function Name: rat_src_margin_adjoint"):]
            get = lambda key: int(re.search(key + r": (\d+)", block).group(1))
            print(json.dumps(dict(shape=label, events=E, vgprs=get("VGPRs"), agprs=get("AGPRs"), sgprs=get("SGPRs"), vgpr_spill=get("VGPRs Spill"),
                                  sgpr_spill=get("SGPRs Spill"), scratch=get(r"ScratchSize \[bytes/lane\]"),
                                  occupancy=get(r"Occupancy \[waves/SIMD\]"), lds=get(r"LDS Size \[bytes/block\]"))))


def setup(rat, pg, mg):
    import numpy as np
    case = pg.LqCubic(12, 4, N)
    prob = rat.DeviceSourceProblem(case.source, case.n, case.m, N, np.eye(case.n), params=case.p)
    ctx = rat.Context(prob, max_batch=1, device=0)
    pol = pg.policy(case, N)
    evs = [mg.to_rat(rat, e) for e in (mg.quadratic_event(case, N, 22), mg.linear_event(case, N, 21, N), mg.quadratic_event(case, N, 24, lo=N // 2),
                                       (None,) + mg.linear_event(case, N, 23, 0)[1:3] + (0, N - 1))]
    return case, ctx, pol, evs


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def measure(a):
    rat, pg, mg = load()
    case, ctx, pol, evs = setup(rat, pg, mg)
    al = [0.0, 0.9]
    for K in a.K:
        noise = rat.UserNoise(case.npn, 0, seed=3)
        t_eval = statistics.median(timed(lambda: ctx.policy_evaluate_noise(*pol, noise=noise, K=K)) for _ in range(3))
        sides = {
            "margin_1": lambda: ctx.policy_margin_gradient(evs[:1], al),
            "margin_4": lambda: ctx.policy_margin_gradient(evs, al),
            "margin_4x1": lambda: [ctx.policy_margin_gradient([e], al) for e in evs],
            "tail_gradient_2": lambda: ctx.policy_tail_gradient(al),
            "tail_gradient_8": lambda: ctx.policy_tail_gradient([0.0, 0.5, 0.8, 0.9, 0.95, 0.98, 0.99, 0.995]),
            "events_1": lambda: ctx.policy_events(evs[:1], thetas=[0.0]),
            "events_4": lambda: ctx.policy_events(evs, thetas=[0.0]),
        }
        for fn in sides.values():
            fn()                                                      # one warm-up of each (the first calls compile the adjoint kernels)
        t = {k: [] for k in sides}
        for _ in range(a.runs):
            for k, fn in sides.items():                               # alternating
                t[k].append(timed(fn))
        out = dict(K=K, evaluate_ms=t_eval)
        for k, v in t.items():
            out[k + "_ms"], out[k + "_spread_ms"] = statistics.median(v), max(v) - min(v)
        out["four_in_one_over_four_single"] = out["margin_4_ms"] / out["margin_4x1_ms"]
        print(json.dumps(out), flush=True)


def trace(a):
    rat, pg, mg = load()
    case, ctx, pol, evs = setup(rat, pg, mg)
    K = a.K[0]
    ctx.policy_evaluate_noise(*pol, noise=rat.UserNoise(case.npn, 0, seed=3), K=K)
    for _ in range(a.runs):
        ctx.policy_margin_gradient(evs, [0.0, 0.9])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("resources", "measure", "trace"))
    ap.add_argument("--csrc", default=os.path.join(ROOT, "ratilqr.jl_amd", "csrc"))
    ap.add_argument("--K", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    dict(resources=resources, measure=measure, trace=trace)[a.mode](a)
