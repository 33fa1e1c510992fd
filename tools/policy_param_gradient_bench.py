"""What rat_policy_param_gradient costs beside rat_policy_gradient and beside finite differences; profiles/policy_param_gradient.md records
what was run.

  resources  no device: rat_src_adjoint_p (source_adjoint_params.h) compiled offline for gfx950 from the translation unit
             csrc/source_model.cpp builds, at 1 x 1 / 6 parameters, 2 x 1 / 3, 5 x 3 / 17, 12 x 4 / 4, 16 and 32, and 12 x 4 / 32 with
             parameter sampling on: registers, spills, scratch, occupancy.  Then rat_src_adjoint (source_adjoint.h) at the five shapes of
             tools/policy_gradient_bench.py: its table must come out as profiles/policy_gradient.md has it.
  measure    one MI355X, one process: the LQ + cubic source of tests/param_gradient_model.py at 12 x 4, N = 50, a fixed closed-loop policy,
             four rows (theta = 0, 0.2 and two KL radii), for 4, 16 and 32 parameters.  Per K: rat_policy_param_gradient against
             rat_policy_gradient on the same evaluation, --runs alternating runs of each behind one warm-up of each, the median and the
             spread (max - min) per side.  The finite-difference route is arithmetic: 2 n_params evaluations at the measured time of
             one rat_policy_evaluate_noise.  The entry points are synchronous."""
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
    import param_gradient_model as pp
    import policy_gradient_model as pg
    import ratilqr.jl_amd as rat
    return rat, pg, pp


def compile_usage(a, tmp, source, header, kernel, n, m, npn, extra=()):
    """the resource remarks of `kernel` of `header` behind `source`, compiled as src_compile does"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    tu = ('#include <hip/hip_runtime.h>\n#include "source_args.h"\n#include "rat_ad.h"\n#include "rat_rng.h"\n'
          '#line 1 "model.hip"\n' + source + f'\n#line 1 "{header}"\n#include "{header}"\n')
    path = os.path.join(tmp, "tu.hip")
    open(path, "w").write(tu)
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-I", a.csrc, f"-DRAT_N={n}", f"-DRAT_M={m}",
           f"-DRAT_PETS_NORMALS={npn}", "-DRAT_PETS_UNIFORMS=0", *extra, "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o",
           os.path.join(tmp, "tu.o")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode:
        sys.exit(p.stderr[-3000:])
    block = p.stderr[p.stderr.index(f"Function Name: {kernel} "):]
    get = lambda key: int(re.search(key + r": (\d+)", block).group(1))
    return dict(vgprs=get("VGPRs"), agprs=get("AGPRs"), sgprs=get("SGPRs"), vgpr_spill=get("VGPRs Spill"), sgpr_spill=get("SGPRs Spill"),
                scratch=get(r"ScratchSize \[bytes/lane\]"), occupancy=get(r"Occupancy \[waves/SIMD\]"), lds=get(r"LDS Size \[bytes/block\]"))


SAMPLING_HOOK = """
#define RAT_USER_PARAMS
template <class R> __device__ void rat_user_params(R &rng, const double *p, double *q) {
    for (int i = 0; i < RAT_N_PARAMS; ++i) q[i] = p[i] * (1.0 + 0.1 * rng.normal());
}
"""


def resources(a):
    _, pg, pp = load()
    shapes = [("1 x 1 / 6 scalar LQ", pp.ScalarLQ(), ()), ("2 x 1 / 3 pendulum", pp.Pendulum(), ()),
              ("2 x 1 / 3 pendulum, Jacobian hook", pp.Pendulum(source=pp.PEND_AD_JAC), ()), ("5 x 3 / 17 LQ + cubic", pp.LqCubic(5, 3, 17), ()),
              ("12 x 4 / 4 LQ + cubic", pp.LqCubic(12, 4, 4), ()), ("12 x 4 / 16 LQ + cubic", pp.LqCubic(12, 4, 16), ()),
              ("12 x 4 / 32 LQ + cubic", pp.LqCubic(12, 4, 32), ())]
    sampled = pp.LqCubic(12, 4, 32)
    sampled.source += SAMPLING_HOOK
    shapes.append(("12 x 4 / 32 LQ + cubic, sampling on", sampled, ("-DRAT_USER_PARAMS_ON=1", "-DRAT_PARAM_NORMALS=32", "-DRAT_PARAM_UNIFORMS=0")))
    with tempfile.TemporaryDirectory() as tmp:
        for label, case, extra in shapes:
            r = compile_usage(a, tmp, case.source, "source_adjoint_params.h", "rat_src_adjoint_p", case.n, case.m, case.npn,
                              (f"-DRAT_N_PARAMS={case.n_params}",) + extra)
            print(json.dumps(dict(kernel="rat_src_adjoint_p", shape=label, **r)))
        sibling = [("1 x 1 scalar LQ", pg.ScalarLQ()), ("2 x 1 pendulum", pg.Pendulum()), ("2 x 1 pendulum, Jacobian hook", pg.Pendulum(source=pg.PEND_JAC)),
                   ("5 x 3 LQ + cubic", pg.LqCubic(5, 3, 2)), ("12 x 4 LQ + cubic", pg.LqCubic(12, 4, 3))]
        for label, case in sibling:
            r = compile_usage(a, tmp, case.source, "source_adjoint.h", "rat_src_adjoint", case.n, case.m, case.npn)
            print(json.dumps(dict(kernel="rat_src_adjoint", shape=label, **r)))


def measure(a):
    import numpy as np
    rat, pg, pp = load()
    rows = dict(kl_bounds=[0.05, 0.2], thetas=[0.0, 0.2])

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3
    for NP in a.params:
        case = pp.LqCubic(12, 4, NP)
        prob = rat.DeviceSourceProblem(case.source, case.n, case.m, N, np.eye(case.n), params=case.p)
        ctx = rat.Context(prob, max_batch=1, device=0)
        pol = pg.policy(case, N)
        for K in a.K:
            noise = rat.UserNoise(case.npn, 0, seed=3)
            t_eval = statistics.median(timed(lambda: ctx.policy_evaluate_noise(*pol, noise=noise, K=K)) for _ in range(3))
            sides = dict(param_gradient=lambda: ctx.policy_param_gradient(**rows), gradient=lambda: ctx.policy_gradient(**rows))
            for fn in sides.values():
                fn()                                                  # one warm-up of each (the first call compiles its adjoint kernel)
            t = {k: [] for k in sides}
            for _ in range(a.runs):
                for k, fn in sides.items():                           # alternating
                    t[k].append(timed(fn))
            out = dict(n_params=NP, K=K, evaluate_ms=t_eval, finite_differences_ms=2 * NP * t_eval)
            for k, v in t.items():
                out[k + "_ms"], out[k + "_spread_ms"] = statistics.median(v), max(v) - min(v)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("resources", "measure"))
    ap.add_argument("--csrc", default=os.path.join(ROOT, "ratilqr.jl_amd", "csrc"))
    ap.add_argument("--K", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--params", type=int, nargs="+", default=[4, 16, 32])
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    dict(resources=resources, measure=measure)[a.mode](a)
