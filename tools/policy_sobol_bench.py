"""What rat_policy_sobol costs beside the rollouts it is made of; profiles/policy_sobol.md records a run.

  resources  no device: rat_src_sobol_rollout (source_sobol.h, -DRAT_RNG_PICK=1) and rat_src_user_noisy_rollout (source_user_noise.h)
             compiled offline for gfx950 from the translation unit csrc/source_model.cpp builds, parameter sampling on, on the pendulum
             2 x 1 and on LQC at 12 x 4 (tests/user_params_model.py: fourteen parameters, twelve normals and a uniform per step):
             registers, spills, scratch, occupancy.
  measure    one MI355X, one process: LQC at 12 x 4, N = 50, a fixed closed-loop policy, parameter sampling on (the generator), d = 4
             groups (the two scaled parameters' normals; the shift's uniform; the six even step normals; the six odd ones and the
             selector uniform).  Per K: one rat_policy_sobol call against (a) d + 2 rat_policy_evaluate_noise calls under the generator
             -- the same number of rollouts, the floor -- --runs alternating runs of each behind one warm-up of each, the median and
             the spread (max - min) per side and the ratio of the medians.  With --host-route K: (b) the route through injected
             streams, the only way to AB_i rollouts without the call -- per variant the host mixes the two streams draw by draw
             (NumPy), hands the parameter streams to rat_policy_params_sampling and the step streams to rat_policy_evaluate_noise;
             generating the two base streams is not timed.  The entry points are synchronous."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 50


def load():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import ratilqr.jl_amd as rat
    import user_params_model as pm
    return rat, pm


def lqc_source(pm):
    return pm.source(pm.LQC, "scale", pi0=10, pi1=11, pi2=0, psh=0.1)


def resources(a):
    _, pm = load()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    shapes = [("2 x 1 pendulum", pm.source(pm.PEND, "scale", pi0=1, pi1=2, pi2=0, psh=0.02), 2, 1, 3, 0, 5),
              ("12 x 4 LQC", lqc_source(pm), 12, 4, 12, 1, 14)]
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for label, text, n, m, npn, npu, npar in shapes:
            for header, entry, extra in (("source_user_noise.h", "rat_src_user_noisy_rollout", []),
                                         ("source_sobol.h", "rat_src_sobol_rollout", ["-DRAT_RNG_PICK=1"])):
                tu = ('#include <hip/hip_runtime.h>\n#include "source_args.h"\n#include "rat_ad.h"\n#include "rat_rng.h"\n'
                      '#line 1 "model.hip"\n' + text + f'\n#line 1 "{header}"\n#include "{header}"\n')
                path = os.path.join(tmp, "tu.hip")
                open(path, "w").write(tu)
                cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-I", a.csrc, f"-DRAT_N={n}", f"-DRAT_M={m}",
                       f"-DRAT_PETS_NORMALS={npn}", f"-DRAT_PETS_UNIFORMS={npu}", "-DRAT_USER_PARAMS_ON=1", f"-DRAT_N_PARAMS={npar}",
                       f"-DRAT_PARAM_NORMALS={pm.PARAM_NORMALS}", f"-DRAT_PARAM_UNIFORMS={pm.PARAM_UNIFORMS}",
                       "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", os.path.join(tmp, "tu.o")] + extra
                p = subprocess.run(cmd, capture_output=True, text=True)
                if p.returncode:
                    sys.exit(p.stderr[-3000:])
                blk = p.stderr[p.stderr.index("Function Name: " + entry):]
                get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
                rows.append(dict(shape=label, kernel=entry, vgprs=get("VGPRs"), agprs=get("AGPRs"), sgprs=get("SGPRs"),
                                 vgpr_spill=get("VGPRs Spill"), sgpr_spill=get("SGPRs Spill"), scratch=get(r"ScratchSize \[bytes/lane\]"),
                                 occupancy=get(r"Occupancy \[waves/SIMD\]")))
                print(json.dumps(rows[-1]), flush=True)
    print(json.dumps(dict(mode="resources", csrc=a.csrc, rows=rows)))


def groups(rat):
    G = rat.SobolGroup
    return [G(param_normals=(0, 1), name="scales"), G(param_uniforms=(0,), name="shift"), G(step_normals=range(0, 12, 2), name="even normals"),
            G(step_normals=range(1, 12, 2), step_uniforms=(0,), name="odd normals + selector")]


def stat(v):
    return dict(runs=[round(t, 3) for t in v], median=sorted(v)[len(v) // 2], spread=max(v) - min(v))


def measure(a):
    import numpy as np
    rat, pm = load()
    rng = np.random.default_rng(1)
    x, l, L = 0.5 * rng.standard_normal((N + 1, 12)), 0.2 * rng.standard_normal((N, 4)), 0.05 * rng.standard_normal((N, 4, 12))
    ctx = rat.Context(rat.DeviceSourceProblem(lqc_source(pm), 12, 4, N, 0.02 * np.eye(12), params=pm.LQC_P))
    gs = groups(rat)
    d = len(gs)
    for log2_k in a.log2_k:
        K = 1 << log2_k
        ctx.set_param_sampling(rat.ParamSampling(pm.PARAM_NORMALS, pm.PARAM_UNIFORMS))
        new = lambda: ctx.policy_sobol(x, l, L, noise=rat.UserNoise(12, 1), groups=gs, K=K, seed_a=1, seed_b=2)
        old = lambda: [ctx.policy_evaluate_noise(x, l, L, noise=rat.UserNoise(12, 1, seed=1 + v), K=K) for v in range(d + 2)]
        r, _ = new(), old()                                           # warm-up: the code objects, the handle's buffers at this K
        ms = {"sobol": [], "evaluate": []}
        for _ in range(a.runs):
            for side, fn in (("sobol", new), ("evaluate", old)):
                t0 = time.perf_counter()
                fn()
                ms[side].append((time.perf_counter() - t0) * 1e3)
        out = dict(mode="measure", K=K, N=N, d=d, rollouts=(d + 2) * K, sobol=stat(ms["sobol"]), evaluate=stat(ms["evaluate"]),
                   S=[round(float(v), 4) for v in r["S"]], T=[round(float(v), 4) for v in r["T"]], n_ok=r["n_ok"], flag=r["flag"])
        out["ratio"] = out["sobol"]["median"] / out["evaluate"]["median"]
        if a.host_route == log2_k:
            g = np.random.default_rng(2)
            A, B = ([g.standard_normal((K, N, 12)), g.random((K, N, 1)), g.standard_normal((K, 2)), g.random((K, 1))] for _ in range(2))
            masks = [(0, 0, 0, 0), (~0, ~0, ~0, ~0)] + [w.words for w in gs]

            def host():
                for pn_m, pu_m, sn_m, su_m in masks:
                    z = []
                    for a_, b_, mk in zip(A, B, (sn_m, su_m, pn_m, pu_m)):
                        cols = [i for i in range(a_.shape[-1]) if (mk >> i) & 1]
                        m_ = a_.copy()
                        m_[..., cols] = b_[..., cols]
                        z.append(m_)
                    ctx.set_param_sampling(rat.ParamSampling(pm.PARAM_NORMALS, pm.PARAM_UNIFORMS, zpn=z[2], zpu=z[3]))
                    ctx.policy_evaluate_noise(x, l, L, noise=rat.UserNoise(12, 1, zn=z[0], zu=z[1]), K=K)

            host()
            th = []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                host()
                th.append((time.perf_counter() - t0) * 1e3)
            out["host_route"] = stat(th)
            out["ratio_host_route"] = out["host_route"]["median"] / out["sobol"]["median"]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("resources", "measure"))
    ap.add_argument("--csrc", default=os.path.join(ROOT, "ratilqr.jl_amd", "csrc"))
    ap.add_argument("--log2-k", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--host-route", type=int, default=16, help="the log2 K at which the injected-stream route is timed too (0: never)")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    dict(resources=resources, measure=measure)[a.mode](a)
