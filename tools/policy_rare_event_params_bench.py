"""What the shifted parameter normals of rat_policy_rare_event_params cost beside rat_policy_rare_event_user with parameter sampling on;
profiles/policy_rare_event_params.md records a run.

  resources  no device: rat_src_rare_rollout (the RAT_RARE_USER_EVENT variant) compiled offline for gfx950 from the translation unit
             csrc/source_model.cpp builds, parameter sampling on, without and with -DRAT_PARAM_SHIFT, on LQC at 12 x 4
             (tests/user_params_model.py: fourteen parameters, twelve normals and a uniform per step) and on the pendulum 2 x 1:
             registers, spills, scratch, occupancy.
  measure    one MI355X, one process: LQC at 12 x 4, N = 50, K = 2^20, n_iter = 4 under a fixed closed-loop policy, the event
             user_params_model.EVENT on the drawn obstacle radius; rat_policy_rare_event_params (adapt both) and
             rat_policy_rare_event_user, --runs alternating runs of each behind one warm-up call of each, the median and the spread
             (max - min) per side and the ratio of the medians.  The entry points are synchronous."""
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
    return pm.source(pm.LQC, "scale", pi0=12, pi1=11, pi2=0, psh=0.1) + "#define EVP 12\n" + pm.EVENT


def resources(a):
    _, pm = load()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    shapes = [("2 x 1 pendulum", pm.source(pm.PEND, "scale", pi0=3, pi1=2, pi2=0, psh=0.02) + "#define EVP 3\n" + pm.EVENT, 2, 1, 3, 0, 5),
              ("12 x 4 LQC", lqc_source(pm), 12, 4, 12, 1, 14)]
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for label, text, n, m, npn, npu, npar in shapes:
            for shift in (False, True):
                tu = ('#define RAT_RNG_SHIFT 1\n#include <hip/hip_runtime.h>\n#include "source_args.h"\n#include "rat_ad.h"\n#include "rat_rng.h"\n'
                      '#line 1 "model.hip"\n' + text + '\n#line 1 "source_rare.h"\n#include "source_rare.h"\n')
                path = os.path.join(tmp, "tu.hip")
                open(path, "w").write(tu)
                cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-I", a.csrc, f"-DRAT_N={n}", f"-DRAT_M={m}",
                       f"-DRAT_PETS_NORMALS={npn}", f"-DRAT_PETS_UNIFORMS={npu}", "-DRAT_N_EVENT=1", "-DRAT_RARE_USER_EVENT=1",
                       "-DRAT_USER_PARAMS_ON=1", f"-DRAT_N_PARAMS={npar}", f"-DRAT_PARAM_NORMALS={pm.PARAM_NORMALS}",
                       f"-DRAT_PARAM_UNIFORMS={pm.PARAM_UNIFORMS}", "-Rpass-analysis=kernel-resource-usage", "-c", path,
                       "-o", os.path.join(tmp, "tu.o")]
                if shift:
                    cmd.append("-DRAT_PARAM_SHIFT=1")
                p = subprocess.run(cmd, capture_output=True, text=True)
                if p.returncode:
                    sys.exit(p.stderr[-3000:])
                blk = p.stderr[p.stderr.index("Function Name: rat_src_rare_rollout"):]
                get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
                rows.append(dict(shape=label, param_shift="on" if shift else "off", vgprs=get("VGPRs"), agprs=get("AGPRs"), sgprs=get("SGPRs"),
                                 vgpr_spill=get("VGPRs Spill"), sgpr_spill=get("SGPRs Spill"), scratch=get(r"ScratchSize \[bytes/lane\]"),
                                 occupancy=get(r"Occupancy \[waves/SIMD\]")))
                print(json.dumps(rows[-1]), flush=True)
    print(json.dumps(dict(mode="resources", csrc=a.csrc, rows=rows)))


def measure(a):
    import numpy as np
    rat, pm = load()
    K = 1 << a.log2_k
    rng = np.random.default_rng(1)
    x, l, L = 0.5 * rng.standard_normal((N + 1, 12)), 0.2 * rng.standard_normal((N, 4)), 0.05 * rng.standard_normal((N, 4, 12))
    p = pm.LQC_P.copy()
    p[12] = 1e-3                                                      # a small obstacle: the level stays below 0 through the n_iter iterations
    ctx = rat.Context(rat.DeviceSourceProblem(lqc_source(pm), 12, 4, N, 0.02 * np.eye(12), params=p))
    ctx.set_param_sampling(rat.ParamSampling(pm.PARAM_NORMALS, pm.PARAM_UNIFORMS))
    noise = rat.UserNoise(12, 1, seed=1)
    new = lambda: ctx.policy_rare_event_params(x, l, L, 0, K, noise=noise, n_event=1, adapt="both", n_iter=a.n_iter, rho=0.1)
    old = lambda: ctx.policy_rare_event_user(x, l, L, 1, 0, K, noise=noise, n_iter=a.n_iter, rho=0.1)
    rn, ro = new(), old()                                             # warm-up: the code objects, the handle's buffers at this K
    ms = {"params": [], "user": []}
    for _ in range(a.runs):
        for side, fn in (("params", new), ("user", old)):
            t0 = time.perf_counter()
            fn()
            ms[side].append((time.perf_counter() - t0) * 1e3)
    stat = lambda v: dict(runs=[round(t, 3) for t in v], median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
    out = dict(mode="measure", K=K, N=N, n_iter=a.n_iter, params=stat(ms["params"]), user=stat(ms["user"]),
               iterations_run=dict(params=rn.n_iter, user=ro.n_iter), prob=dict(params=rn.prob, user=ro.prob))
    out["ratio"] = out["params"]["median"] / out["user"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("resources", "measure"))
    ap.add_argument("--csrc", default=os.path.join(ROOT, "ratilqr.jl_amd", "csrc"))
    ap.add_argument("--log2-k", type=int, default=20)
    ap.add_argument("--n-iter", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    dict(resources=resources, measure=measure)[a.mode](a)
