"""What model parameters drawn per rollout (rat_user_params, include/ratilqr.h "source models") cost in rat_src_user_noisy_rollout;
profiles/policy_user_params.md records a run.

  resources  no device: rat_src_user_noisy_rollout compiled offline for gfx950 from the translation unit csrc/source_model.cpp builds, with
             and without -DRAT_USER_PARAMS_ON, at three shapes -- the pendulum 2 x 1 (three normals), LQC (tests/user_params_model.py:
             fourteen parameters, RAT_N normals and a uniform per step) at 5 x 3 and at 12 x 4 -- and LQ_MIX at 12 x 4 without the flag
             (the kernel that fills 512 registers: its several hundred parameters are beyond the limit of 32, so it has no row with the
             flag): registers, spills, scratch and the seconds of the compile.  --csrc: the directory of the embedded headers.
  measure    one MI355X: rat_policy_evaluate_noise on LQC at 12 x 4, N = 50, K = 2^20 under a fixed closed-loop policy and the device
             generator, --sampling off | identity | scale (off: the hook is defined and not compiled in); the seconds of one call (a
             window of at least --min-seconds behind two warm-up calls; the entry point is synchronous).  --root: the checkout whose
             package and library are loaded; --hookless: the source without the hook (all a parent checkout can compile).
  ab         `measure --sampling off --hookless` in child processes, alternating --root A and --root B, --runs each: median and spread
             (max - min) per side; with the same root on both sides, the run-to-run spread the comparison is read against."""
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


def load(root):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, root)
    import ratilqr.jl_amd as rat
    import user_noise_model as um
    import user_params_model as pm
    return rat, um, pm


def resources(a):
    _, um, pm = load(ROOT)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lq = dict(pi0=10, pi1=11, pi2=0, psh=0.1)
    shapes = [("2 x 1 pendulum", pm.source(pm.PEND, "scale", pi0=1, pi1=2, pi2=0, psh=0.02), 2, 1, 3, 0, 5),
              ("5 x 3 LQC", pm.source(pm.LQC, "scale", **lq), 5, 3, 5, 1, 14), ("12 x 4 LQC", pm.source(pm.LQC, "scale", **lq), 12, 4, 12, 1, 14),
              ("12 x 4 LQ_MIX", um.LQ_MIX, 12, 4, 12, 1, 0)]
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for label, text, n, m, npn, npu, npar in shapes:
            for on in ((False, True) if npar else (False,)):
                tu = ('#include <hip/hip_runtime.h>\n#include "source_args.h"\n#include "rat_ad.h"\n#include "rat_rng.h"\n#line 1 "model.hip"\n' + text +
                      '\n#line 1 "source_user_noise.h"\n#include "source_user_noise.h"\n')
                path = os.path.join(tmp, "tu.hip")
                open(path, "w").write(tu)
                cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-I", a.csrc, f"-DRAT_N={n}", f"-DRAT_M={m}",
                       f"-DRAT_PETS_NORMALS={npn}", f"-DRAT_PETS_UNIFORMS={npu}", "-Rpass-analysis=kernel-resource-usage", "-c", path,
                       "-o", os.path.join(tmp, "tu.o")]
                if on:
                    cmd += ["-DRAT_USER_PARAMS_ON=1", f"-DRAT_N_PARAMS={npar}", f"-DRAT_PARAM_NORMALS={pm.PARAM_NORMALS}",
                            f"-DRAT_PARAM_UNIFORMS={pm.PARAM_UNIFORMS}"]
                t0 = time.perf_counter()
                p = subprocess.run(cmd, capture_output=True, text=True)
                dt = time.perf_counter() - t0
                if p.returncode:
                    sys.exit(p.stderr[-3000:])
                blk = p.stderr[p.stderr.index("Function Name: rat_src_user_noisy_rollout"):]
                get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
                rows.append(dict(shape=label, sampling="on" if on else "off", vgprs=get("VGPRs"), agprs=get("AGPRs"), sgprs=get("SGPRs"),
                                 vgpr_spill=get("VGPRs Spill"), scratch=get(r"ScratchSize \[bytes/lane\]"),
                                 occupancy=get(r"Occupancy \[waves/SIMD\]"), compile_s=round(dt, 2)))
                print(json.dumps(rows[-1]), flush=True)
    print(json.dumps(dict(mode="resources", csrc=a.csrc, rows=rows)))


def seconds(fn, min_seconds):
    fn(); fn()                                                           # warm-up: the code object, the handle's buffers at this K
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds and n >= 3:
            return dt / n


def measure(a):
    import numpy as np
    rat, um, pm = load(a.root)
    K = 1 << a.log2_k
    rng = np.random.default_rng(1)
    x, l, L = 0.5 * rng.standard_normal((N + 1, 12)), 0.2 * rng.standard_normal((N, 4)), 0.05 * rng.standard_normal((N, 4, 12))
    hook = "identity" if a.sampling == "identity" else "scale"
    src = pm.LQC if a.hookless else pm.source(pm.LQC, hook, pi0=10, pi1=11, pi2=0, psh=0.1)
    ctx = rat.Context(rat.DeviceSourceProblem(src, 12, 4, N, 0.02 * np.eye(12), params=pm.LQC_P))
    if a.sampling != "off":
        ctx.set_param_sampling(rat.ParamSampling(pm.PARAM_NORMALS, pm.PARAM_UNIFORMS))
    noise = rat.UserNoise(12, 1, seed=1)
    t = seconds(lambda: ctx.policy_evaluate_noise(x, l, L, noise=noise, K=K), a.min_seconds)
    r = ctx.policy_evaluate_noise(x, l, L, noise=noise, K=K)
    print(json.dumps(dict(mode="measure", root=a.root, sampling=a.sampling, hookless=a.hookless, K=K, N=N, ms=t * 1e3, mean=r["mean"], n_ok=r["n_ok"])))


def ab(a):
    sides = [("a", a.root), ("b", a.root_b or a.root)]
    ms = {"a": [], "b": []}
    for _ in range(a.runs):
        for side, root in sides:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "measure", "--root", root, "--sampling", "off", "--hookless",
                                "--log2-k", str(a.log2_k), "--min-seconds", str(a.min_seconds)], capture_output=True, text=True, timeout=300)
            if p.returncode:
                sys.exit(f"{root}: exit {p.returncode}\n{p.stderr[-2000:]}")
            ms[side].append(json.loads(p.stdout.strip().split("\n")[-1])["ms"])
            print(side, root, ms[side][-1], flush=True)
    stat = lambda v: dict(runs=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
    print(json.dumps(dict(mode="ab", a=stat(ms["a"]), b=stat(ms["b"]), root_a=sides[0][1], root_b=sides[1][1])))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("resources", "measure", "ab"))
    ap.add_argument("--csrc", default=os.path.join(ROOT, "ratilqr.jl_amd", "csrc"))
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--root-b", default=None)
    ap.add_argument("--sampling", choices=("off", "identity", "scale"), default="off")
    ap.add_argument("--hookless", action="store_true")
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--log2-k", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    dict(resources=resources, measure=measure, ab=ab)[a.mode](a)
