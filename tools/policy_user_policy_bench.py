"""What the user's controller (rat_user_policy, include/ratilqr.h "source models") costs in the Monte-Carlo rollout kernels;
profiles/policy_user_policy.md records a run.

  resources  no device: the four rollout kernels (rat_src_noisy_rollout, rat_src_user_noisy_rollout, both rat_src_rare_rollout) compiled
             offline for gfx950 from the translation unit csrc/source_model.cpp builds, at 2 x 1 (the pendulum) and 12 x 4 (LQ_MIX: twelve
             normals and a uniform), for three sources -- hookless, identity hook, clamp + rate limit -- and the registers, spills and
             scratch the compiler reports.  --csrc: the directory of the embedded headers (another checkout's, to compare).
  measure    one MI355X: rat_policy_evaluate_noise on the 12 x 4 LQ_MIX source at N = 50, K = 2^20 under a fixed closed-loop policy and
             the device generator, for --source hookless | identity | rate; the seconds of one call (a window of at least --min-seconds
             behind two warm-up calls; the entry point is synchronous).  --root: the checkout whose package and library are loaded.
  ab         `measure --source hookless` in child processes, alternating --root A and --root B, --runs each: median and spread (max - min)
             per side."""
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
KERNELS = (("source_noisy.h", "rat_src_noisy_rollout", ()), ("source_user_noise.h", "rat_src_user_noisy_rollout", ()),
           ("source_rare.h", "rat_src_rare_rollout", ("-DRAT_RNG_SHIFT_FIRST",)),
           ("source_rare.h", "rat_src_rare_rollout", ("-DRAT_RNG_SHIFT_FIRST", "-DRAT_N_EVENT=1", "-DRAT_RARE_USER_EVENT=1")))


def load(root):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, root)
    import ratilqr.jl_amd as rat
    import user_noise_model as um
    import user_policy_model as up
    return rat, um, up


def texts(um, up):
    """(size label, n, m, normals, uniforms, {source name: text}) for the two sizes"""
    out = []
    for label, base, poff, n, m, npn, npu in (("2 x 1", um.PEND_STATE, 3, 2, 1, 3, 0), ("12 x 4", um.LQ_MIX, "ohi + 1", 12, 4, 12, 1)):
        ev = lambda s: up.with_u_event(s, 900)                        # (the user-event variant of the rare kernel needs rat_user_event)
        out.append((label, n, m, npn, npu, {"hookless": ev(base), "identity": ev(up.source(base, poff, "identity")),
                                            "clamp + rate": ev(up.source(base, poff, "rate"))}))
    return out


def resources(a):
    _, um, up = load(ROOT)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for label, n, m, npn, npu, srcs in texts(um, up):
            for sname, text in srcs.items():
                for header, kernel, extra in KERNELS:
                    shift = "-DRAT_RNG_SHIFT_FIRST" in extra
                    # the translation unit of src_compile (csrc/source_model.cpp), hiprtc's implicit declarations from the HIP headers
                    tu = ("#include <hip/hip_runtime.h>\n" + ("#define RAT_RNG_SHIFT 1\n" if shift else "") +
                          '#include "source_args.h"\n#include "rat_ad.h"\n#include "rat_rng.h"\n#line 1 "model.hip"\n' + text +
                          f'\n#line 1 "{header}"\n#include "{header}"\n')
                    path = os.path.join(tmp, "tu.hip")
                    open(path, "w").write(tu)
                    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-I", a.csrc, f"-DRAT_N={n}", f"-DRAT_M={m}",
                           f"-DRAT_PETS_NORMALS={npn}", f"-DRAT_PETS_UNIFORMS={npu}", "-Rpass-analysis=kernel-resource-usage", "-c", path,
                           "-o", os.path.join(tmp, "tu.o")] + [e for e in extra if e != "-DRAT_RNG_SHIFT_FIRST"]
                    p = subprocess.run(cmd, capture_output=True, text=True)
                    if p.returncode:
                        sys.exit(p.stderr[-3000:])
                    blk = p.stderr[p.stderr.index(f"Function Name: {kernel}"):]
                    get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
                    rows.append(dict(size=label, source=sname, kernel=kernel + (" (user event)" if len(extra) > 1 else ""),
                                     vgprs=get("VGPRs"), agprs=get("AGPRs"), sgprs=get("SGPRs"), vgpr_spill=get("VGPRs Spill"),
                                     scratch=get(r"ScratchSize \[bytes/lane\]"), occupancy=get(r"Occupancy \[waves/SIMD\]"),
                                     lds=get(r"LDS Size \[bytes/block\]")))
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
    rat, um, up = load(a.root)
    K = 1 << a.log2_k
    gp = um.lq_generative(Nh=N)
    base = um.lq_source_problem(gp)
    rng = np.random.default_rng(1)
    x, l, L = 0.5 * rng.standard_normal((N + 1, 12)), 0.2 * rng.standard_normal((N, 4)), 0.05 * rng.standard_normal((N, 4, 12))
    noise = rat.UserNoise(12, 1, seed=1)
    src = um.LQ_MIX if a.source == "hookless" else up.source(um.LQ_MIX, "ohi + 1", a.source)
    params = np.concatenate([base.params, [0.0, 0.0, 1e300]])
    ctx = rat.Context(rat.DeviceSourceProblem(src, 12, 4, N, base.Wtab, params=params))
    # limits the affine law leaves in about half of the (rollout, step) pairs: from a small hookless-equivalent run (limits out of reach)
    ctx.set_params(np.concatenate([base.params, [1e300, 1e300, 1e300]]))
    small = ctx.policy_evaluate_noise(x, l, L, noise=noise, K=4096, want_trajectories=True)
    clamp = float(np.median(np.abs(small["u"]).max(axis=2)))
    ctx.set_params(np.concatenate([base.params, [clamp, 0.5 * clamp, 1e300]]))
    t = seconds(lambda: ctx.policy_evaluate_noise(x, l, L, noise=noise, K=K), a.min_seconds)
    r = ctx.policy_evaluate_noise(x, l, L, noise=noise, K=K)
    print(json.dumps(dict(mode="measure", root=a.root, source=a.source, K=K, N=N, ms=t * 1e3, mean=r["mean"], n_ok=r["n_ok"], clamp=clamp,
                          beyond=float((np.abs(small["u"]) > clamp).any(axis=2).mean()))))


def ab(a):
    ms = {a.root: [], a.root_b: []}
    for _ in range(a.runs):
        for root in (a.root, a.root_b):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "measure", "--root", root, "--source", "hookless",
                                "--log2-k", str(a.log2_k), "--min-seconds", str(a.min_seconds)], capture_output=True, text=True, timeout=300)
            if p.returncode:
                sys.exit(f"{root}: exit {p.returncode}\n{p.stderr[-2000:]}")
            ms[root].append(json.loads(p.stdout.strip().split("\n")[-1])["ms"])
            print(root, ms[root][-1], flush=True)
    side = lambda v: dict(runs=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
    print(json.dumps(dict(mode="ab", a=side(ms[a.root]), b=side(ms[a.root_b]), root_a=a.root, root_b=a.root_b)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("resources", "measure", "ab"))
    ap.add_argument("--csrc", default=os.path.join(ROOT, "ratilqr.jl_amd", "csrc"))
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--root-b", default=None)
    ap.add_argument("--source", choices=("hookless", "identity", "rate"), default="hookless")
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--log2-k", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    dict(resources=resources, measure=measure, ab=ab)[a.mode](a)
