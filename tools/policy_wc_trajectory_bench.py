"""Time per call of the worst-case trajectory moments (rat_policy_worst_case_trajectory) on one MI355X against the only route there was
before it: the trajectories to the host, then weighted NumPy moments.  profiles/policy_wc_trajectory.md records a run.

  measure  for the 12 x 4, N = 50 LQ family and for the pendulum source under a user sampler, K = 2^16 and 2^20 (--ks), one bound and the
           theta = 0 row: the device call after an evaluation; and the host route -- rat_rollout_noisy with x_out / u_out (families) or
           rat_policy_evaluate_noise with trajectories (source), rat_policy_worst_case with weights_out, then for both rows
           mean = w' z and cov = (w z)' z - mean mean' in NumPy (np.einsum, no fixed order).  The bytes of the trajectories are printed so
           that their PCIe time can be held against the difference.  One JSON line per figure.
  md       profiles/policy_wc_trajectory.md from those lines, with the kernels' registers and scratch from the build remarks
           (ratilqr.jl_amd/csrc/policy_mc.remarks).

Every timed window ends in the call's own device wait (the entry points are synchronous)."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ratilqr.jl_amd as rat  # noqa: E402

BOUNDS, THETAS = (0.1,), (0.0,)
PROFILE = os.path.join(ROOT, "profiles", "policy_wc_trajectory.md")


def timed(fn, repeat):
    fn()                                                                 # warm-up: code objects, the handle's buffers at this K
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return dict(median=ts[len(ts) // 2], spread=ts[-1] - ts[0], runs=repeat)


def numpy_moments(x, u, w):
    """mean and covariance of (x_t, u_t) per step under the weights w (0 at a DomainError rollout, whose trajectory may hold NaN)"""
    ok = w > 0
    z = np.concatenate([x[ok], np.pad(u[ok], ((0, 0), (0, 1), (0, 0)))], axis=2)
    wk = w[ok] / w[ok].sum()
    mean = np.einsum("k,kti->ti", wk, z)
    cov = np.einsum("kti,ktj->tij", z * wk[:, None, None], z) - mean[:, :, None] * mean[:, None, :]
    return mean, cov


def lq_case():
    prob, x0, u = rat.synthetic_lq_problem(n=12, m=4, N=50, seed=3, w=1e-2)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, u)
    L = 0.05 * np.random.default_rng(1).standard_normal((50, 4, 12))

    def evaluate(K):
        ctx.policy_evaluate(x_det, u, L, K=K, seed=7)

    def host(K):
        x, uu, cost, _ = ctx.rollout_noisy(x_det, u, L, K=K, seed=7)
        for kw in (dict(kl_bounds=BOUNDS), dict(thetas=THETAS)):
            w = ctx.policy_worst_case(costs=cost, want_weights=True, **kw)["weights"]
            numpy_moments(x, uu, w)
    return ctx, evaluate, host, 12, 4, 50


def pendulum_case():
    import user_noise_model as um
    N = 50
    x_nom, l, L = um.pend_policy(N)
    ctx = rat.Context(rat.DeviceSourceProblem(um.PEND_MIX, 2, 1, N, 1e-3 * np.eye(2), params=[0.1, 0.02, 0.03, 0.25, 0.2]))
    noise = rat.UserNoise(2, 1, seed=77)

    def evaluate(K):
        ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=K)

    def host(K):
        r = ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=K, want_trajectories=True)
        for kw in (dict(kl_bounds=BOUNDS), dict(thetas=THETAS)):
            w = ctx.policy_worst_case(want_weights=True, **kw)["weights"]
            numpy_moments(r["x"], r["u"], w)
    return ctx, evaluate, host, 2, 1, N


def measure(args):
    for name, case in (("lq_12x4_N50", lq_case), ("pendulum_user_noise_N50", pendulum_case)):
        ctx, evaluate, host, n, m, N = case()
        for K in args.ks:
            evaluate(K)
            dev = timed(lambda: ctx.policy_worst_case_trajectory(kl_bounds=BOUNDS, thetas=THETAS), args.repeat)
            ev = timed(lambda: evaluate(K), args.repeat)
            row = dict(case=name, K=K, device_call=dev, evaluation=ev, traj_bytes=8 * K * ((N + 1) * n + N * m))
            if K <= args.host_max_k:
                row["host_route"] = timed(lambda: host(K), max(1, args.repeat // 2))
            evaluate(K)
            print(json.dumps(row), flush=True)


def resources():
    path = os.path.join(ROOT, "ratilqr.jl_amd", "csrc", "policy_mc.remarks")
    if not os.path.exists(path):
        return {}
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: \S*?\d+(wct_[a-z]+)E", line)
        if m:
            cur = out.setdefault(m.group(1), {})
        for key, tag in (("VGPRs:", "vgprs"), ("ScratchSize [bytes/lane]:", "scratch"), ("Occupancy [waves/SIMD]:", "waves")):
            if cur is not None and key in line and "Spill" not in line:
                cur[tag] = line.split(key)[1].split("[")[0].strip()
    return out


def md(args):
    rows = [json.loads(ln) for ln in open(args.json) if ln.startswith("{")] if args.json and os.path.exists(args.json) else []
    out = ["# Worst-case trajectory moments (`rat_policy_worst_case_trajectory`): time per call", ""]
    if not rows:
        out += ["No run recorded yet.  `tools/policy_wc_trajectory_bench.py` (`measure`, then `md`) writes this file; until it has run on an",
                "MI355X the expectation -- the device route wins at K = 2²⁰ by at least the PCIe time of the trajectories -- is neither confirmed",
                "nor refuted, and no rate is promised."]
    else:
        out += ["One bound (d = 0.1) and the θ = 0 row per call, N = 50.  Host route: trajectories to the host, `rat_policy_worst_case` with",
                "`weights_out`, NumPy `einsum` moments for both rows.  Median of the runs (spread = max − min).", "",
                "| case | K | device call, ms | the evaluation it replays, ms | host route, ms | trajectories, MB |", "|---|---|---|---|---|---|"]
        for r in rows:
            h = r.get("host_route")
            out.append(f"| {r['case']} | {r['K']} | {1e3 * r['device_call']['median']:.2f} (± {1e3 * r['device_call']['spread']:.2f}) | "
                       f"{1e3 * r['evaluation']['median']:.2f} | " + (f"{1e3 * h['median']:.1f} (± {1e3 * h['spread']:.1f})" if h else "not run") +
                       f" | {r['traj_bytes'] / 1e6:.0f} |")
    res = resources()
    if res:
        out += ["", "Build remarks (gfx950): " + "; ".join(f"`{k}` {v.get('vgprs')} VGPRs, {v.get('scratch')} B scratch per lane, {v.get('waves')} waves per SIMD"
                                                             for k, v in sorted(res.items())) + "."]
    open(PROFILE, "w").write("\n".join(out) + "\n")
    print("\n".join(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("measure", "md"))
    ap.add_argument("--ks", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--host-max-k", type=int, default=1 << 20)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--json", default=None, help="md: the file holding measure's output lines")
    a = ap.parse_args()
    measure(a) if a.mode == "measure" else md(a)
