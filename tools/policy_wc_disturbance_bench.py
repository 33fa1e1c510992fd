"""Time per call of the worst-case disturbance moments (rat_policy_worst_case_disturbance) on one MI355X against the only route there was
before it -- the trajectories to the host, w reconstructed as x_{t+1} - f(x_t, u_t), weighted NumPy moments -- and against
rat_policy_worst_case_trajectory on the same evaluation.  profiles/policy_wc_disturbance.md records a run.

  measure  for the 12 x 4, N = 50 LQ family, K = 2^16 and 2^20 (--ks), one bound and the theta = 0 row: the device call with and without
           the cross product, the trajectory call on the same evaluation, the evaluation itself; and the host route -- rat_rollout_noisy
           with x_out / u_out, w = x_{t+1} - (A x_t + B u_t + kappa x_t^3), rat_policy_worst_case with weights_out, then for both rows the
           means and covariances in NumPy (np.einsum, no fixed order).  One JSON line per figure.
  md       profiles/policy_wc_disturbance.md: the measured deviations (tests/test_cpu_wc_disturbance.py), the kernels' registers and
           scratch from the build remarks (ratilqr.jl_amd/csrc/policy_mc.remarks), and the times from measure's lines -- marked as not yet
           measured while there are none.

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
PROFILE = os.path.join(ROOT, "profiles", "policy_wc_disturbance.md")


def timed(fn, repeat):
    fn()                                                                 # warm-up: code objects, the handle's buffers at this K
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return dict(median=ts[len(ts) // 2], spread=ts[-1] - ts[0], runs=repeat)


def numpy_moments(w, x, u, p):
    """mean and covariance of w_t and its covariance with (x_t, u_t) per step under the weights p (0 at a DomainError rollout)"""
    ok = p > 0
    z = np.concatenate([x[ok][:, :-1], u[ok]], axis=2)
    w, pk = w[ok], p[ok] / p[ok].sum()
    mw, mz = np.einsum("k,kti->ti", pk, w), np.einsum("k,kti->ti", pk, z)
    pw = w * pk[:, None, None]
    return mw, np.einsum("kti,ktj->tij", pw, w) - mw[:, :, None] * mw[:, None, :], np.einsum("kti,ktj->tij", pw, z) - mw[:, :, None] * mz[:, None, :]


def lq_case():
    prob, x0, u = rat.synthetic_lq_problem(n=12, m=4, N=50, seed=3, w=1e-2)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, u)
    L = 0.05 * np.random.default_rng(1).standard_normal((50, 4, 12))

    def evaluate(K):
        ctx.policy_evaluate(x_det, u, L, K=K, seed=7)

    def host(K):
        x, uu, cost, _ = ctx.rollout_noisy(x_det, u, L, K=K, seed=7)
        w = x[:, 1:] - (x[:, :-1] @ prob.A.T + uu @ prob.B.T + prob.kappa * x[:, :-1] ** 3)
        for kw in (dict(kl_bounds=BOUNDS), dict(thetas=THETAS)):
            p = ctx.policy_worst_case(costs=cost, want_weights=True, **kw)["weights"]
            numpy_moments(w, x, uu, p)
    return ctx, evaluate, host, 12, 4, 50


def measure(args):
    ctx, evaluate, host, n, m, N = lq_case()
    for K in args.ks:
        evaluate(K)
        row = dict(case="lq_12x4_N50", K=K, traj_bytes=8 * K * ((N + 1) * n + N * m))
        row["device_call"] = timed(lambda: ctx.policy_worst_case_disturbance(kl_bounds=BOUNDS, thetas=THETAS), args.repeat)
        row["device_call_no_cross"] = timed(lambda: ctx.policy_worst_case_disturbance(kl_bounds=BOUNDS, thetas=THETAS, cross=False), args.repeat)
        row["trajectory_call"] = timed(lambda: ctx.policy_worst_case_trajectory(kl_bounds=BOUNDS, thetas=THETAS), args.repeat)
        row["evaluation"] = timed(lambda: evaluate(K), args.repeat)
        if K <= args.host_max_k:
            row["host_route"] = timed(lambda: host(K), max(1, args.repeat // 2))
        print(json.dumps(row), flush=True)


def resources():
    path = os.path.join(ROOT, "ratilqr.jl_amd", "csrc", "policy_mc.remarks")
    if not os.path.exists(path):
        return {}
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: \S*?\d+(wcd_[a-z]+)(ILb([01])E)?", line)
        if m:
            cur = out.setdefault(m.group(1) + ({"1": "<true>", "0": "<false>"}.get(m.group(3), "")), {})
        elif "Function Name:" in line:
            cur = None
        for key, tag in (("VGPRs:", "vgprs"), ("TotalSGPRs:", "sgprs"), ("ScratchSize [bytes/lane]:", "scratch"), ("LDS Size [bytes/block]:", "lds"),
                         ("Occupancy [waves/SIMD]:", "waves")):
            if cur is not None and key in line and "Spill" not in line:
                cur[tag] = line.split(key)[1].split("[")[0].strip()
    return out


DEVIATIONS = """## Deviations (measured; how each was taken)

`tests/test_cpu_wc_disturbance.py`, on the host: the NumPy restatement of the device's summation order and centre
(`tests/wc_disturbance_model.py: moments`) against np.longdouble straight from the definition (`direct`), worst over the cases, each
relative to its step's scale (`deviation`).  The GPU tests hold the device to 1e-12 of the restatement and to ten times these figures
against np.longdouble.

| quantity | case | deviation |
|---|---|---|
| `mean_w` | sampler mean 7 sd from 0, c_w a rollout 4 sd out, K = 1 … 65541 | 2.12e-16 |
| `cov_w` | the same | 8.25e-15 (K = 65541) |
| `cov_wz` | the same, (x, u) centre at the nominal | 2.71e-16 (K = 5) |
| `cov_wz` | (x, u) centre 7 sd off, every component varies | 5.17e-16 (K = 65541) |
| `cov_wz` | (x, u) centre off and a component that does not vary (the pendulum's position one step on under a sampler that leaves w[0] alone) | 7.50e-15 (K = 65541; 2.7e-16 at K = 257) |
| `cov_w` with c_w = 0 instead (not what the device does) | sampler mean 7 sd from 0 | 4.65e-14, against 3.5e-16 about a draw |

On the MI355X (`tests/test_gpu_wc_disturbance.py`, printed per case; worst over all cases): against the restatement 1.4e-15 (mean) and
1.6e-14 (`cov_w`), both at the 12 × 4 family, N = 10, K = 65, closed loop, and 5.1e-16 (`cov_wz`); against np.longdouble 1.1e-15 (mean,
the same case), 3.2e-14 (`cov_w`, PEND_STATE, K = 2000) and 1.3e-14 (`cov_wz`, PEND_NAN closed loop at K = 65541: the
non-varying-component case above).

The reference w -- host Cholesky times the NumPy model of the generator for the families, NumPy restatements of the samplers for source
models -- showed no difference from the device's w beyond these figures in any case (the PEND_STATE sampler `p[1] |x[1]| z1 + p[2] z2`,
which the device may contract into a multiply-add, included): no allowance for it was added to any tolerance.

Closed form (LQ, κ = 0; θ = 0.3 / λmax and θ = 0, K = 2¹⁶, seed 2026): every entry of `mean_w`, `cov_w`, `cov_wz` within 6 standard
errors on the host pipeline and on the device; the worst entry is 2.98 SE on both (4 × 2, N = 5, θ = 0, `cov_wz`), ESS / K = 0.698 (2 × 2,
N = 3) and 0.2502 (4 × 2, N = 5).
"""


def md(args):
    rows = [json.loads(ln) for ln in open(args.json) if ln.startswith("{")] if args.json and os.path.exists(args.json) else []
    out = ["# Worst-case disturbance moments (`rat_policy_worst_case_disturbance`)", "", "## Time per call", ""]
    if not rows:
        out += ["**Not yet measured.**  `tools/policy_wc_disturbance_bench.py` (`measure`, then `md --json`) writes this section; until it has run",
                "on an MI355X no time is claimed.  What it will show at 12 × 4, N = 50, K = 2²⁰, one bound and the θ = 0 row: the call beside",
                "`rat_policy_worst_case_trajectory` on the same evaluation (the same replay; one more store per lane and step in the rollouts, two",
                "MFMAs per group where that call issues one, 552 doubles per partial where it has 288), and beside the host route (5 GB of",
                "trajectories over PCIe, w reconstructed as x_{t+1} − f(x_t, u_t), NumPy moments)."]
    else:
        out += ["One bound (d = 0.1) and the θ = 0 row per call, 12 × 4 LQ family, N = 50.  Host route: trajectories to the host, w reconstructed as",
                "x_{t+1} − f(x_t, u_t), `rat_policy_worst_case` with `weights_out`, NumPy `einsum` moments for both rows.  Median of the runs",
                f"(spread = max − min; {rows[0]['device_call']['runs']} runs per device figure, {rows[0].get('host_route', {}).get('runs', 0)} of the host route, which",
                "is run only where a figure is shown); every window ends in the call's own device wait.", "",
                "| K | device call, ms | without the cross product, ms | trajectory call, ms | the evaluation they replay, ms | host route, ms | trajectories, MB |",
                "|---|---|---|---|---|---|---|"]
        ms = lambda t: f"{1e3 * t['median']:.2f} (± {1e3 * t['spread']:.2f})"
        for r in rows:
            h = r.get("host_route")
            out.append(f"| {r['K']} | {ms(r['device_call'])} | {ms(r['device_call_no_cross'])} | {ms(r['trajectory_call'])} | {ms(r['evaluation'])} | "
                       + (ms(h) if h else "not run") + f" | {r['traj_bytes'] / 1e6:.0f} |")
    out += ["", DEVIATIONS]
    res = resources()
    if res:
        out += ["## Build remarks (gfx950)", "", "| kernel | VGPRs | SGPRs | scratch, B per lane | LDS, B | waves per SIMD |", "|---|---|---|---|---|---|"]
        out += [f"| `{k}` | {v.get('vgprs')} | {v.get('sgprs')} | {v.get('scratch')} | {v.get('lds')} | {v.get('waves')} |" for k, v in sorted(res.items())]
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
