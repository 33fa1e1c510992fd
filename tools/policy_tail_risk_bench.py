"""Time per call of the tail risk (rat_policy_tail_risk) on one MI355X; profiles/policy_tail_risk.md records a run.

  measure  K = 2^16, 2^20, 2^24 and 2^27, each in a child process of its own under its own time limit (`one`); a child that fails or runs
           out of time ends the run: nothing more is started on the device.
  one      one K: the device call on the costs an evaluation left on the device (cost = NULL) with 1 and 16 levels and with the weights,
           beside the host route it replaces on the same machine -- the K costs copied out (policy_evaluate with want_costs against the
           same call without), np.partition for the quantile and the sums of (J - v)^+ in NumPy.  Three runs of every figure: median and
           spread (max - min).  The evaluation runs a 2 x 2 LQ problem of four steps, so that 2^27 rollouts are cheap.
  once     a few calls at one K and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own (per-pass kernel times).
  md       profiles/policy_tail_risk.md from the JSON lines of the runs above and csrc/policy_mc.remarks.

Every timed window ends in the call's own device wait (the entry points are synchronous) and lasts at least --min-seconds."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (1 << 16, 1 << 20, 1 << 24, 1 << 27)
A1 = (0.95,)
A16 = (0.0, 0.1, 0.25, 0.5, 0.6, 0.75, 0.8, 0.9, 0.95, 0.975, 0.99, 0.995, 0.999, 0.9995, 0.9999, 0.99999)
HBM_TBS = 6.29                                                          # measured float4 copy (the microarchitecture guide); 8.0 spec


def per_call(fn, min_seconds, warm=2, least=3):
    for _ in range(warm):                                                # warm-up: code objects, the handle's scratch at this K
        fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds and n >= least:
            return dt / n


def three(fn, min_seconds, **kw):
    r = sorted(per_call(fn, min_seconds, **kw) for _ in range(3))
    return dict(median=r[1], spread=r[2] - r[0])


def host_route(J, alphas):
    """What a user who copies the costs out does: np.partition for s_k, then the Rockafellar-Uryasev sums."""
    J = J[~np.isnan(J)]
    n = J.size
    out = []
    for al in alphas:
        a = n * al
        k = min(max(int(np.ceil(a)), 1), n)
        v = np.partition(J, k - 1)[k - 1]
        d = np.maximum(J - v, 0.0)
        out.append((v, v + d.sum() / (n - a), (d * d).sum()))
    return out


def setup():
    import ratilqr.jl_amd as rat
    N = 4
    prob = rat.LQRiskSensitiveProblem(np.eye(2), np.eye(2), Q=np.eye(2), R=2 * np.eye(2), P=np.eye(2), N=N, W=np.array([[2.0, 0.6], [0.6, 1.0]]),
                                      Qf=np.eye(2))
    return rat.Context(prob), np.array([0.5, -1.0]), np.ones((N, 2))


def one(a):
    ctx, x0, l = setup()
    K = a.K
    ev = lambda **kw: ctx.policy_evaluate(x0, l, K=K, seed=1, **kw)
    costs = ev(want_costs=True)["costs"]
    out = dict(mode="one", K=K)
    out["device_a1"] = three(lambda: ctx.policy_tail_risk(A1), a.min_seconds)
    out["device_a16"] = three(lambda: ctx.policy_tail_risk(A16), a.min_seconds)
    out["device_a1_weights"] = three(lambda: ctx.policy_tail_risk(A1, want_weights=True), a.min_seconds)
    out["evaluate"] = three(lambda: ev(), a.min_seconds)
    out["evaluate_want_costs"] = three(lambda: ev(want_costs=True), a.min_seconds)
    out["host_a1"] = three(lambda: host_route(costs, A1), 0.0, warm=1, least=1)
    out["host_a16"] = three(lambda: host_route(costs, A16), 0.0, warm=1, least=1)
    dev, ref = ctx.policy_tail_risk(A16), host_route(costs, A16)
    out["var_equal"] = bool(all(dev["var"][i] == ref[i][0] for i in range(len(A16))))
    out["cvar_max_rel_diff"] = float(max(abs(dev["cvar"][i] / ref[i][1] - 1.0) for i in range(len(A16))))
    # the digit passes that sweep the costs: the digits on which the keys of min and max differ (csrc/policy_mc.hip, tr_key)
    ok = costs[~np.isnan(costs)]
    key = lambda v: (np.float64(v).view(np.uint64) | np.uint64(1 << 63)) if v >= 0 else ~np.float64(v).view(np.uint64)
    x = int(key(ok.min())) ^ int(key(ok.max()))
    out["sweeps"] = 0 if x == 0 else 8 - (64 - x.bit_length()) // 8
    print(json.dumps(out), flush=True)


def measure(a):
    for K in KS:
        limit = 120 + 60 * (K >> 24)                                     # the host route at 2^27 runs sixteen partitions of 1 GiB
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "one", "--K", str(K), "--min-seconds", str(a.min_seconds)], timeout=limit)
        if r.returncode != 0:
            sys.exit(f"K = {K}: the child ended with {r.returncode}; nothing more is started")


def once(a):
    ctx, x0, l = setup()
    ctx.policy_evaluate(x0, l, K=a.K, seed=1)
    for _ in range(3):
        ctx.policy_tail_risk(A16)
    for _ in range(3):
        ctx.policy_tail_risk(A1, want_weights=True)


def resources():
    path = os.path.join(ROOT, "ratilqr.jl_amd", "csrc", "policy_mc.remarks")
    if not os.path.exists(path):
        return ["`policy_mc.remarks` is not there: build the library first."]
    rows, cur = ["| kernel | VGPRs | SGPRs | LDS (B) | scratch (B/lane) | waves/SIMD |", "|---|---|---|---|---|---|"], {}
    for ln in open(path):
        m = re.search(r"remark:\s+(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        cur[m.group(1).split(" ")[0]] = m.group(2)
        if m.group(1).startswith("LDS") and re.search(r"\d(tr_\w+?)E6TrArgs", cur.get("Function", "")):
            name = re.search(r"\d(tr_\w+?)E6TrArgs", cur["Function"]).group(1)
            rows.append(f"| `{name}` | {cur['VGPRs']} | {cur['TotalSGPRs']} | {cur['LDS']} | {cur['ScratchSize']} | {cur['Occupancy']} |")
    return rows


def md(a):
    runs = [json.loads(ln) for f in a.json for ln in open(f) if ln.startswith("{")]
    by = {r["K"]: r for r in runs if r.get("mode") == "one"}
    L = ["# Tail risk of a policy (`rat_policy_tail_risk`): time per call", "",
         "Digit width: 8 bits, 8 passes.  A level's histogram is 256 u32 (`[16][256]` = 16 KiB of LDS a workgroup, several workgroups a compute",
         "unit) and the head of the next launch walks 256 bins a level; 11 bits would save two passes of eight but need 128 KiB of LDS (one",
         "workgroup a compute unit) and a walk of 2048 bins a level in every workgroup.  Costs of one policy share sign and exponent, so the",
         "first one or two passes usually sweep nothing either way.", "",
         "Kernel resources (`-Rpass-analysis=kernel-resource-usage`, gfx950; no GPU needed):", ""] + resources() + [""]
    if not by:
        L += ["No run recorded yet.  `tools/policy_tail_risk_bench.py` (`measure`, `once` under `rocprofv3 --kernel-trace --stats`, `md`) writes",
              "this file; until it has run on an MI355X the times, the ratio to the host route and the GB/s per select pass are not measured."]
    else:
        us = lambda d: f"{d['median'] * 1e6:.0f} µs ± {d['spread'] * 5e5:.0f}"
        ms = lambda d: f"{d['median'] * 1e3:.2f} ms ± {d['spread'] * 5e2:.2f}"
        ks = sorted(by)
        L += ["One MI355X, `tools/policy_tail_risk_bench.py measure`.  Costs of `rat_policy_evaluate` (a 2 x 2 LQ problem, four steps, device",
              "generator) left on the device.  Every figure: median of three runs ± half their spread; a run is a window of at least "
              f"{a.min_seconds:g} s of", "back-to-back synchronous calls after two warm-up calls (the host route: one call after one warm-up call per run).", "",
              "| | " + " | ".join(f"K = 2^{k.bit_length() - 1}" for k in ks) + " |", "|---|" + "---|" * len(ks)]
        row = lambda title, f: L.append(f"| {title} | " + " | ".join(f(by[k]) for k in ks) + " |")
        row("`rat_policy_tail_risk`, cost = NULL, 1 level", lambda r: us(r["device_a1"]))
        row("... 16 levels", lambda r: us(r["device_a16"]))
        row("... 1 level, the weights copied out", lambda r: us(r["device_a1_weights"]))
        row("host: the K costs copied out (`want_costs` against none)", lambda r: f"{(r['evaluate_want_costs']['median'] - r['evaluate']['median']) * 1e3:.2f} ms")
        row("host: `np.partition` + sums, 1 level", lambda r: ms(r["host_a1"]))
        row("host: ... 16 levels", lambda r: ms(r["host_a16"]))
        host = lambda r, k: r["evaluate_want_costs"]["median"] - r["evaluate"]["median"] + r[k]["median"]
        row("host route / device call, 1 level", lambda r: f"{host(r, 'host_a1') / r['device_a1']['median']:.0f}x")
        row("host route / device call, 16 levels", lambda r: f"{host(r, 'host_a16') / r['device_a16']['median']:.0f}x")
        row("passes that sweep the costs (of 8)", lambda r: str(r["sweeps"]))
        row("bytes read / call time, 16 levels (1 + passes + 2 sweeps of 8 K bytes)",
            lambda r: f"{(3 + r['sweeps']) * 8 * r['K'] / r['device_a16']['median'] / 1e12:.2f} TB/s")
        row("VAR equal to the host's, 16 levels", lambda r: str(r["var_equal"]))
        row("CVAR, largest relative difference", lambda r: f"{r['cvar_max_rel_diff']:.1e}")
        L += ["", f"The last but two rows hold the whole call (eleven launches, the read-back and the wait) against the {HBM_TBS} TB/s that a float4",
              "copy reaches on this part (8.0 TB/s specified): a lower bound on what a select pass achieves, exact only as K grows."]
    if a.notes:
        L += ["", open(a.notes).read().rstrip()]
    open(a.out, "w").write("\n".join(L) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("measure", "one", "once", "md"))
    ap.add_argument("--K", type=int, default=1 << 24)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--json", nargs="*", default=[])
    ap.add_argument("--notes", default=None, help="md: a text file appended as it is (kernel statistics, reading)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_tail_risk.md"))
    a = ap.parse_args()
    dict(measure=measure, one=one, once=once, md=md)[a.mode](a)
