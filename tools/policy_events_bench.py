"""The kernels of one rat_policy_events call on one MI355X beside those of rat_policy_worst_case_trajectory on the same evaluation, the
nearest thing there was before it.  profiles/policy_events.md records a run.

  run    the 12 x 4, N = 50 LQ family at K = 2^20 (--K): one policy_evaluate, then ONE call of --what: `events` (16 quadratic events over all
         16 coordinates, one bound and three thetas: 4 rows, with the per-step sums) or `trajectory` (the same 4 rows).  Meant to be the
         program of `rocprofv3 --kernel-trace --stats -- python tools/policy_events_bench.py run --what events`; prints the call's wall time.
  table  from a kernel-trace CSV of such a run: the kernels of the call alone -- everything dispatched from the first wc_var on, which
         leaves the evaluation's own rollouts and reduction out -- with calls, total microseconds and share; and the share of the kernels
         named by --new over the replay's rollouts.

The yardstick is the replay: the call cannot be faster than the rollouts it reruns."""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ratilqr.jl_amd as rat  # noqa: E402

BOUNDS, THETAS = (0.1,), (0.0, 0.02, 0.05)


def run(what, K):
    prob, x0, u = rat.synthetic_lq_problem(n=12, m=4, N=50, seed=3, w=1e-2)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, u)
    L = 0.05 * np.random.default_rng(1).standard_normal((50, 4, 12))
    r = ctx.policy_evaluate(x_det, u, L, K=K, seed=7)
    rng = np.random.default_rng(2)
    evs = []
    for i in range(16):
        A = rng.standard_normal((16, 16))
        evs.append(rat.quadratic_event(A + A.T, rng.standard_normal(16), -10.0 * (i + 1)))
    t0 = time.perf_counter()
    if what == "events":
        out = ctx.policy_events(evs, kl_bounds=BOUNDS, thetas=THETAS, want_steps=True)
        note = f"any: prob {out['thetas']['prob'][0, 16]:.4f} nominal, {out['bounds']['prob'][0, 16]:.4f} at kl 0.1"
    else:
        out = ctx.policy_worst_case_trajectory(kl_bounds=BOUNDS, thetas=THETAS)
        note = f"ess {out['bounds']['ess'][0]:.0f} at kl 0.1"
    dt = time.perf_counter() - t0
    print(f"{what}: K={K} n_ok={r['n_ok']} one call (first on the handle: buffers allocated inside) {dt * 1e3:.1f} ms; {note}")


def table(path, new):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    first = next(i for i, r in enumerate(rows) if "wc_var" in r["Kernel_Name"])
    first = max(j for j in range(first + 1) if "mc_pass1" in rows[j]["Kernel_Name"])     # (the call's chain starts with its own pass 1)
    tot, cnt = {}, {}
    for r in rows[first:]:
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        tot[name] = tot.get(name, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        cnt[name] = cnt.get(name, 0) + 1
    total = sum(tot.values())
    print("| kernel | calls | total, us | share |\n|---|---|---|---|")
    for name in sorted(tot, key=lambda k: -tot[k]):
        print(f"| `{name}` | {cnt[name]} | {tot[name] / 1e3:.0f} | {100.0 * tot[name] / total:.1f} % |")
    print(f"| all | {sum(cnt.values())} | {total / 1e3:.0f} | 100 % |")
    roll = sum(v for k, v in tot.items() if "rollout" in k)
    mine = sum(v for k, v in tot.items() if any(n in k for n in new))
    print(f"\n{', '.join(new)}: {mine / 1e3:.0f} us = {100.0 * mine / roll:.1f} % of the replay's rollouts ({roll / 1e3:.0f} us)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("run", "table"))
    ap.add_argument("--what", choices=("events", "trajectory"), default="events")
    ap.add_argument("--K", type=int, default=1 << 20)
    ap.add_argument("--csv")
    ap.add_argument("--new", nargs="+", default=["ev_eval", "ev_sums", "ev_final"])
    a = ap.parse_args()
    if a.mode == "run":
        run(a.what, a.K)
    else:
        table(a.csv, a.new)
