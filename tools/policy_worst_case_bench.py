"""Time per call of the worst-case cost within the KL ball (rat_policy_worst_case) on one MI355X; profiles/policy_worst_case.md records a run.

  measure  the device call on the K costs an evaluation left on the device (cost = NULL), K = 10^4 and 10^6, 1 and 16 bounds, with and
           without the weights; beside it rat_policy_evaluate's own reduction of the same costs (the evaluation of a zero-step problem is
           not available, so: the call with 16 thetas against the call with none, and the kernel times of `once`), and the host route the
           call replaces: policy_evaluate(want_costs=True) plus the NumPy model of tests/worst_case_model.py on the copied costs -- and,
           beside that, plain NumPy (np.sum, no fixed order) running the same 12 x 16 search.  Three runs of every figure: median and
           spread (max - min).
  once     a few calls at K = 10^6 and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own.
  md       profiles/policy_worst_case.md from the JSON lines of the runs above.

Every timed window ends in the call's own device wait (the entry points are synchronous) and lasts at least --min-seconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ratilqr.jl_amd as rat  # noqa: E402
import worst_case_model as wm  # noqa: E402

KS = (10_000, 1_000_000)
D1 = (0.1,)
D16 = tuple(np.logspace(-3, 0.3, 16))


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


def numpy_plain(J, ds):
    """The device's schedule in plain NumPy: what a user who copies the costs out can do fastest (no fixed order, no centring)."""
    J = J[~np.isnan(J)]
    n, mx, sd = J.size, J.max(), J.std()
    dx = J - mx
    out = []
    for d in ds:
        t0 = np.sqrt(2 * d) / sd
        lo = hi = 0.0
        for p in range(wm.PASSES):
            g = wm._grid(p, lo, hi, t0)
            y = np.exp(g[:, None] * dx[None, :])
            sy = y.sum(1)
            kl = g * ((y * dx).sum(1) / sy) - np.log(sy / n)
            j = int(np.argmax(kl >= d)) if (kl >= d).any() else -1
            if j >= 0:
                lo, hi = (g[j - 1] if j > 0 else lo), g[j]
            else:
                lo = g[-1]
        th = 0.5 * (lo + hi)
        y = np.exp(th * dx)
        out.append(mx + (y * dx).sum() / y.sum())
    return out


def setup():
    prob, x0, u = rat.synthetic_lq_problem()
    ctx = rat.Context(prob)
    sol = ctx.solve(x0, u, 1.0)
    assert sol["status"] == 0
    return ctx, sol


def measure(a):
    ctx, sol = setup()
    out = dict(mode="measure")
    for K in KS:
        ev = lambda **kw: ctx.policy_evaluate(sol["x"], sol["l"], sol["L"], K=K, seed=1, **kw)
        costs = ev(want_costs=True)["costs"]
        for name, ds in (("1", D1), ("16", D16)):
            out[f"device_K{K}_b{name}"] = three(lambda: ctx.policy_worst_case(kl_bounds=ds), a.min_seconds)
        out[f"device_K{K}_b1_weights"] = three(lambda: ctx.policy_worst_case(kl_bounds=D1, want_weights=True), a.min_seconds)
        out[f"device_K{K}_t16"] = three(lambda: ctx.policy_worst_case(thetas=D16), a.min_seconds)
        out[f"device_hostcosts_K{K}_b1"] = three(lambda: ctx.policy_worst_case(kl_bounds=D1, costs=costs), a.min_seconds)
        ev()
        out[f"evaluate_K{K}"] = three(lambda: ev(), a.min_seconds)
        out[f"evaluate_16thetas_K{K}"] = three(lambda: ev(thetas=D16), a.min_seconds)
        out[f"evaluate_want_costs_K{K}"] = three(lambda: ev(want_costs=True), a.min_seconds)
        out[f"model_K{K}_b1"] = three(lambda: wm.worst_case(costs, kl_bounds=D1), 0.0, warm=1, least=1)
        out[f"numpy_plain_K{K}_b1"] = three(lambda: numpy_plain(costs, D1), 0.0, warm=1, least=1)
        ev()
        dchk = D16 if K <= 10_000 else (D16[4], D1[0])
        dev, mdl = ctx.policy_worst_case(kl_bounds=dchk)["bounds"], wm.worst_case(costs, kl_bounds=dchk)["bounds"]
        out[f"max_rel_diff_vs_model_K{K}"] = float(max(np.abs(dev[k] / mdl[k] - 1).max() for k in ("theta", "kl", "bound", "tilt_mean", "ess")))
        one = ctx.policy_worst_case(kl_bounds=D1)["bounds"]
        out[f"bound_K{K}"] = [float(one["bound"][0]), float(one["bound_se"][0]), float(one["ess"][0])]
    print(json.dumps(out))


def once(a):
    ctx, sol = setup()
    ctx.policy_evaluate(sol["x"], sol["l"], sol["L"], thetas=(0.5,), K=KS[1], seed=1)
    for _ in range(3):
        ctx.policy_worst_case(kl_bounds=D1, want_weights=True)
    for _ in range(3):
        ctx.policy_worst_case(kl_bounds=D16)


def md(a):
    runs = [json.loads(l) for f in a.json for l in open(f) if l.startswith("{")]
    r = [x for x in runs if x["mode"] == "measure"][-1]
    us = lambda d: f"{d['median'] * 1e6:.0f} µs ± {d['spread'] * 5e5:.0f}"
    ms = lambda d: f"{d['median'] * 1e3:.1f} ms ± {d['spread'] * 5e2:.1f}"
    L = ["# Worst-case cost within the KL ball (`rat_policy_worst_case`): time per call", "",
         "One MI355X, `tools/policy_worst_case_bench.py` (`measure`, `once` under `rocprofv3 --kernel-trace --stats`, `md`).  The headline LQ",
         "problem (n = 12, m = 4, N = 50), the policy `solve` returned, the costs of `rat_policy_evaluate` with the device generator.  Every",
         "figure: median of three runs ± half their spread; a run is a window of at least 1 s of back-to-back synchronous calls after two",
         "warm-up calls (the two NumPy routes: one call after one warm-up call per run).", "",
         "| call | K = 10⁴ | K = 10⁶ |", "|---|---|---|"]
    row = lambda title, key, f: L.append(f"| {title} | {f(r[key.format(K=KS[0])])} | {f(r[key.format(K=KS[1])])} |")
    row("`rat_policy_worst_case`, cost = NULL, 1 bound", "device_K{K}_b1", us)
    row("... with the weights copied out", "device_K{K}_b1_weights", us)
    row("... 16 bounds", "device_K{K}_b16", us)
    row("... 16 thetas, no bound (no search)", "device_K{K}_t16", us)
    row("... 1 bound, K host costs uploaded", "device_hostcosts_K{K}_b1", us)
    row("`rat_policy_evaluate` (rollouts and reduction), no theta", "evaluate_K{K}", us)
    row("... 16 thetas", "evaluate_16thetas_K{K}", us)
    row("... with the K costs copied out (`want_costs`)", "evaluate_want_costs_K{K}", us)
    row("host: NumPy model (`tests/worst_case_model.py`) on the copied costs, 1 bound", "model_K{K}_b1", ms)
    row("host: the same search in plain NumPy (no fixed order), 1 bound", "numpy_plain_K{K}_b1", ms)
    for K in KS:
        dev = r[f"evaluate_K{K}"]["median"] + r[f"device_K{K}_b1"]["median"]
        host = r[f"evaluate_want_costs_K{K}"]["median"] + r[f"model_K{K}_b1"]["median"]
        fast = r[f"evaluate_want_costs_K{K}"]["median"] + r[f"numpy_plain_K{K}_b1"]["median"]
        L += ["", f"K = {K}, one bound: evaluation + device call {dev * 1e3:.2f} ms; the host route (evaluation with the costs copied out + the NumPy "
                  f"model) {host * 1e3:.1f} ms, {host / dev:.0f}x; with plain NumPy in place of the model {fast * 1e3:.1f} ms, {fast / dev:.0f}x.  "
                  f"Device against model (theta, KL, bound, tilted mean, ESS): largest relative difference "
                  f"{r[f'max_rel_diff_vs_model_K{K}']:.1e}.  bound(0.1) = {r[f'bound_K{K}'][0]:.4f} ± {r[f'bound_K{K}'][1]:.4f}, ESS {r[f'bound_K{K}'][2]:.0f}."]
    if a.notes:
        L += ["", open(a.notes).read().rstrip()]
    open(a.out, "w").write("\n".join(L) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("measure", "once", "md"))
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--json", nargs="*", default=[])
    ap.add_argument("--notes", default=None, help="md: a text file appended as it is (kernel statistics, register counts, reading)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_worst_case.md"))
    a = ap.parse_args()
    dict(measure=measure, once=once, md=md)[a.mode](a)
