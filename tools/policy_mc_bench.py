"""Rollouts per second of Monte-Carlo policy evaluation (rat_policy_evaluate) on one MI355X; profiles/policy_mc.md records a run.

  measure    the new call at K = 10^4 and 10^6 with one theta, on the headline LQ problem (n = 12, m = 4, N = 50), the pendulum source and
             the LQ-as-source problem of tools/source_model_bench.py; compile time of an unseen source and a cache hit, and of the
             Monte-Carlo kernel that the first evaluation of a source problem compiles.  Three runs of
             every figure: median and spread (max - min).
  yardstick  the path a user had before for the family: ctx.rollout_noisy(..., want_x=False, want_u=False) and the same statistics in
             NumPy.  Runs on any build of the library (RATILQR_SO names another one), so the parent commit is timed by the same code.
  once       one call per problem at K = 10^6 and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own.
  md         profiles/policy_mc.md from the JSON lines of the runs above.

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
from test_gpu_source_model import PENDULUM, lq_pair, source_pendulum  # noqa: E402

KS = (10_000, 1_000_000)
THETA = 0.5


def numpy_stats(c, theta):
    c = c[~np.isnan(c)]
    mx = c.max()
    y = np.exp(theta * (c - mx))
    return dict(mean=c.mean(), var=c.var(ddof=1), min=c.min(), max=mx, risk=mx + np.log(y.mean()) / theta,
                risk_se=y.std(ddof=1) / (y.mean() * theta * np.sqrt(c.size)))


def problems(with_source=True):
    prob, x0, u = rat.synthetic_lq_problem()
    out = [("lq_family", prob, x0, u, 1.0)]
    if with_source:
        out.append(("pendulum_source", source_pendulum(), np.array([1.0, 0.0]), np.zeros((25, 1)), 0.5))
        fam, src, lx0, lu = lq_pair()
        out.append(("lq_source", src, lx0, lu, 1.5))
        out.append(("lq_source_family", fam, lx0, lu, 1.5))              # the same problem as a family, beside its source form
    return out


def rate(fn, K, min_seconds):
    fn(); fn()                                                           # warm-up: code objects, the handle's scratch at this K
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds and n >= 3:
            return K * n / dt


def three(fn, K, min_seconds):
    r = sorted(rate(fn, K, min_seconds) for _ in range(3))
    return dict(median=r[1], spread=r[2] - r[0])


def compile_times():
    out = {}
    tag = f"// {time.time_ns()} {os.getpid()}\n"                          # sources unique to this run: no cache serves them
    for key, src in (("compile_first_ms", PENDULUM + tag), ("compile_second_ms", PENDULUM + tag + "//\n"),
                     ("compile_third_ms", PENDULUM + tag + "// //\n"), ("compile_cached_ms", PENDULUM + tag)):
        t = time.perf_counter(); rat.native.source_check(src, 2, 1); out[key] = (time.perf_counter() - t) * 1e3
    return out


def lazy_compile_time():
    """The Monte-Carlo kernel of a source problem is compiled by the first rat_policy_evaluate: that call against the second one."""
    from test_gpu_source_model import N_P, W_P
    ts = []
    for i in range(3):
        prob = rat.DeviceSourceProblem(PENDULUM + f"// {time.time_ns()} {os.getpid()} {i}\n", 2, 1, N_P, W_P, params=[0.1])
        ctx = rat.Context(prob)
        call = lambda: ctx.policy_evaluate(np.array([1.0, 0.0]), np.zeros((N_P, 1)), K=64, seed=1)
        t0 = time.perf_counter(); call(); t1 = time.perf_counter(); call(); t2 = time.perf_counter()
        ts.append(((t1 - t0) - (t2 - t1)) * 1e3)
    return sorted(ts)


def measure(a):
    out = dict(mode="measure", **compile_times())
    out["noisy_kernel_compile_ms"] = lazy_compile_time()
    for name, prob, x0, u, th in problems():
        ctx = rat.Context(prob)
        sol = ctx.solve(x0, u, th)
        assert sol["status"] == 0, name
        for K in KS:
            out[f"{name}_K{K}"] = three(lambda: ctx.policy_evaluate(sol["x"], sol["l"], sol["L"], thetas=(THETA,), K=K, seed=1), K, a.min_seconds)
            if name.endswith("source"):
                for tpw in (16, 32):
                    ctx.debug_set("src_mc_tpw", tpw)
                    out[f"{name}_K{K}_tpw{tpw}"] = three(lambda: ctx.policy_evaluate(sol["x"], sol["l"], sol["L"], thetas=(THETA,), K=K, seed=1),
                                                         K, a.min_seconds)
                ctx.debug_set("src_mc_tpw", 64)
        if name == "lq_family":                                          # results must not change: the new call against the old path's NumPy
            r = ctx.policy_evaluate(sol["x"], sol["l"], sol["L"], thetas=(THETA,), K=KS[1], seed=1)
            ref = numpy_stats(ctx.rollout_noisy(sol["x"], sol["l"], sol["L"], K=KS[1], seed=1, want_x=False, want_u=False)[2], THETA)
            out["max_rel_diff_vs_numpy_K1000000"] = max(abs(r["mean"] - ref["mean"]) / abs(ref["mean"]), abs(r["var"] - ref["var"]) / ref["var"],
                                                        abs(r["risk"][0] - ref["risk"]) / abs(ref["risk"]),
                                                        abs(r["risk_se"][0] - ref["risk_se"]) / ref["risk_se"])
    print(json.dumps(out))


def yardstick(a):
    out = dict(mode="yardstick", so=a.label, **compile_times())
    for name, prob, x0, u, th in problems(with_source=False):
        ctx = rat.Context(prob)
        sol = ctx.solve(x0, u, th)

        def old():
            c = ctx.rollout_noisy(sol["x"], sol["l"], sol["L"], K=K, seed=1, want_x=False, want_u=False)[2]
            return numpy_stats(c, THETA)
        for K in KS:
            out[f"{name}_K{K}"] = three(old, K, a.min_seconds)
    print(json.dumps(out))


def once(a):
    for name, prob, x0, u, th in problems():
        ctx = rat.Context(prob)
        sol = ctx.solve(x0, u, th)
        for _ in range(3):
            ctx.policy_evaluate(sol["x"], sol["l"], sol["L"], thetas=(THETA,), K=KS[1], seed=1)


def md(a):
    runs = [json.loads(l) for f in a.json for l in open(f) if l.startswith("{")]
    new = [r for r in runs if r["mode"] == "measure"][-1]
    olds = [r for r in runs if r["mode"] == "yardstick"]
    fmt = lambda d: f"{d['median'] / 1e6:.2f} M ± {d['spread'] / 2e6:.2f} M"
    L = ["# Monte-Carlo policy evaluation (`rat_policy_evaluate`): rollouts/s, compile time, the reduction's share", "",
         "One MI355X, `tools/policy_mc_bench.py` (`measure`, `yardstick`, `once` under `rocprofv3 --kernel-trace --stats`, `md`).  One θ = 0.5,",
         "device generator, the policy `solve` returned.  Every figure: median of three runs ± half their spread; a run is a window of at",
         "least 1 s of back-to-back synchronous calls after two warm-up calls.", "",
         "| problem | K = 10⁴, rollouts/s | K = 10⁶, rollouts/s |", "|---|---|---|"]
    names = dict(lq_family="LQ family, n = 12, m = 4, N = 50 (headline)", pendulum_source="pendulum source, n = 2, m = 1, N = 25",
                 lq_source="LQ + cubic as source, n = 4, m = 2, N = 12", lq_source_family="the same problem as a family")
    for k, title in names.items():
        L.append(f"| {title}: `rat_policy_evaluate` | {fmt(new[k + '_K10000'])} | {fmt(new[k + '_K1000000'])} |")
        for tpw in (32, 16):
            if f"{k}_K10000_tpw{tpw}" in new:
                L.append(f"| ... `src_mc_tpw` = {tpw} | {fmt(new[f'{k}_K10000_tpw{tpw}'])} | {fmt(new[f'{k}_K1000000_tpw{tpw}'])} |")
    for o in olds:
        L.append(f"| LQ family (headline): `rollout_noisy` + NumPy statistics, library of {o['so']} | {fmt(o['lq_family_K10000'])} | {fmt(o['lq_family_K1000000'])} |")
    L += ["", f"New call against the old path's NumPy statistics at K = 10⁶ (mean, variance, risk, risk_se): largest relative difference "
              f"{new['max_rel_diff_vs_numpy_K1000000']:.1e}.", "",
          "| compile (`rat_source_check`, pendulum) | first of the process | second | third | cache hit |", "|---|---|---|---|---|",
          f"| this commit (the two model kernels, as before) | {new['compile_first_ms']:.0f} ms | {new['compile_second_ms']:.0f} ms | {new['compile_third_ms']:.0f} ms | {new['compile_cached_ms']:.3f} ms |"]
    for o in olds:
        L.append(f"| library of {o['so']} | {o['compile_first_ms']:.0f} ms | {o['compile_second_ms']:.0f} ms | {o['compile_third_ms']:.0f} ms | {o['compile_cached_ms']:.3f} ms |")
    nk = new.get("noisy_kernel_compile_ms")
    if nk:
        L += ["", f"The Monte-Carlo kernel of a source problem (`rat_src_noisy_rollout`, a module of its own) is compiled by the first "
                  f"`rat_policy_evaluate` on the problem: {nk[1]:.0f} ms (median of three unseen sources; {nk[0]:.0f} – {nk[2]:.0f} ms), "
                  "the first call against the second."]
    if a.notes:
        L += ["", open(a.notes).read().rstrip()]
    open(a.out, "w").write("\n".join(L) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("measure", "yardstick", "once", "md"))
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--json", nargs="*", default=[])
    ap.add_argument("--label", default="this commit", help="yardstick: which build of the library is loaded")
    ap.add_argument("--notes", default=None, help="md: a text file appended as it is (kernel statistics, reading)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_mc.md"))
    a = ap.parse_args()
    dict(measure=measure, yardstick=yardstick, once=once, md=md)[a.mode](a)
