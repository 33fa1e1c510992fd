"""Rollouts per second of Monte-Carlo policy evaluation under user-written noise (rat_policy_evaluate_noise) on one MI355X, beside
rat_policy_evaluate (model noise) on the same problems; profiles/policy_noise.md records a run.

  measure    rat_policy_evaluate_noise at K = 10^4 and 10^6 with one theta on the pendulum source (n = 2, m = 1, N = 25) and the LQ family
             written as source (n = 12, m = 4, N = 30; tests/user_noise_model.py), each with a sampler that is the Gaussian chol(W) z
             and with a two-component mixture chosen by a uniform draw; rat_policy_evaluate on the same handle, policy and K; the first
             call's compile time against a cached one.  Three runs of every figure: median and spread (max - min).
  yardstick  rat_policy_evaluate alone on the same problems without a sampler.  RATILQR_TREE names the checkout whose package (and
             library) is loaded, so the parent commit is timed by the same code in the same job.
  md         profiles/policy_noise.md from the JSON lines of the runs above.

Every timed window ends in the call's own device wait (the entry points are synchronous) and lasts at least --min-seconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("RATILQR_TREE", ROOT))
import ratilqr.jl_amd as rat  # noqa: E402
import user_noise_model as um  # noqa: E402

KS = (10_000, 1_000_000)
THETA = 0.5
S_PEND = np.array([0.03, 0.05])


def problems(samplers):
    """(name, problem, policy, {sampler name: (source, normals, uniforms)}): with samplers=False the sources carry none (any build)."""
    N = 25
    x_nom, l, L = um.pend_policy(N)
    p = [0.1, S_PEND[0], S_PEND[1], 0.25, 0.2]
    src = um.PEND_DIAG if samplers else um.PEND_PLAIN
    pend = {"gauss": (um.PEND_DIAG, 2, 0), "mixture": (um.PEND_MIX, 2, 1)}
    out = [("pendulum", lambda s: rat.DeviceSourceProblem(s, 2, 1, N, np.diag(S_PEND ** 2), params=p), src, (x_nom, l, L), pend)]
    gp = um.lq_generative(Nh=30)
    rng = np.random.default_rng(1)
    xl = 0.5 * rng.standard_normal((31, 12))
    lq = {"gauss": (um.LQ_GAUSS, 12, 0), "mixture": (um.LQ_MIX, 12, 1)}
    out.append(("lq_source", lambda s: um.lq_source_problem(gp, s, mean=False), um.LQ_GAUSS if samplers else um.LQ_FCH,
                (xl, 0.2 * rng.standard_normal((30, 4)), 0.05 * rng.standard_normal((30, 4, 12))), lq))
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


def measure(a):
    out = dict(mode="measure")
    for name, make, _, (x, l, L), samplers in problems(True):
        for sname, (src, npn, npu) in samplers.items():
            tag = f"// {time.time_ns()} {os.getpid()}\n"                  # a source unique to this run: no cache serves it
            ctx = rat.Context(make(src + tag))
            noise = rat.UserNoise(npn, npu, seed=1)
            call = lambda K=64: ctx.policy_evaluate_noise(x, l, L, noise=noise, thetas=(THETA,), K=K)
            t0 = time.perf_counter(); r = call(); t1 = time.perf_counter(); call(); t2 = time.perf_counter()
            assert r["n_ok"] == 64
            out[f"{name}_{sname}_first_call_ms"], out[f"{name}_{sname}_cached_call_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
            for K in KS:
                out[f"{name}_{sname}_K{K}"] = three(lambda: call(K), K, a.min_seconds)
            if sname == "gauss":                                          # the model noise on the same handle: W is the sampler's covariance
                for K in KS:
                    out[f"{name}_model_K{K}"] = three(lambda: ctx.policy_evaluate(x, l, L, thetas=(THETA,), K=K, seed=1), K, a.min_seconds)
                g, w = call(KS[1]), ctx.policy_evaluate(x, l, L, thetas=(THETA,), K=KS[1], seed=1)
                out[f"{name}_gauss_vs_model_mean_in_se"] = abs(g["mean"] - w["mean"]) / np.hypot(g["se_mean"], w["se_mean"])
    print(json.dumps(out))


def yardstick(a):
    out = dict(mode="yardstick", so=a.label)
    for name, make, src, (x, l, L), _ in problems(False):
        ctx = rat.Context(make(src))
        for K in KS:
            out[f"{name}_model_K{K}"] = three(lambda: ctx.policy_evaluate(x, l, L, thetas=(THETA,), K=K, seed=1), K, a.min_seconds)
    print(json.dumps(out))


def md(a):
    runs = [json.loads(ln) for f in a.json for ln in open(f) if ln.startswith("{")]
    new = [r for r in runs if r["mode"] == "measure"][-1]
    olds = [r for r in runs if r["mode"] == "yardstick"]
    fmt = lambda d: f"{d['median'] / 1e6:.1f} M ± {d['spread'] / 2e6:.1f} M"
    T = ["# Monte-Carlo policy evaluation under user-written noise (`rat_policy_evaluate_noise`): rollouts/s, compile time, registers", "",
         "One MI355X, `tools/policy_noise_bench.py` (`measure`, `yardstick`, `md`).  One θ = 0.5, device generator, a fixed closed-loop policy.",
         "Every figure: median of three runs ± half their spread; a run is a window of at least 1 s of back-to-back synchronous calls after",
         "two warm-up calls.", "", "| problem, noise | K = 10⁴, rollouts/s | K = 10⁶, rollouts/s | against model noise (this commit), 10⁴ / 10⁶ |", "|---|---|---|---|"]
    names = dict(pendulum="pendulum source, n = 2, m = 1, N = 25", lq_source="LQ + cubic as source, n = 12, m = 4, N = 30")
    for k, title in names.items():
        m4, m6 = new[f"{k}_model_K10000"], new[f"{k}_model_K1000000"]
        T.append(f"| {title}: `rat_policy_evaluate`, model noise N(0, W) | {fmt(m4)} | {fmt(m6)} | 1 / 1 |")
        for o in olds:
            T.append(f"| ... the same, library of {o['so']} | {fmt(o[k + '_model_K10000'])} | {fmt(o[k + '_model_K1000000'])} | "
                     f"{o[k + '_model_K10000']['median'] / m4['median']:.2f} / {o[k + '_model_K1000000']['median'] / m6['median']:.2f} |")
        for s, st in (("gauss", "sampler = chol(W) z"), ("mixture", "two-component mixture, one uniform")):
            a4, a6 = new[f"{k}_{s}_K10000"], new[f"{k}_{s}_K1000000"]
            T.append(f"| ... `rat_policy_evaluate_noise`, {st} | {fmt(a4)} | {fmt(a6)} | {a4['median'] / m4['median']:.2f} / {a6['median'] / m6['median']:.2f} |")
    T += ["", "| first call (compiles `rat_src_user_noisy_rollout` for an unseen source), K = 64 | first | second (module loaded) |", "|---|---|---|"]
    for k, title in names.items():
        for s in ("gauss", "mixture"):
            T.append(f"| {title}, {s} | {new[f'{k}_{s}_first_call_ms']:.0f} ms | {new[f'{k}_{s}_cached_call_ms']:.2f} ms |")
    T += ["", "Gaussian sampler against model noise at K = 10⁶ (other streams, the same distribution), difference of the means in standard errors: " +
          ", ".join(f"{names[k].split(',')[0]} {new[k + '_gauss_vs_model_mean_in_se']:.2f}" for k in names) + "."]
    if a.notes:
        T += ["", open(a.notes).read().rstrip()]
    open(a.out, "w").write("\n".join(T) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("measure", "yardstick", "md"))
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--json", nargs="*", default=[])
    ap.add_argument("--label", default="this commit", help="yardstick: which build of the library is loaded")
    ap.add_argument("--notes", default=None, help="md: a text file appended as it is (kernel resources, reading)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_noise.md"))
    a = ap.parse_args()
    dict(measure=measure, yardstick=yardstick, md=md)[a.mode](a)
