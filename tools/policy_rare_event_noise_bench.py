"""Time of rare-event estimation for source models under user-written noise (rat_policy_rare_event_noise) on one MI355X, beside
rat_policy_rare_event on the same LQ problem as a family; profiles/policy_rare_event_noise.md records a run.

  measure    at K = 2^20, N = 50: one shifted pass (n_iter = 0 under a fixed shift) and a call with four iterations that all run, on the
             pendulum source (PEND_STATE, three normals a step) and on the 12 x 4 LQ_GAUSS source (twelve normals through chol(W));
             the family call (rat_policy_rare_event) on the same LQ problem, same policy, same event, in the same run -- the yardstick;
             the first call's compile time of rat_src_rare_rollout for an unseen source against a call with the module loaded.
             Three runs of every figure: median and spread (max - min).
  md         profiles/policy_rare_event_noise.md from the JSON line of the run above.

Every timed window ends in the call's own device wait (the entry points are synchronous) and lasts at least --min-seconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import ratilqr.jl_amd as rat  # noqa: E402
import user_noise_model as um  # noqa: E402

K, N = 1 << 20, 50


def seconds(fn, min_seconds):
    fn(); fn()                                                           # warm-up: code objects, the handle's scratch at this K
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds and n >= 3:
            return dt / n


def three(fn, min_seconds):
    r = sorted(seconds(fn, min_seconds) for _ in range(3))
    return dict(median=r[1] * 1e3, spread=(r[2] - r[0]) * 1e3)


def far_event(call, ev0):
    """ev0 moved far out, so that four iterations at rho = 0.1 run: the 1 - 1e-5 quantile of the plain margins plus two standard deviations"""
    M = call(ev0, n_iter=0, want_margins=True).margins
    M = M[np.isfinite(M)]
    return rat.Event(ev0.Q, ev0.a, ev0.b - (np.quantile(M, 1 - 1e-5) + 2.0 * M.std()), ev0.steps)


def measure(a):
    out = dict(mode="measure", K=K, N=N)
    tag = f"// {time.time_ns()} {os.getpid()}\n"                          # sources unique to this run: no cache serves them
    x_nom, l, L = um.pend_policy(N)
    gp = um.lq_generative(Nh=N)
    rng = np.random.default_rng(1)
    xl, ll, Ll = 0.5 * rng.standard_normal((N + 1, 12)), 0.2 * rng.standard_normal((N, 4)), 0.05 * rng.standard_normal((N, 4, 12))
    cases = [("pendulum", rat.DeviceSourceProblem(um.PEND_STATE + tag, 2, 1, N, 1e-3 * np.eye(2), params=um.PEND_STATE_P), 3, (x_nom, l, L),
              rat.halfspace(np.array([1.0, 0.0, 0.0]), 0.0, steps=(1, N))),
             ("lq_source", um.lq_source_problem(gp, um.LQ_GAUSS + tag, mean=False), 12, (xl, ll, Ll),
              rat.halfspace(np.random.default_rng(9).standard_normal(16), 0.0, steps=(N - 5, N)))]
    for name, prob, P, (x, lv, Lv), ev0 in cases:
        ctx = rat.Context(prob)
        noise = rat.UserNoise(P, 0, seed=1)
        call = lambda ev, Kc=K, **kw: ctx.policy_rare_event_noise(x, lv, Lv, ev, Kc, noise=noise, **kw)
        t0 = time.perf_counter(); call(ev0, 64, n_iter=0); t1 = time.perf_counter(); call(ev0, 64, n_iter=0); t2 = time.perf_counter()
        out[f"{name}_first_call_ms"], out[f"{name}_cached_call_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
        ev = far_event(call, ev0)
        r = call(ev, n_iter=4)
        out[f"{name}_iters_ran"], out[f"{name}_flag"] = r.n_iter, r.flag
        out[f"{name}_pass"] = three(lambda: call(ev, shift=r.shift, n_iter=0), a.min_seconds)
        out[f"{name}_call4"] = three(lambda: call(ev, n_iter=4), a.min_seconds)
    # the yardstick: the same LQ problem as a family (kappa and all), W = the sampler's covariance
    lq = gp.lq
    fam = rat.LQRiskSensitiveProblem(lq.A, lq.B, Q=lq.Q, R=lq.R, N=N, W=gp.nchol @ gp.nchol.T, Qf=lq.Qf, kappa=lq.kappa)
    ctx = rat.Context(fam)
    ev0 = cases[1][4]
    call = lambda ev, **kw: ctx.policy_rare_event(xl, ll, Ll, ev, K, seed=1, **kw)
    ev = far_event(call, ev0)
    r = call(ev, n_iter=4)
    out["family_iters_ran"] = r.n_iter
    out["family_pass"] = three(lambda: call(ev, shift=r.shift, n_iter=0), a.min_seconds)
    out["family_call4"] = three(lambda: call(ev, n_iter=4), a.min_seconds)
    print(json.dumps(out))


def md(a):
    runs = [json.loads(ln) for f in a.json for ln in open(f) if ln.startswith("{")]
    new = [r for r in runs if r["mode"] == "measure"][-1]
    fmt = lambda d: f"{d['median']:.2f} ms ± {d['spread'] / 2:.2f}"
    T = ["# Rare safety events under user-written noise (`rat_policy_rare_event_noise`): time, compile time, kernel resources", "",
         f"One MI355X, `tools/policy_rare_event_noise_bench.py` (`measure`, `md`).  K = 2^20, N = {new['N']}, a fixed closed-loop policy, a",
         "half-space event placed far out (the 1 − 1e-5 quantile of the plain margins plus two of their standard deviations), so that four",
         "iterations at ρ = 0.1 run (the table says how many did).  Every figure: median of three runs ± half",
         "their spread; a run is a window of at least 1 s of back-to-back synchronous calls after two warm-up calls.", "",
         "| problem | one shifted pass (`n_iter = 0`) | a call with four iterations | iterations that ran |", "|---|---|---|---|"]
    names = dict(pendulum="pendulum source `PEND_STATE`, n = 2, m = 1, three normals a step",
                 lq_source="12 × 4 `LQ_GAUSS` source, twelve normals a step", family="the same LQ problem as a family, `rat_policy_rare_event` (yardstick)")
    for k, title in names.items():
        T.append(f"| {title} | {fmt(new[k + '_pass'])} | {fmt(new[k + '_call4'])} | {new[k + '_iters_ran']} |")
    T += ["", f"LQ source against the family call in the same run: {new['lq_source_pass']['median'] / new['family_pass']['median']:.2f}× per pass, "
          f"{new['lq_source_call4']['median'] / new['family_call4']['median']:.2f}× per four-iteration call "
          "(the parent recorded 5.3 ms and 34 ms for the family in `profiles/policy_rare_event.md`, on another problem of the same size).", "",
          "| first call (compiles `rat_src_rare_rollout` for an unseen source), K = 64 | first | second (module loaded) |", "|---|---|---|"]
    for k in ("pendulum", "lq_source"):
        T.append(f"| {names[k]} | {new[k + '_first_call_ms']:.0f} ms | {new[k + '_cached_call_ms']:.2f} ms |")
    if a.notes:
        T += ["", open(a.notes).read().rstrip()]
    open(a.out, "w").write("\n".join(T) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("measure", "md"))
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--json", nargs="*", default=[])
    ap.add_argument("--notes", default=None, help="md: a text file appended as it is (kernel resources, reading)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_rare_event_noise.md"))
    a = ap.parse_args()
    dict(measure=measure, md=md)[a.mode](a)
