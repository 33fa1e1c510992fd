"""Time of safety events the user writes (rat_policy_events_user, rat_policy_rare_event_user) on one MI355X, beside the quadratic calls on
the same recorded evaluation and beside the host route; profiles/policy_events_user.md records a run.

  measure    the 12 x 4 LQ_GAUSS source (tests/user_noise_model.py) at K = 2^20, N = 50 under a fixed closed-loop policy, one
             rat_policy_evaluate_noise, then on that recorded evaluation, one kl_bound and theta = 0, no per-step sums:
               rat_policy_events_user with 1 and with 16 half-spaces x[i % n] - q[i] written as rat_user_event;
               rat_policy_events with the same 1 and 16 half-spaces as linear events (Q = NULL);
               the host route: the evaluation again with x_out / u_out, then the same margins and counts in NumPy (--host-runs times,
               once by default: it moves 6.8 GB);
             and rat_policy_rare_event_user beside rat_policy_rare_event_noise at one half-space placed far out: one shifted pass
             (n_iter = 0) and a call with four iterations.
             Three runs of every device figure: median and spread (max - min).
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
import user_event_model as ue  # noqa: E402
import user_noise_model as um  # noqa: E402

N = 50
BENCH16 = "    for (int i = 0; i < 16; ++i) g[i] = x[i % RAT_N] - q[i];\n"


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


def measure(a):
    K = 1 << a.log2_k
    out = dict(mode="measure", K=K, N=N)
    gp = um.lq_generative(Nh=N)
    base = um.lq_source_problem(gp, source=um.LQ_GAUSS, mean=False)
    off = base.params.size
    rng = np.random.default_rng(1)
    x, l, L = 0.5 * rng.standard_normal((N + 1, 12)), 0.2 * rng.standard_normal((N, 4)), 0.05 * rng.standard_normal((N, 4, 12))
    src = ue.source(um.LQ_GAUSS, "half", off, body=BENCH16)
    prob = rat.DeviceSourceProblem(src, 12, 4, N, base.Wtab, params=np.concatenate([base.params, np.zeros(16)]))
    ctx = rat.Context(prob)
    noise = rat.UserNoise(12, 0, seed=1)
    # thresholds from a small evaluation: about one rollout in ten crosses each
    small = ctx.policy_evaluate_noise(x, l, L, noise=noise, K=4096, want_trajectories=True)
    q = np.array([np.quantile(small["x"][:, :, i % 12].max(axis=1), 0.9) for i in range(16)])
    ctx.set_params(np.concatenate([base.params, q]))
    out["evaluate"] = three(lambda: ctx.policy_evaluate_noise(x, l, L, noise=noise, K=K), a.min_seconds)
    kw = dict(kl_bounds=(0.1,), thetas=(0.0,))
    for E in (1, 16):
        evs = [rat.halfspace(np.eye(12)[i % 12], -q[i]) for i in range(E)]
        u_ = ctx.policy_events_user(E, **kw)
        q_ = ctx.policy_events(evs, **kw)
        out[f"same_counts_{E}"] = bool(np.array_equal(u_["thetas"]["n_viol"], q_["thetas"]["n_viol"]))
        out[f"user_{E}"] = three(lambda: ctx.policy_events_user(E, **kw), a.min_seconds)
        out[f"quadratic_{E}"] = three(lambda: ctx.policy_events(evs, **kw), a.min_seconds)
    # the host route: trajectories out, NumPy
    def host(E):
        r = ctx.policy_evaluate_noise(x, l, L, noise=noise, K=K, want_costs=True, want_trajectories=True)
        ok = ~np.isnan(r["costs"])
        return [int(((r["x"][:, :, i % 12].max(axis=1) - q[i] > 0) & ok).sum()) for i in range(E)]
    for E in (1, 16):
        ts = []
        for _ in range(a.host_runs):
            t0 = time.perf_counter(); host(E); ts.append((time.perf_counter() - t0) * 1e3)
        out[f"host_{E}_ms"] = ts
    # the rare-event calls at one half-space far out: the 1 - 1e-5 quantile of the plain margins plus two standard deviations
    ctx.set_params(np.concatenate([base.params, np.zeros(16)]))
    M = ctx.policy_rare_event_user(x, l, L, 1, 0, K, noise=noise, n_iter=0, want_margins=True).margins
    M = M[np.isfinite(M)]
    far = float(np.quantile(M, 1 - 1e-5) + 2.0 * M.std())
    ctx.set_params(np.concatenate([base.params, [far], np.zeros(15)]))
    ev = rat.halfspace(np.eye(12)[0], -far)
    user = lambda **k: ctx.policy_rare_event_user(x, l, L, 1, 0, K, noise=noise, **k)
    quad = lambda **k: ctx.policy_rare_event_noise(x, l, L, ev, K, noise=noise, **k)
    for name, call in (("rare_user", user), ("rare_quadratic", quad)):
        r = call(n_iter=4)
        out[f"{name}_iters_ran"], out[f"{name}_prob"] = r.n_iter, r.prob
        out[f"{name}_pass"] = three(lambda: call(shift=r.shift, n_iter=0), a.min_seconds)
        out[f"{name}_call4"] = three(lambda: call(n_iter=4), a.min_seconds)
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("measure",))
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--log2-k", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=1)
    a = ap.parse_args()
    dict(measure=measure)[a.mode](a)
