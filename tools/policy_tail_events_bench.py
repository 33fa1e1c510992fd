"""Time per call of rat_policy_tail_events on one MI355X, beside what it is measured against.  profiles/policy_tail_events.md records a run.

  measure  the 12 x 4 LQ problem of bench.py's family at N = 50, K = 2^20 (--k), four quadratic events with step_out, on ONE evaluation:
             tail_events        the call at alpha = 0, 0.9, 0.99, 0.999 (tle_sums: the liveness schedule)
             tail_events_dense  the same call with the switch tail_dense on (ev_sums on the same tail weights)
             events             rat_policy_events with four theta rows (ev_sums on exp-tilt weights: the same kernel at this commit and
                                at its parent -- the yardstick)
             tail_risk          the tail chain alone (rat_policy_tail_risk on the stored costs)
             host_route         what the call replaces: margin_out and weights_out to the host and the join in NumPy, alpha[0] only
           ALTERNATING run by run in one process after a warm-up round, median and spread (max - min) of --repeat (7).  One JSON line.
           Under `rocprofv3 --kernel-trace --stats` the same run gives the split of a call into ev_eval / tle_sums / the tail chain.
  md       the table from measure's line (--json)

Every timed window ends in the call's own device wait (the entry points are synchronous)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ratilqr.jl_amd as rat  # noqa: E402

N, SEED = 50, 7
ALPHAS = (0.0, 0.9, 0.99, 0.999)
THETAS = (0.0, 0.01, 0.02, 0.04)


def stats(ts):
    ts = sorted(ts)
    return dict(median=ts[len(ts) // 2], spread=ts[-1] - ts[0], runs=len(ts))


def alternating(fns, repeat):
    """every function once to warm up, then `repeat` rounds of all of them in turn: {name: median, spread, runs}"""
    for fn in fns.values():
        fn()
    ts = {k: [] for k in fns}
    for _ in range(repeat):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    return {k: stats(v) for k, v in ts.items()}


def measure(args):
    prob, x0, l = rat.synthetic_lq_problem(n=12, m=4, N=N, seed=3, w=1e-2)
    ctx = rat.Context(prob)
    L = 0.05 * np.random.default_rng(1).standard_normal((N, 4, 12))
    x_det = ctx.rollout_open(x0, l)
    K = args.k
    r = ctx.policy_evaluate(x_det, l, L, K=K, seed=SEED)
    # an obstacle, a lane edge, an actuator limit and an ellipsoid at the end of the horizon, sized from the nominal trajectory so that a
    # few per cent of the rollouts violate each
    sd = float(np.sqrt(r["var"])) if r["var"] > 0 else 1.0
    evs = [rat.ball([0, 1], x_det[N // 2, :2] + 0.3, 0.25, steps=(N // 4, 3 * N // 4)),
           rat.halfspace(np.eye(12)[2], -(np.abs(x_det[:, 2]).max() + 0.3)),
           rat.halfspace(np.eye(16)[12], -(np.abs(l[:, 0]).max() + 0.2)),
           rat.quadratic_event(np.eye(12), -2.0 * x_det[N], float(x_det[N] @ x_det[N]) - 0.5, steps=N)]

    def dense():
        ctx.debug_set("tail_dense", 1)
        try:
            ctx.policy_tail_events(evs, ALPHAS, want_steps=True)
        finally:
            ctx.debug_set("tail_dense", 0)

    def host():
        M = ctx.policy_events(evs, thetas=(0.0,), want_margins=True)["margins"]
        w = ctx.policy_tail_risk(ALPHAS[:1], want_weights=True)["weights"]
        with np.errstate(invalid="ignore"):
            A = M > 0
        return A @ w, np.where(np.isnan(M), 0.0, M) @ w

    row = dict(case="lq_12x4_N50", K=K, n_event=len(evs), alphas=ALPHAS, thetas=[t / sd for t in THETAS])
    th = tuple(t / sd for t in THETAS)
    row.update(alternating(dict(tail_events=lambda: ctx.policy_tail_events(evs, ALPHAS, want_steps=True), tail_events_dense=dense,
                                events=lambda: ctx.policy_events(evs, thetas=th, want_steps=True),
                                tail_risk=lambda: ctx.policy_tail_risk(ALPHAS), host_route=host), args.repeat))
    out = ctx.policy_tail_events(evs, ALPHAS)["levels"]
    row["prob"] = out["prob"].tolist()
    print(json.dumps(row), flush=True)


def md(args):
    rows = [json.loads(ln) for ln in open(args.json) if ln.startswith("{")] if args.json and os.path.exists(args.json) else []
    out = ["## Time per call, ms: median (± spread) of alternating runs", ""]
    if not rows:
        out += ["**Not timed yet.**"]
    else:
        ms = lambda t: f"{1e3 * t['median']:.2f} (± {1e3 * t['spread']:.2f})"
        out += ["| K | (a) tail_events, liveness schedule | (a') tail_events, dense sums on tail weights | (b) events, four theta rows | tail-risk chain alone | (c) host route, alpha[0] |",
                "|---|---|---|---|---|---|"]
        for r in rows:
            out.append(f"| {r['K']} | {ms(r['tail_events'])} | {ms(r['tail_events_dense'])} | {ms(r['events'])} | {ms(r['tail_risk'])} | {ms(r['host_route'])} |")
    print("\n".join(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("measure", "md"))
    ap.add_argument("--k", type=int, default=1 << 20)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--json", default=None, help="md: the file holding measure's output line")
    a = ap.parse_args()
    measure(a) if a.mode == "measure" else md(a)
