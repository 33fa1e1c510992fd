"""Time per call of the tail calls (rat_policy_tail_trajectory / _disturbance / _params) on one MI355X: each beside its worst-case sibling
at the same row count (the dense schedule on exp-tilt weights), beside itself with the switch tail_dense on (the dense kernels on the
SAME tail weights: what the liveness schedule replaces), and against the host route (x_out / u_out plus policy_tail_risk's weights_out
per level, NumPy moments).  profiles/policy_tail_scenarios.md records a run.

  measure  the LQ + cubic source 12 x 4 with fourteen parameters (tests/user_params_model, its "scale" hook), N = 50, K = 2^16 and 2^20
           (--ks), 1 row (alpha = 0.9 / theta = 0.5) and 16 rows (alpha = 0, 0.06 ... 0.9 / sixteen thetas), ALTERNATING run by run in
           one process, median of --repeat (5); then the evaluation itself and, up to --host-max-k, the host route.  One JSON line per
           (K, rows).
  md       the tables from measure's lines (--json) and the kernels' registers and scratch from the build remarks
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
import user_params_model as pm  # noqa: E402

N, SEED = 50, 7
ROWS = {1: ((0.9,), (0.5,)), 16: (tuple(0.06 * i for i in range(16)), tuple(0.05 * i for i in range(16)))}


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
    c = pm.case("lq12")
    p = c.p.copy()
    p[13] = 50.0
    ctx = rat.Context(c.problem("scale", p=p, N=N))
    ctx.set_param_sampling(rat.ParamSampling(pm.PARAM_NORMALS, pm.PARAM_UNIFORMS))
    r0 = np.random.default_rng(3)
    x_nom, l, L = 0.5 * r0.standard_normal((N + 1, c.n)), 0.8 * r0.standard_normal((N, c.m)), 0.1 * r0.standard_normal((N, c.m, c.n))

    def evaluate(K, **kw):
        return ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=SEED), K=K, **kw)

    def dense(fn, al):
        ctx.debug_set("tail_dense", 1)
        try:
            fn(al)
        finally:
            ctx.debug_set("tail_dense", 0)

    def host(K, al):
        r = evaluate(K, want_costs=True, want_trajectories=True)
        z = np.concatenate([r["x"][:, :-1], r["u"]], axis=2)
        for a in al:
            w = ctx.policy_tail_risk((a,), want_weights=True)["weights"]
            keep = w > 0
            zk, wk = z[keep], w[keep]
            mean = np.einsum("k,kti->ti", wk, zk)
            d = zk - mean
            np.einsum("k,kti,ktj->tij", wk, d, d)

    for K in args.ks:
        for R, (al, th) in ROWS.items():
            evaluate(K)
            row = dict(case="lqc_12x4_N50_P14", K=K, rows=R)
            row.update(alternating(dict(
                tail_trajectory=lambda: ctx.policy_tail_trajectory(al), tail_trajectory_dense=lambda: dense(ctx.policy_tail_trajectory, al),
                wc_trajectory=lambda: ctx.policy_worst_case_trajectory(thetas=th),
                tail_disturbance=lambda: ctx.policy_tail_disturbance(al), tail_disturbance_dense=lambda: dense(ctx.policy_tail_disturbance, al),
                wc_disturbance=lambda: ctx.policy_worst_case_disturbance(thetas=th),
                tail_params=lambda: ctx.policy_tail_params(al), tail_params_dense=lambda: dense(ctx.policy_tail_params, al),
                wc_params=lambda: ctx.policy_worst_case_params(thetas=th), tail_risk=lambda: ctx.policy_tail_risk(al)), args.repeat))
            row.update(alternating(dict(evaluation=lambda: evaluate(K)), args.repeat))
            if K <= args.host_max_k and R == 1:
                row.update(alternating(dict(host_route=lambda: host(K, al)), max(1, args.repeat // 2)))
            print(json.dumps(row), flush=True)


def resources():
    path = os.path.join(ROOT, "ratilqr.jl_amd", "csrc", "policy_mc.remarks")
    if not os.path.exists(path):
        return {}
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: \S*?\d+((?:wc[tdp]|tl[tdp])_(?:moments|weights|levels))((?:ILb[01]E?)*(?:Lb[01]E)*)", line)
        if m:
            cur = out.setdefault(m.group(1) + ("<" + ", ".join(re.findall(r"Lb([01])", m.group(2))) + ">" if m.group(2) else ""), {})
        elif "Function Name:" in line:
            cur = None
        for key, tag in (("VGPRs:", "vgprs"), ("AGPRs:", "agprs"), ("TotalSGPRs:", "sgprs"), ("ScratchSize [bytes/lane]:", "scratch"),
                         ("LDS Size [bytes/block]:", "lds"), ("Occupancy [waves/SIMD]:", "waves")):
            if cur is not None and key in line and "Spill" not in line:
                cur[tag] = line.split(key)[1].split("[")[0].strip()
    return out


def md(args):
    rows = [json.loads(ln) for ln in open(args.json) if ln.startswith("{")] if args.json and os.path.exists(args.json) else []
    out = ["## Time per call, ms: median (± spread) of alternating runs", ""]
    if not rows:
        out += ["**Not yet measured.**"]
    else:
        ms = lambda t: f"{1e3 * t['median']:.2f} (± {1e3 * t['spread']:.2f})" if t else "not run"
        out += ["| K | rows | call | liveness schedule | dense kernels, tail weights | worst-case sibling | tail-risk chain alone | evaluation | host route |",
                "|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            for name in ("trajectory", "disturbance", "params"):
                out.append(f"| {r['K']} | {r['rows']} | {name} | {ms(r['tail_' + name])} | {ms(r['tail_' + name + '_dense'])} | {ms(r['wc_' + name])} | "
                           f"{ms(r['tail_risk'])} | {ms(r['evaluation'])} | {ms(r.get('host_route')) if name == 'trajectory' else ''} |")
    res = resources()
    if res:
        out += ["", "## Build remarks (gfx950)", "", "| kernel | VGPRs | AGPRs | SGPRs | scratch, B per lane | LDS, B | waves per SIMD |", "|---|---|---|---|---|---|---|"]
        out += [f"| `{k}` | {v.get('vgprs')} | {v.get('agprs')} | {v.get('sgprs')} | {v.get('scratch')} | {v.get('lds')} | {v.get('waves')} |" for k, v in sorted(res.items())]
    print("\n".join(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("measure", "md"))
    ap.add_argument("--ks", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--host-max-k", type=int, default=1 << 16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--json", default=None, help="md: the file holding measure's output lines")
    a = ap.parse_args()
    measure(a) if a.mode == "measure" else md(a)
