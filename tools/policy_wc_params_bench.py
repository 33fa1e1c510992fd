"""Time per call of the worst-case parameter moments (rat_policy_worst_case_params) on one MI355X beside rat_policy_worst_case_trajectory on
the same evaluation -- the same replay; the difference is what the parameter part costs -- and against the only route there was before
it: sample_params to the host, rat_policy_worst_case with weights_out per row, weighted NumPy moments.  profiles/policy_wc_params.md
records a run.

  measure  the LQ + cubic source 12 x 4 with fourteen parameters (tests/user_params_model.LQC, its "scale" hook), N = 50, K = 2^16 and
           2^20 (--ks), one bound and the theta = 0 row: the new call with and without the cost sums and the trajectory call, ALTERNATING
           run by run in one process, then the evaluation itself and, up to --host-max-k, the host route.  One JSON line per K.
  md       profiles/policy_wc_params.md's tables from measure's lines (--json) and the kernels' registers and scratch from the build
           remarks (ratilqr.jl_amd/csrc/policy_mc.remarks).

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

BOUNDS, THETAS = (0.1,), (0.0,)
N, SEED = 50, 7


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


def numpy_moments(q, J, p):
    """mean and covariance of q and its covariance with J under the weights p (0 at a DomainError rollout)"""
    ok = p > 0
    q, J, pk = q[ok], J[ok], p[ok] / p[ok].sum()
    mq, mJ = pk @ q, pk @ J
    pq = q * pk[:, None]
    return mq, pq.T @ q - np.outer(mq, mq), pq.T @ J - mq * mJ


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

    def host(K):
        J = evaluate(K, want_costs=True)["costs"]
        q = ctx.sample_params(K, seed=SEED)
        for kw in (dict(kl_bounds=BOUNDS), dict(thetas=THETAS)):
            numpy_moments(q, J, ctx.policy_worst_case(want_weights=True, **kw)["weights"])

    for K in args.ks:
        evaluate(K)
        row = dict(case="lqc_12x4_N50_P14", K=K)
        row.update(alternating(dict(params_call=lambda: ctx.policy_worst_case_params(kl_bounds=BOUNDS, thetas=THETAS),
                                    params_call_no_cost=lambda: ctx.policy_worst_case_params(kl_bounds=BOUNDS, thetas=THETAS, cost=False),
                                    trajectory_call=lambda: ctx.policy_worst_case_trajectory(kl_bounds=BOUNDS, thetas=THETAS)), args.repeat))
        row.update(alternating(dict(evaluation=lambda: evaluate(K)), args.repeat))
        if K <= args.host_max_k:
            row.update(alternating(dict(host_route=lambda: host(K)), max(1, args.repeat // 2)))
            evaluate(K)
        print(json.dumps(row), flush=True)


def resources():
    path = os.path.join(ROOT, "ratilqr.jl_amd", "csrc", "policy_mc.remarks")
    if not os.path.exists(path):
        return {}
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: \S*?\d+(wcp_[a-z]+)(ILb([01])ELb([01])E)?", line)
        if m:
            cur = out.setdefault(m.group(1) + (f"<TWO={m.group(3)}, CROSS={m.group(4)}>" if m.group(2) else ""), {})
        elif "Function Name:" in line:
            cur = None
        for key, tag in (("VGPRs:", "vgprs"), ("AGPRs:", "agprs"), ("TotalSGPRs:", "sgprs"), ("ScratchSize [bytes/lane]:", "scratch"),
                         ("LDS Size [bytes/block]:", "lds"), ("Occupancy [waves/SIMD]:", "waves")):
            if cur is not None and key in line and "Spill" not in line:
                cur[tag] = line.split(key)[1].split("[")[0].strip()
    return out


def md(args):
    rows = [json.loads(ln) for ln in open(args.json) if ln.startswith("{")] if args.json and os.path.exists(args.json) else []
    out = ["## Time per call", ""]
    if not rows:
        out += ["**Not yet measured.**"]
    else:
        ms = lambda t: f"{1e3 * t['median']:.2f} (± {1e3 * t['spread']:.2f})" if t else "not run"
        out += ["| K | new call, ms | without the cost sums, ms | trajectory call, ms | the evaluation they replay, ms | host route, ms |", "|---|---|---|---|---|---|"]
        out += [f"| {r['K']} | {ms(r['params_call'])} | {ms(r['params_call_no_cost'])} | {ms(r['trajectory_call'])} | {ms(r['evaluation'])} | {ms(r.get('host_route'))} |"
                for r in rows]
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
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--json", default=None, help="md: the file holding measure's output lines")
    a = ap.parse_args()
    measure(a) if a.mode == "measure" else md(a)
