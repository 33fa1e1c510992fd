"""Cases of tests/test_gpu_source_step_parent.py, shared with tests/golden/make_source_step_golden.py (which records what the commit BEFORE
csrc/source_step.h computed on them: tests/golden/source_step_parent.npz).

The rollout kernels of source models take their guards, NaN predicate, gain-row product, affine law and choice of parameters from one
header; these cases are the smallest at which those pieces can go wrong: the 2 x 1 pendulum (three normals) at N = 6 and the 12 x 4
LQ_MIX (twelve normals and a uniform) at N = 4, K = 3 (the K tail inside a wavefront), K = 65 (the 64 lanes a workgroup carries, plus
one) and, for rat_policy_evaluate_noise alone, K = 2^16 + 5 (one past a host chunk); open and closed loop; the device generator and
injected draws; no hook, the identity hook, clamp + rate; parameter sampling off and on (the event kernel forms q again); a NaN that
first appears from f, c, the sampler, h and the hook at a step other than 0 on some rollouts, and an input that is NaN already.

run(name) -> {key: array or str} as tests/policy_host_cases.py has it (flatten, call and UNEXPECTED are its own)."""
import numpy as np

import ratilqr.jl_amd as rat
import user_noise_model as um
import user_params_model as pm
import user_policy_model as up
from policy_host_cases import UNEXPECTED, call, flatten  # noqa: F401  (the recorder prints UNEXPECTED)

K_TAIL, K_LANES_1, K_CHUNK_1 = 3, 64 + 1, (1 << 16) + 5
ENTRY_POINTS = ("policy_evaluate", "policy_evaluate_noise", "policy_worst_case_disturbance", "policy_rare_event_noise",
                "policy_rare_event_user", "policy_events_user", "solve")
PEND_N = 6
WC = dict(kl_bounds=(0.1,), thetas=(0.5,))


def small(c, K):
    """whether a call's full arrays fit the fixture: every trajectory at 2 x 1, those of the K tail at 12 x 4 (the costs and the moments of
    the w_out replay are recorded at every K)"""
    return c.n == 2 or K == K_TAIL


def wc_rows(c):
    return WC if c.n == 2 else dict(thetas=(0.5,), cross=False)


def setting(name):
    """(case of tests/user_policy_model.py, N, closed-loop policy) for "pend" (N = 6) and "lq12" (N = 4)"""
    c = up.case(name)
    if name == "pend":
        x_nom, l, L = um.pend_policy(PEND_N)
        return c, PEND_N, (x_nom, l, 4.0 * L)
    return c, c.N, c.policy


def problem(c, N, hook, base=None, q=None):
    base = c.base if base is None else base
    src = base if hook is None else up.source(base, c.poff, hook)
    return rat.DeviceSourceProblem(src, c.n, c.m, N, c.W, params=c.params(q))


def injected(c, N, K, seed=43):
    r = np.random.default_rng(seed)
    return c.user_noise(zn=r.standard_normal((K, N, c.npn)), zu=r.random((K, N, c.npu)) if c.npu else None)


def sampler_calls(res, key, ctx, c, N, pol, K, closed, inject, rare):
    """rat_policy_evaluate_noise with trajectories, the w_out replay behind it, and the two rare-event passes on the same policy"""
    x_nom, l, L = pol if closed else (pol[0][0], pol[1], None)
    noise = injected(c, N, K) if inject else c.user_noise(seed=77)
    call(res, f"{key}/policy_evaluate_noise", lambda: ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, thetas=(0.0, 0.3), K=K, want_costs=True,
                                                                                 want_trajectories=small(c, K) and not (inject and K > K_TAIL)))
    if not inject:
        call(res, f"{key}/policy_worst_case_disturbance", lambda: ctx.policy_worst_case_disturbance(**wc_rows(c)))
    if rare:
        ev = rat.halfspace(np.eye(c.n)[0], -(np.abs(pol[0][:, 0]).max() + 0.1))
        shift = 0.3 * np.arange(1, N * c.npn + 1, dtype=float).reshape(N, c.npn) / (N * c.npn)
        for sname, s in (("zero_shift", None), ("shifted", shift)):
            call(res, f"{key}/policy_rare_event_noise/{sname}",
                 lambda: ctx.policy_rare_event_noise(x_nom, l, L, ev, K, noise=c.user_noise(), seed=5, shift=s, n_iter=1, rho=0.2, want_margins=True,
                                                     want_logw=True))


def w_calls(res, key, ctx, c, N, pol, K, closed, inject):
    """rat_policy_evaluate (the Cholesky kernel) on the same policy"""
    x_nom, l, L = pol if closed else (pol[0][0], pol[1], None)
    z = np.random.default_rng(41).standard_normal((K, N, c.n)) if inject else None
    call(res, f"{key}/policy_evaluate", lambda: ctx.policy_evaluate(x_nom, l, L, thetas=(0.0, 0.3), K=K, z=z, seed=9, want_costs=True))


def case_hooks(name):
    def run_case():
        res = {}
        c, N, pol = setting(name)
        for hook in (None, "identity", "rate"):
            ctx = rat.Context(problem(c, N, hook))
            for K in (K_TAIL, K_LANES_1):
                for closed, inject in ((True, False), (False, False), (True, True)):
                    key = f"{hook}/K{K}/{'closed' if closed else 'open'}/{'injected' if inject else 'generator'}"
                    sampler_calls(res, key, ctx, c, N, pol, K, closed, inject, rare=not inject)
                    w_calls(res, key, ctx, c, N, pol, K, closed, inject)
        return res
    return run_case


def case_one_past_a_chunk():
    res = {}
    c, N, pol = setting("pend")
    ctx = rat.Context(problem(c, N, "rate"))
    x_nom, l, L = pol
    call(res, "rate/closed/generator/policy_evaluate_noise",
         lambda: ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=77), thetas=(0.0, 0.3), K=K_CHUNK_1, want_costs=True))
    return res


def case_params(name):
    """parameter sampling off and on: the rollout's own q in the sampler kernel, both rare kernels and, formed again, the event kernel"""
    def run_case():
        res = {}
        c = pm.case(name)
        x_nom, l, L = c.policy
        ctx = rat.Context(c.problem("scale", event=True))
        for on in (False, True):
            ctx.set_param_sampling(c.sampling(injected=False) if on else None)
            for K in (K_TAIL, K_LANES_1):
                key = f"sampling{int(on)}/K{K}"
                call(res, f"{key}/policy_evaluate_noise", lambda: ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=21), thetas=(0.0, 0.3), K=K,
                                                                                             want_costs=True, want_trajectories=small(c, K)))
                call(res, f"{key}/policy_events_user", lambda: ctx.policy_events_user(1, want_steps=True, want_margins=True, **WC))
                call(res, f"{key}/policy_worst_case_disturbance", lambda: ctx.policy_worst_case_disturbance(**wc_rows(c)))
                call(res, f"{key}/policy_rare_event_user", lambda: ctx.policy_rare_event_user(x_nom, l, L, 1, 0, K, noise=c.user_noise(), seed=5, n_iter=1,
                                                                                               rho=0.2, want_margins=True, want_logw=True))
                ev = rat.halfspace(np.eye(c.n)[0], -0.5)
                call(res, f"{key}/policy_rare_event_noise", lambda: ctx.policy_rare_event_noise(x_nom, l, L, ev, K, noise=c.user_noise(), seed=5, n_iter=1,
                                                                                                 rho=0.2, want_margins=True, want_logw=True))
        return res
    return run_case


# ---- DomainErrors: the pendulum with a NaN from one function where the angle has passed TH (x_0 starts near 1, the sampler moves it by
# about 0.3 |x_0| a step, so some rollouts pass it and none does at step 0) -----------------------------------------------------------------
TH = 1.3
_NAN = f"((x[0] > {TH}) ? sqrt({TH} - x[0]) : 0.0)"
_SAMPLER = um.PEND_STATE[len(um.PEND_FCH):]
NAN_SOURCES = {
    "f": um.PEND_FCH.replace("xn[0] = x[0] + dt * x[1];", f"xn[0] = x[0] + dt * x[1] + {_NAN};") + _SAMPLER,
    "c": um.PEND_FCH.replace("+ 0.01 * k * x[0];", f"+ 0.01 * k * x[0] + {_NAN};") + _SAMPLER,
    "h": um.PEND_FCH.replace("return 2.0 * (x[0] * x[0] + x[1] * x[1]);", f"return 2.0 * (x[0] * x[0] + x[1] * x[1]) + {_NAN};") + _SAMPLER,
    "w": um.PEND_STATE.replace("    w[0] = p[1] * fabs(x[0]) * z0;", f"    w[0] = p[1] * fabs(x[0]) * z0 + {_NAN};"),
}
assert all(src != um.PEND_STATE for src in NAN_SOURCES.values())


def case_domain_errors():
    res = {}
    c, N, pol = setting("pend")
    x_nom, l, L = pol
    ev = rat.halfspace(np.eye(2)[0], -1.2)
    runs = [(where, problem(c, N, None, base=src)) for where, src in NAN_SOURCES.items()]
    runs.append(("hook", problem(c, N, "nan", q=np.array([1e300, 1e300, TH]))))
    for where, prob in runs:
        ctx = rat.Context(prob)
        ok = call(res, f"{where}/policy_evaluate_noise", lambda: ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=77), K=K_LANES_1,
                                                                                             want_costs=True, want_trajectories=True))
        if ok:                                                         # (on some rollouts only, and where the angle passed TH at a step > 0)
            r = ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=77), K=K_LANES_1, want_costs=True, want_trajectories=True)
            dom, ang = np.isnan(r["costs"]), r["x"][:, :, 0]
            assert 0 < dom.sum() < K_LANES_1, (where, dom.sum())
            assert not np.any(ang[:, 0] > TH) and np.all(np.nanmax(np.where(np.isnan(ang[dom]), -np.inf, ang[dom]), axis=1) > TH), where
        call(res, f"{where}/policy_worst_case_disturbance", lambda: ctx.policy_worst_case_disturbance(**WC))
        call(res, f"{where}/policy_rare_event_noise", lambda: ctx.policy_rare_event_noise(x_nom, l, L, ev, K_LANES_1, noise=c.user_noise(), seed=5, n_iter=1,
                                                                                            rho=0.2, want_margins=True, want_logw=True))
        if where != "w":                                               # (the Cholesky kernel calls no sampler)
            call(res, f"{where}/policy_evaluate", lambda: ctx.policy_evaluate(x_nom, l, L, K=K_LANES_1, seed=9, want_costs=True))
    # an input that is NaN already: l_2 on the open loop.  By the rule no DomainError; the costs are NaN all the same
    ctx = rat.Context(problem(c, N, None))
    l_nan = l.copy()
    l_nan[2] = np.nan
    call(res, "input/policy_evaluate_noise", lambda: ctx.policy_evaluate_noise(x_nom[0], l_nan, None, noise=c.user_noise(seed=77), K=K_TAIL, want_costs=True,
                                                                                want_trajectories=True))
    call(res, "input/policy_evaluate", lambda: ctx.policy_evaluate(x_nom[0], l_nan, None, K=K_TAIL, seed=9, want_costs=True))
    return res


def case_solve():
    """two iterations of iLEQG on the 12 x 4 LQ source and on the pendulum: the row product of rat_src_rollout's line-search candidates"""
    res = {}
    gp = um.lq_generative(Nh=4)
    r = np.random.default_rng(8)
    two = rat.ileqg.make_opts(iter_max=2)
    ctx = rat.Context(um.lq_source_problem(gp), two)
    call(res, "lq12/solve", lambda: ctx.solve(0.5 * r.standard_normal(12), 0.1 * r.standard_normal((4, 4)), 0.3))
    c, N, pol = setting("pend")
    ctx = rat.Context(problem(c, N, None), two)
    call(res, "pend/solve", lambda: ctx.solve(pol[0][0], pol[1], 0.5))
    return res


CASES = {
    "pend_hooks": case_hooks("pend"),
    "lq12_hooks": case_hooks("lq12"),
    "one_past_a_chunk": case_one_past_a_chunk,
    "pend_params": case_params("pend"),
    "lq12_params": case_params("lq12"),
    "domain_errors": case_domain_errors,
    "solve": case_solve,
}


def run(name):
    return {f"{name}/{k}": v for k, v in CASES[name]().items()}
