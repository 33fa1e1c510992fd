"""Cases of tests/test_gpu_moment_replays_parent.py, shared with tests/golden/make_moment_replays_golden.py (which records what the commit
BEFORE the three moment replays shared one kernel skeleton and one host tail computed on them: tests/golden/moment_replays_parent.npz).

rat_policy_worst_case_trajectory / _disturbance / _params and rat_policy_tail_trajectory / _disturbance / _params run one schedule over
the rollouts -- groups of four to the wavefronts of WT_SLOTS workgroups, a liveness word per group for the tail calls, an LDS reduction
over the wavefronts into a partial per slot, the slots summed in *_final -- and the tests that hold tail to dense and alpha = 0 to
theta = 0 bit for bit pass whether or not a change to that schedule keeps every sum in its order.  These cases are the smallest at which
the schedule can go wrong: K = 3 (the K tail inside one group, 31 of 32 wavefronts idle), K = 129 = 4 WT_WAVES WT_SLOTS + 1 (one wavefront
gets a second group) under twelve worst-case rows (a second row batch of four) and eleven levels, K = 2^16 + 5 (the += across chunks),
the open loop, DomainErrors and an all-NaN sample, the fourteen-parameter source (one parameter tile, ldx = n), the tiny source with
P = 17 and 32 (two tiles), and every refusal of the replays' host path.

run(name) -> {key: array or str} as tests/policy_host_cases.py has it (flatten, call and UNEXPECTED are its own)."""
import numpy as np

import ratilqr.jl_amd as rat
import user_noise_model as um
import user_params_model as pm
import wc_params_model as wp
from policy_host_cases import UNEXPECTED, call, flatten  # noqa: F401  (the recorder prints UNEXPECTED)
from test_cpu_wc_params import lqc_p
from test_gpu_tail_scenarios import lq, step_context, step_eval
from test_gpu_user_noise import pend_problem
from test_gpu_wc_params import L_OPEN, X0, tiny_context, tiny_evaluate

K_GROUP_TAIL, K_SECOND_GROUP, K_TWO_CHUNKS = 3, 4 * 4 * 8 + 1, (1 << 16) + 5
ENTRY_POINTS = ("policy_worst_case_trajectory", "policy_worst_case_disturbance", "policy_worst_case_params", "policy_tail_trajectory",
                "policy_tail_disturbance", "policy_tail_params")
BOUNDS9 = (0.01, 0.02, 0.05, 0.1, 0.2, 0.5, 1.0, 1.5, 2.0)
THETAS3 = (0.0, 0.3, 1.0)
ALPHAS11 = tuple(0.1 * i for i in range(10)) + (1.0 - 0.5 / K_SECOND_GROUP,)


def state_calls(res, key, ctx, wc, alphas, refused=False, crosses=(True,), denses=(0,)):
    """the trajectory and the disturbance call and their tail siblings on the last evaluation; wc: the worst-case rows' keywords, None:
    the tail calls alone; alphas None: the worst-case calls alone"""
    if wc is not None:
        call(res, f"{key}/policy_worst_case_trajectory/rows", lambda: ctx.policy_worst_case_trajectory(**wc), refused)
        for cross in crosses:
            call(res, f"{key}/policy_worst_case_disturbance/cross{int(cross)}", lambda: ctx.policy_worst_case_disturbance(cross=cross, **wc), refused)
    for dense in denses if alphas is not None else ():
        ctx.debug_set("tail_dense", dense)
        try:
            call(res, f"{key}/policy_tail_trajectory/dense{dense}", lambda: ctx.policy_tail_trajectory(alphas), refused)
            for cross in crosses:
                call(res, f"{key}/policy_tail_disturbance/dense{dense}_cross{int(cross)}", lambda: ctx.policy_tail_disturbance(alphas, cross=cross),
                     refused)
        finally:
            ctx.debug_set("tail_dense", 0)


def param_calls(res, key, ctx, wc, alphas, refused=False, costs=(True, False)):
    for cost in costs:
        if wc is not None:
            call(res, f"{key}/policy_worst_case_params/cost{int(cost)}", lambda: ctx.policy_worst_case_params(cost=cost, **wc), refused)
        if alphas is not None:
            call(res, f"{key}/policy_tail_params/cost{int(cost)}", lambda: ctx.policy_tail_params(alphas, cost=cost), refused)


def lq_evaluated(n, m, N, K, closed=True):
    prob, x0, l, L = lq(n, m, N)
    ctx = rat.Context(prob)
    if closed:
        ctx.policy_evaluate(ctx.rollout_open(x0, l), l, L, K=K, seed=5)
    else:
        ctx.policy_evaluate(x0, l, None, K=K, seed=5)
    return ctx


def case_lq_1x1_K3():
    res = {}
    ctx = lq_evaluated(1, 1, 1, K_GROUP_TAIL)
    state_calls(res, "closed", ctx, dict(kl_bounds=(0.1, np.inf), thetas=(0.0, 0.3)), (0.0, 0.5, 0.9, 1.0 - 0.5 / K_GROUP_TAIL), crosses=(True, False),
                denses=(0, 1))
    return res


def case_lq_5x3_K129_rows():
    res = {}
    ctx = lq_evaluated(5, 3, 4, K_SECOND_GROUP)
    state_calls(res, "closed", ctx, dict(kl_bounds=BOUNDS9, thetas=THETAS3), ALPHAS11, crosses=(True, False), denses=(0, 1))
    return res


def case_lq_12x4_two_chunks():
    res = {}
    ctx = lq_evaluated(12, 4, 3, K_TWO_CHUNKS)
    state_calls(res, "closed", ctx, dict(kl_bounds=(0.1,), thetas=(0.0, 0.3)), (0.0, 0.9))
    return res


def case_lq_open_loop():
    res = {}
    ctx = lq_evaluated(3, 2, 5, 70, closed=False)
    state_calls(res, "open", ctx, dict(kl_bounds=(0.1, 1.0), thetas=(0.0, 0.5)), (0.0, 0.5, 0.9))
    return res


def case_lq_domain_errors():
    """the step source of tests/test_gpu_tail_scenarios.py whose sampler fails above a threshold, then with every draw failing"""
    res = {}
    ctx = step_context(nan_above=1.0)
    r = step_eval(ctx, K_SECOND_GROUP)
    assert 0 < np.isnan(r["costs"]).sum() < K_SECOND_GROUP
    state_calls(res, "some", ctx, dict(kl_bounds=(0.1, np.inf), thetas=(0.0, 0.5)), (0.0, 0.5, 0.9), denses=(0, 1))
    ctx.set_params([0.5, 0.0, -1e9])
    assert step_eval(ctx, 9)["n_ok"] == 0
    state_calls(res, "all", ctx, dict(kl_bounds=(0.1,), thetas=(0.0,)), (0.0, 0.9))
    return res


def case_source_P14():
    """the LQ + cubic source with fourteen parameters under its rat_user_noise, parameter sampling on"""
    res = {}
    c = pm.case("lq12")
    N, p = 3, lqc_p()
    ctx = rat.Context(c.problem("scale", p=p, N=N))
    ctx.set_param_sampling(rat.ParamSampling(pm.PARAM_NORMALS, pm.PARAM_UNIFORMS))
    r0 = np.random.default_rng(3)
    x_nom, l, L = 0.5 * r0.standard_normal((N + 1, c.n)), 0.8 * r0.standard_normal((N, c.m)), 0.1 * r0.standard_normal((N, c.m, c.n))
    ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=21), K=K_SECOND_GROUP)
    wc, al = dict(kl_bounds=(0.1, np.inf), thetas=(0.0, 0.5)), (0.0, 0.5, 0.9, 1.0 - 0.5 / K_SECOND_GROUP)
    state_calls(res, "closed", ctx, wc, al, denses=(0, 1))
    param_calls(res, "closed", ctx, wc, al)
    return res


def case_tiny(P, K):
    def run_case():
        res = {}
        ctx, _ = tiny_context(P)
        tiny_evaluate(ctx, K, seed=7)
        param_calls(res, "open", ctx, dict(kl_bounds=(0.1, np.inf), thetas=(0.0, 0.5)), (0.0, 0.5, 0.9, 1.0 - 0.5 / K))
        return res
    return run_case


def case_refusals():
    """every refusal of the replays' host path, as its text; a refusal leaves the handle usable (the call after it is recorded too)"""
    res = {}
    wc, al = dict(kl_bounds=(0.1,)), (0.5,)
    mu, Cq, a, b = wp.tiny_tables(3)

    def tiny3():
        ctx = rat.Context(rat.DeviceSourceProblem(wp.tiny_source(3, Cq, a, b, "gauss", None), 1, 1, 2, np.eye(1), params=mu))
        ctx.set_param_sampling(rat.ParamSampling(3, 0))
        return ctx
    # no evaluation to replay
    prob, x0, l, L = lq(5, 3, 4)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)
    state_calls(res, "no_evaluation", ctx, wc, al, refused=True)
    tiny = tiny3()
    param_calls(res, "no_evaluation", tiny, wc, al, refused=True, costs=(True,))
    # an evaluation on injected draws
    ctx.policy_evaluate(x_det, l, L, z=np.random.default_rng(0).standard_normal((8, 4, 5)))
    state_calls(res, "injected", ctx, wc, al, refused=True)
    tiny.policy_evaluate_noise(X0, L_OPEN, None, noise=rat.UserNoise(1, 0, zn=np.zeros((4, 2, 1))))
    param_calls(res, "injected", tiny, wc, al, refused=True, costs=(True,))
    # the rows' own rules on a proper evaluation: no level, alpha = 1, a negative kl_bound; then a good call on the same handle
    ctx.policy_evaluate(x_det, l, L, K=20, seed=1)
    tiny_evaluate(tiny, 20, seed=1)
    for name, kw, alphas in (("n_alpha_0", None, ()), ("alpha_1", None, (1.0,)), ("negative_kl_bound", dict(kl_bounds=(0.1, -0.1)), None)):
        state_calls(res, name, ctx, kw, alphas, refused=True)
        param_calls(res, name, tiny, kw, alphas, refused=True, costs=(True,))
    state_calls(res, "after_refusals", ctx, wc, al)
    param_calls(res, "after_refusals", tiny, wc, al, costs=(True,))
    # the parameters changed behind the evaluation: the replayed costs are no longer the evaluation's (the message carries the counts)
    tiny.set_params(mu + 0.5)
    state_calls(res, "set_params", tiny, wc, al, refused=True)
    param_calls(res, "set_params", tiny, wc, al, refused=True, costs=(True,))
    tiny.set_params(mu)
    tiny_evaluate(tiny, 20, seed=1)
    param_calls(res, "set_params_back", tiny, wc, al, costs=(True,))
    # a parameter call with sampling off
    N = 3
    x_nom, pl, pL = um.pend_policy(N)
    src = rat.Context(pend_problem(um.PEND_STATE, N, um.PEND_STATE_P))
    src.policy_evaluate_noise(x_nom, pl, pL, noise=rat.UserNoise(3, 0, seed=1), K=16)
    param_calls(res, "sampling_off", src, wc, al, refused=True, costs=(True,))
    # rows x (N + 1) above WT_MAX_ROWSTEPS = 3640 (10 x 401) and rows x N above WD_MAX_ROWSTEPS = 1899 (5 x 400): refused before any launch
    long_prob = rat.LQRiskSensitiveProblem(np.eye(2), np.eye(2), Q=np.eye(2), R=np.eye(2), N=400, W=np.eye(2), Qf=np.eye(2))
    lc = rat.Context(long_prob)
    lc.policy_evaluate(np.zeros(2), np.zeros((400, 2)), K=4, seed=1)
    ten, five = tuple(0.05 * i for i in range(10)), tuple(0.05 * i for i in range(5))
    call(res, "rowsteps/policy_worst_case_trajectory/ten", lambda: lc.policy_worst_case_trajectory(thetas=ten), refused=True)
    call(res, "rowsteps/policy_tail_trajectory/ten", lambda: lc.policy_tail_trajectory(ten), refused=True)
    call(res, "rowsteps/policy_worst_case_disturbance/five", lambda: lc.policy_worst_case_disturbance(thetas=five), refused=True)
    call(res, "rowsteps/policy_tail_disturbance/five", lambda: lc.policy_tail_disturbance(five), refused=True)
    return res


CASES = {
    "lq_1x1_K3": case_lq_1x1_K3,
    "lq_5x3_K129_rows": case_lq_5x3_K129_rows,
    "lq_12x4_two_chunks": case_lq_12x4_two_chunks,
    "lq_open_loop": case_lq_open_loop,
    "lq_domain_errors": case_lq_domain_errors,
    "source_P14": case_source_P14,
    "tiny_P17": case_tiny(17, K_SECOND_GROUP),
    "tiny_P32": case_tiny(32, K_TWO_CHUNKS),
    "refusals": case_refusals,
}


def run(name):
    return {f"{name}/{k}": v for k, v in CASES[name]().items()}
