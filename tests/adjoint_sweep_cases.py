"""Cases of tests/test_gpu_adjoint_sweeps_parent.py, shared with tests/golden/make_adjoint_sweeps_golden.py (which records what the commit
BEFORE the three adjoint kernels shared one team skeleton and the margin gradient ended in replay_finish computed on them:
tests/golden/adjoint_sweeps_parent.npz).

rat_policy_gradient / _tail_gradient (rat_src_adjoint), rat_policy_param_gradient / _tail_param_gradient (rat_src_adjoint_p) and
rat_policy_margin_gradient (rat_src_margin_adjoint) sweep every rollout with a team of sixteen lanes; the tests that hold them to the
NumPy models do so within a tolerance, which a moved fused multiply-add or an exchange read from the wrong lane of a dead column can stay
inside.  These cases are the smallest at which a moved line can go wrong: 1 x 1 with N = 1, the 2 x 1 pendulum with N = 3 with and
without rat_user_f_jacobian (the barrier path), 5 x 3 with N = 2 (dead lanes in both halves of the tile), 12 x 4 with N = 3 (the full
tile), each closed and open loop (L == NULL in the close of a step), K = 7 (a team of the last wavefront past the chunk's end), one
evaluation across a chunk boundary, rollouts without a cost inside a wavefront, rollouts with a cost and non-finite sensitivities, both
row sources, 0, 15, 16, 17 and 32 parameters, parameter sampling, grad_x0 alone, one, two and four events, linear events alone, t* = N,
t* = -1 beside a cost, events of one call whose t* differ, and every refusal the three calls' own tests provoke.

run(name) -> {key: array or str} as tests/policy_host_cases.py has it (flatten, call and UNEXPECTED are its own)."""
import ctypes as C
import re

import numpy as np

import margin_gradient_model as mg
import param_gradient_model as pp
import policy_gradient_model as pg
import ratilqr.jl_amd as rat
import user_noise_model as un
import user_params_model as upm
from policy_host_cases import UNEXPECTED, call, flatten  # noqa: F401  (the recorder prints UNEXPECTED)
from ratilqr.jl_amd import _native as nv

ENTRY_POINTS = ("policy_gradient", "policy_tail_gradient", "policy_param_gradient", "policy_tail_param_gradient", "policy_margin_gradient")
SEED, K_TEAM_TAIL, K_TWO_CHUNKS, K_NO_COST = 11, 7, (1 << 16) + 5, 23
KL, TH, AL = (0.05, np.inf), (0.0, 0.7), (0.0, 0.9)
POLICY_HOOK = "#define RAT_USER_POLICY\n__device__ void rat_user_policy(int k, const double *x, const double *u_prev, double *u, const double *p) {}\n"

# the pendulums whose sampler fails where a normal exceeds 1 (PEND_NAN's rule at a threshold that K = 23 rollouts of three steps meet):
# plain (one normal a step) and with its parameters opened (two)
PEND_NAN_1 = un.PEND_NAN.replace("(z > 3.0) ? sqrt(3.0 - z)", "(z > 1.0) ? sqrt(1.0 - z)")
PEND_AD_NAN_1 = pp.PEND_AD.replace("w[1] = 0.1 * rng.normal();", "const double z = rng.normal();\n    w[1] = (z > 1.0) ? sqrt(1.0 - z) : 0.1 * z;")
assert PEND_NAN_1 != un.PEND_NAN and PEND_AD_NAN_1 != pp.PEND_AD


def context(case, N):
    return rat.Context(rat.DeviceSourceProblem(case.source, case.n, case.m, N, np.eye(case.n), params=case.p), max_batch=1, device=0)


def evaluate(ctx, case, pol, K, seed=SEED):
    x_nom, l, L = pol
    return ctx.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(case.npn, 0, seed=seed), K=K, want_costs=True)


def evaluated(case, N, K, closed=True):
    ctx = context(case, N)
    evaluate(ctx, case, pg.policy(case, N, closed), K)
    return ctx


def events(evs):
    return [mg.to_rat(rat, e) for e in evs]


def cost_calls(res, key, ctx, wc=dict(kl_bounds=KL, thetas=TH), alphas=AL, refused=False):
    """both row sources of rat_src_adjoint's calls; wc / alphas None: the other alone"""
    if wc is not None:
        call(res, f"{key}/policy_gradient/rows", lambda: ctx.policy_gradient(**wc), refused)
    if alphas is not None:
        call(res, f"{key}/policy_tail_gradient/rows", lambda: ctx.policy_tail_gradient(alphas), refused)


def param_calls(res, key, ctx, wc=dict(kl_bounds=KL, thetas=TH), alphas=AL, refused=False):
    if wc is not None:
        call(res, f"{key}/policy_param_gradient/rows", lambda: ctx.policy_param_gradient(**wc), refused)
    if alphas is not None:
        call(res, f"{key}/policy_tail_param_gradient/rows", lambda: ctx.policy_tail_param_gradient(alphas), refused)


def margin_call(res, key, ctx, evs, alphas=AL, refused=False):
    call(res, f"{key}/policy_margin_gradient/E{len(evs)}", lambda: ctx.policy_margin_gradient(events(evs), alphas), refused)


def margin_calls(res, key, ctx, case, N):
    """four events at once (two linear, two quadratic; the first one's window is the terminal step alone, so t* = N beside events whose
    t* lies below), the first alone, the two linear ones (quad == 0) and the two quadratic ones"""
    evs = mg.four_events(case, N)
    margin_call(res, key + "/four", ctx, evs)
    margin_call(res, key + "/terminal_alone", ctx, evs[:1])
    margin_call(res, key + "/linear", ctx, [evs[0], evs[2]])
    margin_call(res, key + "/quadratic", ctx, [evs[1], evs[3]])


def size_case(make, make_p, N):
    """one size: the cost and the margin gradients on pg's case, the parameter gradient on pp's, closed and open loop, K = 7"""
    def run_case():
        res = {}
        for closed in (True, False):
            loop = "closed" if closed else "open"
            case = make()
            ctx = evaluated(case, N, K_TEAM_TAIL, closed)
            cost_calls(res, loop, ctx)
            margin_calls(res, loop, ctx, case, N)
            for tag, mk in make_p:
                param_calls(res, f"{loop}/{tag}", evaluated(mk(), N, K_TEAM_TAIL, closed))
        return res
    return run_case


def case_pendulum_jacobian():
    """rat_user_f_jacobian: lane 0 of the team calls it, the columns go through LDS between two barriers"""
    res = {}
    for closed in (True, False):
        loop = "closed" if closed else "open"
        case = pg.Pendulum(source=pg.PEND_JAC)
        ctx = evaluated(case, 3, K_TEAM_TAIL, closed)
        cost_calls(res, loop, ctx)
        margin_calls(res, loop, ctx, case, 3)
        param_calls(res, loop, evaluated(pp.Pendulum(source=pp.PEND_AD_JAC), 3, K_TEAM_TAIL, closed))
    return res


def case_two_chunks():
    """as test_across_a_chunk_boundary of each gradient's test: the linear 2 x 1 source, N = 2, K = 2^16 + 5"""
    res = {}
    case, N = pg.Lin2(), 2
    ctx = evaluated(case, N, K_TWO_CHUNKS)
    cost_calls(res, "closed", ctx, dict(thetas=TH))
    margin_call(res, "closed", ctx, [mg.linear_event(case, N, 21, N)])
    param_calls(res, "closed", evaluated(pp.Lin2(), N, K_TWO_CHUNKS), dict(thetas=TH))
    return res


def case_no_cost():
    """rollouts without a cost (NaN: DomainError) between rollouts with one, in the wavefronts of K = 23"""
    res = {}
    N = 3
    case = pg.Pendulum(source=PEND_NAN_1, p=(0.1, 0.1))
    case.npn = 1
    ctx = context(case, N)
    bad = np.isnan(evaluate(ctx, case, pg.policy(case, N), K_NO_COST)["costs"])
    assert 0 < bad.sum() < K_NO_COST and (bad & (np.arange(K_NO_COST) % 4 % 3 != 0)).any(), bad   # (one of them on an inner team)
    res["plain/costs_nan"] = bad.astype(np.float64)
    cost_calls(res, "plain", ctx)
    margin_calls(res, "plain", ctx, case, N)
    casep = pp.Pendulum(source=PEND_AD_NAN_1)
    ctxp = context(casep, N)
    badp = np.isnan(evaluate(ctxp, casep, pg.policy(casep, N), K_NO_COST)["costs"])
    assert 0 < badp.sum() < K_NO_COST, badp
    res["params/costs_nan"] = badp.astype(np.float64)
    param_calls(res, "params", ctxp)
    # every rollout a DomainError
    allnan = pg.Pendulum(source=un.PEND_NAN, p=(0.1, np.nan))
    allnan.npn = 1
    ctx = context(allnan, N)
    assert evaluate(ctx, allnan, pg.policy(allnan, N), 8)["n_ok"] == 0
    cost_calls(res, "all", ctx, dict(kl_bounds=(0.1,), thetas=(0.0,)), (0.5,))
    margin_call(res, "all", ctx, mg.four_events(allnan, N))
    return res


def case_nonfinite():
    """a cost but a NaN or an Inf in the sensitivities: the sources of the three test_nonfinite_sensitivities_* tests, K = 64"""
    res = {}
    pol = (np.array([[1.0], [1.0], [0.0]]), np.array([[1.0], [0.0]]), np.array([[[0.5]], [[0.5]]]))
    case = pg.SqrtCost([0.5, 0.5, 0.0, 0.0, 1.0, 0.3])
    ctx = context(case, 2)
    assert evaluate(ctx, case, pol, 64)["n_ok"] == 64
    cost_calls(res, "sqrt_cost", ctx, dict(thetas=TH), (0.0,))
    casep = pp.SqrtParam()
    ctx = context(casep, 2)
    assert evaluate(ctx, casep, pol, 64)["n_ok"] == 64
    param_calls(res, "sqrt_param", ctx, dict(thetas=TH), (0.0,))
    cased, pold = mg.sqrt_dyn_setup()
    ctx = context(cased, 2)
    assert evaluate(ctx, cased, pold, 64)["n_ok"] == 64
    margin_call(res, "sqrt_dyn", ctx, [(None, np.array([1.0, 0.0]), -0.3, 2, 2)])
    margin_call(res, "sqrt_dyn/early", ctx, [(None, np.array([1.0, 0.5]), -0.3, 1, 1)], (0.0,))
    return res


def case_margin_nan():
    """t* = -1 beside a cost: SqrtDyn with sigma = 1e200.  Half of the rollouts draw w_0 = 0 and stay small; the others reach |x_1| and
    |u_1| near 1e200, whose squares overflow: the cost is Inf (a cost), and the margin x_1^2 - u_1^2 of the first event, whose window is
    step 1 alone, is Inf - Inf = NaN.  The second event, linear at t = N, is finite for every rollout, so the two events' t* differ in
    the rollouts where the first has none."""
    res = {}
    _, pol = mg.sqrt_dyn_setup()
    case = mg.SqrtDyn([0.5, 0.5, 1.0, 0.2, 2.0, 1e200])
    ctx = context(case, 2)
    ev = evaluate(ctx, case, pol, 16)
    assert ev["n_ok"] == 16 and 0 < np.isinf(ev["costs"]).sum() < 16
    res["costs_inf"] = np.isinf(ev["costs"]).astype(np.float64)
    evs = [(np.array([[1.0, 0.0], [0.0, -1.0]]), np.zeros(2), 0.0, 1, 1), (None, np.array([1.0, 0.0]), -0.3, 2, 2)]
    margin_call(res, "both", ctx, evs, (0.0, 0.5))
    margin_call(res, "nan_alone", ctx, evs[:1], (0.0, 0.5))
    return res


def case_params():
    """the parameter counts at the tile boundary, no parameters, sampling on, grad_x0 alone"""
    res = {}
    N = 3
    for NP in (15, 16, 17):
        param_calls(res, f"lq5x3p{NP}", evaluated(pp.LqCubic(5, 3, NP), N, K_TEAM_TAIL))
    # no parameters: the pendulum with its parameters as literals
    none = pp.Pendulum()
    none.source = none.source.replace("/ p[0]", "/ 1.3").replace("p[1] *", "0.1 *").replace("p[2] *", "0.8 *")
    c0 = rat.Context(rat.DeviceSourceProblem(none.source, 2, 1, N, np.eye(2), params=np.zeros(0)), max_batch=1, device=0)
    evaluate(c0, none, pg.policy(none, N), K_TEAM_TAIL)
    param_calls(res, "no_params", c0)
    th, rows, buf, gx = np.zeros(1), np.zeros(nv.WC_NSTAT), np.zeros(4), np.full(2, 7.0)

    def grad_p_of_nothing():
        nv.check(nv.lib().rat_policy_param_gradient(c0.h, None, C.c_int32(0), nv.P(th), C.c_int32(1), nv.P(rows), nv.P(buf), None, nv.P(gx), None, None))
    call(res, "no_params/policy_param_gradient/grad_p_out", grad_p_of_nothing, refused=True)
    res["no_params/grad_x0_left_alone"] = gx.copy()
    # grad_x0 alone on a problem that has parameters: every other output null
    case = pp.Pendulum()
    ctx = evaluated(case, N, K_TEAM_TAIL)
    rows2, gx2, nf = np.zeros((2, nv.WC_NSTAT)), np.zeros((2, 2)), C.c_int64(-1)
    th2, al2, trows = np.array(TH), np.array(AL), np.zeros((2, nv.TR_NSTAT))

    def x0_alone():
        nv.check(nv.lib().rat_policy_param_gradient(ctx.h, None, C.c_int32(0), nv.P(th2), C.c_int32(2), nv.P(rows2), None, None, nv.P(gx2), None, C.byref(nf)))
        return dict(rows=rows2.copy(), grad_x0=gx2.copy(), n_nonfinite=int(nf.value))

    def x0_alone_tail():
        nv.check(nv.lib().rat_policy_tail_param_gradient(ctx.h, nv.P(al2), C.c_int32(2), nv.P(trows), None, None, nv.P(gx2), None, None))
        return dict(rows=trows.copy(), grad_x0=gx2.copy())
    call(res, "x0_alone/policy_param_gradient/native", x0_alone)
    call(res, "x0_alone/policy_tail_param_gradient/native", x0_alone_tail)
    # parameter sampling on: every rollout at its own q
    cs = pp.Pendulum(source=pp.PEND_AD_JAC_SAMPLED)
    cx = context(cs, N)
    cx.set_param_sampling(rat.ParamSampling(2, 1))
    evaluate(cx, cs, pg.policy(cs, N), K_TEAM_TAIL)
    param_calls(res, "sampled", cx)
    cost_calls(res, "sampled", cx, dict(thetas=(0.0,)), None, refused=True)
    return res


def case_refusals():
    """every refusal that test_refusals_leave_the_handle_usable of the three calls' tests provokes, as its text, and the call after it"""
    res = {}
    N, K = 3, 16
    one = dict(thetas=(0.0,))
    # the cost gradients and the margin gradient on the plain pendulum
    case = pg.Pendulum()
    ctx, pol = context(case, N), pg.policy(case, N)
    evs = mg.four_events(case, N)
    cost_calls(res, "no_evaluation", ctx, one, (0.5,), refused=True)
    margin_call(res, "no_evaluation", ctx, evs[:1], refused=True)
    evaluate(ctx, case, pol, K)
    cost_calls(res, "nothing_to_compute", ctx, dict(), None, refused=True)
    cost_calls(res, "alpha_1", ctx, None, (1.0,), refused=True)
    cost_calls(res, "n_alpha_0", ctx, None, (), refused=True)
    cost_calls(res, "negative_kl_bound", ctx, dict(kl_bounds=(0.1, -0.1)), None, refused=True)
    margin_call(res, "alpha_1", ctx, evs[:1], (1.0,), refused=True)
    margin_call(res, "n_alpha_0", ctx, evs[:1], (), refused=True)
    margin_call(res, "n_event_0", ctx, [], refused=True)
    margin_call(res, "n_event_5", ctx, evs + evs[:1], refused=True)
    margin_call(res, "window", ctx, [(None, np.ones(3), 0.0, 2, N + 1)], refused=True)
    margin_call(res, "not_finite", ctx, [(None, np.array([1.0, np.inf, 0.0]), 0.0, 0, N)], refused=True)
    cost_calls(res, "after_refusals", ctx, one, (0.5,))
    margin_call(res, "after_refusals", ctx, evs[:1])
    # rows x N above the cap
    big = pg.Pendulum()
    cb = context(big, 106)
    evaluate(cb, big, pg.policy(big, 106), 4)
    cost_calls(res, "rowsteps", cb, dict(kl_bounds=np.full(16, 0.1), thetas=np.full(16, 0.5)), None, refused=True)
    cb = context(big, 53)
    evaluate(cb, big, pg.policy(big, 53), 4)
    margin_call(res, "rowsteps", cb, mg.four_events(big, 53), np.linspace(0.0, 0.9, 16), refused=True)
    # a family
    prob, x0, u = rat.synthetic_lq_problem()
    cf = rat.Context(prob, max_batch=1, device=0)
    cost_calls(res, "family", cf, one, (0.5,), refused=True)
    param_calls(res, "family", cf, one, (0.5,), refused=True)
    call(res, "family/policy_margin_gradient/E1", lambda: cf.policy_margin_gradient([rat.halfspace(np.ones(prob.n), 0.0)], [0.5]), refused=True)
    # a source with rat_user_policy: the headers' own refusal, through the compile-error mapping
    cp = pg.Pendulum(source=POLICY_HOOK + un.PEND_DIAG)
    cc = context(cp, N)
    evaluate(cc, cp, pol, K)
    cost_calls(res, "user_policy", cc, one, (0.5,), refused=True)
    margin_call(res, "user_policy", cc, evs[:1], refused=True)
    # the replay guard: the parameters changed behind the evaluation; an evaluation later the calls serve again
    ctx.set_params([0.1, 0.07, 0.1])
    cost_calls(res, "set_params", ctx, one, (0.5,), refused=True)
    margin_call(res, "set_params", ctx, evs[:1], refused=True)
    evaluate(ctx, case, pol, K)
    cost_calls(res, "set_params_evaluated", ctx, one, (0.5,))
    margin_call(res, "set_params_evaluated", ctx, evs[:1])
    # parameter sampling switched on, and off again
    cs = pg.Pendulum(source=upm.source(un.PEND_DIAG, "scale", 1, 2, 0, 0.0))
    cx = context(cs, N)
    cx.set_param_sampling(rat.ParamSampling(upm.PARAM_NORMALS, upm.PARAM_UNIFORMS))
    evaluate(cx, cs, pol, K)
    cost_calls(res, "sampling_on", cx, one, (0.5,), refused=True)
    margin_call(res, "sampling_on", cx, evs[:1], refused=True)
    cx.set_param_sampling(None)
    evaluate(cx, cs, pol, K)
    cost_calls(res, "sampling_off", cx, one, (0.5,))
    margin_call(res, "sampling_off", cx, evs[:1])
    # the parameter gradients on the pendulum with its parameters opened
    casep = pp.Pendulum()
    ctxp = context(casep, N)
    param_calls(res, "no_evaluation", ctxp, one, (0.5,), refused=True)
    evaluate(ctxp, casep, pol, K)
    param_calls(res, "nothing_to_compute", ctxp, dict(), None, refused=True)
    param_calls(res, "alpha_1", ctxp, None, (1.0,), refused=True)
    param_calls(res, "after_refusals", ctxp, one, (0.5,))
    # a source without RAT_USER_PARAMS_AD: the parameter header's refusal; the cost gradient serves it
    plain = pg.Pendulum()
    cpl = context(plain, N)
    evaluate(cpl, plain, pol, K)
    param_calls(res, "no_params_ad", cpl, one, (0.5,), refused=True)
    cost_calls(res, "no_params_ad", cpl, one, None)
    ctxp.set_params([1.3, 0.12, 0.8])
    param_calls(res, "set_params", ctxp, one, (0.5,), refused=True)
    evaluate(ctxp, casep, pol, K)
    param_calls(res, "set_params_evaluated", ctxp, one, (0.5,))
    return res


CASES = {
    "scalar_1x1_N1": size_case(lambda: pg.ScalarLQ(), (("p6", lambda: pp.ScalarLQ()),), 1),
    "pendulum_2x1_N3": size_case(lambda: pg.Pendulum(), (("p3", lambda: pp.Pendulum()),), 3),
    "pendulum_jacobian": case_pendulum_jacobian,
    "lq_5x3_N2": size_case(lambda: pg.LqCubic(5, 3, 2), (("p17", lambda: pp.LqCubic(5, 3, 17)),), 2),
    "lq_12x4_N3": size_case(lambda: pg.LqCubic(12, 4, 3), (("p32", lambda: pp.LqCubic(12, 4, 32)),), 3),
    "two_chunks": case_two_chunks,
    "no_cost": case_no_cost,
    "nonfinite": case_nonfinite,
    "margin_nan": case_margin_nan,
    "params": case_params,
    "refusals": case_refusals,
}


def compile_error(text):
    """A refusal that carries the compiler's words holds three things that are not the library's: the compiler's scratch directory, which
    is another one in every process; the line of the header's #error, which moves with the header's comment; and whatever the compiler
    goes on to say behind that #error (it stops there in one process and reports the kernel's follow-on errors in another, for the same
    library and source).  The first two are taken out and the text ends with the #error's own caret line; every other character stays."""
    text = re.sub(r"\S*/include/(source_\w+\.h)", r"\1", text)
    text = re.sub(r"(source_\w+\.h):\d+:\d+:", r"\1:", text)
    text = re.sub(r"(?m)^ *\d+ \|", "     |", text)
    return re.sub(r"(?s)(\n *\|  \^\n).*", r"\1", text, count=1)


def run(name):
    res = CASES[name]()
    return {f"{name}/{k}": compile_error(v) if k.endswith("/error") and "does not compile" in v else v for k, v in res.items()}
