"""Cases of tests/test_gpu_event_sums_parent.py, shared with tests/golden/make_event_sums_golden.py (which records what the commit BEFORE
ev_sums / tle_sums and ev_final / tle_final shared one body each computed on them: tests/golden/event_sums_parent.npz).

rat_policy_events / _user run ev_sums and ev_final behind each chunk of the replay; rat_policy_tail_events / _user run tle_sums and
tle_final, or ev_sums on the tail weights under the switch tail_dense.  The tests that hold these calls to the NumPy models do so within
a tolerance, which a partial read at another address, a tree fed in another order or a selection exchanged for a product can stay inside.
These cases are the smallest at which the shared body can go wrong:

rows      1, EV_ROWS = 4 (one full batch), 5 (a second batch with nr = 1: the liveness word shifted by r0 = 4), 16 tail levels and the
          32 rows of a KL call; KL calls mix kl_bounds and thetas, tail calls give as many levels, alpha = 0 among them
events    1 and EV_MAX = 16 (bit 16, the "any" column, live), quadratic and linear ones, windows t_lo = t_hi
step_out  present and absent (nsteps, with it ny and every partial's address), with and without margin_out
K         7 (slots 1 .. 7 get no rollout: mx stays -Inf there; no multiple of 4), 2049 (a lane's second trip) and 2^16 + 5 (two chunks:
          first is false on the second, the last liveness group is cut)
NaN       rollouts without a cost (the power law's DomainErrors) and a user event that writes nothing on the cheap rollouts (a NaN
          margin where a tail row has no weight: tle_sums' (y != 0) selection)
rows that hold no numbers: a sample without any cost (EMPTY), a KL radius beyond the sample's reach (saturated), a level thinner than
one rollout; and every refusal the four calls' own tests provoke of the events, the limit on the partial sums and the handle.

The 12 x 4 LQ family at N = 3 and the 2 x 1 pendulum source at N = 4.  Every tail call is recorded a second time under tail_dense.
margin_out is recorded at the two small K alone.

run(name) -> {key: array or str} as tests/policy_host_cases.py has it (flatten, call and UNEXPECTED are its own)."""
import numpy as np

import events_model as em
import ratilqr.jl_amd as rat
import user_event_model as ue
import user_noise_model as um
from policy_host_cases import UNEXPECTED, call, flatten  # noqa: F401  (the recorder prints UNEXPECTED)
from test_gpu_events import event_set
from test_gpu_tail_events import half_spaces, levels

ENTRY_POINTS = ("policy_events", "policy_events_user", "policy_tail_events", "policy_tail_events_user")
TAIL_ENTRY_POINTS = ENTRY_POINTS[2:]
K_SMALL, K_LANES, K_CHUNKS = 7, 2049, (1 << 16) + 5
SEED = 5
# kl_bounds and thetas of a KL call by its number of rows; 100 lies beyond the reach log K of every sample here: a saturated row
KL_ROWS = {1: ((0.1,), ()), 4: ((0.05, 1.0), (0.0, 0.7)), 5: ((0.05, 100.0), (0.0, 0.3, 0.7)),
           32: (tuple(np.round(np.linspace(0.01, 2.0, 16), 4)), tuple(np.round(np.linspace(0.0, 1.5, 16), 4)))}

# sixteen entries on the pendulum: fourteen half-spaces on the two state components in turn, one that is written only where the state is
# far out (the cheap rollouts keep a NaN margin), and one that is never written
PEND_EVENTS = ("    for (int i = 0; i < 14; ++i) g[i] = x[i % 2] - q[i];\n"
               "    if (2.0 * (x[0] * x[0] + x[1] * x[1]) > q[14]) g[14] = q[15] - x[1];\n")
PEND_N, PEND_P, PEND_NQ = 4, [0.1, 0.05, 0.1], 16


def events_calls(res, key, ctx, evs, rows, steps, margins, refused=False):
    """the KL call with `rows` rows and the tail call with as many levels (KL calls of 32 rows: 16 levels), that one under tail_dense too;
    evs: a list of events, or the n_event of the user's"""
    user = isinstance(evs, int)
    kl, th = KL_ROWS[rows]
    al = levels(min(rows, 16), ctx.debug_get("mc_cost_K"))
    kw = dict(want_steps=steps, want_margins=margins)
    tag = f"E{evs if user else len(evs)}_R{rows}_steps{int(steps)}_margins{int(margins)}"
    if user:
        call(res, f"{key}/policy_events_user/{tag}", lambda: ctx.policy_events_user(evs, kl_bounds=kl, thetas=th, **kw), refused)
    else:
        call(res, f"{key}/policy_events/{tag}", lambda: ctx.policy_events(evs, kl_bounds=kl, thetas=th, **kw), refused)
    tail_calls(res, key, ctx, evs, al, tag, kw, refused)


def tail_calls(res, key, ctx, evs, al, tag, kw, refused=False):
    user = isinstance(evs, int)
    ep = "policy_tail_events_user" if user else "policy_tail_events"
    fn = (lambda: ctx.policy_tail_events_user(evs, al, **kw)) if user else (lambda: ctx.policy_tail_events(evs, al, **kw))
    call(res, f"{key}/{ep}/{tag}", fn, refused)
    ctx.debug_set("tail_dense", 1)
    try:
        call(res, f"{key}/{ep}/{tag}_dense", fn, refused)
    finally:
        ctx.debug_set("tail_dense", 0)


# ---- the 12 x 4 LQ family ---------------------------------------------------------------------------------------------------------------
def lq_context(K):
    """the 12 x 4 family at N = 3 evaluated at K under a closed-loop policy; the events are sized from its first rollouts"""
    N = 3
    prob, x0, _ = rat.synthetic_lq_problem(n=12, m=4, N=N, seed=15, w=0.09)
    r = np.random.default_rng(12)
    l, L = 0.5 * r.standard_normal((N, 4)), 0.1 * r.standard_normal((N, 4, 12))
    ctx = rat.Context(prob, max_batch=1, device=0)
    x_det = ctx.rollout_open(x0, l)
    x, u, cost, _ = ctx.rollout_noisy(x_det, l, L, K=min(K, 64), seed=SEED)
    ctx.policy_evaluate(x_det, l, L, K=K, seed=SEED)
    return ctx, event_set(x, u, cost, np.random.default_rng(K)), half_spaces(x, cost, 16, N)


def case_lq(K):
    def run_case():
        res = {}
        ctx, nine, sixteen = lq_context(K)
        small = K < K_CHUNKS
        events_calls(res, "nine", ctx, nine, 5, True, small)
        events_calls(res, "nine", ctx, nine, 5, False, False)
        events_calls(res, "nine", ctx, nine, 4, True, False)
        events_calls(res, "nine", ctx, nine, 1, False, small)
        events_calls(res, "nine", ctx, nine, 32, K != K_LANES, False)
        events_calls(res, "sixteen_linear", ctx, sixteen, 4, True, small)
        events_calls(res, "sixteen_linear", ctx, sixteen, 5, False, False)
        events_calls(res, "one_linear", ctx, sixteen[-1:], 1, True, False)       # (its window is step N alone)
        events_calls(res, "one_quadratic", ctx, nine[3:4], 5, K == K_SMALL, False)
        return res
    return run_case


# ---- the pendulum source with its own events -----------------------------------------------------------------------------------------------
def pend_context(K):
    """the pendulum at N = 4 evaluated at K; the events' thresholds are sized from the trajectories, the fifteenth is written on about
    the outer half of the rollouts"""
    N = PEND_N
    prob = rat.DeviceSourceProblem(ue.source(um.PEND_DIAG, "sixteen", len(PEND_P), body=PEND_EVENTS), 2, 1, N, 1e-3 * np.eye(2),
                                   params=np.concatenate([PEND_P, np.zeros(PEND_NQ)]))
    ctx = rat.Context(prob, max_batch=1, device=0)
    evaluate = lambda: ctx.policy_evaluate_noise(*um.pend_policy(N), noise=rat.UserNoise(2, 0, seed=SEED), K=K, want_costs=True, want_trajectories=True)
    r = evaluate()
    x = r["x"]
    assert r["n_ok"] == K
    far = 2.0 * (x ** 2).sum(axis=2).max(axis=1)
    q = [em.between(x[:, :, i % 2].max(axis=1), 0.1 + 0.06 * i) for i in range(14)] + [em.between(far, 0.5), em.between(x[:, :, 1].min(axis=1), 0.3)]
    ctx.set_params(np.concatenate([PEND_P, q]))
    assert np.array_equal(evaluate()["costs"], r["costs"])                        # (the model does not read the events' parameters)
    return ctx, x


def case_pendulum(K):
    def run_case():
        res = {}
        ctx, x = pend_context(K)
        small = K < K_CHUNKS
        events_calls(res, "user", ctx, 16, 5, True, small)
        events_calls(res, "user", ctx, 16, 5, False, False)
        events_calls(res, "user", ctx, 16, 4, False, small)
        events_calls(res, "user", ctx, 16, 1, True, False)
        events_calls(res, "user", ctx, 16, 32, K != K_LANES, False)
        events_calls(res, "user", ctx, 1, 4, True, False)
        events_calls(res, "user", ctx, 15, 5, True, False)                        # (the last one the entry with NaN margins)
        if small:
            M = ctx.policy_tail_events_user(15, (0.0,), want_margins=True)["margins"][14]
            assert 0 < np.isnan(M).sum() < K, M                                   # (rollouts on which the entry was never written)
            res["user/margin_14_nan"] = np.isnan(M).astype(np.float64)
        # the same rollouts under quadratic events: ev_eval in front of the same sums
        Q = np.array([[1.0, 0.2, 0.0], [0.0, 0.5, 0.1], [0.0, 0.0, 0.3]])
        evs = [rat.halfspace([1.0, 0.0], -em.between(x[:, :, 0].max(axis=1), 0.6)),
               rat.quadratic_event(Q, [0.1, -0.3, 0.2], -em.between(np.einsum("kti,ij,ktj->kt", x[:, :, :2], Q[:2, :2], x[:, :, :2]).max(axis=1), 0.5)),
               rat.halfspace([0.0, 1.0], -em.between(x[:, PEND_N, 1], 0.7), steps=PEND_N)]
        events_calls(res, "quadratic", ctx, evs, 5, True, small)
        return res
    return run_case


# ---- rollouts without a cost, samples without any ------------------------------------------------------------------------------------------
def case_no_cost():
    """the power law started so close to zero that the noise drives states negative: DomainError rollouts among the others at K = 2049 and
    K = 7; then started below zero: no rollout has a cost"""
    res = {}
    N = 3
    for K in (K_LANES, K_SMALL):
        ctx = rat.Context(rat.PowerLawRiskSensitiveProblem(2, N, 1e-2 * np.eye(2), a=1.3, b=1.5, p=2.5, hconst=1.0), max_batch=1, device=0)
        l, L = 0.2 * np.ones((N, 2)), 0.05 * np.ones((N, 2, 2))
        x_det = ctx.rollout_open(np.array([0.1, 0.1]), l)
        x, u, cost, _ = ctx.rollout_noisy(x_det, l, L, K=K, seed=SEED)
        bad = np.isnan(ctx.policy_evaluate(x_det, l, L, K=K, seed=SEED, want_costs=True)["costs"])
        assert np.array_equal(bad, np.isnan(cost))
        if K == K_LANES:
            assert 0 < bad.sum() < K, bad.sum()
        res[f"K{K}/costs_nan"] = bad.astype(np.float64)
        evs = event_set(x, u, cost, np.random.default_rng(K))
        events_calls(res, f"K{K}/nine", ctx, evs, 5, True, True)
        events_calls(res, f"K{K}/nine", ctx, evs, 4, False, False)
        events_calls(res, f"K{K}/sixteen_linear", ctx, half_spaces(x, cost, 16, N), 1, True, False)
    ctx = rat.Context(rat.PowerLawRiskSensitiveProblem(4, 2, 1e-4 * np.eye(4), a=1.3, b=1.5, p=2.5, hconst=1.0), max_batch=1, device=0)
    assert ctx.policy_evaluate(np.full(4, -0.5), 0.01 * np.ones((2, 4)), K=9, seed=1)["n_ok"] == 0
    ev = [rat.halfspace(np.eye(4)[0], 0.0), rat.quadratic_event(np.eye(8), np.zeros(8), -1.0, steps=1)]
    events_calls(res, "empty", ctx, ev, 5, True, True)
    events_calls(res, "empty", ctx, ev, 1, False, False)
    return res


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------------
def case_refusals():
    """what the four calls refuse of the events, of the partial sums and of the handle, as its text, and the calls after it"""
    res = {}
    N = 3
    prob, x0, _ = rat.synthetic_lq_problem(n=2, m=1, N=N, seed=5, w=0.09)
    ctx = rat.Context(prob, max_batch=1, device=0)
    r = np.random.default_rng(2)
    l, L = 0.5 * r.standard_normal((N, 1)), 0.1 * r.standard_normal((N, 1, 2))
    x_det = ctx.rollout_open(x0, l)
    ev = [rat.halfspace([1.0, 0.0], 0.0)]
    one = dict(want_steps=False, want_margins=False)

    def quad(key, c, evs, refused=True, al=(0.5,)):
        call(res, f"{key}/policy_events/E{len(evs)}", lambda: c.policy_events(evs, kl_bounds=(0.1,), thetas=(0.0,)), refused)
        tail_calls(res, key, c, evs, al, f"E{len(evs)}", one, refused)

    def user(key, c, E, refused=True, al=(0.5,)):
        call(res, f"{key}/policy_events_user/E{E}", lambda: c.policy_events_user(E, kl_bounds=(0.1,), thetas=(0.0,)), refused)
        tail_calls(res, key, c, E, al, f"E{E}", one, refused)

    quad("no_evaluation", ctx, ev)
    ctx.policy_evaluate(x_det, l, L, K=20, seed=1)
    quad("n_event_0", ctx, [])
    quad("n_event_17", ctx, ev * 17)
    quad("window_reversed", ctx, [rat.halfspace([1.0, 0.0], 0.0, steps=(2, 1))])
    quad("window_past_N", ctx, [rat.halfspace([1.0, 0.0], 0.0, steps=N + 1)])
    quad("a_not_finite", ctx, ev + [rat.halfspace([np.nan, 0.0], 0.0)])
    quad("b_not_finite", ctx, [rat.halfspace([1.0, 0.0], np.inf)])
    quad("Q_not_finite", ctx, [rat.quadratic_event(np.array([[1.0, np.inf, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), [0.0, 0.0, 0.0], 0.0)])
    quad("window_before_finiteness", ctx, [rat.halfspace([np.nan, 0.0], 0.0, steps=(2, 1))])
    user("family", ctx, 1)
    quad("after_refusals", ctx, ev, refused=False)
    # the problem changed behind the evaluation: the replay guard's count; the problem back and evaluated again, the calls serve
    p2, _, _ = rat.synthetic_lq_problem(n=2, m=1, N=N, seed=10, w=0.09)
    ctx.set_problem(p2)
    quad("problem_changed", ctx, ev)
    ctx.set_problem(prob)
    ctx.policy_evaluate(x_det, l, L, K=20, seed=1)
    quad("problem_back", ctx, ev, refused=False)
    # the 64 MiB of partial sums, with step_out alone
    long_prob = rat.LQRiskSensitiveProblem(np.eye(2), np.eye(2), Q=np.eye(2), R=np.eye(2), N=4000, W=np.eye(2), Qf=np.eye(2))
    lc = rat.Context(long_prob, max_batch=1, device=0)
    lc.policy_evaluate(np.zeros(2), np.zeros((4000, 2)), K=4, seed=1)
    sixteen = tuple(0.05 * i for i in range(16))
    call(res, "partial_sums/policy_events/steps", lambda: lc.policy_events(ev, kl_bounds=sixteen, want_steps=True), True)
    tail_calls(res, "partial_sums", lc, ev, sixteen, "steps", dict(want_steps=True, want_margins=False), True)
    call(res, "partial_sums/policy_events/no_steps", lambda: lc.policy_events(ev, kl_bounds=sixteen))
    tail_calls(res, "partial_sums", lc, ev, sixteen, "no_steps", one)
    # the user's events: the count, a handle without an evaluation, parameters changed behind one
    src = rat.Context(rat.DeviceSourceProblem(ue.source(um.PEND_DIAG, "half", len(PEND_P)), 2, 1, N, 1e-3 * np.eye(2), params=PEND_P + [0.9]),
                      max_batch=1, device=0)
    user("no_evaluation", src, 1)
    evaluate = lambda: src.policy_evaluate_noise(*um.pend_policy(N), noise=rat.UserNoise(2, 0, seed=SEED), K=20)
    evaluate()
    user("n_event_0", src, 0)
    user("n_event_17", src, 17)
    user("after_refusals", src, 1, refused=False)
    src.set_params([0.1, 0.07, 0.1, 0.9])
    user("set_params", src, 1)
    quad("set_params", src, ev)
    evaluate()
    user("set_params_evaluated", src, 1, refused=False)
    src.policy_evaluate_noise(*um.pend_policy(N), noise=rat.UserNoise(2, 0, zn=np.zeros((4, N, 2))))
    user("injected", src, 1)
    return res


CASES = {
    "lq_12x4_K7": case_lq(K_SMALL),
    "lq_12x4_K2049": case_lq(K_LANES),
    "lq_12x4_two_chunks": case_lq(K_CHUNKS),
    "pendulum_K7": case_pendulum(K_SMALL),
    "pendulum_K2049": case_pendulum(K_LANES),
    "pendulum_two_chunks": case_pendulum(K_CHUNKS),
    "no_cost": case_no_cost,
    "refusals": case_refusals,
}


def run(name):
    return {f"{name}/{k}": v for k, v in CASES[name]().items()}
