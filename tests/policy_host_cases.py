"""Cases of tests/test_gpu_policy_host_parent.py, shared with tests/golden/make_policy_host_golden.py (which records what the commit BEFORE
the policy analyses shared their host path computed on them: tests/golden/policy_host_parent.npz).

The policy entry points of csrc/driver.cpp -- rat_rollout_noisy, rat_policy_evaluate, rat_policy_evaluate_noise and, on the stored costs,
rat_policy_worst_case, rat_policy_tail_risk, rat_policy_worst_case_trajectory, rat_policy_events, and rat_policy_rare_event -- pack the
policy, chunk the rollouts, key the chunks and reduce the costs through one set of helpers, so the tests that hold one analysis to another
bit for bit no longer see a mistake inside a helper.  These cases are the smallest at which the packing can go wrong: n = 3, m = 2, N = 5
(padding live in every dimension, an odd horizon for the Box-Muller pair tail), W constant and time-varying, closed and open loop (the pack
then holds x_0 alone), injected draws and the generator, K = 70 (no multiple of 4 or 16, one chunk) and K = 2^16 + 37 (two chunks: the chunk
key and the + k0 offsets); the power law with and without DomainErrors; a general size (the dense pack); a source model under N(0, W) and
one under its own rat_user_noise with two normals and one uniform per step.

run(name) -> {key: array or str}, per call its layout and values (flatten).  A call the library refuses is recorded as its error text
(return code name and rat_last_error); UNEXPECTED collects the refusals a case did not expect, and the successes where it expected one,
for the recorder to print.  An array of more than 4096 elements is kept as the SHA-256 of its bytes and its first and last eight values."""
import dataclasses
import hashlib

import numpy as np

import ratilqr.jl_amd as rat
import user_noise_model as um
from test_gpu_source_model import LQ_SOURCE

K_SMALL, K_TWO_CHUNKS = 70, (1 << 16) + 37
THETAS = (0.0, 0.3, 1.0)
ENTRY_POINTS = ("rollout_noisy", "policy_evaluate", "policy_evaluate_noise", "policy_worst_case", "policy_tail_risk",
                "policy_worst_case_trajectory", "policy_events", "policy_rare_event")
UNEXPECTED = []


# ---- recording ----------------------------------------------------------------------------------------------------------------------
def flatten(out):
    """One call's result -- arrays, scalars, nested dicts / tuples / dataclasses of them -- as (layout, values): a line per array (name,
    dtype, shape, and the SHA-256 of its bytes where it has more than 4096 elements) and every array's elements in that order as float64
    (counts and flags are exact there), the first and last eight of a hashed one."""
    lines, vals = [], []

    def walk(key, v):
        if v is None:
            return
        if dataclasses.is_dataclass(v):
            v = dataclasses.asdict(v)
        if isinstance(v, dict):
            for k, w in v.items():
                walk(f"{key}/{k}" if key else str(k), w)
        elif isinstance(v, (tuple, list)):
            for i, w in enumerate(v):
                walk(f"{key}/{i}" if key else str(i), w)
        else:
            a = np.ascontiguousarray(v)
            line = f"{key} {a.dtype} {a.shape}"
            if a.size > 4096:
                line += " sha256=" + hashlib.sha256(a.tobytes()).hexdigest()
                a = np.concatenate([a.ravel()[:8], a.ravel()[-8:]])
            lines.append(line)
            vals.append(a.ravel().astype(np.float64))

    walk("", out)
    return "\n".join(lines), np.concatenate(vals) if vals else np.zeros(0)


def call(res, key, fn, refused=False):
    """Record fn()'s result under key/layout and key/values, or the refusal's text under key/error; refused: whether the case expects a
    refusal."""
    try:
        res[key + "/layout"], res[key + "/values"] = flatten(fn())
        ok = True
    except rat.RatError as e:
        res[key + "/error"] = str(e)
        ok = False
    if ok == refused:
        UNEXPECTED.append(key + (": expected a refusal" if ok else ": refused, " + res[key + "/error"]))
    return ok


# ---- what runs on the stored costs, and the rare event ---------------------------------------------------------------------------------
def events_for(n, m):
    d = n + m
    Q = np.diag(np.linspace(1.0, 2.0, d))
    Q[0, d - 1] = 0.3                                               # not symmetric: Q is used as given
    return [rat.halfspace(np.eye(n)[0], -0.2), rat.quadratic_event(Q, -0.1 * np.ones(d), -1.5, steps=(1, 3))]


def stored_costs(res, key, ctx, replay_refused):
    """rat_policy_worst_case (two bounds, one theta, weights), rat_policy_tail_risk, and the two replays, on the last evaluation's costs"""
    call(res, f"{key}/policy_worst_case", lambda: ctx.policy_worst_case(kl_bounds=(0.1, 1.0), thetas=(0.5,), want_weights=True))
    call(res, f"{key}/policy_tail_risk", lambda: ctx.policy_tail_risk((0.5, 0.9), want_weights=True))
    call(res, f"{key}/policy_worst_case_trajectory", lambda: ctx.policy_worst_case_trajectory(kl_bounds=(0.1, 1.0), thetas=(0.5,)), replay_refused)
    call(res, f"{key}/policy_events", lambda: ctx.policy_events(events_for(ctx.n, ctx.m), kl_bounds=(0.1, 1.0), thetas=(0.5,), want_steps=True,
                                                                 want_margins=True), replay_refused)


def rare_event(res, key, ctx, x_nom, l, L, K, refused):
    lin, quad = events_for(ctx.n, ctx.m)
    shift = 0.05 * np.arange(1, ctx.N * ctx.n + 1, dtype=float).reshape(ctx.N, ctx.n) / (ctx.N * ctx.n)
    for name, ev, s in (("linear", lin, None), ("quadratic_shifted", quad, shift)):
        call(res, f"{key}/policy_rare_event/{name}",
             lambda: ctx.policy_rare_event(x_nom, l, L, ev, K, seed=5, shift=s, n_iter=2, rho=0.2, want_margins=True, want_logw=True), refused)


def w_noise_calls(res, key, ctx, x_nom, l, L, K, inject, source=False, rare=True):
    """every entry point that draws from N(0, W(k)), on one policy: injected draws (seeded here) or the generator"""
    wide = ctx.n > 12 or ctx.m > 4
    z = np.random.default_rng(41).standard_normal((K, ctx.N, ctx.n)) if inject else None
    call(res, f"{key}/rollout_noisy", lambda: ctx.rollout_noisy(x_nom, l, L, K=K, z=z, seed=9), refused=source)
    call(res, f"{key}/policy_evaluate", lambda: ctx.policy_evaluate(x_nom, l, L, thetas=THETAS, K=K, z=z, seed=9, want_costs=True))
    stored_costs(res, key, ctx, replay_refused=wide or inject or source)
    if rare:
        rare_event(res, key, ctx, x_nom, l, L, K, refused=wide or source)


# ---- the problems ---------------------------------------------------------------------------------------------------------------------
def lq_parts(W_tv):
    """The LQ + cubic problem at (3, 2, 5), every cost term scaled by 1 + 0.05 k so that LQ_SOURCE restates it; W dense, so its factor is not
    diagonal.  (family problem, source problem, x_nom, l, L)"""
    rng = np.random.default_rng(2)
    n, m, N = 3, 2, 5
    A, B = 0.9 * np.linalg.qr(rng.standard_normal((n, n)))[0], rng.standard_normal((n, m)) / np.sqrt(n)
    Q, R, P = np.eye(n), 0.3 * np.eye(m), 0.05 * rng.standard_normal((m, n))
    qv, rv, q0, kap, Qf = 0.1 * rng.standard_normal(n), 0.1 * rng.standard_normal(m), 0.2, 0.02, np.eye(n)
    G = rng.standard_normal((N, n, n))
    W = 1e-2 * (np.einsum("tij,tkj->tik", G, G) / n + np.eye(n))
    W = W if W_tv else W[0]
    s = 1.0 + 0.05 * np.arange(N)
    fam = rat.LQRiskSensitiveProblem(A, B, Q=s[:, None, None] * Q, R=s[:, None, None] * R, P=s[:, None, None] * P, qv=s[:, None] * qv,
                                     rv=s[:, None] * rv, q0=s * q0, N=N, W=W, Qf=Qf, kappa=kap)
    params = np.concatenate([A.T.ravel(), B.T.ravel(), Q.T.ravel(), R.T.ravel(), P.T.ravel(), qv, rv, [q0, kap], Qf.T.ravel()])
    src = rat.DeviceSourceProblem(LQ_SOURCE, n, m, N, W, params=params)
    return fam, src, rng.standard_normal((N + 1, n)), 0.3 * rng.standard_normal((N, m)), 0.2 * rng.standard_normal((N, m, n))


def case_lq(W_tv):
    def run_case():
        res = {}
        fam, _, x_nom, l, L = lq_parts(W_tv)
        ctx = rat.Context(fam)
        for closed in (True, False):
            for inject in (True, False):
                xa, La = (x_nom, L) if closed else (x_nom[0], None)
                w_noise_calls(res, f"{'closed' if closed else 'open'}/{'injected' if inject else 'generator'}", ctx, xa, l, La, K_SMALL, inject)
        return res
    return run_case


def case_lq_two_chunks():
    res = {}
    fam, _, x_nom, l, L = lq_parts(False)
    w_noise_calls(res, "closed/generator", rat.Context(fam), x_nom, l, L, K_TWO_CHUNKS, False)
    return res


def case_powerlaw():
    """a parameter set that stays in the domain, and one whose noise drives some states below zero (DomainError flags on 23 or 24 of the
    70 rollouts)"""
    res = {}
    N = 5
    for name, w, x0 in (("in_domain", 1e-4, [0.6, 0.4]), ("domain_errors", 1e-2, [0.1, 0.1])):
        ctx = rat.Context(rat.PowerLawRiskSensitiveProblem(2, N, w * np.eye(2), a=1.3, b=1.5, p=2.5, hconst=1.0))
        l, L = 0.2 * np.ones((N, 2)), 0.05 * np.ones((N, 2, 2))
        w_noise_calls(res, f"{name}/open", ctx, np.array(x0), l, None, K_SMALL, False)
        w_noise_calls(res, f"{name}/closed", ctx, ctx.rollout_open(np.array(x0), l), l, L, K_SMALL, False, rare=False)
    return res


def case_general_size():
    res = {}
    prob, x0, u = rat.synthetic_lq_problem(n=14, m=5, N=4, seed=3, kappa=0.02, w=1e-2)
    ctx = rat.Context(prob)
    rng = np.random.default_rng(4)
    x_nom, l, L = rng.standard_normal((5, 14)), 0.3 * rng.standard_normal((4, 5)), 0.1 * rng.standard_normal((4, 5, 14))
    for closed in (True, False):
        for inject in (True, False):
            xa, La = (x_nom, L) if closed else (x_nom[0], None)
            w_noise_calls(res, f"{'closed' if closed else 'open'}/{'injected' if inject else 'generator'}", ctx, xa, l, La, K_SMALL, inject,
                          rare=closed and inject)
    return res


def case_source_w_noise():
    res = {}
    for W_tv in (False, True):
        _, src, x_nom, l, L = lq_parts(W_tv)
        ctx = rat.Context(src)
        for closed, inject in ((True, True), (True, False), (False, False)):
            xa, La = (x_nom, L) if closed else (x_nom[0], None)
            w_noise_calls(res, f"W_tv{int(W_tv)}/{'closed' if closed else 'open'}/{'injected' if inject else 'generator'}", ctx, xa, l, La,
                          K_SMALL, inject, source=True, rare=closed and inject and not W_tv)
    return res


PEND_N, PEND_P = 5, [0.1, 0.02, 0.03, 0.25, 0.2]


def pend_ctx(W=None):
    return rat.Context(rat.DeviceSourceProblem(um.PEND_MIX, 2, 1, PEND_N, 1e-3 * np.eye(2) if W is None else W, params=PEND_P))


def user_noise(K, inject, seed=77):
    if not inject:
        return rat.UserNoise(2, 1, seed=seed)
    rng = np.random.default_rng(43)
    return rat.UserNoise(2, 1, zn=rng.standard_normal((K, PEND_N, 2)), zu=rng.random((K, PEND_N, 1)))


def case_user_noise(K):
    def run_case():
        res = {}
        ctx = pend_ctx()
        x_nom, l, L = um.pend_policy(PEND_N)
        for closed in (True, False):
            for inject in (True, False):
                key = f"{'closed' if closed else 'open'}/{'injected' if inject else 'generator'}"
                xa, La = (x_nom, L) if closed else (x_nom[0], None)
                call(res, f"{key}/policy_evaluate_noise", lambda: ctx.policy_evaluate_noise(xa, l, La, noise=user_noise(K, inject), thetas=THETAS,
                                                                                             K=K, want_costs=True, want_trajectories=True))
                stored_costs(res, key, ctx, replay_refused=inject)
        # without the trajectories the generator runs in one launch
        call(res, "closed/generator_one_launch/policy_evaluate_noise",
             lambda: ctx.policy_evaluate_noise(x_nom, l, L, noise=user_noise(K, False), thetas=THETAS, K=K, want_costs=True))
        return res
    return run_case


def case_refusals():
    """bad calls on live handles, and that the handle serves the next valid call"""
    res = {}
    fam, _, x_nom, l, L = lq_parts(False)
    ctx = rat.Context(fam)
    px, pl, pL = um.pend_policy(PEND_N)
    pend = pend_ctx()
    for name, kw in (("n_theta_17", dict(thetas=np.zeros(17), K=4)), ("negative_theta", dict(thetas=(0.5, -0.1), K=4)), ("K_0", dict(K=0))):
        call(res, f"{name}/policy_evaluate", lambda: ctx.policy_evaluate(x_nom, l, L, seed=1, **kw), refused=True)
        call(res, f"{name}/policy_evaluate_noise", lambda: pend.policy_evaluate_noise(px, pl, pL, noise=rat.UserNoise(2, 1, seed=1), **kw), refused=True)
    call(res, "after_refusals/policy_evaluate", lambda: ctx.policy_evaluate(x_nom, l, L, thetas=THETAS, K=K_SMALL, seed=9, want_costs=True))
    # a W that is not positive definite on a source problem whose N(0, W) kernel no call has compiled yet: refused before anything is
    # compiled or grown; rat_user_noise does not read W; and with a proper W the same handle evaluates
    bad = pend_ctx(W=np.array([[1.0, 2.0], [2.0, 1.0]]))
    call(res, "non_pd_W/policy_evaluate", lambda: bad.policy_evaluate(px, pl, pL, thetas=THETAS, K=K_SMALL, seed=3, want_costs=True), refused=True)
    call(res, "non_pd_W/policy_evaluate_noise", lambda: bad.policy_evaluate_noise(px, pl, pL, noise=user_noise(K_SMALL, False), thetas=THETAS,
                                                                                  K=K_SMALL, want_costs=True))
    bad.set_problem(rat.DeviceSourceProblem(um.PEND_MIX, 2, 1, PEND_N, 1e-3 * np.eye(2), params=PEND_P))
    call(res, "non_pd_W/then_pd/policy_evaluate", lambda: bad.policy_evaluate(px, pl, pL, thetas=THETAS, K=K_SMALL, seed=3, want_costs=True))
    # an injected stream is missing
    zn = np.random.default_rng(3).standard_normal((4, PEND_N, 2))
    call(res, "missing_stream/policy_evaluate_noise", lambda: pend.policy_evaluate_noise(px, pl, pL, noise=rat.UserNoise(2, 1, zn=zn), K=4), refused=True)
    # a replay after the parameters changed: the replayed costs are no longer the evaluation's
    call(res, "set_params/policy_evaluate_noise", lambda: pend.policy_evaluate_noise(px, pl, pL, noise=user_noise(K_SMALL, False), thetas=THETAS,
                                                                                     K=K_SMALL, want_costs=True))
    pend.set_params([0.1, 0.04, 0.03, 0.25, 0.2])
    call(res, "set_params/policy_worst_case_trajectory", lambda: pend.policy_worst_case_trajectory(kl_bounds=(0.1,)), refused=True)
    call(res, "set_params/policy_events", lambda: pend.policy_events(events_for(2, 1), kl_bounds=(0.1,)), refused=True)
    return res


CASES = {
    "lq": case_lq(False),
    "lq_W_tv": case_lq(True),
    "lq_two_chunks": case_lq_two_chunks,
    "powerlaw": case_powerlaw,
    "general_size": case_general_size,
    "source_w_noise": case_source_w_noise,
    "user_noise": case_user_noise(K_SMALL),
    "user_noise_two_chunks": case_user_noise(K_TWO_CHUNKS),
    "refusals": case_refusals,
}


def run(name):
    return {f"{name}/{k}": v for k, v in CASES[name]().items()}
