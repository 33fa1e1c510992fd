"""rat_policy_rare_event on the device (Context.policy_rare_event; csrc/rare_event.hip) against rat_policy_events bit for bit where the
two coincide, against tests/rare_event_model.py (the NumPy model of the whole call) and against a closed form.

Tolerances.  TOL_MODEL = 1e-12 of the event's scale for per-rollout quantities (margins, log-weights): tests/test_gpu_events.py's figure
for a restated order, and tests/test_gpu_policy_mc.py's for a host rollout of the same dynamics (chains of at most a few hundred
multiply-adds, each ~1e-16 relative per term; 1e-12 leaves decades over that).  They are taken against the model run under the DEVICE's
shift, so that they measure the rollout and not the adaptation.  TOL_SUM = 1e-11 relative for the fixed-order sums (tests/
test_gpu_policy_mc.py: K <= 2^13 terms of one sign err by at most K 2^-53 ~ 1e-12; a decade over that), which is also what the shift --
a ratio of two such sums, taken against sum w |xi| / sum w <= 1 + |s| -- and the trace's |s| are held to against the model's own
adaptation.  The trace's elite effective sample size is a ratio of sums of weights, so it carries the log-weights' error as well:
3 TOL_SUM + 4 TOL_MODEL (1 + max |logw|), derived where it is asserted, against the model under the device's shift of that iteration.
Counts and flags are exact: the helper asserts on the host that every level's order statistic is further than the margins' tolerance
from its neighbours and from zero, and that no final margin is within it of zero, so rounding cannot move a rollout across a boundary."""
import ctypes as C

import numpy as np
import pytest

import ratilqr.jl_amd as rat
import rare_event_model as rm
from ratilqr.jl_amd import _native as nv
from test_cpu_rare_event import K_CLOSED, N_ITER_CLOSED, RHO, SEED, linear_case, linear_event

pytestmark = pytest.mark.gpu
TOL_MODEL, TOL_SUM = 1e-12, 1e-11
ARG, UNSUPPORTED, NO_PROBLEM = 1, 2, 4
DECAY_SOURCE = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) { xn[0] = 0.9 * x[0] + u[0]; }
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) { return x[0] * x[0] + u[0] * u[0]; }
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return x[0] * x[0]; }
"""


def small_case(N=3):
    prob, x, l, L = linear_case()
    p = rat.LQRiskSensitiveProblem(prob.A, prob.B, Q=np.eye(2), R=np.eye(1), N=N, W=np.asarray(prob.Wtab), Qf=np.eye(2))
    return p, x[:N + 1], l[:N], L[:N]


def mid_case():
    """(5, 2, 7), kappa != 0"""
    r = np.random.default_rng(5)
    n, m, N = 5, 2, 7
    A = 0.8 * np.linalg.qr(r.standard_normal((n, n)))[0]
    G = r.standard_normal((n, n))
    prob = rat.LQRiskSensitiveProblem(A, r.standard_normal((n, m)) / np.sqrt(n), Q=np.eye(n), R=np.eye(m), N=N, W=0.02 * (G @ G.T / n + np.eye(n)),
                                      Qf=np.eye(n), kappa=0.01)
    return prob, r.standard_normal(n), 0.1 * r.standard_normal((N, m)), 0.2 * r.standard_normal((N, m, n))


def big_case():
    """(12, 4, 50) with a time-varying dense W"""
    r = np.random.default_rng(7)
    n, m, N = 12, 4, 50
    A = 0.9 * np.linalg.qr(r.standard_normal((n, n)))[0]
    G = r.standard_normal((N, n, n))
    W = 1e-2 * (np.einsum("tij,tkj->tik", G, G) / n + np.eye(n))
    prob = rat.LQRiskSensitiveProblem(A, r.standard_normal((n, m)) / np.sqrt(n), Q=np.eye(n), R=0.1 * np.eye(m), N=N, W=W, Qf=np.eye(n))
    return prob, r.standard_normal(n), 0.1 * r.standard_normal((N, m)), 0.1 * r.standard_normal((N, m, n))


def power_case():
    """(4, 4, 10) power law held so close to zero (x about 0.0115, three standard deviations of a step's noise) that the noise drives some
    states negative: DomainErrors"""
    N = 10
    prob = rat.PowerLawRiskSensitiveProblem(4, N, 1.6e-5 * np.eye(4), a=1.3, b=1.5, p=2.5, hconst=1.0)
    return prob, np.full(4, 0.03), 0.05 * np.ones((N, 4)), 0.05 * np.ones((N, 4, 4))


def closed_loop(ctx, prob, x0, l, L):
    """the policy about the noise-free trajectory from x0"""
    return (np.asarray(x0), l, L) if np.ndim(x0) == 2 else (ctx.rollout_open(x0, l), l, L)


def rarefy(prob, x, l, L, ev0, K, seed, q=0.998):
    """ev0 with b moved so that about 1 - q of the plain rollouts violate it: between two neighbouring margins, never on one"""
    Q, a, b, lo, hi = ev0.dense(prob.n, prob.m, prob.N)
    M = rm.one_pass(prob, x, l, L, (Q, a, b, lo, hi), seed, 0, K, np.zeros((prob.N, prob.n)))[0]
    v = np.sort(M[np.isfinite(M)])
    i = min(int(q * v.size), v.size - 2)
    return rat.Event(Q, a, b - 0.5 * (v[i] + v[i + 1]), (lo, hi))


def scale_of(mdl, ev):
    M = mdl["margins"]
    return abs(ev.b) + (float(np.nanmax(np.abs(M - ev.b))) if np.isfinite(M).any() else 0.0) + np.finfo(float).tiny


def assert_separated(levels, M, sc):
    """the host side of "counts are exact": no boundary of the model -- the levels' order statistics, and zero for the final margins M
    (None: levels only) -- is within the margins' tolerance of a rollout"""
    tol = 10 * TOL_MODEL * sc
    for gamma, code, v, k in levels:
        if code in (2, 3):
            continue
        assert abs(v[k - 1]) > tol
        if k >= 2:
            assert v[k - 1] - v[k - 2] > tol
        if k < v.size:
            assert v[k] - v[k - 1] > tol
    if M is not None:
        assert not np.any(np.abs(M[np.isfinite(M)]) <= tol)


def parity(prob, x, l, L, ev, K, seed, n_iter, rho, label):
    ctx = rat.Context(prob)
    x, l, L = closed_loop(ctx, prob, x, l, L)
    mdl = rm.rare_event(prob, x, l, L, ev, K, seed=seed, n_iter=n_iter, rho=rho)
    sc = scale_of(mdl, ev)
    assert_separated(mdl["levels"], mdl["margins"], sc)
    r = ctx.policy_rare_event(x, l, L, ev, K, seed=seed, n_iter=n_iter, rho=rho, want_margins=True, want_logw=True)
    # the adaptation against the model's own
    assert (r.flag, r.n_iter) == (mdl["flag"], mdl["n_iter"]), label
    s_tol = TOL_SUM * (1.0 + np.abs(mdl["shift"]).max())
    ds = float(np.abs(r.shift - mdl["shift"]).max())
    tr, tm = r.trace, mdl["trace"]
    assert np.array_equal(np.isnan(tr), np.isnan(tm)), label
    run = ~np.isnan(tm[:, 0])
    dl = float(np.abs(tr[run, 0] - tm[run, 0]).max()) if run.any() else 0.0
    upd = ~np.isnan(tm[:, 1])
    print(f"{label}: flag {r.flag} after {r.n_iter} iterations, levels {tm[run, 0]}, |E| {tm[upd, 1]}, PROB {r.prob:.4e} SE {r.prob_se:.2e} "
          f"N_VIOL {r.n_viol} N_DOMAIN {r.n_domain}; shift dev {ds:.2e} (tol {s_tol:.2e}) level dev {dl / sc:.2e}")
    assert ds <= s_tol, label
    assert dl <= 10 * TOL_MODEL * sc + s_tol * sc, label              # a level is a margin under a shift that is off by at most s_tol
    assert np.array_equal(tr[upd, 1], tm[upd, 1]), label              # elite counts
    assert np.allclose(tr[upd, 3], tm[upd, 3], rtol=0, atol=s_tol * np.sqrt(prob.N * prob.n)), label
    # The elite weights of iteration j against the model under the DEVICE's shift of that iteration (the call again with n_iter = j: the
    # passes are keyed by their index alone), so that what is measured is the weights and not the adaptation before them.  The level is
    # then one rollout's margin: TOL_MODEL.  The effective sample size is (sum_E w)^2 / sum_E w^2, w_i = exp(logw_i - max logw): the
    # maximum is one number in both sums and cancels, every logw_i is within d = TOL_MODEL lw_sc of the model's (the bound the final
    # pass's log-weights are held to below), so each w_i is off by at most d relative, (sum w)^2 by 2 d and sum w^2 by 2 d: 4 d; the two
    # fixed-order sums add TOL_SUM each, the first of them squared: 3 TOL_SUM.
    evd = ev.dense(prob.n, prob.m, prob.N)
    s_j = np.zeros((prob.N, prob.n))
    for j in np.flatnonzero(upd):
        if j:
            s_j = ctx.policy_rare_event(x, l, L, ev, K, seed=seed, n_iter=int(j), rho=rho).shift
        Mj, lwj, domj, xij = rm.one_pass(prob, x, l, L, evd, seed, int(j) + 1, K, s_j)
        lvl = rm.level(Mj, rho)
        assert_separated([lvl], None, sc)
        assert lvl[1] == 0 and abs(tr[j, 0] - lvl[0]) <= TOL_MODEL * sc, (label, j)
        _, cnt, ess = rm.adapt(Mj, lwj, domj, xij, s_j, lvl[0])
        ess_tol = 3 * TOL_SUM + 4 * TOL_MODEL * (1.0 + float(np.abs(lwj).max()))
        print(f"{label}: iteration {j} elite ESS {tr[j, 2]:.6f}, dev {abs(tr[j, 2] - ess) / ess:.2e} (tol {ess_tol:.2e})")
        assert tr[j, 1] == cnt and abs(tr[j, 2] - ess) <= ess_tol * ess, (label, j)
    # the final pass against the model under the device's own shift
    fin = rm.rare_event(prob, x, l, L, ev, K, seed=seed, shift=r.shift, n_iter=0)
    Mm, ok = fin["margins"], ~np.isnan(fin["margins"])
    assert np.array_equal(np.isnan(r.margins), ~ok), label
    dm = float(np.abs(r.margins[ok] - Mm[ok]).max() / sc) if ok.any() else 0.0
    lw_sc = 1.0 + float(np.abs(fin["logw"]).max())
    dw = float(np.abs(r.logw - fin["logw"]).max() / lw_sc)
    print(f"{label}: final margins {dm:.2e} logw {dw:.2e} of scale; PROB model {fin['prob']:.6e}")
    assert dm <= TOL_MODEL and dw <= TOL_MODEL, (label, dm, dw)
    assert (r.n_viol, r.n_ok, r.n_domain) == (fin["n_viol"], fin["n_ok"], fin["n_domain"]), label
    for k in ("prob", "prob_se", "ess"):
        assert np.isclose(getattr(r, k), fin[k], rtol=TOL_SUM + 2 * TOL_MODEL * lw_sc, atol=0, equal_nan=True), (label, k, getattr(r, k), fin[k])
    assert abs(r.logw_max - fin["logw_max"]) <= TOL_MODEL * lw_sc and abs(r.logw_min - fin["logw_min"]) <= TOL_MODEL * lw_sc, label
    return r, mdl


# ---- 1. bit anchor ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 16, 1000])
@pytest.mark.parametrize("which", ["small", "big"])
def test_without_shift_the_margins_are_policy_events_bit_for_bit(which, K):
    """shift_in = NULL, n_iter = 0: the final pass is rat_policy_evaluate's noise at the seed, so the margins are rat_policy_events' of that
    evaluation bit for bit (a linear and a quadratic, non-symmetric event), every logw is 0 and PROB is the plain count ratio.  K = 1, 16,
    1000: a single lane group, a full group of sixteen, a ragged last group and a ragged last wavefront."""
    prob, x0, l, L = small_case(3) if which == "small" else big_case()
    ctx = rat.Context(prob)
    x, l, L = closed_loop(ctx, prob, x0, l, L)
    n, m, N = prob.n, prob.m, prob.N
    d = n + m
    r = np.random.default_rng(2)
    Qn = r.standard_normal((d, d))                                    # not symmetric
    ref = ctx.policy_evaluate(x, l, L, K=K, seed=SEED + K, want_costs=True)
    assert ref["n_ok"] == K
    for ev in (rat.halfspace(r.standard_normal(d), 0.1), rat.quadratic_event(Qn, r.standard_normal(d), -float(np.trace(Qn @ Qn.T)) ** 0.5, steps=(1, N))):
        want = ctx.policy_events([ev], thetas=[0.0], want_margins=True)
        got = ctx.policy_rare_event(x, l, L, ev, K, seed=SEED + K, n_iter=0, want_margins=True, want_logw=True)
        assert np.array_equal(got.margins, want["margins"][0]), (which, K)
        assert np.all(got.logw == 0.0) and got.logw_max == 0.0 and got.logw_min == 0.0
        assert got.n_ok == K and got.n_viol == want["thetas"]["n_viol"][0, 0] and got.prob == got.n_viol / got.n_ok
        assert got.flag == nv.RE_NOT_REACHED and got.n_iter == 0 and np.isnan(got.level) and np.all(got.shift == 0.0)


# ---- 2. model parity ----------------------------------------------------------------------------------------------------------------
def test_model_parity_linear_event():
    prob, x, l, L = linear_case()
    ev = rarefy(prob, x, l, L, rat.halfspace(np.array([1.0, 0.5, 0.25]), 0.0, steps=prob.N - 1), 4096, 11)
    r, _ = parity(prob, x, l, L, ev, 4096, 11, 4, 0.1, "(2,1,4) linear")
    assert r.n_iter >= 2


def test_model_parity_disc_event_with_a_non_symmetric_q():
    prob, x0, l, L = mid_case()
    x = rm.rollout(prob, x0, l, None, np.zeros((1, prob.N, prob.n)))[0][0]
    Q = np.zeros((7, 7))
    Q[0, 0] = Q[1, 1] = -1.0
    Q[0, 1], Q[1, 0] = 0.3, -0.3                                      # cancels in z' Q z: the same disc, a Q that is not symmetric
    c = x[prob.N, :2] + np.array([0.9, -0.7])
    a = np.zeros(7)
    a[:2] = 2.0 * c
    ev = rarefy(prob, x, l, L, rat.quadratic_event(Q, a, -float(c @ c), steps=(2, prob.N)), 4096, 12)
    parity(prob, x, l, L, ev, 4096, 12, 4, 0.1, "(5,2,7) disc")


def test_model_parity_full_tile_with_time_varying_w():
    prob, x0, l, L = big_case()
    x = rm.rollout(prob, x0, l, None, np.zeros((1, prob.N, prob.n)))[0][0]
    a = np.random.default_rng(9).standard_normal(16)
    ev = rarefy(prob, x, l, L, rat.halfspace(a, 0.0, steps=(prob.N - 5, prob.N)), 4096, 13)
    parity(prob, x, l, L, ev, 4096, 13, 4, 0.1, "(12,4,50) W(t)")


def test_model_parity_power_law_with_domain_errors():
    prob, x0, l, L = power_case()
    x = rm.rollout(prob, x0, l, None, np.zeros((1, prob.N, prob.n)))[0][0]
    ev = rarefy(prob, x, l, L, rat.halfspace(np.array([1.0, -0.5, 0.0, 0.25]), 0.0, steps=(1, prob.N)), 4096, 14)
    r, mdl = parity(prob, x, l, L, ev, 4096, 14, 4, 0.1, "power law (4,4,10)")
    assert 0 < r.n_domain < 4096


# ---- 3. closed form -----------------------------------------------------------------------------------------------------------------
def test_closed_form_on_the_device_where_plain_monte_carlo_sees_nothing():
    """p = Phi(-4.7534) ~ 1e-6 exactly (tests/test_cpu_rare_event.py), K = 2^16, at the seed the model was checked with"""
    prob, x, l, L = linear_case()
    ev, exact = linear_event(1e-6)
    ctx = rat.Context(prob)
    r = ctx.policy_rare_event(x, l, L, ev, K_CLOSED, seed=SEED, n_iter=N_ITER_CLOSED, rho=RHO)
    print(f"p = {exact:.6e}: PROB {r.prob:.6e} SE {r.prob_se:.3e} ({abs(r.prob - exact) / r.prob_se:.2f} sigma), SE/PROB {r.prob_se / r.prob:.3e} "
          f"against plain {np.sqrt((1 - exact) / (exact * K_CLOSED)):.3e}, {r.n_iter} iterations, ESS {r.ess:.0f}")
    assert r.flag == nv.RE_OK
    assert abs(r.prob - exact) <= 5.0 * r.prob_se
    ctx.policy_evaluate(x, l, L, K=K_CLOSED, seed=SEED)
    plain = ctx.policy_events([ev], thetas=[0.0])
    assert plain["thetas"]["n_viol"][0, 0] == 0                      # the gap this call fills


# ---- 4. edges -----------------------------------------------------------------------------------------------------------------------
def test_deterministic_windows_and_an_unreachable_event():
    prob, x, l, L = linear_case()
    ctx = rat.Context(prob)
    N, K = prob.N, 1000
    ex = np.array([1.0, 0.0, 0.0])
    for ev, p in ((rat.halfspace(ex, 1.0 - x[0, 0], steps=0), 1.0), (rat.halfspace(ex, -1.0 - x[0, 0], steps=0), 0.0),      # x_0 is no random variable
                  (rat.halfspace(np.array([0.0, 0.0, 1.0]), 0.5, steps=N), 1.0), (rat.halfspace(np.array([0.0, 0.0, 1.0]), -0.5, steps=N), 0.0)):   # u_N = 0
        r = ctx.policy_rare_event(x, l, L, ev, K, seed=3, n_iter=2, rho=0.1, want_margins=True)
        assert r.prob == p and r.prob_se == 0.0 and np.all(r.margins == (1.0 if p else -1.0) * (1.0 if ev.steps == 0 else 0.5))
        assert r.flag == (nv.RE_OK if p else nv.RE_NOT_REACHED) and r.n_viol == (K if p else 0)
    r = ctx.policy_rare_event(x, l, L, rat.halfspace(np.zeros(3), -1.0), K, seed=3, n_iter=3, rho=0.1)
    assert r.flag == nv.RE_NOT_REACHED and r.prob == 0.0 and r.n_iter == 3 and r.level == -1.0


def raw(ctx, x, l, L, K=64, seed=1, Q=None, a=None, b=0.0, lo=0, hi=0, shift=None, n_iter=1, rho=0.1, null_a=False, null_stats=False):
    stats = np.zeros(nv.RE_NSTAT)
    a = nv.f64(np.zeros(ctx.n + ctx.m) if a is None else a)
    return nv.lib().rat_policy_rare_event(ctx.h, nv.P(nv.f64(x)), nv.P(nv.f64(l)), nv.P(nv.cm3(L)), C.c_int64(K), C.c_uint64(seed),
                                          nv.P(None if Q is None else nv.f64(Q)), None if null_a else nv.P(a), C.c_double(b), C.c_int32(lo), C.c_int32(hi),
                                          nv.P(None if shift is None else nv.f64(shift)), C.c_int32(n_iter), C.c_double(rho),
                                          None if null_stats else nv.P(stats), None, None, None, None)


def test_refusals():
    prob, x, l, L = linear_case()
    ctx = rat.Context(prob)
    N, bad = prob.N, np.array([1.0, np.inf, 0.0])
    assert raw(ctx, x, l, L) == 0
    for kw in (dict(K=0), dict(K=(1 << 27) + 1), dict(n_iter=-1), dict(n_iter=33), dict(rho=0.0), dict(rho=0.500001), dict(rho=float("nan")),
               dict(lo=-1), dict(lo=2, hi=1), dict(hi=N + 1), dict(a=bad), dict(b=float("nan")), dict(Q=np.full((3, 3), np.nan)),
               dict(shift=np.full((N, 2), np.inf)), dict(null_a=True), dict(null_stats=True)):
        assert raw(ctx, x, l, L, **kw) == ARG, kw
    assert raw(ctx, x, l, L, hi=N) == 0                               # the handle stays usable
    wide = rat.LQRiskSensitiveProblem(0.5 * np.eye(14), np.ones((14, 1)), Q=np.eye(14), R=np.eye(1), N=3, W=np.eye(14), Qf=np.eye(14))
    assert raw(rat.Context(wide), np.zeros((4, 14)), np.zeros((3, 1)), np.zeros((3, 1, 14))) == UNSUPPORTED
    # a source model: the shift is defined on the family rollout
    src = rat.DeviceSourceProblem(DECAY_SOURCE, 1, 1, 3, 1e-2 * np.eye(1))
    assert raw(rat.Context(src), np.zeros((4, 1)), np.zeros((3, 1)), np.zeros((3, 1, 1))) == UNSUPPORTED
    # a handle without a problem
    assert raw(rat.Context(None), np.zeros((4, 2)), np.zeros((3, 1)), np.zeros((3, 1, 2)), a=np.zeros(3)) == NO_PROBLEM
    # a horizon whose shift does not fit the kernel's LDS copy: N = 256 runs, 257 is refused
    for N_long, rc in ((256, 0), (257, UNSUPPORTED)):
        long = rat.LQRiskSensitiveProblem(prob.A, prob.B, Q=np.eye(2), R=np.eye(1), N=N_long, W=1e-2 * np.eye(2), Qf=np.eye(2))
        assert raw(rat.Context(long), np.zeros((N_long + 1, 2)), np.zeros((N_long, 1)), np.zeros((N_long, 1, 2)), hi=N_long) == rc, N_long


def test_the_recorded_evaluation_still_replays_and_the_call_repeats_its_bits():
    prob, x0, l, L = mid_case()
    ctx = rat.Context(prob)
    x, l, L = closed_loop(ctx, prob, x0, l, L)
    ev = rat.halfspace(np.eye(7)[0], -x[prob.N, 0] - 0.8, steps=prob.N)
    ref = ctx.policy_evaluate(x, l, L, K=777, seed=5, thetas=[0.1], want_costs=True)
    before = ctx.policy_events([ev], kl_bounds=[0.05], thetas=[0.0], want_margins=True)
    tilt = ctx.policy_worst_case(thetas=[0.1])["thetas"]
    a = ctx.policy_rare_event(x, l, L, ev, 3000, seed=9, n_iter=3, rho=0.2, want_margins=True, want_logw=True)
    b = ctx.policy_rare_event(x, l, L, ev, 3000, seed=9, n_iter=3, rho=0.2, want_margins=True, want_logw=True)
    for k in ("prob", "prob_se", "ess", "n_viol", "n_ok", "n_domain", "logw_max", "logw_min", "flag", "n_iter", "level"):
        assert getattr(a, k) == getattr(b, k), k
    for k in ("shift", "trace", "margins", "logw"):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), k
    after = ctx.policy_events([ev], kl_bounds=[0.05], thetas=[0.0], want_margins=True)
    assert np.array_equal(before["margins"], after["margins"])
    for part in ("bounds", "thetas"):
        for k in before[part]:
            assert np.array_equal(before[part][k], after[part][k], equal_nan=True), (part, k)
    again = ctx.policy_worst_case(thetas=[0.1])["thetas"]                # the recorded costs, read by another call
    for k in tilt:
        assert np.array_equal(tilt[k], again[k], equal_nan=True), k
    assert ref["n_ok"] == 777
