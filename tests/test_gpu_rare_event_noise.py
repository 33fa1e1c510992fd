"""rat_policy_rare_event_noise on the device (Context.policy_rare_event_noise; csrc/source_rare.h, re_elite_rng of csrc/rare_event.hip)
against rat_policy_events behind rat_policy_evaluate_noise bit for bit where the two coincide, against tests/rare_event_noise_model.py
(the NumPy model of the whole call) and against the closed form of tests/test_cpu_rare_event_noise.py.

Tolerances are tests/test_gpu_rare_event.py's, justified there: TOL_MODEL = 1e-12 of the event's scale for per-rollout quantities, taken
against the model under the DEVICE's shift; TOL_SUM = 1e-11 relative for the fixed-order sums, the shift and the trace's |s|; the elite
effective sample size 3 TOL_SUM + 4 TOL_MODEL (1 + max |logw|).  Counts and flags are exact: the same host-side separation asserts."""
import ctypes as C

import numpy as np
import pytest

import ratilqr.jl_amd as rat
import rare_event_model as rm
import rare_event_noise_model as nm
import user_noise_model as um
from ratilqr.jl_amd import _native as nv
from test_cpu_rare_event import K_CLOSED, N_ITER_CLOSED, RHO, linear_case, linear_event
from test_cpu_rare_event_noise import SEED
from test_gpu_rare_event import TOL_MODEL, TOL_SUM, assert_separated, scale_of

pytestmark = pytest.mark.gpu
ARG, UNSUPPORTED, NO_PROBLEM = 1, 2, 4


def pend_problem(src, N, params):
    return rat.DeviceSourceProblem(src, 2, 1, N, 1e-3 * np.eye(2), params=params)


def pend_case(N=5):
    """PEND_STATE (2, 1, N): three normals a step -- an odd count, the spare Box-Muller output"""
    x_nom, l, L = um.pend_policy(N)
    mod = nm.Model(nm.pend_f, nm.pend_state_noise, um.PEND_STATE_P, 2, 1, N, 3, c=um.pend_c, h=um.pend_h)
    return pend_problem(um.PEND_STATE, N, um.PEND_STATE_P), mod, rat.UserNoise(3, 0), x_nom, l, L


def lq_case(N=3):
    """the 12 x 4 LQ_GAUSS source: twelve normals a step through chol(W)"""
    gp = um.lq_generative(Nh=N)
    prob = um.lq_source_problem(gp, source=um.LQ_GAUSS, mean=False)
    f, noise = nm.lq_gauss_model(gp)
    r = np.random.default_rng(21)
    x_nom = 0.3 * r.standard_normal((N + 1, 12))
    return prob, nm.Model(f, noise, prob.params, 12, 4, N, 12), rat.UserNoise(12, 0), x_nom, 0.1 * r.standard_normal((N, 4)), 0.1 * r.standard_normal((N, 4, 12))


CASES = {"pend": pend_case, "lq": lq_case}


def two_events(d, N):
    r = np.random.default_rng(2)
    Qn = r.standard_normal((d, d))                                    # not symmetric
    return (rat.halfspace(r.standard_normal(d), 0.1),
            rat.quadratic_event(Qn, r.standard_normal(d), -float(np.trace(Qn @ Qn.T)) ** 0.5, steps=(1, N)))


# ---- 1. bit anchor ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 17, 64, 65, 1000])
@pytest.mark.parametrize("which", ["pend", "lq"])
def test_without_shift_the_margins_are_policy_events_bit_for_bit(which, K):
    """shift = None, n_iter = 0: the final pass is rat_policy_evaluate_noise's generator at the seed, so the margins are rat_policy_events'
    of that evaluation bit for bit (a half-space and a quadratic, non-symmetric event over (1, N)), every logw is 0 and PROB is the plain
    count ratio.  K: a lone lane, a ragged group of sixteen, a full wavefront, one lane into the next wavefront, a ragged tail."""
    prob, _, noise, x, l, L = CASES[which]()
    ctx = rat.Context(prob)
    seed = SEED + K
    ref = ctx.policy_evaluate_noise(x, l, L, noise=rat.UserNoise(noise.normals_per_step, 0, seed=seed), K=K, want_costs=True)
    assert ref["n_ok"] == K
    for ev in two_events(prob.n + prob.m, prob.N):
        want = ctx.policy_events([ev], thetas=[0.0], want_margins=True)
        got = ctx.policy_rare_event_noise(x, l, L, ev, K, noise=noise, seed=seed, n_iter=0, want_margins=True, want_logw=True)
        assert np.array_equal(got.margins, want["margins"][0]), (which, K)
        assert np.all(got.logw == 0.0) and got.logw_max == 0.0 and got.logw_min == 0.0
        assert got.n_ok == K and got.n_viol == want["thetas"]["n_viol"][0, 0] and got.prob == got.n_viol / got.n_ok
        assert got.flag == nv.RE_NOT_REACHED and got.n_iter == 0 and np.isnan(got.level) and np.all(got.shift == 0.0)
        assert got.shift.shape == (prob.N, noise.normals_per_step)
        if K == 1000:                                                 # every packing of the kernel: lanes beyond tpw hold no rollout
            for tpw in (16, 32):
                ctx.debug_set("src_mc_tpw", tpw)
                assert np.array_equal(ctx.policy_rare_event_noise(x, l, L, ev, K, noise=noise, seed=seed, n_iter=0, want_margins=True).margins,
                                      got.margins), tpw
            ctx.debug_set("src_mc_tpw", 64)


# ---- 2. K-independence --------------------------------------------------------------------------------------------------------------
def test_a_rollouts_noise_does_not_depend_on_k():
    """across the 2^16 staging boundary of the parent calls: the first 1000 margins at K = 2^16 + 3 are the margins at K = 1000"""
    prob, _, noise, x, l, L = pend_case()
    ctx = rat.Context(prob)
    ev = two_events(3, prob.N)[1]
    shift = 0.1 * np.random.default_rng(4).standard_normal((prob.N, 3))
    for s in (None, shift):
        a = ctx.policy_rare_event_noise(x, l, L, ev, 1000, noise=noise, seed=7, shift=s, n_iter=0, want_margins=True, want_logw=True)
        b = ctx.policy_rare_event_noise(x, l, L, ev, (1 << 16) + 3, noise=noise, seed=7, shift=s, n_iter=0, want_margins=True, want_logw=True)
        assert np.array_equal(a.margins, b.margins[:1000]) and np.array_equal(a.logw, b.logw[:1000])
        assert np.unique(b.margins[-8:]).size == 8


# ---- 3. model parity ----------------------------------------------------------------------------------------------------------------
def rarefy(mod, x, l, L, ev0, K, seed, q=0.998):
    """ev0 with b moved so that about 1 - q of the plain rollouts violate it: between two neighbouring margins, never on one"""
    Q, a, b, lo, hi = ev0.dense(mod.n, mod.m, mod.N)
    M = nm.one_pass(mod, x, l, L, (Q, a, b, lo, hi), seed, 0, K, np.zeros((mod.N, mod.P)))[0]
    v = np.sort(M[np.isfinite(M)])
    i = min(int(q * v.size), v.size - 2)
    return rat.Event(Q, a, b - 0.5 * (v[i] + v[i + 1]), (lo, hi))


def parity(prob, mod, noise, x, l, L, ev, K, seed, n_iter, rho, label):
    """tests/test_gpu_rare_event.parity for the noise call"""
    ctx = rat.Context(prob)
    call = lambda **kw: ctx.policy_rare_event_noise(x, l, L, ev, K, noise=noise, seed=seed, rho=rho, **kw)
    mdl = nm.rare_event_noise(mod, x, l, L, ev, K, seed=seed, n_iter=n_iter, rho=rho)
    sc = scale_of(mdl, ev)
    assert_separated(mdl["levels"], mdl["margins"], sc)
    r = call(n_iter=n_iter, want_margins=True, want_logw=True)
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
    assert np.allclose(tr[upd, 3], tm[upd, 3], rtol=0, atol=s_tol * np.sqrt(mod.N * mod.P)), label
    # the elite weights of iteration j against the model under the DEVICE's shift of that iteration (the call again with n_iter = j)
    evd = ev.dense(mod.n, mod.m, mod.N)
    s_j = np.zeros((mod.N, mod.P))
    for j in np.flatnonzero(upd):
        if j:
            s_j = call(n_iter=int(j)).shift
        Mj, lwj, domj, xij = nm.one_pass(mod, x, l, L, evd, seed, int(j) + 1, K, s_j)
        lvl = rm.level(Mj, rho)
        assert_separated([lvl], None, sc)
        assert lvl[1] == 0 and abs(tr[j, 0] - lvl[0]) <= TOL_MODEL * sc, (label, j)
        _, cnt, ess = rm.adapt(Mj, lwj, domj, xij, s_j, lvl[0])
        ess_tol = 3 * TOL_SUM + 4 * TOL_MODEL * (1.0 + float(np.abs(lwj).max()))
        print(f"{label}: iteration {j} elite ESS {tr[j, 2]:.6f}, dev {abs(tr[j, 2] - ess) / ess:.2e} (tol {ess_tol:.2e})")
        assert tr[j, 1] == cnt and abs(tr[j, 2] - ess) <= ess_tol * ess, (label, j)
    # the final pass against the model under the device's own shift
    fin = nm.rare_event_noise(mod, x, l, L, ev, K, seed=seed, shift=r.shift, n_iter=0)
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


def test_model_parity_pendulum_half_space_on_the_angle():
    prob, mod, noise, x, l, L = pend_case()
    ev = rarefy(mod, x, l, L, rat.halfspace(np.array([1.0, 0.0, 0.0]), 0.0, steps=(1, prob.N)), 4096, 11)
    r, _ = parity(prob, mod, noise, x, l, L, ev, 4096, 11, 3, 0.1, "pendulum (2,1,5), 3 normals")
    assert r.n_iter >= 2 and np.any(r.shift != 0.0)


def test_model_parity_full_tile_with_a_non_symmetric_q():
    prob, mod, noise, x, l, L = lq_case()
    r = np.random.default_rng(6)
    Q = 0.2 * r.standard_normal((16, 16))                             # not symmetric
    ev = rarefy(mod, x, l, L, rat.quadratic_event(Q, r.standard_normal(16), 0.0, steps=(1, prob.N)), 4096, 12)
    parity(prob, mod, noise, x, l, L, ev, 4096, 12, 3, 0.1, "LQ_GAUSS (12,4,3), 12 normals")


# ---- 4. closed form -----------------------------------------------------------------------------------------------------------------
def test_closed_form_on_the_device_where_plain_monte_carlo_sees_nothing():
    """p = Phi(-4.7534) ~ 1e-6 exactly, K = 2^16, at the seed the model was checked with (tests/test_cpu_rare_event_noise.py)"""
    prob, x, l, L = linear_case()
    ev, exact = linear_event(1e-6)
    ctx = rat.Context(nm.lin_source_problem(prob))
    noise = rat.UserNoise(2, 0, seed=SEED)
    r = ctx.policy_rare_event_noise(x, l, L, ev, K_CLOSED, noise=noise, n_iter=N_ITER_CLOSED, rho=RHO)
    print(f"p = {exact:.6e}: PROB {r.prob:.6e} SE {r.prob_se:.3e} ({abs(r.prob - exact) / r.prob_se:.2f} sigma), SE/PROB {r.prob_se / r.prob:.3e} "
          f"against plain {np.sqrt((1 - exact) / (exact * K_CLOSED)):.3e}, {r.n_iter} iterations, ESS {r.ess:.0f}")
    assert r.flag == nv.RE_OK
    assert abs(r.prob - exact) <= 5.0 * r.prob_se
    ctx.policy_evaluate_noise(x, l, L, noise=noise, K=K_CLOSED)
    plain = ctx.policy_events([ev], thetas=[0.0])
    assert plain["thetas"]["n_viol"][0, 0] == 0                      # the gap this call fills
    assert rat.rare_event_probability_noise(nm.lin_source_problem(prob), x, l, L, ev, noise, K=K_CLOSED, n_iter=N_ITER_CLOSED, rho=RHO).prob == r.prob


# ---- 5. edges -----------------------------------------------------------------------------------------------------------------------
def test_domain_errors_of_the_sampler_are_counted():
    """PEND_NAN: a NaN disturbance beyond three standard deviations -- the rollouts rat_policy_evaluate_noise counts in n_domain"""
    N, K = 5, 4096
    x_nom, l, L = um.pend_policy(N)
    ctx = rat.Context(pend_problem(um.PEND_NAN, N, [0.1, 0.05]))
    ref = ctx.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(1, 0, seed=9), K=K, want_costs=True)
    assert 0 < ref["n_domain"] < K
    r = ctx.policy_rare_event_noise(x_nom, l, L, rat.halfspace(np.array([0.0, 1.0, 0.0]), 0.0), K, noise=rat.UserNoise(1, 0, seed=9), n_iter=0,
                                    want_margins=True)
    assert np.array_equal(np.isnan(r.margins), np.isnan(ref["costs"]))
    assert (r.n_domain, r.n_ok) == (ref["n_domain"], ref["n_ok"]) and r.flag == nv.RE_NOT_REACHED


def test_an_overdraw_is_an_argument_error_and_the_handle_stays_usable():
    N, K = 4, 100
    x_nom, l, L = um.pend_policy(N)
    ctx = rat.Context(pend_problem(um.PEND_OVER, N, [0.1, 0.03, 0.05]))
    ev = rat.halfspace(np.array([1.0, 0.0, 0.0]), -1.2)
    with pytest.raises(rat.RatError, match=r"RAT_ERR_ARG.*normals_per_step = 2, uniforms_per_step = 0"):
        ctx.policy_rare_event_noise(x_nom, l, L, ev, K, noise=rat.UserNoise(2, 0, seed=3), n_iter=2)
    r = ctx.policy_rare_event_noise(x_nom, l, L, ev, K, noise=rat.UserNoise(3, 0, seed=3), n_iter=2)
    assert r.n_ok == K and r.shift.shape == (N, 3)


def test_deterministic_window_and_an_unreachable_event():
    prob, _, noise, x, l, L = pend_case()
    ctx = rat.Context(prob)
    K, ex = 1000, np.array([1.0, 0.0, 0.0])
    for ev, p in ((rat.halfspace(ex, 1.0 - x[0, 0], steps=0), 1.0), (rat.halfspace(ex, -1.0 - x[0, 0], steps=0), 0.0)):   # x_0 is no random variable
        r = ctx.policy_rare_event_noise(x, l, L, ev, K, noise=noise, seed=3, n_iter=2, rho=0.1, want_margins=True)
        assert r.prob == p and r.prob_se == 0.0 and np.all(r.margins == r.margins[0]) and abs(r.margins[0] - (1.0 if p else -1.0)) < 1e-15
        assert r.flag == (nv.RE_OK if p else nv.RE_NOT_REACHED) and r.n_viol == (K if p else 0)
    r = ctx.policy_rare_event_noise(x, l, L, rat.halfspace(np.zeros(3), -1.0), K, noise=noise, seed=3, n_iter=3, rho=0.1)
    assert r.flag == nv.RE_NOT_REACHED and r.prob == 0.0 and r.n_iter == 3 and r.level == -1.0


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def raw(ctx, x, l, L, K=64, npn=3, npu=0, seed=1, Q=None, a=None, b=0.0, lo=0, hi=0, shift=None, n_iter=1, rho=0.1, null_a=False, null_stats=False):
    stats = np.zeros(nv.RE_NSTAT)
    a = nv.f64(np.zeros(ctx.n + ctx.m) if a is None else a)
    return nv.lib().rat_policy_rare_event_noise(ctx.h, nv.P(nv.f64(x)), nv.P(nv.f64(l)), nv.P(nv.cm3(L)), C.c_int64(K), C.c_int32(npn), C.c_int32(npu),
                                                C.c_uint64(seed), nv.P(None if Q is None else nv.f64(Q)), None if null_a else nv.P(a), C.c_double(b),
                                                C.c_int32(lo), C.c_int32(hi), nv.P(None if shift is None else nv.f64(shift)), C.c_int32(n_iter),
                                                C.c_double(rho), None if null_stats else nv.P(stats), None, None, None, None)


def test_refusals():
    prob, _, _, x, l, L = pend_case()
    ctx = rat.Context(prob)
    N, bad = prob.N, np.array([1.0, np.inf, 0.0])
    assert raw(ctx, x, l, L) == 0
    for kw in (dict(K=0), dict(K=(1 << 27) + 1), dict(n_iter=-1), dict(n_iter=33), dict(rho=0.0), dict(rho=0.500001), dict(rho=float("nan")),
               dict(lo=-1), dict(lo=2, hi=1), dict(hi=N + 1), dict(a=bad), dict(b=float("nan")), dict(Q=np.full((3, 3), np.nan)),
               dict(shift=np.full((N, 3), np.inf)), dict(null_a=True), dict(null_stats=True), dict(npn=0), dict(npn=-1), dict(npu=-1)):
        assert raw(ctx, x, l, L, **kw) == ARG, kw
    assert raw(ctx, x, l, L, npn=13) == UNSUPPORTED
    assert raw(ctx, x, l, L, npn=2) == ARG                            # PEND_STATE draws three: an overdraw
    assert raw(ctx, x, l, L, hi=N) == 0                               # the handle stays usable
    # the old call on the same source handle: still refused
    stats = np.zeros(nv.RE_NSTAT)
    assert nv.lib().rat_policy_rare_event(ctx.h, nv.P(nv.f64(x)), nv.P(nv.f64(l)), nv.P(nv.cm3(L)), C.c_int64(64), C.c_uint64(1), None,
                                          nv.P(nv.f64(np.zeros(3))), C.c_double(0.0), C.c_int32(0), C.c_int32(0), None, C.c_int32(1),
                                          C.c_double(0.1), nv.P(stats), None, None, None, None) == UNSUPPORTED
    # a source without a sampler: the compiler's log
    plain = rat.Context(pend_problem(um.PEND_PLAIN, N, [0.1]))
    assert raw(plain, x, l, L, npn=2) == ARG and "RAT_USER_NOISE" in nv.lib().rat_last_error().decode()
    # not a source model: a family, a general size, no problem
    fam, xf, lf, Lf = linear_case()
    assert raw(rat.Context(fam), xf, lf, Lf, npn=2) == UNSUPPORTED
    wide = rat.LQRiskSensitiveProblem(0.5 * np.eye(14), np.ones((14, 1)), Q=np.eye(14), R=np.eye(1), N=3, W=np.eye(14), Qf=np.eye(14))
    assert raw(rat.Context(wide), np.zeros((4, 14)), np.zeros((3, 1)), np.zeros((3, 1, 14))) == UNSUPPORTED
    assert raw(rat.Context(None), np.zeros((4, 2)), np.zeros((3, 1)), np.zeros((3, 1, 2)), a=np.zeros(3)) == NO_PROBLEM
    # the horizon limit of the existing call: N = 256 runs, 257 is refused
    for N_long, rc in ((256, 0), (257, UNSUPPORTED)):
        long = rat.Context(pend_problem(um.PEND_STATE, N_long, um.PEND_STATE_P))
        assert raw(long, np.tile(x[0], (N_long + 1, 1)), np.zeros((N_long, 1)), np.zeros((N_long, 1, 2)), hi=N_long) == rc, N_long
    with pytest.raises(ValueError):
        ctx.policy_rare_event_noise(x, l, L, rat.halfspace(np.zeros(3), -1.0), 4, noise=rat.UserNoise(3, 0, zn=np.zeros((4, N, 3))))


# ---- 7. the recorded evaluation, and the same bits twice ------------------------------------------------------------------------------
def test_the_recorded_evaluation_still_replays_and_the_call_repeats_its_bits():
    prob, mod, noise, x, l, L = pend_case()
    ctx = rat.Context(prob)
    ev = rarefy(mod, x, l, L, rat.halfspace(np.array([1.0, 0.0, 0.0]), 0.0, steps=prob.N), 3000, 9, q=0.99)   # rare enough to adapt
    ref = ctx.policy_evaluate_noise(x, l, L, noise=rat.UserNoise(3, 0, seed=5), K=777, thetas=[0.1], want_costs=True)
    before = ctx.policy_events([ev], kl_bounds=[0.05], thetas=[0.0], want_margins=True)
    a = ctx.policy_rare_event_noise(x, l, L, ev, 3000, noise=noise, seed=9, n_iter=3, rho=0.2, want_margins=True, want_logw=True)
    b = ctx.policy_rare_event_noise(x, l, L, ev, 3000, noise=noise, seed=9, n_iter=3, rho=0.2, want_margins=True, want_logw=True)
    for k in ("prob", "prob_se", "ess", "n_viol", "n_ok", "n_domain", "logw_max", "logw_min", "flag", "n_iter", "level"):
        assert getattr(a, k) == getattr(b, k), k
    for k in ("shift", "trace", "margins", "logw"):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), k
    assert a.n_iter >= 1 and np.any(a.shift != 0.0)
    after = ctx.policy_events([ev], kl_bounds=[0.05], thetas=[0.0], want_margins=True)
    assert np.array_equal(before["margins"], after["margins"])
    for part in ("bounds", "thetas"):
        for k in before[part]:
            assert np.array_equal(before[part][k], after[part][k], equal_nan=True), (part, k)
    assert ref["n_ok"] == 777
