"""Safety events the user writes, on the device (rat_policy_events_user / Context.policy_events_user: rat_src_user_events of
csrc/source_events.h; rat_policy_rare_event_user / Context.policy_rare_event_user: csrc/source_rare.h under RAT_RARE_USER_EVENT).

The test events of tests/user_event_model.py are single IEEE operations, so NumPy gives the device's bits: margins are compared bit for
bit.  The weighted slots go through tests/events_model.py's own reduction (user_event_model.reduce) and its compare helper `deviation`
under tests/test_gpu_events.py's bound for a restated order, TOL_MODEL = 1e-12 (of the event's scale for MARGIN_MEAN: every g here is
a coordinate minus a parameter, or a min / max of such, so |g| <= max |z| + max |q|); counts and MARGIN_MAX are exact.  A half-space
through the user path and through rat_policy_events (a = e_0, b = -q) is the same in every bit: 1 x_0 plus exact zeros plus b is
x_0 - q, and both paths share ev_sums and ev_final.

An event's parameters sit behind the model's in p.  The tests size them from the evaluation's own trajectories and set them with
set_params afterwards: the replay guard holds the replayed COSTS against the stored ones, and an event parameter moves no cost."""
import ctypes as C

import numpy as np
import pytest

import ratilqr.jl_amd as rat
import events_model as em
import user_event_model as ue
from ratilqr.jl_amd import _native as nv
from test_cpu_rare_event import K_CLOSED, N_ITER_CLOSED, RHO
from test_cpu_user_event import N_WALK, SEED_WALK, walk_case
from test_gpu_events import TOL_MODEL, both
from wc_trajectory_model import weights_from_rows

pytestmark = pytest.mark.gpu
ARG, UNSUPPORTED = 1, 2
KS = (1, 63, 65, (1 << 16) + 5)
BOUNDS, THETAS = (0.1,), (0.0,)


def evaluated(which, name, N, K, seed=11, q=None):
    """a context of the source `which` with the event `name`, evaluated under its sampler: (ctx, prob, policy, noise, evaluation, evoff)"""
    case, npn = ue.CASES[which]
    prob, x_nom, l, L, off = case(name, N, q)
    ctx = rat.Context(prob)
    noise = rat.UserNoise(npn, 0, seed=seed)
    r = ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=K, want_costs=True, want_trajectories=True)
    return ctx, prob, (x_nom, l, L), noise, r, off


def set_event(ctx, prob, off, q):
    ctx.set_params(np.concatenate([prob.params[:off], q]))


# ---- 1. against the model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box", "moving", "window", "16"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", [1, 8])
@pytest.mark.parametrize("which", ["di", "lq"])
def test_against_the_model(which, N, K, name):
    """K: a lone rollout, both sides of a wavefront, two replay chunks with a tail.  N = 1: the window 3 .. 5 never opens (NaN margins,
    probability 0); N = 8: it opens and closes inside the horizon."""
    ctx, prob, _, _, r, off = evaluated(which, name, N, K)
    x, u, costs = r["x"], r["u"], r["costs"]
    q = ue.thresholds(name, x, u, costs)
    set_event(ctx, prob, off, q)
    E = ue.BODIES[name][1]
    out = ctx.policy_events_user(E, kl_bounds=BOUNDS, thetas=THETAS, want_steps=True, want_margins=True)
    wc = ctx.policy_worst_case(kl_bounds=BOUNDS, thetas=THETAS)
    for part in ("bounds", "thetas"):
        for k in wc[part]:
            assert np.array_equal(out[part][k], wc[part][k], equal_nan=True), (part, k)
    o = both(out)
    g = ue.g_user(name, x, u, q)
    y, dead = weights_from_rows(costs, o["theta"], o["flag"])
    mdl = ue.reduce(g, costs, y, dead)
    assert out["margins"].shape == (E, K)
    assert np.array_equal(out["margins"], mdl["margins"][:E], equal_nan=True)                 # bit for bit; NaN meets NaN
    ok = ~np.isnan(costs)
    zmax = max(float(np.abs(x[ok]).max()), float(np.abs(u[ok]).max())) if ok.any() else 0.0
    sc = np.full(E + 1, zmax + float(np.abs(q).max()))
    dp, dm = em.deviation(o, mdl, sc, N)
    viol = int(o["n_viol"][0, E])
    print(f"{which} N={N} K={K} {name}: {viol} of {int(ok.sum())} violate some event; model prob {dp:.2e} margin mean {dm:.2e}")
    assert dp <= TOL_MODEL and dm <= TOL_MODEL, (dp, dm)
    for r_ in range(o["theta"].size):
        assert np.array_equal(o["n_viol"][r_], mdl["n_viol"][r_]) and np.array_equal(o["margin_max"][r_], mdl["margin_max"][r_], equal_nan=True)
        for e in range(E + 1):
            d_row = max(BOUNDS[r_] if r_ < len(BOUNDS) else o["kl"][r_], 0.0)
            assert o["prob_robust"][r_, e] == rat.kl_event_bound(o["n_viol"][r_, e] / int(ok.sum()), d_row)
    if name == "window" and N == 1 or name == "16":                   # an event that is never written: NaN margins, probability 0
        e = 0 if name == "window" else 15
        assert np.isnan(out["margins"][e]).all() and np.all(o["prob"][:, e] == 0.0) and np.all(o["n_viol"][:, e] == 0)
    if K >= 63 and not (name == "window" and N == 1):
        assert viol > 0                                               # the thresholds sit inside the spread
    bare = both(ctx.policy_events_user(E, kl_bounds=BOUNDS, thetas=THETAS))                   # without per-step sums and margins: the same slots
    for k in ("prob", "prob_se", "margin_mean", "margin_max", "first_mean", "n_viol", "prob_robust"):
        assert np.array_equal(bare[k], o[k], equal_nan=True), k


# ---- 2. against the quadratic path, bit for bit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,steps", [("half", None), ("window", (3, 5))])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("which", ["di", "lq"])
def test_a_half_space_is_rat_policy_events_in_every_bit(which, K, name, steps):
    N = 8
    ctx, prob, _, _, r, off = evaluated(which, name, N, K, seed=12)
    q = ue.thresholds(name, r["x"], r["u"], r["costs"])
    set_event(ctx, prob, off, q)
    kw = dict(kl_bounds=BOUNDS, thetas=THETAS, want_steps=True, want_margins=True)
    got = ctx.policy_events_user(1, **kw)
    want = ctx.policy_events([rat.halfspace(np.eye(prob.n)[0], -q[0], steps=steps)], **kw)
    assert np.array_equal(got["margins"], want["margins"], equal_nan=True)
    for part in ("bounds", "thetas"):
        for k in want[part]:
            assert np.array_equal(got[part][k], want[part][k], equal_nan=True), (part, k)
    assert np.array_equal(got["margins"], ctx.policy_events_user(1, **kw)["margins"], equal_nan=True)


# ---- 3. the rare-event call -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 63, 65, 1000])
@pytest.mark.parametrize("which", ["di", "lq"])
def test_without_shift_the_margins_are_policy_events_users(which, K):
    """n_iter = 0, no shift: plain Monte Carlo on rat_policy_evaluate_noise's noise at the seed -- every row of E_16 (the one on u, the one
    never written) and the box, bit for bit; every logw is 0"""
    N = 8
    for name, picks in (("16", (0, 3, 13, 14, 15)), ("box", (0,))):
        ctx, prob, (x, l, L), noise, r, off = evaluated(which, name, N, K, seed=13)
        set_event(ctx, prob, off, ue.thresholds(name, r["x"], r["u"], r["costs"]))
        E = ue.BODIES[name][1]
        want = ctx.policy_events_user(E, thetas=THETAS, want_margins=True)
        for e in picks:
            got = ctx.policy_rare_event_user(x, l, L, E, e, K, noise=noise, n_iter=0, want_margins=True, want_logw=True)
            assert np.array_equal(got.margins, want["margins"][e], equal_nan=True), (name, e)
            assert np.all(got.logw == 0.0) and got.n_ok == K and got.n_viol == want["thetas"]["n_viol"][0, e]
            assert got.flag == nv.RE_NOT_REACHED and got.n_iter == 0 and got.shift.shape == (N, noise.normals_per_step)
        if K == 1000:                                                 # every packing of the kernel: lanes beyond tpw hold no rollout
            for tpw in (16, 32):
                ctx.debug_set("src_mc_tpw", tpw)
                again = ctx.policy_rare_event_user(x, l, L, E, picks[-1], K, noise=noise, n_iter=0, want_margins=True)
                assert np.array_equal(again.margins, want["margins"][picks[-1]], equal_nan=True), tpw
            ctx.debug_set("src_mc_tpw", 64)


def same_result(a, b):
    for k in ("prob", "prob_se", "ess", "n_viol", "n_ok", "n_domain", "logw_max", "logw_min", "flag", "n_iter", "level"):
        assert getattr(a, k) == getattr(b, k) or (getattr(a, k) != getattr(a, k) and getattr(b, k) != getattr(b, k)), k
    for k in ("shift", "trace", "margins", "logw"):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), k


@pytest.mark.parametrize("which", ["di", "lq"])
def test_the_adapted_call_is_rat_policy_rare_event_noise_in_every_bit(which):
    """E_half at n_iter = 3 against the same half-space through rat_policy_rare_event_noise: stats, trace, shift, margins, logw"""
    N, K = 8, 4096
    ctx, prob, (x, l, L), noise, r, off = evaluated(which, "half", N, K, seed=14)
    q = np.array([em.between(r["x"][:, :, 0].max(axis=1), 0.995)])    # rare enough for the level to climb
    set_event(ctx, prob, off, q)
    kw = dict(noise=noise, seed=5, n_iter=3, rho=0.1, want_margins=True, want_logw=True)
    a = ctx.policy_rare_event_user(x, l, L, 1, 0, K, **kw)
    b = ctx.policy_rare_event_noise(x, l, L, rat.halfspace(np.eye(prob.n)[0], -q[0]), K, **kw)
    same_result(a, b)
    assert a.n_iter >= 2 and np.any(a.shift != 0.0) and np.any(a.logw != 0.0)
    same_result(a, ctx.policy_rare_event_user(x, l, L, 1, 0, K, **kw))                        # two calls return the same bits


def test_closed_form_where_plain_monte_carlo_sees_nothing():
    """the random walk's x_N - c > 0 at p = Phi(-4.7534) ~ 1e-6, K = 2^16, at the seed the reference estimator was checked with
    (tests/test_cpu_user_event.py)"""
    mod, x0, l, c, exact = walk_case()
    prob = rat.DeviceSourceProblem(ue.source(ue.WALK, "half_at", 2), 1, 1, N_WALK, np.eye(1), params=np.concatenate([ue.WALK_P, [c, N_WALK]]))
    ctx = rat.Context(prob)
    noise = rat.UserNoise(1, 0, seed=SEED_WALK)
    r = ctx.policy_rare_event_user(x0, l, None, 1, 0, K_CLOSED, noise=noise, n_iter=N_ITER_CLOSED, rho=RHO)
    print(f"p = {exact:.6e}: PROB {r.prob:.6e} SE {r.prob_se:.3e} ({abs(r.prob - exact) / r.prob_se:.2f} sigma), "
          f"{r.n_iter} iterations, ESS {r.ess:.0f}")
    assert r.flag == nv.RE_OK
    assert abs(r.prob - exact) <= 5.0 * r.prob_se
    ctx.policy_evaluate_noise(x0, l, None, noise=noise, K=K_CLOSED)
    assert ctx.policy_events_user(1, thetas=THETAS)["thetas"]["n_viol"][0, 0] == 0            # the gap this call fills


# ---- 4. refusals and state -------------------------------------------------------------------------------------------------------------------
def raw_events(ctx, n_event, n_theta=1):
    rows, ev = np.zeros((n_theta, nv.WC_NSTAT)), np.zeros((n_theta, 18, nv.EV_NSTAT))
    return nv.lib().rat_policy_events_user(ctx.h, C.c_int32(n_event), None, C.c_int32(0), nv.P(np.zeros(max(n_theta, 1))), C.c_int32(n_theta),
                                           nv.P(rows), nv.P(ev), None, None)


def raw_rare(ctx, x, l, L, n_event=1, event=0, K=64, npn=2, n_iter=1):
    stats = np.zeros(nv.RE_NSTAT)
    return nv.lib().rat_policy_rare_event_user(ctx.h, nv.P(nv.f64(x)), nv.P(nv.f64(l)), nv.P(nv.cm3(L)), C.c_int64(K), C.c_int32(npn), C.c_int32(0),
                                               C.c_uint64(1), C.c_int32(n_event), C.c_int32(event), None, C.c_int32(n_iter), C.c_double(0.1),
                                               nv.P(stats), None, None, None, None)


def last_error():
    return nv.lib().rat_last_error().decode()


def test_refusals_and_the_handle_goes_on():
    N, K = 4, 100
    ctx, prob, (x, l, L), noise, r, off = evaluated("di", "half", N, K, q=[0.5])
    assert raw_events(ctx, 1) == 0 and raw_rare(ctx, x, l, L) == 0
    # n_event and event outside their ranges
    for ne in (0, 17, -1):
        assert raw_events(ctx, ne) == ARG and raw_rare(ctx, x, l, L, n_event=ne) == ARG, ne
    for e in (-1, 1):
        assert raw_rare(ctx, x, l, L, n_event=1, event=e) == ARG, e
    assert raw_events(ctx, 1, n_theta=0) == ARG                       # rat_policy_events' own: no row
    assert raw_rare(ctx, x, l, L, npn=0) == ARG and raw_rare(ctx, x, l, L, npn=13) == UNSUPPORTED and raw_rare(ctx, x, l, L, K=0) == ARG
    good = ctx.policy_events_user(1, thetas=THETAS, want_margins=True)
    # not a source model
    fam, x0, u0 = rat.synthetic_lq_problem(n=2, m=1, N=N, seed=3, w=1e-2)
    fc = rat.Context(fam)
    fc.policy_evaluate(x0, u0, K=8, seed=1)
    assert raw_events(fc, 1) == UNSUPPORTED and "not a source model" in last_error()
    assert raw_rare(fc, x, l, L) == UNSUPPORTED and "not a source model" in last_error()
    # a source without the event: the message says what to define; the handle still answers rat_policy_events
    plain = rat.Context(rat.DeviceSourceProblem(ue.DI, 2, 1, N, 1e-3 * np.eye(2), params=ue.DI_P))
    plain.policy_evaluate_noise(x, l, L, noise=noise, K=K)
    assert raw_events(plain, 1) == ARG and "RAT_USER_EVENT" in last_error() and "rat_user_event(k, x, u, g, p)" in last_error()
    assert raw_rare(plain, x, l, L) == ARG and "RAT_USER_EVENT" in last_error()
    ev = [rat.halfspace([1.0, 0.0], -0.5)]
    assert np.array_equal(plain.policy_events(ev, thetas=THETAS, want_margins=True)["margins"], good["margins"])
    # a compile error in the event that only the event kernels meet (the whole text is compiled when the problem is set, so a plain syntax
    # error is refused there; RAT_N_EVENT is defined for the event kernels alone): a source that insists on its own n_event.  The log
    # names the line of the user's text, and the handle stays usable
    guard = "#if defined(RAT_N_EVENT) && RAT_N_EVENT != 2\n#error \"this event is written for n_event == 2\"\n#endif\n"
    src = ue.source(ue.DI + guard, "half", 3)
    line = src[:src.index("#error")].count("\n") + 1
    pk = rat.Context(rat.DeviceSourceProblem(src, 2, 1, N, 1e-3 * np.eye(2), params=np.concatenate([ue.DI_P, [0.5]])))
    pk.policy_evaluate_noise(x, l, L, noise=noise, K=K)
    for rc in (raw_events(pk, 1), raw_rare(pk, x, l, L, n_event=1)):
        assert rc == ARG and f"model.hip:{line}:" in last_error() and "written for n_event == 2" in last_error(), last_error()
    assert np.array_equal(pk.policy_events(ev, thetas=THETAS, want_margins=True)["margins"], good["margins"])
    assert raw_events(pk, 2) == 0 and raw_rare(pk, x, l, L, n_event=2) == 0
    assert np.array_equal(pk.policy_events_user(2, thetas=THETAS, want_margins=True)["margins"][0], good["margins"][0])
    # an evaluation under N(0, W), and one on injected draws: rat_policy_events' own refusals
    ctx.policy_evaluate(x, l, L, K=16, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rat_user_noise"):
        ctx.policy_events_user(1, thetas=THETAS)
    ctx.policy_evaluate_noise(x, l, L, noise=rat.UserNoise(2, 0, zn=np.zeros((4, N, 2))))
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*injected"):
        ctx.policy_events_user(1, thetas=THETAS)
    fresh = rat.Context(prob)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no evaluation"):
        fresh.policy_events_user(1, thetas=THETAS)
    # a parameter the dynamics read, changed after the evaluation: the replay guard; an event parameter alone moves no cost
    ctx.policy_evaluate_noise(x, l, L, noise=noise, K=K)
    again = ctx.policy_events_user(1, thetas=THETAS, want_margins=True)
    assert np.array_equal(again["margins"], good["margins"])          # two calls, two evaluations at one seed: the same bits
    ctx.set_params(np.concatenate([[0.2], prob.params[1:]]))
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*changed since the evaluation"):
        ctx.policy_events_user(1, thetas=THETAS)
    ctx.set_params(np.concatenate([prob.params[:off], [0.25]]))
    moved = ctx.policy_events_user(1, thetas=THETAS, want_margins=True)
    assert np.array_equal(moved["margins"][0], ue.per_rollout(ue.g_user("half", r["x"], r["u"], [0.25]), r["costs"])[0][0])


def test_another_n_event_compiles_another_module_on_the_same_handle():
    """E_16's source asked for 15 events: entry 15 is beyond RAT_N_EVENT and simply not read; asked for 16 again, the same bits as before"""
    ctx, prob, _, _, r, off = evaluated("di", "16", 8, 65, seed=15)
    set_event(ctx, prob, off, ue.thresholds("16", r["x"], r["u"], r["costs"]))
    a = ctx.policy_events_user(16, thetas=THETAS, want_margins=True)
    b = ctx.policy_events_user(15, thetas=THETAS, want_margins=True)
    c = ctx.policy_events_user(16, thetas=THETAS, want_margins=True)
    assert np.array_equal(a["margins"][:15], b["margins"], equal_nan=True) and np.array_equal(a["margins"], c["margins"], equal_nan=True)
    for k in ("prob", "n_viol", "margin_mean"):
        assert np.array_equal(a["thetas"][k][:, :15], b["thetas"][k][:, :15], equal_nan=True), k
        assert np.array_equal(a["thetas"][k][:, 16], b["thetas"][k][:, 15], equal_nan=True), k   # "any" loses nothing with the unwritten event
