"""rat_policy_rare_event_params on the device (Context.policy_rare_event_params; csrc/source_params.h under RAT_PARAM_SHIFT, csrc/source_rare.h,
re_elite_rng and re_update of csrc/rare_event.hip): against rat_policy_rare_event_noise / _user bit for bit where the parameter shift is
zero and not adapted, against tests/rare_event_params_model.py (the NumPy model of the whole call), against the closed forms of
tests/test_cpu_rare_event_params.py at the seeds confirmed there, and every refusal.

Tolerances are tests/test_gpu_rare_event.py's, justified there: TOL_MODEL = 1e-12 of the event's scale for per-rollout quantities, taken
against the model under the DEVICE's shifts; TOL_SUM = 1e-11 relative for the fixed-order sums, both shifts and both norms.  Counts and
flags are exact: the same host-side separation asserts.

Shapes: the pendulum (2, 1, N = 5, three step normals) and the 12 x 4 source (N = 3, twelve normals and a uniform) of
tests/user_params_model.py, two parameter normals and a parameter uniform; no K above the existing rare-event tests'."""
import ctypes as C
import types

import numpy as np
import pytest

import rare_event_model as rm
import rare_event_params_model as rp
import ratilqr.jl_amd as rat
import user_params_model as pm
from ratilqr.jl_amd import _native as nv
from test_gpu_rare_event import TOL_MODEL, TOL_SUM, assert_separated, scale_of

pytestmark = pytest.mark.gpu
ARG, UNSUPPORTED, NO_PROBLEM = 1, 2, 4
SAMPLING = lambda: rat.ParamSampling(pm.PARAM_NORMALS, pm.PARAM_UNIFORMS)


def context(c, p=None):
    ctx = rat.Context(rat.DeviceSourceProblem(c.source, c.n, c.m, c.N, c.W, params=c.p if p is None else p))
    ctx.set_param_sampling(SAMPLING())
    return ctx


@pytest.fixture(scope="module")
def cases():
    return {name: rp.ParityCase(name) for name in ("pend", "lq12")}


def same(a, b, label):
    for k in ("prob", "prob_se", "ess", "n_viol", "n_ok", "n_domain", "logw_max", "logw_min", "flag", "n_iter", "level"):
        assert getattr(a, k) == getattr(b, k) or (np.isnan(getattr(a, k)) and np.isnan(getattr(b, k))), (label, k)
    for k in ("shift", "trace", "margins", "logw"):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), (label, k)


# ---- 5. bit anchor ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 17, 64, 65, 1000])
@pytest.mark.parametrize("name", ["pend", "lq12"])
def test_a_zero_parameter_shift_that_is_not_adapted_returns_the_existing_calls_bits(cases, name, K):
    """sampling on, pshift_in zeros, adapt = "step": margins, logw, stats, shift and trace of policy_rare_event_user (n_event = 1) and of
    policy_rare_event_noise (n_event = 0) at the same seed, bit for bit; param_shift and param_trace all zeros"""
    c = cases[name]
    ctx = context(c)
    x, l, L = c.policy
    noise = rat.UserNoise(c.npn, c.npu, seed=40 + K)
    r = np.random.default_rng(K)
    ev = rat.halfspace(r.standard_normal(c.n + c.m), 0.1, steps=(1, c.N))
    kw = dict(noise=noise, n_iter=2, rho=0.2, want_margins=True, want_logw=True)
    zero = np.zeros(pm.PARAM_NORMALS)
    for tpw in ((64, 16, 32) if K == 1000 else (64,)):
        ctx.debug_set("src_mc_tpw", tpw)
        for want, got in ((ctx.policy_rare_event_user(x, l, L, 1, 0, K, **kw),
                           ctx.policy_rare_event_params(x, l, L, 0, K, n_event=1, param_shift=zero, adapt="step", **kw)),
                          (ctx.policy_rare_event_noise(x, l, L, ev, K, **kw),
                           ctx.policy_rare_event_params(x, l, L, ev, K, param_shift=None, adapt="step", **kw))):
            same(want, got, (name, K, tpw))
            assert got.param_shift.shape == (pm.PARAM_NORMALS,) and np.all(got.param_shift == 0.0)
            assert got.param_trace.shape == (2,) and np.all(got.param_trace[~np.isnan(got.trace[:, 3])] == 0.0)
            assert np.array_equal(np.isnan(got.param_trace), np.isnan(got.trace[:, 3]))
    ctx.debug_set("src_mc_tpw", 64)


# ---- 6. model parity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pend", "lq12"])
def test_model_parity_on_an_event_that_reads_a_drawn_parameter(cases, name):
    c = cases[name]
    K, seed, n_iter, rho = 4096, 11 if name == "pend" else 12, 3, 0.1
    p = c.rarefied(K, seed)
    mod, ctx = c.model(p), context(c, p)
    x, l, L = c.policy
    noise = rat.UserNoise(c.npn, c.npu)
    call = lambda **kw: ctx.policy_rare_event_params(x, l, L, 0, K, noise=noise, seed=seed, rho=rho, n_event=1, **kw)
    mdl = rp.rare_event_params(mod, x, l, L, None, K, seed=seed, n_iter=n_iter, rho=rho)
    ev = types.SimpleNamespace(b=0.0)
    sc = scale_of(mdl, ev)
    assert_separated(mdl["levels"], mdl["margins"], sc)
    r = call(n_iter=n_iter, want_margins=True, want_logw=True)
    assert (r.flag, r.n_iter) == (mdl["flag"], mdl["n_iter"]), name
    s_tol = TOL_SUM * (1.0 + max(np.abs(mdl["shift"]).max(), np.abs(mdl["param_shift"]).max()))
    ds, dp = float(np.abs(r.shift - mdl["shift"]).max()), float(np.abs(r.param_shift - mdl["param_shift"]).max())
    tr, tm = r.trace, mdl["trace"]
    assert np.array_equal(np.isnan(tr), np.isnan(tm)) and np.array_equal(np.isnan(r.param_trace), np.isnan(mdl["param_trace"])), name
    run, upd = ~np.isnan(tm[:, 0]), ~np.isnan(tm[:, 1])
    dl = float(np.abs(tr[run, 0] - tm[run, 0]).max()) if run.any() else 0.0
    print(f"{name}: flag {r.flag} after {r.n_iter} iterations, levels {tm[run, 0]}, |E| {tm[upd, 1]}, PROB {r.prob:.4e} SE {r.prob_se:.2e} N_VIOL "
          f"{r.n_viol}; shift dev {ds:.2e} param shift {r.param_shift} dev {dp:.2e} (tol {s_tol:.2e}) level dev {dl / sc:.2e}")
    assert ds <= s_tol and dp <= s_tol, name
    assert dl <= 10 * TOL_MODEL * sc + s_tol * sc, name
    assert np.array_equal(tr[upd, 1], tm[upd, 1]), name                # elite counts
    assert np.allclose(tr[upd, 3], tm[upd, 3], rtol=0, atol=s_tol * np.sqrt(mod.N * mod.P)), name
    assert np.allclose(r.param_trace[upd], mdl["param_trace"][upd], rtol=0, atol=s_tol * np.sqrt(mod.PN)), name
    assert r.n_iter >= 2 and np.any(r.param_shift != 0.0) and np.any(r.shift != 0.0)
    # the final pass against the model under the device's own shifts
    fin = rp.rare_event_params(mod, x, l, L, None, K, seed=seed, shift=r.shift, param_shift=r.param_shift, n_iter=0)
    Mm, ok = fin["margins"], ~np.isnan(fin["margins"])
    assert np.array_equal(np.isnan(r.margins), ~ok), name
    dm = float(np.abs(r.margins[ok] - Mm[ok]).max() / sc)
    lw_sc = 1.0 + float(np.abs(fin["logw"]).max())
    dw = float(np.abs(r.logw - fin["logw"]).max() / lw_sc)
    print(f"{name}: final margins {dm:.2e} logw {dw:.2e} of scale; PROB model {fin['prob']:.6e}")
    assert dm <= TOL_MODEL and dw <= TOL_MODEL, (name, dm, dw)
    assert (r.n_viol, r.n_ok, r.n_domain) == (fin["n_viol"], fin["n_ok"], fin["n_domain"]), name
    for k in ("prob", "prob_se", "ess"):
        assert np.isclose(getattr(r, k), fin[k], rtol=TOL_SUM + 2 * TOL_MODEL * lw_sc, atol=0, equal_nan=True), (name, k, getattr(r, k), fin[k])
    assert abs(r.logw_max - fin["logw_max"]) <= TOL_MODEL * lw_sc and abs(r.logw_min - fin["logw_min"]) <= TOL_MODEL * lw_sc, name


# ---- 7. K-independence ------------------------------------------------------------------------------------------------------------------
def test_a_rollouts_parameters_and_noise_do_not_depend_on_k(cases):
    c = cases["pend"]
    ctx = context(c)
    x, l, L = c.policy
    r = np.random.default_rng(4)
    kw = dict(noise=rat.UserNoise(c.npn, c.npu), seed=7, shift=0.1 * r.standard_normal((c.N, c.npn)), param_shift=np.array([0.7, -0.4]),
              n_iter=0, n_event=1, want_margins=True, want_logw=True)
    a = ctx.policy_rare_event_params(x, l, L, 0, 1000, **kw)
    b = ctx.policy_rare_event_params(x, l, L, 0, (1 << 16) + 3, **kw)
    assert np.array_equal(a.margins, b.margins[:1000]) and np.array_equal(a.logw, b.logw[:1000])
    assert np.unique(b.margins[-8:]).size == 8 and np.array_equal(b.param_shift, [0.7, -0.4])


# ---- 8. the feature itself --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,adapt,seed,n_event", [("a", "params", rp.SEED_A, 1), ("b", "both", rp.SEED_B, 0)])
def test_closed_form_at_beta_six_where_the_existing_call_sees_nothing(which, adapt, seed, n_event):
    """P = Phi(-6) = 9.87e-10 at K = 2^14, at the seeds the model met the cap PROB_SE / PROB <= 0.10 with (tests/test_cpu_rare_event_params.py);
    (a) through rat_user_event, (b) through the half-space x_1 > c"""
    src, p, _, exact = rp.closed_case(which)
    x, l, L = rp.closed_policy()
    ctx = rat.Context(rat.DeviceSourceProblem(src, 1, 1, 1, np.eye(1), params=p))
    ctx.set_param_sampling(rat.ParamSampling(1, 0))
    noise = rat.UserNoise(1, 0, seed=seed)
    kw = dict(noise=noise, n_iter=rp.N_ITER_CLOSED, rho=rp.RHO_CLOSED)
    event = 0 if n_event else rat.halfspace(np.array([1.0, 0.0]), -p[2], steps=1)
    r = ctx.policy_rare_event_params(x, l, L, event, rp.K_CLOSED, adapt=adapt, n_event=n_event, **kw)
    print(f"({which}) exact {exact:.6e}: PROB {r.prob:.6e} SE {r.prob_se:.3e} ({abs(r.prob - exact) / r.prob_se:.2f} sigma), SE/PROB "
          f"{r.prob_se / r.prob:.3e}, {r.n_iter} iterations, param shift {r.param_shift}, shift {r.shift.ravel()}")
    assert r.flag == nv.RE_OK
    assert abs(r.prob - exact) <= 4.0 * r.prob_se
    if which == "a":
        assert np.all(r.shift == 0.0)
    old = ctx.policy_rare_event_user(x, l, L, 1, 0, rp.K_CLOSED, **kw)  # what the parent can do: the parameter normal is not shifted
    assert old.n_viol == 0 and old.flag == nv.RE_NOT_REACHED and old.prob == 0.0
    if which == "b":
        prob = rat.DeviceSourceProblem(src, 1, 1, 1, np.eye(1), params=p)
        again = rat.rare_event_probability_params(prob, x, l, L, event, noise, rat.ParamSampling(1, 0), K=rp.K_CLOSED, adapt=adapt,
                                                  n_iter=rp.N_ITER_CLOSED, rho=rp.RHO_CLOSED)
        assert again.prob == r.prob and np.array_equal(again.param_shift, r.param_shift)


# ---- 9. adapt = "params" and adapt = "step" ------------------------------------------------------------------------------------------------
def test_the_part_that_is_not_adapted_stays_and_is_still_applied(cases):
    c = cases["pend"]
    K, seed = 4096, 11
    p = c.rarefied(K, seed)
    mod, ctx = c.model(p), context(c, p)
    x, l, L = c.policy
    r = np.random.default_rng(3)
    s_in, ps_in = 0.1 * r.standard_normal((c.N, c.npn)), np.array([0.5, -0.3])
    kw = dict(noise=rat.UserNoise(c.npn, c.npu), seed=seed, shift=s_in, param_shift=ps_in, n_event=1, rho=0.1)
    a = ctx.policy_rare_event_params(x, l, L, 0, K, adapt="params", n_iter=3, **kw)
    assert np.array_equal(a.shift, s_in) and np.any(a.param_shift != ps_in) and a.n_iter >= 2
    assert np.all(a.trace[~np.isnan(a.trace[:, 3]), 3] == a.trace[0, 3]) and abs(a.trace[0, 3] - np.sqrt((s_in ** 2).sum())) <= TOL_SUM
    b = ctx.policy_rare_event_params(x, l, L, 0, K, adapt="step", n_iter=3, **kw)
    assert np.array_equal(b.param_shift, ps_in) and np.any(b.shift != s_in) and b.n_iter >= 2
    assert np.all(np.abs(b.param_trace[~np.isnan(b.param_trace)] - np.sqrt((ps_in ** 2).sum())) <= TOL_SUM)
    for mode in ("params", "step"):                                   # both fixed parts are applied and counted: logw is the model's
        got = ctx.policy_rare_event_params(x, l, L, 0, K, adapt=mode, n_iter=0, want_margins=True, want_logw=True, **kw)
        fin = rp.rare_event_params(mod, x, l, L, None, K, seed=seed, shift=s_in, param_shift=ps_in, n_iter=0)
        lw_sc = 1.0 + float(np.abs(fin["logw"]).max())
        assert np.any(fin["logw"] != 0.0) and float(np.abs(got.logw - fin["logw"]).max()) <= TOL_MODEL * lw_sc, mode
        assert np.array_equal(got.shift, s_in) and np.array_equal(got.param_shift, ps_in)
    # the model's iterations under adapt = "params": the same parameter shift, the step shift untouched
    mdl = rp.rare_event_params(mod, x, l, L, None, K, seed=seed, shift=s_in, param_shift=ps_in, adapt_mode="params", n_iter=3, rho=0.1)
    assert_separated(mdl["levels"], None, scale_of(mdl, types.SimpleNamespace(b=0.0)))
    assert float(np.abs(a.param_shift - mdl["param_shift"]).max()) <= TOL_SUM * (1.0 + np.abs(mdl["param_shift"]).max()) and a.n_iter == mdl["n_iter"]


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------------------
def raw(ctx, x, l, L, K=64, npn=3, npu=0, seed=1, n_event=1, event=0, a=None, pshift=None, adapt=3, n_iter=1, rho=0.1):
    stats = np.zeros(nv.RE_NSTAT)
    a = nv.f64(np.zeros(ctx.n + ctx.m) if a is None else a)
    return nv.lib().rat_policy_rare_event_params(ctx.h, nv.P(nv.f64(x)), nv.P(nv.f64(l)), nv.P(nv.cm3(L)), C.c_int64(K), C.c_int32(npn),
                                                 C.c_int32(npu), C.c_uint64(seed), C.c_int32(n_event), C.c_int32(event), None, nv.P(a),
                                                 C.c_double(0.0), C.c_int32(0), C.c_int32(0), None, nv.P(None if pshift is None else nv.f64(pshift)),
                                                 C.c_int32(adapt), C.c_int32(n_iter), C.c_double(rho), nv.P(stats), None, None, None, None, None, None)


def test_refusals_each_followed_by_a_call_that_succeeds(cases):
    c = cases["pend"]
    x, l, L = c.policy
    ctx = context(c)
    err = lambda: nv.lib().rat_last_error().decode()
    ok = lambda: raw(ctx, x, l, L) == 0
    assert ok()
    ctx.set_param_sampling(None)                                      # parameter sampling off
    assert raw(ctx, x, l, L) == ARG and "rat_policy_params_sampling" in err()
    ctx.set_param_sampling(rat.ParamSampling(0, 1))                   # nothing to shift
    assert raw(ctx, x, l, L) == ARG and "param_normals is 0" in err()
    ctx.set_param_sampling(rat.ParamSampling(13, 1))                  # wider than a shift row
    assert raw(ctx, x, l, L) == UNSUPPORTED
    ctx.set_param_sampling(rat.ParamSampling(2, 1, zpn=np.zeros((64, 2)), zpu=np.full((64, 1), 0.5)))   # injected parameter streams
    assert raw(ctx, x, l, L) == UNSUPPORTED and "injected" in err()
    ctx.set_param_sampling(SAMPLING())
    assert ok()
    for kw, rc in ((dict(adapt=0), ARG), (dict(adapt=4), ARG), (dict(pshift=[0.0, np.inf]), ARG), (dict(pshift=[np.nan, 0.0]), ARG),
                   (dict(n_event=-1), ARG), (dict(n_event=17), ARG), (dict(event=1), ARG), (dict(event=-1), ARG), (dict(npn=0), ARG),
                   (dict(npn=13), UNSUPPORTED), (dict(K=0), ARG), (dict(n_iter=33), ARG), (dict(rho=0.0), ARG)):
        assert raw(ctx, x, l, L, **kw) == rc, kw
        assert ok(), kw
    # a problem that is not a source model, and no problem
    fam = rat.LQRiskSensitiveProblem(0.5 * np.eye(2), np.ones((2, 1)), Q=np.eye(2), R=np.eye(1), N=c.N, W=np.eye(2), Qf=np.eye(2))
    assert raw(rat.Context(fam), x, l, L, n_event=0) == UNSUPPORTED
    assert raw(rat.Context(None), x, l, L, n_event=0, a=np.zeros(3)) == NO_PROBLEM
    # the Python surface refuses what it can see
    with pytest.raises(ValueError):
        ctx.policy_rare_event_params(x, l, L, 0, 64, noise=rat.UserNoise(c.npn, c.npu), n_event=1, adapt="neither")
    with pytest.raises(ValueError):
        ctx.policy_rare_event_params(x, l, L, 0, 64, noise=rat.UserNoise(c.npn, c.npu), n_event=1, param_shift=np.zeros(3))
    assert ok()


def test_the_recorded_evaluation_still_replays_and_the_call_repeats_its_bits(cases):
    c = cases["pend"]
    K, seed = 3000, 9
    p = c.rarefied(K, seed, q=0.99)
    ctx = context(c, p)
    x, l, L = c.policy
    ref = ctx.policy_evaluate_noise(x, l, L, noise=rat.UserNoise(c.npn, c.npu, seed=5), K=777, thetas=[0.1], want_costs=True)
    ev = rat.halfspace(np.array([1.0, 0.0, 0.0]), -0.5, steps=c.N)
    before = ctx.policy_events([ev], kl_bounds=[0.05], thetas=[0.0], want_margins=True)
    before_user = ctx.policy_events_user(1, thetas=[0.0], want_margins=True)
    kw = dict(noise=rat.UserNoise(c.npn, c.npu), seed=seed, n_iter=3, rho=0.2, n_event=1, want_margins=True, want_logw=True)
    a, b = ctx.policy_rare_event_params(x, l, L, 0, K, **kw), ctx.policy_rare_event_params(x, l, L, 0, K, **kw)
    same(a, b, "twice")
    assert np.array_equal(a.param_shift, b.param_shift) and np.array_equal(a.param_trace, b.param_trace, equal_nan=True)
    assert a.n_iter >= 1 and np.any(a.param_shift != 0.0)
    after = ctx.policy_events([ev], kl_bounds=[0.05], thetas=[0.0], want_margins=True)
    assert np.array_equal(before["margins"], after["margins"])
    for part in ("bounds", "thetas"):
        for k in before[part]:
            assert np.array_equal(before[part][k], after[part][k], equal_nan=True), (part, k)
    assert np.array_equal(before_user["margins"], ctx.policy_events_user(1, thetas=[0.0], want_margins=True)["margins"])
    assert ref["n_ok"] == 777
