"""rat_policy_tail_events / rat_policy_tail_events_user on the GPU (csrc/policy_mc.hip: tle_sums and tle_final behind the replay, on the
levels, weights and liveness words of the tail chain).

Per case: the rows against policy_tail_risk bit for bit; margins, N_VIOL, MARGIN_MAX and the alpha = 0 row against rat_policy_events on
the same evaluation bit for bit; every slot and step_out against tests/tail_events_model.py at TOL_MODEL, the figure
tests/test_gpu_events.py holds the same slots to against tests/events_model.py; PROB <= PROB_ROBUST on every RAT_TR_OK row; the liveness
schedule against the dense sums on the same weights (switch tail_dense) bit for bit; the call without step_out; the same call again.

Shapes: the 2 x 1 LQ family at N = 3, the 4 x 4 power-law family at N = 2 (DomainErrors), a 1 x 1 and the 12 x 4 source under
rat_user_noise at N = 3.  K = 7 (one group of four and a ragged one, far under a workgroup), EV_SLOTS MC_THREADS + 1 = 2049 (one above a
multiple of MC_THREADS: one lane takes a second rollout) and the replay's chunk + 1 (a second chunk of one rollout).  Levels: 1, EV_ROWS,
EV_ROWS + 1 and 16 of them, 0 among them, 1 - 0.5 / K (thinner than one rollout) last."""
import os
import re

import numpy as np
import pytest

import ratilqr.jl_amd as rat
import events_model as em
import tail_events_model as te
import user_event_model as ue
import user_noise_model as um
from ratilqr.jl_amd import _native as nv
from test_gpu_events import TOL_MODEL, event_set
from test_gpu_tail_scenarios import CLOSED_SRC, lq
from test_gpu_user_noise import pend_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = 1, 2
EV_ROWS, EV_SLOTS, MC_THREADS = 4, 8, 256                             # (csrc/policy_mc.h)
EV_KEYS = ("prob", "prob_se", "margin_mean", "margin_max", "first_mean", "n_viol", "prob_robust", "event_flag")


def replay_chunk():
    """the chunk of the replays' shared host path (mc_chunk of csrc/driver.cpp), read from there"""
    text = open(os.path.join(ROOT, "ratilqr.jl_amd", "csrc", "driver.cpp")).read()
    shift = re.search(r"static int64_t mc_chunk\(int64_t K\) \{ return std::min<int64_t>\(K, 1 << (\d+)\); \}", text).group(1)
    assert (1 << int(shift)) == em.CHUNK                              # (the model's order of summation assumes the same one)
    return 1 << int(shift)


K_SMALL, K_LANES, K_CHUNKS = 7, EV_SLOTS * MC_THREADS + 1, replay_chunk() + 1


def levels(count, K):
    """`count` levels: 0 first, a level thinner than one rollout last (from two on), the rest spread below 0.99"""
    if count == 1:
        return (0.0,)
    inner = tuple(np.round(np.linspace(0.3, 0.99, count - 2), 4)) if count > 2 else ()
    return (0.0,) + inner + (1.0 - 0.5 / K,)


def same(a, b, label, keys=None):
    for k in (a if keys is None else keys):
        assert np.array_equal(a[k], b[k], equal_nan=True), (label, k)


def rows_are_tail_risk(ctx, lv, alphas, label):
    tr = ctx.policy_tail_risk(alphas)
    for k in tr:
        if k != "weights":
            assert np.array_equal(lv[k], tr[k], equal_nan=True), (label, k)


def against_model(out, mdl, sc, N, E, ok, label):
    lv = out["levels"]
    M = out["margins"]
    K = ok.size
    assert M.shape == (E, K) and np.isnan(M[:, ~ok]).all()
    assert np.array_equal(np.isnan(M), np.isnan(mdl["margins"][:E]))  # (an event that is never written, or every g NaN: NaN meets NaN)
    with np.errstate(invalid="ignore"):
        dm_r = float(np.nanmax(np.append(np.abs(M[:, ok] - mdl["margins"][:E][:, ok]) / sc[:E, None], 0.0)))
    dp, dm = te.deviation(lv, mdl, sc, N)
    print(f"{label}: margins {dm_r:.2e}; model prob {dp:.2e} margin mean {dm:.2e}")
    assert dm_r <= TOL_MODEL and dp <= TOL_MODEL and dm <= TOL_MODEL, (label, dm_r, dp, dm)
    assert np.array_equal(lv["event_flag"], mdl["event_flag"]) and np.array_equal(lv["flag"], mdl["flag"])
    live = ~np.isin(lv["flag"], (2, 3))
    for k in ("prob", "prob_se", "margin_mean", "margin_max", "first_mean", "n_viol", "prob_robust", "step"):
        assert np.isnan(lv[k][~live]).all(), (label, k)
    with np.errstate(invalid="ignore"):
        viol = M > 0
    if live.any():
        assert np.array_equal(lv["n_viol"][live], np.broadcast_to(np.append(viol.sum(axis=1), viol.any(axis=0).sum()), lv["n_viol"][live].shape)), label
        assert np.all(lv["prob"][live][:, E:] >= lv["prob"][live][:, :E].max(axis=1, keepdims=True)), label
    okrow = lv["flag"] == 0
    assert np.all(lv["prob"][okrow] <= lv["prob_robust"][okrow]), (label, "PROB <= PROB_ROBUST")       # checked, not assumed
    assert np.array_equal(lv["prob_robust"][lv["alpha"] == 0.0], lv["prob"][lv["alpha"] == 0.0], equal_nan=True), label


def common(ctx, call, nominal, alphas, label):
    """what every case holds of one call (call(alphas, **kw) -> dict) beside the model: the rows, the nominal row of the sibling
    (nominal(**kw) -> its theta = 0 part and margins), the dense sums, the call without step_out and the call again"""
    out = call(alphas, want_steps=True, want_margins=True)
    lv = out["levels"]
    rows_are_tail_risk(ctx, lv, alphas, label)
    nom, margins = nominal(want_steps=True, want_margins=True)
    assert np.array_equal(out["margins"], margins, equal_nan=True), (label, "margins")
    for k in EV_KEYS + ("step",):                                     # alpha = 0 is the sibling's theta = 0 row
        assert np.array_equal(lv[k][0], nom[k][0], equal_nan=True), (label, "alpha = 0", k)
    for k in ("n_viol", "margin_max"):                                # unweighted: the same on every row
        assert np.array_equal(lv[k], np.broadcast_to(nom[k][0], lv[k].shape), equal_nan=True), (label, k)
    again = call(alphas, want_steps=True, want_margins=True)
    same(lv, again["levels"], (label, "again"))
    assert np.array_equal(out["margins"], again["margins"], equal_nan=True)
    bare = call(alphas)
    assert "step" not in bare["levels"] and bare["margins"] is None
    same(bare["levels"], lv, (label, "without step_out"))
    ctx.debug_set("tail_dense", 1)                                   # rat_policy_events' own sums on the same weights: the same bits
    try:
        same(lv, call(alphas, want_steps=True)["levels"], (label, "dense"))
    finally:
        ctx.debug_set("tail_dense", 0)
    return out


def check_quadratic(ctx, x, u, costs, evs, alphas, label):
    n, m, N = x.shape[2], u.shape[2], u.shape[1]
    dense = [e.dense(n, m, N) for e in evs]

    def nominal(**kw):
        o = ctx.policy_events(evs, thetas=(0.0,), **kw)
        return o["thetas"], o["margins"]
    out = common(ctx, lambda al, **kw: ctx.policy_tail_events(evs, al, **kw), nominal, alphas, label)
    against_model(out, te.tail_events(x, u, costs, alphas, dense), em.scales(x, u, costs, dense), N, len(evs), ~np.isnan(costs), label)
    return out


def half_spaces(x, costs, count, N):
    """`count` linear events on the state components in turn, thresholds inside the spread, the last one watched at step N alone"""
    ok = ~np.isnan(costs)
    xs = x[ok] if ok.any() else np.zeros((1,) + x.shape[1:])
    n = x.shape[2]
    evs = [rat.halfspace(np.eye(n)[i % n], -em.between(xs[:, :, i % n].max(axis=1), 0.15 + 0.05 * i)) for i in range(count - 1)]
    return evs + [rat.halfspace(np.eye(n)[0], -em.between(xs[:, N, 0], 0.5), steps=N)]


# ---- the families ----------------------------------------------------------------------------------------------------------------------------
def evaluate_family(ctx, x0, l, L, K, seed=5):
    x_det = ctx.rollout_open(x0, l)
    r = ctx.policy_evaluate(x_det, l, L, K=K, seed=seed, want_costs=True)
    x, u, cost, _ = ctx.rollout_noisy(x_det, l, L, K=K, seed=seed)
    assert np.array_equal(cost, r["costs"], equal_nan=True)
    return r, x, u, cost


@pytest.mark.parametrize("K,rows", [(K_SMALL, EV_ROWS), (K_LANES, 16), (K_CHUNKS, EV_ROWS + 1)])
def test_lq_family(K, rows):
    """2 x 1, N = 3: the nine events of tests/test_gpu_events.py (Q given, windows of a single step, nobody, everybody, the boundary)"""
    prob, x0, l, L = lq(2, 1, 3)
    ctx = rat.Context(prob)
    _, x, u, cost = evaluate_family(ctx, x0, l, L, K)
    evs = event_set(x, u, cost, np.random.default_rng(K))
    al = levels(rows, K)
    out = check_quadratic(ctx, x, u, cost, evs, al, f"lq 2 x 1, K = {K}, {rows} levels")
    lv = out["levels"]
    assert lv["flag"][-1] == 1 and np.all(lv["event_flag"][-1] == 1)  # thinner than one rollout: the rollout that costs the most
    top = int(np.argmax(cost))
    with np.errstate(invalid="ignore"):
        viol = out["margins"][:, top] > 0
    assert np.array_equal(lv["prob"][-1], np.append(viol, viol.any()).astype(float)) and np.all(lv["prob_robust"][-1][lv["n_viol"][-1] > 0] == 1.0)
    assert np.all(lv["step"][:, 4, 1:] == 0.0) and np.all(lv["step"][:, 5, :3] == 0.0)        # outside a single-step window: 0


def test_one_event_sixteen_events_and_no_q():
    """n_event = 1 and 16, Q == NULL; one level alone, and a level alone against the level among sixteen"""
    prob, x0, l, L = lq(2, 1, 3)
    ctx = rat.Context(prob)
    K = 4 * MC_THREADS + 1
    _, x, u, cost = evaluate_family(ctx, x0, l, L, K)
    al = levels(16, K)
    evs = half_spaces(x, cost, 16, 3)
    assert all(e.dense(2, 1, 3)[0] is None for e in evs)
    full = check_quadratic(ctx, x, u, cost, evs, al, "sixteen linear events, sixteen levels")
    one = check_quadratic(ctx, x, u, cost, evs[:1], (0.0,), "one linear event, one level")
    for k in EV_KEYS + ("step",):                                     # an entry does not depend on the other events or levels
        assert np.array_equal(one["levels"][k][0, 0], full["levels"][k][0, 0], equal_nan=True), k
    for i in (3, EV_ROWS, 15):
        alone = ctx.policy_tail_events(evs, (al[i],), want_steps=True)["levels"]
        for k in alone:
            assert np.array_equal(alone[k][0], full["levels"][k][i], equal_nan=True), (i, k)


@pytest.mark.parametrize("K,rows", [(K_SMALL, 1), (K_LANES, EV_ROWS + 1)])
def test_power_law_family(K, rows):
    """4 x 4, N = 2, started so close to zero that the noise drives states negative: DomainError rollouts carry no weight"""
    N = 2
    prob = rat.PowerLawRiskSensitiveProblem(4, N, 1e-4 * np.eye(4), a=1.3, b=1.5, p=2.5, hconst=1.0)
    ctx = rat.Context(prob)
    r, x, u, cost = evaluate_family(ctx, np.full(4, 0.03), 0.01 * np.ones((N, 4)), 0.05 * np.ones((N, 4, 4)), K)
    evs = event_set(x, u, cost, np.random.default_rng(K))
    out = check_quadratic(ctx, x, u, cost, evs, levels(rows, K), f"power law 4 x 4, K = {K}, {rows} levels")
    if K == K_LANES:
        assert r["n_domain"] > 0 and np.isnan(out["margins"][:, np.isnan(cost)]).all()
        assert np.all(out["levels"]["n_viol"][:, 7] == r["n_ok"])     # the everybody event counts the OK rollouts


def test_an_empty_sample_is_nan_but_for_the_flag():
    N = 2
    prob = rat.PowerLawRiskSensitiveProblem(4, N, 1e-4 * np.eye(4), a=1.3, b=1.5, p=2.5, hconst=1.0)
    ctx = rat.Context(prob)
    r = ctx.policy_evaluate(np.full(4, -0.5), 0.01 * np.ones((N, 4)), K=9, seed=1)
    assert r["n_ok"] == 0
    out = ctx.policy_tail_events([rat.halfspace(np.eye(4)[0], 0.0)], (0.0, 0.5), want_steps=True, want_margins=True)
    lv = out["levels"]
    assert np.all(lv["flag"] == 2) and np.all(lv["event_flag"] == 2) and np.isnan(out["margins"]).all()
    for k in ("prob", "prob_se", "margin_mean", "margin_max", "first_mean", "n_viol", "prob_robust", "step"):
        assert np.isnan(lv[k]).all(), k


# ---- source models under rat_user_noise ------------------------------------------------------------------------------------------------------
def check_user(ctx, name, E, x, u, costs, q, alphas, label):
    def nominal(**kw):
        o = ctx.policy_events_user(E, thetas=(0.0,), **kw)
        return o["thetas"], o["margins"]
    out = common(ctx, lambda al, **kw: ctx.policy_tail_events_user(E, al, **kw), nominal, alphas, label)
    g = ue.g_user(name, x, u, q)
    mdl = te.reduce(g, ue.windows(g), costs, alphas)
    assert np.array_equal(out["margins"], mdl["margins"][:E], equal_nan=True)                 # bit for bit; NaN meets NaN
    ok = ~np.isnan(costs)
    sc = np.full(E + 1, max(float(np.abs(x[ok]).max()), float(np.abs(u[ok]).max())) + float(np.abs(q).max()))
    against_model(out, mdl, sc, u.shape[1], E, ok, label)
    return out


@pytest.mark.parametrize("K,rows", [(K_SMALL, EV_ROWS + 1), (K_CHUNKS, EV_ROWS)])
def test_source_1x1(K, rows):
    """the random walk of tests/user_event_model.py at N = 3: its own half-space (rat_policy_tail_events_user) and quadratic events"""
    N = 3
    prob = rat.DeviceSourceProblem(ue.source(ue.WALK, "half", len(ue.WALK_P)), 1, 1, N, 1e-3 * np.eye(1), params=np.concatenate([ue.WALK_P, [0.0]]))
    ctx = rat.Context(prob)
    x_nom, l = np.array([0.5]), np.zeros((N, 1))
    r = ctx.policy_evaluate_noise(x_nom, l, None, noise=rat.UserNoise(1, 0, seed=11), K=K, want_costs=True, want_trajectories=True)
    x, u, costs = r["x"], r["u"], r["costs"]
    q = ue.thresholds("half", np.concatenate([x, x], axis=2), u, costs)      # (thresholds reads two state components; "half" uses the first)
    ctx.set_params(np.concatenate([ue.WALK_P, q]))
    al, label = levels(rows, K), f"walk 1 x 1, K = {K}, {rows} levels"
    user = check_user(ctx, "half", 1, x, u, costs, q, al, label)
    evs = [rat.halfspace([1.0, 0.0], -q[0]), rat.quadratic_event(np.array([[1.0, 0.2], [0.0, 0.5]]), [0.1, -0.3], -em.between((x[:, N, 0] ** 2), 0.7), steps=N)]
    quad = check_quadratic(ctx, x, u, costs, evs, al, label + ", quadratic")
    assert np.array_equal(quad["margins"][0], user["margins"][0])     # the half-space both ways: 1 x_0 - c is x_0 - c
    for k in ("prob", "n_viol", "first_mean", "margin_mean"):
        assert np.array_equal(quad["levels"][k][:, 0], user["levels"][k][:, 0], equal_nan=True), k


@pytest.mark.parametrize("K,rows", [(K_SMALL, 16), (K_LANES, EV_ROWS)])
def test_source_12x4(K, rows):
    """the 12 x 4 linear source at N = 3: the sixteen user events (one on u, one never written) and the nine quadratic ones"""
    N = 3
    prob, x_nom, l, L, off = ue.lq_case("16", N)
    ctx = rat.Context(prob)
    r = ctx.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(12, 0, seed=11), K=K, want_costs=True, want_trajectories=True)
    x, u, costs = r["x"], r["u"], r["costs"]
    q = ue.thresholds("16", x, u, costs)
    ctx.set_params(np.concatenate([prob.params[:off], q]))
    al, label = levels(rows, K), f"lq source 12 x 4, K = {K}, {rows} levels"
    out = check_user(ctx, "16", 16, x, u, costs, q, al, label)
    assert np.isnan(out["margins"][15]).all() and np.all(out["levels"]["prob"][:, 15] == 0.0)     # never written: NaN margins, probability 0
    check_quadratic(ctx, x, u, costs, event_set(x, u, costs, np.random.default_rng(K)), al, label + ", quadratic")


# ---- the exact cases of tests/test_cpu_tail_events.py through the device -------------------------------------------------------------------
def test_monotone_and_anti_monotone_cases():
    """J = x_1 on the 1 x 1 source of the closed form at N = 1, the event on x_1: with M = x_1 - c the violators are the most expensive
    rollouts, PROB = min(1, N_VIOL / TAIL_N) = PROB_ROBUST; with M = c - x_1 the cheapest, PROB = max(0, 1 - N_OK (1 - p) / TAIL_N).
    K = 1024, alpha = 0.75: (1 - alpha) N_OK = 256, no ties among Gaussian draws."""
    K, alpha, tail = 1024, 0.75, 256.0
    ctx = rat.Context(rat.DeviceSourceProblem(CLOSED_SRC, 1, 1, 1, np.eye(1), params=[0.7]))
    r = ctx.policy_evaluate_noise(np.array([0.3]), np.array([[-0.1]]), None, noise=rat.UserNoise(1, 0, seed=17), K=K, want_costs=True, want_trajectories=True)
    J = r["costs"]
    assert r["n_ok"] == K and np.array_equal(J, r["x"][:, 1, 0]) and np.unique(J).size == K
    s = np.sort(J)
    eps = np.finfo(float).eps
    for nv in (1, 100, 256, 257, 700):
        c = 0.5 * (s[K - nv - 1] + s[K - nv])                         # nv costs lie above c
        lv = ctx.policy_tail_events([rat.halfspace([1.0, 0.0], -c, steps=1)], (0.0, alpha))["levels"]
        want = min(1.0, nv / tail)
        assert lv["tail_n"][1] == tail and np.all(lv["n_viol"] == nv)
        assert abs(lv["prob"][1, 0] - want) <= 4 * eps * want and lv["prob"][1, 0] <= lv["prob_robust"][1, 0] and abs(lv["prob_robust"][1, 0] - want) <= 4 * eps * want
        assert lv["prob"][0, 0] == nv / K == lv["prob_robust"][0, 0]
    for nv in (1, 768, 769, 900, 1023):
        c = 0.5 * (s[nv - 1] + s[nv])                                 # nv costs lie below c
        lv = ctx.policy_tail_events([rat.halfspace([-1.0, 0.0], c, steps=1)], (alpha,))["levels"]
        want = max(0.0, 1.0 - K * (1.0 - nv / K) / tail)
        assert lv["n_viol"][0, 0] == nv and abs(lv["prob"][0, 0] - want) <= 4 * eps * max(want, eps)
        assert lv["prob"][0, 0] <= lv["prob_robust"][0, 0] == min(1.0, nv / tail)


# ---- the Python mirror and the C call ---------------------------------------------------------------------------------------------------------
def test_the_python_mirror_returns_the_c_calls_arrays():
    prob, x0, l, L = lq(2, 1, 3)
    ctx = rat.Context(prob)
    K = 50
    _, x, u, cost = evaluate_family(ctx, x0, l, L, K)
    evs = half_spaces(x, cost, 2, 3)
    al = (0.0, 0.8)
    out = ctx.policy_tail_events(evs, al, want_steps=True, want_margins=True)
    E, Q, a, b, lo, hi = ctx._events_dense(evs)
    alp = nv.f64(np.array(al))
    rows, ev, step, margins = np.zeros((2, 8)), np.zeros((2, E + 1, 8)), np.zeros((2, E + 1, 4)), np.zeros((E, K))
    assert nv.lib().rat_policy_tail_events(ctx.h, E, None, nv.P(a), nv.P(b), nv.PI(lo), nv.PI(hi), nv.P(alp), 2, nv.P(rows), nv.P(ev), nv.P(step),
                                           nv.P(margins)) == 0
    lv = out["levels"]
    for i, k in enumerate(nv.TR_SLOTS):
        assert np.array_equal(lv[k], rows[:, i], equal_nan=True), k
    for i, k in enumerate(nv.EV_SLOTS):
        assert np.array_equal(lv["event_flag" if k == "flag" else k], ev[:, :, i], equal_nan=True), k
    assert np.array_equal(lv["step"], step) and np.array_equal(out["margins"], margins)


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    prob, x0, l, L = lq(2, 1, 3)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)
    ev = [rat.halfspace([1.0, 0.0], 0.0)]
    name = "rat_policy_tail_events"
    with pytest.raises(rat.RatError, match=f"RAT_ERR_ARG.*{name}.*no evaluation"):           # nothing to replay yet
        ctx.policy_tail_events(ev, (0.5,))
    ctx.policy_evaluate(x_det, l, L, K=20, seed=1)
    for bad in ((1.0,), (-0.1,), (np.nan,), (), tuple(0.05 * i for i in range(17))):          # rat_policy_tail_risk's rules for the levels
        with pytest.raises(rat.RatError, match=f"RAT_ERR_ARG.*{name}"):
            ctx.policy_tail_events(ev, bad)
    bad_events = ([], ev * 17, [rat.halfspace([1.0, 0.0], 0.0, steps=(2, 1))], [rat.halfspace([1.0, 0.0], 0.0, steps=4)],
                  [rat.halfspace([1.0, 0.0], 0.0, steps=(-1, 2))], [rat.halfspace([np.nan, 0.0], 0.0)], [rat.halfspace([1.0, 0.0], np.inf)],
                  [rat.quadratic_event(np.array([[1.0, np.inf, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), [0.0, 0.0, 0.0], 0.0)])
    for evs in bad_events:                                                                   # rat_policy_events' own, with its code
        with pytest.raises(rat.RatError, match=f"RAT_ERR_ARG.*{name}"):
            ctx.policy_tail_events(evs, (0.5,))
    assert ctx.policy_tail_events(ev, (0.0,))["levels"]["event_flag"][0, 0] == 0             # ... leave the handle usable
    lib = nv.lib()
    al, rows, evo = nv.f64(np.array([0.5])), np.zeros(8), np.zeros(16)
    a1, b1, w = nv.f64(np.array([1.0, 0.0, 0.0])), nv.f64(np.zeros(1)), np.zeros(1, dtype=np.int32)
    assert lib.rat_policy_tail_events(ctx.h, 1, None, nv.P(a1), nv.P(b1), nv.PI(w), nv.PI(w), nv.P(al), 1, None, nv.P(evo), None, None) == ARG
    assert b"rat_policy_tail_events: null alpha / output" in lib.rat_last_error()
    assert lib.rat_policy_tail_events(ctx.h, 1, None, None, nv.P(b1), nv.PI(w), nv.PI(w), nv.P(al), 1, nv.P(rows), nv.P(evo), None, None) == ARG
    assert b"null a / b / t_lo / t_hi" in lib.rat_last_error()
    assert lib.rat_policy_tail_events(None, 1, None, nv.P(a1), nv.P(b1), nv.PI(w), nv.PI(w), nv.P(al), 1, nv.P(rows), nv.P(evo), None, None) == ARG
    with pytest.raises(rat.RatError, match=f"RAT_ERR_UNSUPPORTED.*{name}_user.*not a source model"):
        ctx.policy_tail_events_user(1, (0.5,))
    ctx.policy_tail_risk((0.5,), costs=np.arange(20.0))                                      # uploaded costs are no evaluation's
    with pytest.raises(rat.RatError, match=f"RAT_ERR_ARG.*{name}.*no evaluation's"):
        ctx.policy_tail_events(ev, (0.5,))
    ctx.policy_evaluate(x_det, l, L, z=np.random.default_rng(0).standard_normal((8, 3, 2)))  # injected draws are not kept
    with pytest.raises(rat.RatError, match=f"RAT_ERR_UNSUPPORTED.*{name}.*injected"):
        ctx.policy_tail_events(ev, (0.5,))
    # the problem changed behind the evaluation: the replay guard's count
    ctx.policy_evaluate(x_det, l, L, K=50, seed=1)
    good = ctx.policy_tail_events(ev, (0.5,))["levels"]
    p2, _, _ = rat.synthetic_lq_problem(n=2, m=1, N=3, seed=10, w=0.09)                      # (another A and B; lq's seed is n + N = 5)
    ctx.set_problem(p2)
    with pytest.raises(rat.RatError, match=f"RAT_ERR_ARG.*{name}.*50 replayed.*changed since the evaluation"):
        ctx.policy_tail_events(ev, (0.5,))
    ctx.set_problem(prob)
    assert ctx.policy_evaluate(x_det, l, L, K=50, seed=1)["n_ok"] == 50
    same(good, ctx.policy_tail_events(ev, (0.5,))["levels"], "after the refusals")
    # a source model under N(0, W), and under its sampler with injected draws; the user call's own
    N = 3
    x_nom, pl, pL = um.pend_policy(N)
    src = rat.Context(pend_problem(um.PEND_STATE, N, um.PEND_STATE_P))
    src.policy_evaluate(x_nom, pl, pL, K=16, seed=1)
    with pytest.raises(rat.RatError, match=f"RAT_ERR_UNSUPPORTED.*{name}.*rat_user_noise"):
        src.policy_tail_events(ev, (0.5,))
    src.policy_evaluate_noise(x_nom, pl, pL, noise=rat.UserNoise(3, 0, zn=np.zeros((4, N, 3))))
    with pytest.raises(rat.RatError, match=f"RAT_ERR_UNSUPPORTED.*{name}.*injected"):
        src.policy_tail_events(ev, (0.5,))
    assert src.policy_evaluate_noise(x_nom, pl, pL, noise=rat.UserNoise(3, 0, seed=1), K=16)["n_ok"] == 16
    assert src.policy_tail_events(ev, (0.5,))["levels"]["flag"][0] == 0
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_ARG.*RAT_USER_EVENT"):               # a source without the event (the compiler's log)
        src.policy_tail_events_user(1, (0.5,))
    for ne in (0, 17):
        with pytest.raises(rat.RatError, match=f"RAT_ERR_ARG.*{name}_user.*n_event"):
            src.policy_tail_events_user(ne, (0.5,))
    with pytest.raises(rat.RatError, match=f"RAT_ERR_ARG.*{name}_user"):
        src.policy_tail_events_user(1, (1.0,))
    assert src.policy_tail_events(ev, (0.5,))["levels"]["flag"][0] == 0                      # ... and the handle goes on
    # general sizes
    wide_prob, wx0, wu = rat.synthetic_lq_problem(n=16, m=4, N=5, seed=3, w=1e-2)
    wide = rat.Context(wide_prob)
    wide.policy_evaluate(wx0, wu, K=8, seed=1)
    with pytest.raises(rat.RatError, match=f"RAT_ERR_UNSUPPORTED.*{name}.*n <= 12"):
        wide.policy_tail_events([rat.halfspace(np.ones(16), 0.0)], (0.5,))
    # too many rows x steps for the partial sums, with n_alpha rows: the message says how many fit
    long_prob = rat.LQRiskSensitiveProblem(np.eye(2), np.eye(2), Q=np.eye(2), R=np.eye(2), N=4000, W=np.eye(2), Qf=np.eye(2))
    lc = rat.Context(long_prob)
    lc.policy_evaluate(np.zeros(2), np.zeros((4000, 2)), K=4, seed=1)
    with pytest.raises(rat.RatError, match=f"RAT_ERR_UNSUPPORTED.*{name}.*64 MiB.*12 rows fit"):
        lc.policy_tail_events([rat.halfspace([1.0, 0.0], 0.0)], tuple(0.05 * i for i in range(16)), want_steps=True)
    assert lc.policy_tail_events([rat.halfspace([1.0, 0.0], 0.0)], tuple(0.05 * i for i in range(12)), want_steps=True)["levels"]["step"].shape == (12, 2, 4001)
