"""Safety events of a policy on the device (rat_policy_events, Context.policy_events): violation probabilities of quadratic events under q
and under every row's tilt, formed by replaying the last evaluation (csrc/policy_mc.hip: ev_eval, ev_sums, ev_final).

Reference trajectories as in tests/test_gpu_wc_trajectory.py: rat_rollout_noisy with the same seed for the families, policy_evaluate_noise's
x / u for a source model.  From them tests/events_model.py: `events` restates the device's order (margins and every weighted slot held to
1e-12 of the event's scale, the project's figure for a restated order) and `direct` is np.longdouble (held to ten times the deviation
tests/test_cpu_events.py measures between the two).  Counts are held exactly; only rollouts whose np.longdouble margin lies within 1e-9 of
the event's scale of zero may be left out of the comparison of the indicators, none at K <= 65 and at most 1e-3 of them across a chunk."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
import user_noise_model as um
from events_model import between, deviation, direct, events, scales
from test_cpu_events import CPU_DEV_MARGIN, CPU_DEV_PROB
from test_gpu_user_noise import pend_problem
from test_gpu_wc_trajectory import family
from wc_trajectory_model import weights_from_rows

pytestmark = pytest.mark.gpu
TOL_MODEL = 1e-12
KS = (1, 3, 4, 5, 63, 64, 65)
K_CHUNK = 65536 + 5
NOBODY, EVERYBODY, BOUNDARY = 6, 7, 8
LINEAR = (0, 1, 4, NOBODY, EVERYBODY)


def event_set(x, u, costs, rng):
    """The nine events, sized from the spread of the rollouts that have a cost: thresholds sit between two neighbouring per-rollout
    values, never on one."""
    ok = ~np.isnan(np.asarray(costs))
    K, T, n = x.shape
    m, N = u.shape[2], T - 1
    xs, us = (x[ok], u[ok]) if ok.any() else (np.zeros((1, T, n)), np.zeros((1, N, m)))
    d = n + m
    z = np.zeros((xs.shape[0], T, d))
    z[:, :, :n], z[:, :N, n:] = xs, us
    A = rng.standard_normal((d, d))
    Qd, ad = A + A.T, rng.standard_normal(d)                          # symmetric, mixed signs
    qz = np.einsum("kti,ij,ktj->kt", z, Qd, z) + z @ ad
    c2 = xs[:, N, :2].mean(axis=0)
    au = np.concatenate([np.zeros(n), np.ones(m)])              # on u alone: at step N it must meet zeros
    return [rat.halfspace(np.eye(n)[0], -between(xs[:, :, 0].max(axis=1), 0.6)),
            rat.halfspace(np.eye(d)[d - 1], -between(us[:, :, m - 1].max(axis=1), 0.7)),
            rat.ball([0, 1], c2, 1.2 * xs[:, N, :2].std() + 0.1 * (1.0 + np.abs(c2).max())),
            rat.quadratic_event(Qd, ad, -between(qz.max(axis=1), 0.5)),
            rat.halfspace(np.eye(n)[1], 1.0 - xs[0, 0, 1], steps=0),
            rat.quadratic_event(np.eye(d), au, -between((xs[:, N] ** 2).sum(axis=1), 0.5), steps=N),
            rat.halfspace(np.ones(d), -1e30),
            rat.halfspace(np.zeros(d), 1.0, steps=(min(1, N), N)),
            rat.quadratic_event(np.zeros((d, d)), np.zeros(d), 0.0)]


def both(out):
    return {k: np.concatenate([out["bounds"][k], out["thetas"][k]]) for k in out["bounds"]}


def same_bits(a, b, label):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (label, k)


def check(ctx, x, u, costs, evs, bounds, thetas, label):
    """one call against policy_worst_case's rows, the model, the extended-precision answer and the slots' own identities; returns it"""
    n, m, N, K = x.shape[2], u.shape[2], u.shape[1], costs.size
    E = len(evs)
    out = ctx.policy_events(evs, kl_bounds=bounds, thetas=thetas, want_steps=True, want_margins=True)
    wc = ctx.policy_worst_case(kl_bounds=bounds, thetas=thetas)
    for part in ("bounds", "thetas"):
        for k in wc[part]:
            assert np.array_equal(out[part][k], wc[part][k], equal_nan=True), (label, part, k)
    o = both(out)
    dense = [e.dense(n, m, N) for e in evs]
    y, dead = weights_from_rows(costs, o["theta"], o["flag"])
    mdl, ref = events(x, u, costs, y, dead, dense), direct(x, u, costs, y, dead, dense)
    sc = scales(x, u, costs, dense)
    ok = ~np.isnan(costs)
    n_ok = int(ok.sum())
    M = out["margins"]
    assert M.shape == (E, K) and np.isnan(M[:, ~ok]).all()
    dm_r = float(np.max(np.abs(M[:, ok] - mdl["margins"][:E][:, ok]) / sc[:E, None])) if n_ok else 0.0
    dp, dm = deviation(o, mdl, sc, N)
    ep, em = deviation(o, ref, sc, N)
    print(f"{label}: margins {dm_r:.2e}; model prob {dp:.2e} margin mean {dm:.2e}; longdouble prob {ep:.2e} margin mean {em:.2e}")
    assert dm_r <= TOL_MODEL and dp <= TOL_MODEL and dm <= TOL_MODEL, (label, dm_r, dp, dm)
    assert ep <= 10 * CPU_DEV_PROB and em <= 10 * CPU_DEV_MARGIN, (label, ep, em)
    # counts: exact, against np.longdouble wherever its margin is not within 1e-9 of scale of zero
    Md = ref["margins"][:E]
    with np.errstate(invalid="ignore"):
        near = ok[None, :] & (np.abs(Md) <= 1e-9 * sc[:E, None])
        near[BOUNDARY if E > BOUNDARY else E:] = False                # (the boundary event sits on zero by construction: exactly 0 on both sides)
        viol = M > 0
        assert np.array_equal(viol[~near], (Md > 0)[~near]), label
    left = near.sum(axis=1)
    assert np.all(left == 0) if K <= 65 else np.all(left <= 1e-3 * K), (label, left)
    anyv = viol.any(axis=0)
    for r in range(o["theta"].size):
        if o["flag"][r] in (2, 3):
            for k in ("prob", "prob_se", "margin_mean", "margin_max", "first_mean", "n_viol", "prob_robust", "step"):
                assert np.isnan(o[k][r]).all(), (label, k)
            continue
        assert np.array_equal(o["n_viol"][r], np.append(viol.sum(axis=1), anyv.sum())), label
        with np.errstate(invalid="ignore"):
            assert np.array_equal(o["margin_max"][r], np.append(np.nanmax(M[:, ok], axis=1), np.nanmax(M[:, ok]))), label
        assert np.all(o["prob"][r, E] >= o["prob"][r, :E]) and np.all(o["step"][r, E] >= o["step"][r, :E].max(axis=0)), label
        d_row = max(bounds[r] if r < len(bounds) else o["kl"][r], 0.0)
        for e in range(E + 1):
            assert o["prob_robust"][r, e] == rat.kl_event_bound(o["n_viol"][r, e] / n_ok, d_row), (label, r, e)
            if o["flag"][r] == 0:
                assert o["prob"][r, e] <= o["prob_robust"][r, e], (label, r, e)
    assert np.array_equal(o["event_flag"], np.repeat(o["flag"][:, None], E + 1, axis=1))
    return out


def named_checks(o, N, n_ok):
    """the nine-event set's own identities, on rows that hold numbers"""
    live = ~np.isin(o["flag"], (2, 3))
    if not live.any() or n_ok == 0:
        return
    assert np.all(o["prob"][live, NOBODY] == 0.0) and np.isnan(o["first_mean"][live, NOBODY]).all() and np.all(o["n_viol"][live, NOBODY] == 0)
    assert np.all(o["prob"][live, EVERYBODY] == 1.0) and np.all(o["first_mean"][live, EVERYBODY] == min(1, N))
    assert np.all(o["prob"][live, BOUNDARY] == 0.0) and np.all(o["margin_mean"][live, BOUNDARY] == 0.0) and np.all(o["margin_max"][live, BOUNDARY] == 0.0)
    assert np.all(o["step"][live, 4, 1:] == 0.0) and np.all(o["step"][live, 5, :N] == 0.0)      # outside a window: 0
    assert np.all(o["prob"][live, 9] == 1.0)                          # "any" holds the everybody event


def subsets(ctx, evs, full, bounds, thetas, label):
    """the same events in smaller company, and the linear ones without a Q: entries do not depend on the other events"""
    o = both(full)
    keys = ("prob", "prob_se", "margin_mean", "margin_max", "first_mean", "n_viol", "prob_robust", "step")
    pick = (3, 0, EVERYBODY)
    sub = ctx.policy_events([evs[i] for i in pick], kl_bounds=bounds, thetas=thetas, want_steps=True, want_margins=True)
    s = both(sub)
    for j, i in enumerate(pick):
        for k in keys:
            assert np.array_equal(s[k][:, j], o[k][:, i], equal_nan=True), (label, "subset", i, k)
        assert np.array_equal(sub["margins"][j], full["margins"][i], equal_nan=True)
    lin = ctx.policy_events([evs[i] for i in LINEAR], kl_bounds=bounds, thetas=thetas, want_steps=True, want_margins=True)
    li = both(lin)
    n, m, N = ctx.n, ctx.m, ctx.N
    for j, i in enumerate(LINEAR):
        Q, a, b, lo, hi = evs[i].dense(n, m, N)
        assert Q is None
        assert np.array_equal(li["n_viol"][:, j], o["n_viol"][:, i], equal_nan=True), (label, "linear", i)
        for k in ("prob", "prob_se", "first_mean", "step"):
            assert np.allclose(li[k][:, j], o[k][:, i], rtol=0, atol=TOL_MODEL * max(N, 1), equal_nan=True), (label, "linear", i, k)
        sc = max(np.nanmax(np.abs(full["margins"][i])) if np.isfinite(full["margins"][i]).any() else 0.0, abs(b))
        assert np.allclose(lin["margins"][j], full["margins"][i], rtol=0, atol=TOL_MODEL * sc, equal_nan=True), (label, "linear", i)
    # without the per-step sums and the margins: the same slots
    bare = both(ctx.policy_events(evs, kl_bounds=bounds, thetas=thetas))
    for k in keys[:-1]:
        assert np.array_equal(bare[k], o[k], equal_nan=True), (label, "bare", k)
    assert "step" not in bare


def rows_for(r):
    """a searched radius, the nominal distribution and a tilt of one standard deviation of the costs (tests/test_gpu_wc_trajectory.py)"""
    sd = np.sqrt(r["var"]) if r["n_ok"] >= 2 and r["var"] > 0 else 1.0
    return (0.1,), (0.0, 1.0 / sd)


def run_family(ctx, prob_tuple, K, closed, label, seed=5, with_subsets=False):
    _, x0, l, L = prob_tuple
    x_det = ctx.rollout_open(x0, l)
    x_nom, gains = (x_det, L) if closed else (x0, None)
    r = ctx.policy_evaluate(x_nom, l, gains, K=K, seed=seed, want_costs=True)
    x, u, cost, _ = ctx.rollout_noisy(x_nom, l, gains, K=K, seed=seed)
    assert np.array_equal(cost, r["costs"], equal_nan=True)
    evs = event_set(x, u, cost, np.random.default_rng(K))
    bounds, thetas = rows_for(r)
    out = check(ctx, x, u, cost, evs, bounds, thetas, label)
    named_checks(both(out), u.shape[1], r["n_ok"])
    if with_subsets:
        subsets(ctx, evs, out, bounds, thetas, label)
    return r, out


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("N", [1, 2, 5])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_families_against_model_and_longdouble(which, N, closed):
    """K = 1, 3, 4, 5, 63, 64, 65 per problem, horizon and loop: the tail of a group of sixteen rollouts, more than one group, more than
    one workgroup of ev_eval (K = 65: five groups).  The power-law problem loses rollouts to DomainErrors."""
    p = family(which, N)
    ctx = rat.Context(p[0])
    for K in KS:
        run_family(ctx, p, K, closed, f"family {which} N={N} K={K} closed={closed}", with_subsets=(K == 65))


def test_power_law_across_a_chunk():
    """K = 65536 + 5, N = 2: the second chunk holds five rollouts under its own Philox key, and its sums are added to the first one's
    partials.  DomainError rollouts hold NaN: no weight, no count."""
    p = family(2, 2)
    ctx = rat.Context(p[0])
    r, out = run_family(ctx, p, K_CHUNK, True, "power law across a chunk")
    assert r["n_domain"] > 0 and np.isnan(out["margins"][:, np.isnan(r["costs"])]).all()
    o = both(out)
    assert np.all(o["n_viol"][:, EVERYBODY] == r["n_ok"])


@pytest.mark.parametrize("closed", [False, True])
def test_pendulum_under_its_own_noise(closed):
    """A source model under rat_user_noise; PEND_NAN draws NaN beyond three standard deviations (DomainErrors whose trajectories hold NaN
    from that step on).  K = 65536 + 5 crosses a chunk once."""
    N = 4
    x_nom, l, L = um.pend_policy(N)
    ctx = rat.Context(pend_problem(um.PEND_NAN, N, [0.1, 0.05]))
    for K in (5, 65) + ((K_CHUNK,) if closed else ()):
        xa, La = (x_nom, L) if closed else (x_nom[0], None)
        r = ctx.policy_evaluate_noise(xa, l, La, noise=rat.UserNoise(1, 0, seed=21), K=K, want_costs=True, want_trajectories=True)
        evs = event_set(r["x"], r["u"], r["costs"], np.random.default_rng(K))
        out = check(ctx, r["x"], r["u"], r["costs"], evs, (0.2,), (0.0, 1.0), f"pendulum K={K} closed={closed}")
        named_checks(both(out), N, r["n_ok"])
        if K == K_CHUNK:
            assert r["n_domain"] > 0


def test_a_one_step_linear_event_is_the_trajectory_mean():
    """For the event z_j + b at step t alone, MARGIN_MEAN - b is policy_worst_case_trajectory's mean of coordinate j at step t."""
    prob, x0, l, L = family(0, 3)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)
    ctx.policy_evaluate(x_det, l, L, K=301, seed=4)
    picks = [(0, 0), (5, 1), (11, 3), (12, 0), (15, 2)]                # (coordinate of (x, u), step)
    evs = [rat.halfspace(np.eye(16)[j], 0.5, steps=t) for j, t in picks]
    bounds, thetas = (0.1, np.inf), (0.0, 0.4)
    ev = both(ctx.policy_events(evs, kl_bounds=bounds, thetas=thetas))
    tr = both(ctx.policy_worst_case_trajectory(kl_bounds=bounds, thetas=thetas))
    for i, (j, t) in enumerate(picks):
        mean = tr["mean_x"][:, t, j] if j < 12 else tr["mean_u"][:, t, j - 12]
        sc = 0.5 + np.abs(mean).max()
        assert np.all(np.abs((ev["margin_mean"][:, i] - 0.5) - mean) <= TOL_MODEL * sc), (j, t)


def test_same_bits_again_row_by_row_and_a_saturated_row():
    prob, x0, l, L = family(0, 3)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)
    r = ctx.policy_evaluate(x_det, l, L, K=301, seed=4, want_costs=True)
    x, u, cost, _ = ctx.rollout_noisy(x_det, l, L, K=301, seed=4)
    evs = event_set(x, u, cost, np.random.default_rng(1))
    bounds, thetas = (0.01, 0.3, np.inf), (0.0, 0.4)
    a = ctx.policy_events(evs, kl_bounds=bounds, thetas=thetas, want_steps=True, want_margins=True)
    b = ctx.policy_events(evs, kl_bounds=bounds, thetas=thetas, want_steps=True, want_margins=True)
    for part in ("bounds", "thetas"):
        same_bits(a[part], b[part], part)
    assert np.array_equal(a["margins"], b["margins"])
    assert list(a["bounds"]["flag"]) == [0, 0, 1]
    for i, d in enumerate(bounds):
        one = ctx.policy_events(evs, kl_bounds=(d,), want_steps=True)["bounds"]
        for k in one:
            assert np.array_equal(one[k][0], a["bounds"][k][i], equal_nan=True), (i, k)
    one = ctx.policy_events(evs, thetas=(0.4,), want_steps=True)["thetas"]
    for k in one:
        assert np.array_equal(one[k][0], a["thetas"][k][1], equal_nan=True), k
    # the saturated row reports the events of the rollout that costs the most
    k = int(np.argmax(cost))
    viol = a["margins"][:, k] > 0
    assert np.array_equal(a["bounds"]["prob"][2], np.append(viol, viol.any()).astype(float))
    assert np.array_equal(a["bounds"]["margin_mean"][2][:9], a["margins"][:, k])
    # margins are a sample like the costs: their own tail risk (and the replay has nothing left after it)
    tr = ctx.policy_tail_risk([0.9], costs=a["margins"][3])
    assert tr["flag"][0] == 0 and tr["var"][0] <= tr["cvar"][0] <= a["thetas"]["margin_max"][0, 3]
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no evaluation"):
        ctx.policy_events(evs, thetas=(0.0,))


def test_a_changed_problem_is_caught_and_the_handle_goes_on():
    N = 3
    x_nom, l, L = um.pend_policy(N)
    ctx = rat.Context(pend_problem(um.PEND_STATE, N, um.PEND_STATE_P))
    noise = rat.UserNoise(3, 0, seed=6)
    ev = [rat.halfspace([1.0, 0.0], -1.0)]
    ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=100)
    good = ctx.policy_events(ev, thetas=(0.0,))
    ctx.set_params([0.1, 0.25, 0.02])
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*changed since the evaluation"):
        ctx.policy_events(ev, thetas=(0.0,))
    assert ctx.policy_evaluate_noise(x_nom, l, L, noise=noise, K=100)["n_ok"] == 100
    other = ctx.policy_events(ev, thetas=(0.0,))
    assert not np.array_equal(other["thetas"]["margin_mean"], good["thetas"]["margin_mean"])


def test_refusals():
    prob, x0, l, L = family(1, 3)
    ctx = rat.Context(prob)
    x_det = ctx.rollout_open(x0, l)
    ev = [rat.halfspace([1.0, 0.0], 0.0)]
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no evaluation"):                    # nothing to replay yet
        ctx.policy_events(ev, thetas=(0.0,))
    ctx.policy_evaluate(x_det, l, L, K=20, seed=1)
    for kw in (dict(), dict(kl_bounds=(-0.1,)), dict(kl_bounds=(np.nan,)), dict(thetas=(np.inf,)), dict(thetas=(-1.0,)),
               dict(kl_bounds=np.ones(17)), dict(thetas=np.ones(17))):                       # rat_policy_worst_case's argument refusals
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG"):
            ctx.policy_events(ev, **kw)
    bad = ([], ev * 17, [rat.halfspace([1.0, 0.0], 0.0, steps=(2, 1))], [rat.halfspace([1.0, 0.0], 0.0, steps=4)],
           [rat.halfspace([1.0, 0.0], 0.0, steps=(-1, 2))], [rat.halfspace([np.nan, 0.0], 0.0)], [rat.halfspace([1.0, 0.0], np.inf)],
           [rat.quadratic_event(np.array([[1.0, np.inf], [0.0, 1.0]]), [0.0, 0.0], 0.0)])
    for evs in bad:                                                                          # the events' own
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG"):
            ctx.policy_events(evs, thetas=(0.0,))
    assert ctx.policy_events(ev, thetas=(0.0,))["thetas"]["event_flag"][0, 0] == 0           # ... leave the handle usable
    ctx.policy_worst_case(kl_bounds=(0.1,), costs=np.arange(20.0))                           # uploaded costs are no evaluation's
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no evaluation"):
        ctx.policy_events(ev, thetas=(0.0,))
    z = np.random.default_rng(0).standard_normal((8, 3, 2))
    ctx.policy_evaluate(x_det, l, L, z=z)                                                    # injected draws are not kept
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*injected"):
        ctx.policy_events(ev, thetas=(0.0,))
    # a source model under N(0, W); and under its sampler with injected draws
    N = 3
    x_nom, pl, pL = um.pend_policy(N)
    src = rat.Context(pend_problem(um.PEND_STATE, N, um.PEND_STATE_P))
    src.policy_evaluate(x_nom, pl, pL, K=16, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rat_user_noise"):
        src.policy_events(ev, thetas=(0.0,))
    src.policy_evaluate_noise(x_nom, pl, pL, noise=rat.UserNoise(3, 0, zn=np.zeros((4, N, 3))))
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*injected"):
        src.policy_events(ev, thetas=(0.0,))
    assert src.policy_evaluate_noise(x_nom, pl, pL, noise=rat.UserNoise(3, 0, seed=1), K=16)["n_ok"] == 16
    assert src.policy_events(ev, thetas=(0.0,))["thetas"]["flag"][0] == 0
    # general sizes
    wide_prob, wx0, wu = rat.synthetic_lq_problem(n=16, m=4, N=5, seed=3, w=1e-2)
    wide = rat.Context(wide_prob)
    wide.policy_evaluate(wx0, wu, K=8, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*n <= 12"):
        wide.policy_events([rat.halfspace(np.ones(16), 0.0)], thetas=(0.0,))
    # too many rows x steps for the partial sums: the message says how many fit
    long_prob = rat.LQRiskSensitiveProblem(np.eye(2), np.eye(2), Q=np.eye(2), R=np.eye(2), N=3000, W=np.eye(2), Qf=np.eye(2))
    lc = rat.Context(long_prob)
    lc.policy_evaluate(np.zeros(2), np.zeros((3000, 2)), K=4, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*64 MiB.*16 rows fit"):
        lc.policy_events(ev, kl_bounds=0.1 * np.arange(1, 11), thetas=0.1 * np.arange(10), want_steps=True)
    assert lc.policy_events(ev, kl_bounds=(0.1,), want_steps=True)["bounds"]["step"].shape == (1, 2, 3001)


def test_an_empty_sample_is_nan():
    """Every rollout of the power-law problem fails when it starts below zero: RAT_WC_EMPTY rows, NaN slots, the flag alone is kept."""
    prob, _, l, _ = family(2, 3)
    ctx = rat.Context(prob)
    r = ctx.policy_evaluate(np.array([-0.5, -0.5]), l, K=9, seed=1)
    assert r["n_ok"] == 0
    out = ctx.policy_events([rat.halfspace([1.0, 0.0], 0.0)], kl_bounds=(0.1,), thetas=(0.0,), want_steps=True, want_margins=True)
    for part in ("bounds", "thetas"):
        assert out[part]["flag"][0] == 2 and np.all(out[part]["event_flag"] == 2)
        for k in ("prob", "prob_se", "margin_mean", "margin_max", "first_mean", "n_viol", "prob_robust", "step"):
            assert np.isnan(out[part][k]).all(), k
    assert np.isnan(out["margins"]).all()
