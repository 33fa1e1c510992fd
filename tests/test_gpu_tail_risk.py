"""The tail risk of a policy on the device (rat_policy_tail_risk, Context.policy_tail_risk; csrc/policy_mc.hip): against the NumPy restatement
of the device's schedule (tests/tail_risk_model.py), an independent answer from the sorted sample, the samples a radix select gets wrong,
its own repeatability promises, rat_policy_evaluate and rat_policy_worst_case on the same costs, and a source model whose sampler fails
some rollouts."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
import user_noise_model as um
from tail_risk_model import EMPTY, NONFINITE, OK, SATURATED, SLOTS, direct, rank_of, tail_risk
from test_gpu_policy_mc import noisy_problems
from test_gpu_user_noise import pend_problem

pytestmark = pytest.mark.gpu
KEYS = tuple(k for k in SLOTS if k != "flag")
EXACT = ("alpha", "var", "tail_n")


def same(a, b, rtol):
    """equal where both are NaN or the same infinity, within rtol elsewhere"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= rtol * np.abs(b))))


def bits(a, b):
    """the same bits (NaN equals NaN; a quantile of zero is +0.0 on both sides)"""
    return all(np.array_equal(np.asarray(a[k]).view(np.int64), np.asarray(b[k]).view(np.int64)) for k in SLOTS)


@pytest.fixture(scope="module")
def ctx():
    """a handle without a problem: host costs need none"""
    return rat.Context(None)


def costs_of(K):
    rng = np.random.default_rng(K)
    return 3.0 + 2.0 * rng.standard_normal(K) ** 2


def whole_level(K):
    """a level m / K near one third whose product with K is the integer m again"""
    for m in range(K // 3, K):
        if m > 0 and float(np.float64(K) * np.float64(m / K)) == m:
            return m / K
    return 0.0


def levels16(K):
    """sixteen levels: alpha[0] = 0.9 carries the weights; 0; up to 1 - 1e-9; 0.9 twice; one with n alpha an integer"""
    return np.array([0.9, 0.0, 0.5, 0.75, 0.95, 0.99, 0.999, 0.9999, 1.0 - 1e-5, 1.0 - 1e-6, 1.0 - 1e-9, 0.25, 0.1, 0.9, whole_level(K), 0.6])


def against_the_model(got, mdl, what):
    assert np.array_equal(got["flag"], mdl["flag"]), what
    for key in KEYS:
        if key in EXACT:
            assert np.array_equal(got[key].view(np.int64), mdl[key].view(np.int64)), (what, key, got[key], mdl[key])
        elif key == "kl":                                             # (a log's argument carries 1e-16: that much is absolute in KL, which can be 0)
            assert same(got[key], mdl[key], 1e-12) or np.all(np.abs(got[key] - mdl[key]) <= 1e-12 * np.abs(mdl[key]) + 1e-15), (what, got[key], mdl[key])
        else:
            assert same(got[key], mdl[key], 1e-12), (what, key, got[key], mdl[key])


# ---- 1. injected costs at the sizes where the grid can go wrong ------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 255, 256, 257, 65535, 65536, 65537, 70001])
def test_injected_costs_against_the_model_and_the_sorted_sample(ctx, K):
    """T = 65536 is the grid's stride: one element per lane, then a second row.  Against the model VAR, FLAG and TAIL_N bit for bit (a
    count has no rounding, a = n alpha is one product) and 1e-12 for the rest (the order of summation is restated: what is left are ulps
    of log and contracted multiply-adds); against the sorted sample 1e-11, and 1e-9 for CVAR_SE and ESS."""
    J = costs_of(K)
    al = levels16(K)
    got = ctx.policy_tail_risk(al, costs=J, want_weights=True)
    mdl = tail_risk(J, al, want_weights=True)
    against_the_model(got, mdl, K)
    assert got["weights"].shape == (K,) and same(got["weights"], mdl["weights"], 1e-12)
    whole = float(np.float64(K) * np.float64(al[14]))
    assert whole == round(whole)
    srt = np.sort(J)
    for i, a in enumerate(al):
        ref = direct(J, a)
        assert got["flag"][i] == ref["flag"], (K, a)
        assert got["var"][i] == ref["var"] == srt[rank_of(K, a)[1] - 1] or ref["flag"] == SATURATED, (K, a)
        for key in ("cvar", "tail_n", "kl"):
            assert same(got[key][i], ref[key], 1e-11), (K, a, key, got[key][i], ref[key])
        for key in ("cvar_se", "ess"):
            assert same(got[key][i], ref[key], 1e-9), (K, a, key, got[key][i], ref[key])
    assert same(got["weights"], direct(J, al[0])["weights"], 1e-12)
    assert all(got[k][0] == got[k][13] or np.isnan(got[k][0]) for k in SLOTS)       # the duplicate level: the same row


# ---- 2. what a radix select gets wrong --------------------------------------------------------------------------------------------------
def _hard_cases():
    K = 70001
    rng = np.random.default_rng(70)
    chain = [2.5]
    for _ in range(299):
        chain.append(np.nextafter(chain[-1], np.inf))
    mixed = rng.standard_normal(K)
    mixed[::7] = 0.0
    mixed[3::7] = -0.0
    mixed[5::11] = 5e-324 * rng.integers(1, 1000, mixed[5::11].size)          # denormals of either sign
    mixed[6::13] = -5e-324 * rng.integers(1, 1000, mixed[6::13].size)
    third = costs_of(K)
    third[::3] = np.nan
    return {
        "all equal": np.full(K, 2.5),
        "two values": np.where(rng.random(K) < 0.3, 7.25, 1.5),
        "neighbours": rng.permutation(np.resize(np.array(chain), K)),             # 300 values that differ in the last digit alone
        "mixed signs": mixed,
        "every third NaN": third,
        "one decimal": np.round(costs_of(K), 1),
    }


HARD = _hard_cases()


@pytest.mark.parametrize("name", list(HARD))
def test_samples_a_radix_select_gets_wrong(ctx, name):
    """VAR is np.sort(J_ok)[k - 1] bit for bit (zero counts as +0.0); the slots that depend on the counts c_gt and c_eq follow the model to
    1e-12.  The levels 0.3333 and 0.77777 make n alpha no integer, so that with ties the atom at v is split: asserted for the tied cases."""
    J = HARD[name]
    al = np.array([0.0, 0.3333, 0.5, 0.77777, 0.9, 0.999, 1.0 - 1e-9])
    got = ctx.policy_tail_risk(al, costs=J, want_weights=True)
    mdl = tail_risk(J, al, want_weights=True)
    srt = np.sort(J[~np.isnan(J)])
    n = srt.size
    for i, a in enumerate(al):
        k = rank_of(n, a)[1]
        want = srt[k - 1] + 0.0
        assert got["var"][i] == want and np.float64(got["var"][i]).view(np.int64) == np.float64(want).view(np.int64), (name, a, got["var"][i], want)
    against_the_model(got, mdl, name)
    assert same(got["weights"], mdl["weights"], 1e-12) and abs(got["weights"].sum() - 1.0) <= 1e-12
    assert np.all(got["weights"][np.isnan(J)] == 0.0)
    if name in ("all equal", "two values", "neighbours", "one decimal"):
        r = mdl["tail_n"][[1, 3]] - mdl["c_gt"][[1, 3]]                           # the mass on the atom at v
        assert np.all((0.0 < r) & (r < mdl["c_eq"][[1, 3]])), (name, r, mdl["c_eq"])
    for i in (1, 3):
        ref = direct(J, al[i])
        assert same(got["cvar"][i], ref["cvar"], 1e-11) or abs(got["cvar"][i] - ref["cvar"]) <= 1e-11 * np.abs(srt).max(), (name, al[i])
        assert abs(got["kl"][i] - ref["kl"]) <= 1e-11 * abs(ref["kl"]) + 1e-15 and same(got["ess"][i], ref["ess"], 1e-9), (name, al[i])
    if name == "all equal":
        assert got["flag"].tolist() == [OK] * 6 + [SATURATED] and np.all(got["cvar"] == 2.5) and same(got["ess"], np.full(7, n), 1e-12)


def test_flags_and_weights_of_the_degenerate_samples(ctx):
    S = np.array([1.0, 2.0, 5.0, np.nan, 5.0, 5.0, 0.5])
    s = ctx.policy_tail_risk((0.9, 0.0), costs=S, want_weights=True)
    assert s["flag"].tolist() == [SATURATED, OK] and s["var"][0] == s["cvar"][0] == 5.0 and np.isnan(s["cvar_se"][0]) and s["ess"][0] == 3.0
    assert same(s["kl"][0], np.log(2.0), 1e-15) and np.array_equal(s["weights"], np.where(S == 5.0, 1.0 / 3.0, 0.0))
    assert s["var"][1] == 0.5 and same(s["cvar"][1], 18.5 / 6.0, 1e-15) and s["tail_n"][1] == 6.0
    e = ctx.policy_tail_risk((0.0, 0.5), costs=np.full(7, np.nan), want_weights=True)
    assert np.all(e["flag"] == EMPTY) and np.all(e["weights"] == 0.0) and e["alpha"].tolist() == [0.0, 0.5]
    assert all(np.all(np.isnan(e[k])) for k in KEYS if k != "alpha")
    for inf in (np.inf, -np.inf):
        Ji = costs_of(300); Ji[3] = inf
        f = ctx.policy_tail_risk((0.0, 0.5), costs=Ji)
        assert np.all(f["flag"] == NONFINITE) and all(np.all(np.isnan(f[k])) for k in KEYS if k != "alpha")
    t = ctx.policy_tail_risk((0.9, 0.95), costs=costs_of(10))         # K = 10: one rollout's worth of tail is OK, half a rollout's is not
    assert t["flag"].tolist() == [OK, SATURATED] and same(t["cvar"], np.full(2, costs_of(10).max()), 1e-15)


# ---- 3. the same bits ------------------------------------------------------------------------------------------------------------------
def test_bits_repeat_and_do_not_depend_on_the_company_or_the_origin_of_the_costs():
    prob, x0, l, L = noisy_problems()[1]                             # the 2 x 2 noisy LQ problem
    c = rat.Context(prob)
    ev = c.policy_evaluate(x0, l, thetas=(0.3,), K=5000, seed=3, want_costs=True)
    al = levels16(5000)
    from_dev = c.policy_tail_risk(al, want_weights=True)             # cost = NULL: the evaluation's costs
    again = c.policy_tail_risk(al, want_weights=True)
    assert bits(from_dev, again) and np.array_equal(from_dev["weights"], again["weights"]) and from_dev["weights"].shape == (5000,)
    assert set(from_dev["flag"].tolist()) == {OK, SATURATED}
    from_host = c.policy_tail_risk(al, costs=ev["costs"], want_weights=True)
    assert bits(from_dev, from_host) and np.array_equal(from_dev["weights"], from_host["weights"])
    for i, a in enumerate(al):                                       # a level among fifteen others against the level alone
        one = c.policy_tail_risk((a,), costs=ev["costs"])
        assert all(np.array_equal(one[k][:1].view(np.int64), from_dev[k][i:i + 1].view(np.int64)) for k in SLOTS), (i, a)
    against_the_model(from_dev, tail_risk(ev["costs"], al), "evaluation")


# ---- 4. against the existing calls -----------------------------------------------------------------------------------------------------
def test_against_policy_evaluate_and_the_kl_ball():
    prob, x0, l, L = noisy_problems()[1]
    c = rat.Context(prob)
    ev = c.policy_evaluate(x0, l, K=5000, seed=11, want_costs=True)
    al = np.array([0.0, 0.5, 0.9, 0.99, 0.999, 1.0 - 1e-12])
    r = c.policy_tail_risk(al)
    assert abs(r["cvar"][0] - ev["mean"]) <= 1e-12 * abs(ev["mean"]) and r["tail_n"][0] == ev["n_ok"] == 5000
    assert r["var"][0] == ev["min"] and r["var"][-1] == r["cvar"][-1] == ev["max"] and r["flag"].tolist() == [OK] * 5 + [SATURATED]
    assert np.all((ev["min"] <= r["var"]) & (r["var"] <= r["cvar"]) & (r["cvar"] <= ev["max"])) and np.all(np.diff(r["cvar"]) >= 0)
    assert same(r["cvar_se"][0], ev["se_mean"], 1e-12)
    for i in range(al.size):
        b = c.policy_worst_case(kl_bounds=(r["kl"][i],))["bounds"]["bound"][0]
        assert r["cvar"][i] <= b * (1.0 + 1e-11), (al[i], r["cvar"][i], b)
    # the evaluation is still the handle's: the trajectory moments replay it; after an upload there is nothing to replay
    t = c.policy_worst_case_trajectory(thetas=(0.0,))
    assert t["thetas"]["flag"][0] == 0
    up = c.policy_tail_risk((0.9,), costs=ev["costs"])
    assert up["var"][0] == r["var"][2] and up["cvar"][0] == r["cvar"][2]
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no evaluation to replay"):
        c.policy_worst_case_trajectory(thetas=(0.0,))
    assert bits(c.policy_tail_risk(al), r) and c.debug_get("mc_cost_K") == 5000        # the handle goes on working, on the uploaded costs
    wc = c.policy_worst_case(kl_bounds=(0.1,))["bounds"]             # ... which serve the other function's cost = NULL too
    assert wc["flag"][0] == 0 and ev["mean"] < wc["bound"][0] < ev["max"]


def test_refusals_on_a_live_handle_leave_it_usable():
    prob, x0, l, L = noisy_problems()[1]
    c = rat.Context(prob)
    J = costs_of(100)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no rat_policy_evaluate"):
        c.policy_tail_risk((0.5,))                                   # cost = NULL before any evaluation
    for al in ((-0.1,), (np.nan,), (1.0,), np.full(17, 0.5), ()):
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG"):
            c.policy_tail_risk(al, costs=J)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*K must be positive"):
        c.policy_tail_risk((0.5,), costs=np.zeros(0))
    c.policy_evaluate(x0, l, K=64, seed=1)
    import ctypes as C
    L_ = rat.native.lib()
    a, out = np.array([0.5]), np.zeros(8)
    rc = L_.rat_policy_tail_risk(c.h, None, C.c_int64(65), rat.native.P(a), C.c_int32(1), rat.native.P(out), None)
    assert rc == 1 and "64" in L_.rat_last_error().decode()          # K mismatch
    rc = L_.rat_policy_tail_risk(c.h, None, C.c_int64(64), rat.native.P(a), C.c_int32(1), rat.native.P(out), None)
    assert rc == 0 and out[7] == OK and out[4] == 32.0
    assert c.policy_tail_risk((0.5,))["cvar"][0] == out[2]            # K = 0 stands for that K
    h = c.policy_tail_risk((0.5,), costs=J)
    assert same(h["cvar"][0], direct(J, 0.5)["cvar"], 1e-11) and c.debug_get("mc_cost_K") == 100


# ---- 5. a source model whose sampler fails some rollouts ------------------------------------------------------------------------------
def test_source_model_with_domain_errors():
    N, K = 5, 3000
    x0, l = np.array([0.4, -0.3]), 0.1 * np.ones((N, 1))
    c = rat.Context(pend_problem(um.PEND_NAN, N, [0.1, 0.05]))
    r = c.policy_evaluate_noise(x0, l, noise=rat.UserNoise(1, 0, seed=77), K=K, want_costs=True)
    bad = np.isnan(r["costs"])
    assert 0 < r["n_domain"] == bad.sum() < K // 10                  # a normal beyond three sigma in some of the 15 000 draws
    al = (0.9, 0.0, 0.5, 0.99)
    got = c.policy_tail_risk(al, want_weights=True)
    mdl = tail_risk(r["costs"], al, want_weights=True)
    against_the_model(got, mdl, "source")
    assert np.all(got["flag"] == OK) and got["tail_n"][1] == r["n_ok"] and got["var"][1] == r["min"]
    assert abs(got["cvar"][1] - r["mean"]) <= 1e-12 * abs(r["mean"])
    w = got["weights"]
    assert w.shape == (K,) and np.all(w[bad] == 0.0) and abs(w.sum() - 1.0) <= 1e-12 and same(w, mdl["weights"], 1e-12)
    assert same(got["cvar"][0], direct(r["costs"], 0.9)["cvar"], 1e-11) and same(w[~bad] @ r["costs"][~bad], got["cvar"][0], 1e-12)
