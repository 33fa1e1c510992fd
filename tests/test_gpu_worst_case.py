"""The worst-case cost of a policy within the KL ball on the device (rat_policy_worst_case, Context.policy_worst_case; csrc/policy_mc.hip):
against the NumPy restatement of the device's schedule (tests/worst_case_model.py), an independent extended-precision bisection, its own
repeatability promises, rat_policy_evaluate's entropic risk, the closed-form LEQG value, and a source model under a user-written sampler."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
import user_noise_model as um
from leqg_exact import breakdown_theta, exact_value, random_lq
from test_gpu_policy_mc import noisy_problems
from test_gpu_user_noise import pend_problem
from worst_case_model import EMPTY, NONFINITE, OK, SATURATED, SLOTS, direct, worst_case

pytestmark = pytest.mark.gpu
DS = (0.0, 1e-6, 0.1, 1.0, 3.0)
KEYS = tuple(k for k in SLOTS if k != "flag")


def same(a, b, rtol):
    """equal where both are NaN or the same infinity, within rtol elsewhere"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= rtol * np.abs(b))))


def bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in SLOTS)


@pytest.fixture(scope="module")
def ctx():
    """a handle without a problem: host costs need none"""
    return rat.Context(None)


def costs_of(K):
    rng = np.random.default_rng(K)
    return 3.0 + 2.0 * rng.standard_normal(K) ** 2


# ---- 1. injected costs at the sizes where the grid can go wrong ------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 255, 256, 257, 65535, 65536, 65537, 70001])
def test_injected_costs_against_the_model_and_the_bisection(ctx, K):
    """T = 65536 is the grid's stride: one element per lane, then a second row.  Against the model 1e-12 (the order of summation is
    restated: what is left are ulps of exp / expm1 / log and contracted multiply-adds), against the bisection 1e-11 for BOUND, TILT_MEAN
    and KL and 1e-9 for theta* (the bound is flat at theta*; the rest is first order in the theta error)."""
    J = costs_of(K)
    ths = (0.0, 0.05, 0.7, 40.0)
    got = ctx.policy_worst_case(kl_bounds=DS, thetas=ths, costs=J, want_weights=True)
    mdl = worst_case(J, kl_bounds=DS, thetas=ths, want_weights=True)
    for part in ("bounds", "thetas"):
        assert np.array_equal(got[part]["flag"], mdl[part]["flag"]), part
        for key in KEYS:
            assert same(got[part][key], mdl[part][key], 1e-12), (part, key)
    assert got["weights"].shape == (K,) and same(got["weights"], mdl["weights"], 1e-12)
    b = got["bounds"]
    for i, d in enumerate(DS):
        ref = direct(J, d)
        assert b["flag"][i] == ref["flag"], d
        assert same(b["theta"][i], ref["theta"], 1e-9), (d, b["theta"][i], ref["theta"])
        for key in ("bound", "tilt_mean", "kl"):
            assert same(b[key][i], ref[key], 1e-11), (d, key, b[key][i], ref[key])
    assert np.all(got["thetas"]["flag"] == OK) and got["thetas"]["ess"][0] == K and got["thetas"]["theta"].tolist() == list(ths)


# ---- 2. the same bits ------------------------------------------------------------------------------------------------------------------
def test_bits_repeat_and_do_not_depend_on_the_company_or_the_origin_of_the_costs():
    prob, x0, l, L = noisy_problems()[1]                             # the 2 x 2 noisy LQ problem
    c = rat.Context(prob)
    ev = c.policy_evaluate(x0, l, thetas=(0.3,), K=5000, seed=3, want_costs=True)
    ds16 = np.concatenate([[0.0], np.logspace(-6, 0.7, 14), [np.inf]])
    ths = (0.0, 0.01, 0.3)
    from_dev = c.policy_worst_case(kl_bounds=ds16, thetas=ths, want_weights=True)          # cost = NULL: the evaluation's costs
    again = c.policy_worst_case(kl_bounds=ds16, thetas=ths, want_weights=True)
    assert bits(from_dev["bounds"], again["bounds"]) and bits(from_dev["thetas"], again["thetas"])
    assert np.array_equal(from_dev["weights"], again["weights"]) and from_dev["weights"].shape == (5000,)
    assert set(from_dev["bounds"]["flag"].tolist()) == {OK, SATURATED} and from_dev["bounds"]["flag"][-1] == SATURATED
    from_host = c.policy_worst_case(kl_bounds=ds16, thetas=ths, costs=ev["costs"], want_weights=True)
    assert bits(from_dev["bounds"], from_host["bounds"]) and bits(from_dev["thetas"], from_host["thetas"])
    assert np.array_equal(from_dev["weights"], from_host["weights"])
    for i, d in enumerate(ds16):                                     # sixteen bounds in one call against sixteen calls of one
        one = c.policy_worst_case(kl_bounds=(d,), costs=ev["costs"])["bounds"]
        assert all(np.array_equal(one[k][0], from_dev["bounds"][k][i], equal_nan=True) for k in SLOTS), (i, d)
    for i, t in enumerate(ths):
        one = c.policy_worst_case(thetas=(t,), costs=ev["costs"])["thetas"]
        assert all(np.array_equal(one[k][0], from_dev["thetas"][k][i], equal_nan=True) for k in SLOTS), (i, t)
    # the entropic risk of rat_policy_evaluate, recovered from a theta row
    t = from_dev["thetas"]
    assert abs((t["bound"][2] - t["kl"][2] / 0.3) - ev["risk"][0]) <= 1e-12 * abs(ev["risk"][0])
    assert t["tilt_mean"][0] == ev["mean"] and t["bound"][0] == ev["mean"] and t["ess"][0] == ev["n_ok"] and same(t["bound_se"][0], ev["se_mean"], 1e-14)


# ---- 3. theta rows and weights ----------------------------------------------------------------------------------------------------------
def test_theta_rows_and_weights(ctx):
    J = costs_of(70001)
    J[[5, 69999]] = np.nan                                           # two DomainError rollouts
    ok = ~np.isnan(J)
    r = ctx.policy_worst_case(kl_bounds=(0.1, 1e-6), costs=J, want_weights=True)
    b, w = r["bounds"], r["weights"]
    t = ctx.policy_worst_case(thetas=(b["theta"][0], b["theta"][1], 0.0), costs=J)["thetas"]
    for i in (0, 1):                                                 # at theta* a theta row reproduces the bound row
        for key in KEYS:
            assert same(t[key][i], b[key][i], 1e-12), (i, key, t[key][i], b[key][i])
    assert t["theta"][2] == 0.0 and t["kl"][2] == 0.0 and t["ess"][2] == ok.sum() and same(t["bound"][2], J[ok].mean(), 1e-13)
    assert abs(w.sum() - 1.0) <= 1e-12 and abs(w[ok] @ J[ok] - b["tilt_mean"][0]) <= 1e-12 * abs(b["tilt_mean"][0])
    assert np.all(w[~ok] == 0.0) and np.all(w[ok] > 0.0)
    assert same(1.0 / (w[ok] ** 2).sum(), b["ess"][0], 1e-11)
    # without bounds the weights are theta[0]'s
    wt = ctx.policy_worst_case(thetas=(b["theta"][0],), costs=J, want_weights=True)["weights"]
    assert np.array_equal(wt, w)
    # a saturated row: 1 / n_max on the maxima
    S = np.array([1.0, 2.0, 5.0, np.nan, 5.0, 5.0, 0.5])
    s = ctx.policy_worst_case(kl_bounds=(np.log(2.0) + 0.1,), costs=S, want_weights=True)
    assert s["bounds"]["flag"][0] == SATURATED and s["bounds"]["theta"][0] == np.inf and s["bounds"]["ess"][0] == 3.0
    assert s["bounds"]["bound"][0] == s["bounds"]["tilt_mean"][0] == 5.0 and s["bounds"]["tilt_var"][0] == 0.0 and np.isnan(s["bounds"]["bound_se"][0])
    assert same(s["bounds"]["kl"][0], np.log(2.0), 1e-15)
    assert np.array_equal(s["weights"], np.where(S == 5.0, 1.0 / 3.0, 0.0))
    # empty and non-finite samples, all costs equal
    e = ctx.policy_worst_case(kl_bounds=(0.0, 0.1), thetas=(0.5,), costs=np.full(7, np.nan), want_weights=True)
    assert np.all(e["bounds"]["flag"] == EMPTY) and e["thetas"]["flag"][0] == EMPTY and np.all(e["weights"] == 0.0)
    assert all(np.all(np.isnan(e["bounds"][k])) and np.all(np.isnan(e["thetas"][k])) for k in KEYS)
    Ji = costs_of(300); Ji[3] = np.inf
    f = ctx.policy_worst_case(kl_bounds=(0.0, 0.1), thetas=(0.5,), costs=Ji)
    assert np.all(f["bounds"]["flag"] == NONFINITE) and f["thetas"]["flag"][0] == NONFINITE
    assert all(np.all(np.isnan(f["bounds"][k])) and np.all(np.isnan(f["thetas"][k])) for k in KEYS)
    q = ctx.policy_worst_case(kl_bounds=(0.0, 0.1), thetas=(3.0,), costs=np.full(300, 2.5))
    assert q["bounds"]["flag"].tolist() == [OK, SATURATED] and q["bounds"]["bound"].tolist() == [2.5, 2.5] and q["thetas"]["bound"][0] == 2.5
    assert q["thetas"]["kl"][0] == 0.0 and q["thetas"]["ess"][0] == 300


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle_leave_it_usable():
    prob, x0, l, L = noisy_problems()[1]
    c = rat.Context(prob)
    J = costs_of(100)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no rat_policy_evaluate"):
        c.policy_worst_case(kl_bounds=(0.1,))                        # cost = NULL before any evaluation
    for kw in (dict(kl_bounds=(-0.1,)), dict(kl_bounds=(np.nan,)), dict(kl_bounds=np.full(17, 0.1)), dict(thetas=(-1.0,)), dict(thetas=(np.inf,)),
               dict(thetas=np.zeros(17)), dict()):
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG"):
            c.policy_worst_case(costs=J, **kw)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*K must be positive"):
        c.policy_worst_case(kl_bounds=(0.1,), costs=np.zeros(0))     # K = 0 with host costs
    c.policy_evaluate(x0, l, K=64, seed=1)
    L_ = rat.native.lib()
    import ctypes as C
    d, out = np.array([0.1]), np.zeros(8)
    rc = L_.rat_policy_worst_case(c.h, None, C.c_int64(65), rat.native.P(d), C.c_int32(1), None, C.c_int32(0), rat.native.P(out), None, None)
    assert rc == 1 and "64" in L_.rat_last_error().decode()          # K mismatch
    rc = L_.rat_policy_worst_case(c.h, None, C.c_int64(64), rat.native.P(d), C.c_int32(1), None, C.c_int32(0), rat.native.P(out), None, None)
    assert rc == 0 and out[7] == OK and out[1] > 0
    a = c.policy_worst_case(kl_bounds=(0.1,))["bounds"]              # K = 0 stands for that K
    assert np.array_equal(a["bound"], out[2:3])
    # host costs stay in the buffer: a later cost = NULL call uses them, until the next evaluation
    h = c.policy_worst_case(kl_bounds=(0.1,), costs=J)["bounds"]
    assert same(h["bound"][0], direct(J, 0.1)["bound"], 1e-11) and c.debug_get("mc_cost_K") == 100
    assert bits(c.policy_worst_case(kl_bounds=(0.1,))["bounds"], h)
    r = c.policy_evaluate(x0, l, K=64, seed=1, want_costs=True)
    assert np.array_equal(c.policy_worst_case(kl_bounds=(0.1,))["bounds"]["bound"], a["bound"]) and r["n_ok"] == 64


# ---- 5. the closed form ---------------------------------------------------------------------------------------------------------------
def test_bound_is_the_closed_form_dual_of_the_solved_policy():
    """BOUND(d) of K = 200 000 rollouts lies within 5 BOUND_SE of min_theta [exact risk(theta) + d / theta] of the policy that solve returned
    (the problem and policy of test_entropic_risk_of_the_solved_policy_is_the_solvers_value; the exact risk is exact_value's).  d is chosen
    on the CPU from the closed form alone, d = theta_t^2 risk'(theta_t) at theta_t = 0.1 of the open-loop plan's breakdown theta, so that
    the minimiser lies below the 0.15 that the sibling test allows; that the minimum over the grid is interior (such a d exists) and that
    the closed form at twice the minimiser is finite (the estimator's variance is) are asserted before the GPU is touched.  The grid: 25
    points on [0.01, 0.15] of the breakdown, then 21 between the neighbours of the best; the dual is flat at its minimum, so the last
    spacing (0.6 % of theta*) leaves an error of order 1e-5 of d / theta*, far below BOUND_SE."""
    n, m, Nn = 12, 4, 50
    prob, x0, u = random_lq(n, m, Nn, seed=212)
    Z, X0 = np.zeros((Nn, m, n)), np.zeros((Nn + 1, n))
    th_bd = breakdown_theta(prob, x0, u, Z, X0)
    ctx = rat.Context(prob)
    sol = ctx.solve(x0, u, 0.15 * th_bd)
    assert sol["status"] == 0

    def risk(th):
        v, ok = exact_value(prob, x0, sol["l"], None, sol["L"], sol["x"], th)
        assert ok, th
        return v
    t_t = 0.1 * th_bd
    h = 1e-3 * t_t
    d = t_t ** 2 * (risk(t_t + h) - risk(t_t - h)) / (2 * h)          # at the minimiser of risk(theta) + d / theta: risk'(theta) = d / theta^2
    coarse = np.linspace(0.01, 0.15, 25) * th_bd
    dual = np.array([risk(t) + d / t for t in coarse])
    i = int(np.argmin(dual))
    assert d > 0 and 0 < i < coarse.size - 1, (d, i)                  # an interior minimum below 0.15 of the breakdown
    fine = np.linspace(coarse[i - 1], coarse[i + 1], 21)
    dual_f = np.array([risk(t) + d / t for t in fine])
    j = int(np.argmin(dual_f))
    assert abs(fine[j] - t_t) < 0.02 * t_t
    assert exact_value(prob, x0, sol["l"], None, sol["L"], sol["x"], 2.0 * fine[j])[1]        # finite variance at the minimiser
    ctx.policy_evaluate(sol["x"], sol["l"], sol["L"], K=200000, seed=2024)
    b = ctx.policy_worst_case(kl_bounds=(d,))["bounds"]
    assert b["flag"][0] == OK and b["ess"][0] > 1000 and b["bound_se"][0] > 0
    assert abs(b["bound"][0] - dual_f[j]) <= 5.0 * b["bound_se"][0], (b["bound"][0], dual_f[j], b["bound_se"][0], b["theta"][0], fine[j], b["ess"][0])
    assert b["theta"][0] <= 0.15 * th_bd and abs(b["kl"][0] - d) <= 1e-11 * d


# ---- 6. a source model under its own sampler ----------------------------------------------------------------------------------------------
def test_source_model_under_a_user_sampler():
    N, K = 5, 3000
    x_nom, l, L = um.pend_policy(N)
    c = rat.Context(pend_problem(um.PEND_STATE, N, um.PEND_STATE_P))
    r = c.policy_evaluate_noise(x_nom, l, L, noise=rat.UserNoise(3, 0, seed=77), K=K, want_costs=True)
    ds, ths = (0.0, 0.05, 0.5), (0.0, 2.0)
    got = c.policy_worst_case(kl_bounds=ds, thetas=ths, want_weights=True)
    mdl = worst_case(r["costs"], kl_bounds=ds, thetas=ths, want_weights=True)
    for part in ("bounds", "thetas"):
        assert np.array_equal(got[part]["flag"], mdl[part]["flag"]) and np.all(got[part]["flag"] == OK)
        for key in KEYS:
            assert same(got[part][key], mdl[part][key], 1e-12), (part, key)
    assert same(got["weights"], mdl["weights"], 1e-12) and got["weights"].shape == (K,)
    b = got["bounds"]
    assert b["bound"][0] == r["mean"] and r["mean"] < b["bound"][1] < b["bound"][2] < r["max"]
    assert same(b["bound"][1], direct(r["costs"], 0.05)["bound"], 1e-11)
