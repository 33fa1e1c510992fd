"""rat_policy_tail_risk without a device: the NumPy model of the device's select and sums (tail_risk_model.py) against an independent answer
from the sorted sample, the identities of the quantile and the conditional value at risk, the inequality against the KL-ball bound of
worst_case_model.py, the flags, and the symbol, its declarations and its argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ratilqr.jl_amd as rat
from ratilqr.jl_amd import _native as nv
from tail_risk_model import EMPTY, NONFINITE, OK, SATURATED, SLOTS, direct, key_of, tail_risk, value_of
from worst_case_model import worst_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ratilqr.h")).read()
ALPHAS = (0.0, 0.5, 0.9, 0.99, 1.0 - 1e-12)


def close(a, b, rtol):
    return a == b or abs(a - b) <= rtol * abs(b)


def costs_of(K, seed=None):
    rng = np.random.default_rng(K if seed is None else seed)
    return 3.0 + 2.0 * rng.standard_normal(K) ** 2                   # chi-square-like: a heavy right tail


# ---- 1. the model against the independent answer ----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 257, 5000])
def test_model_agrees_with_the_sorted_sample(K):
    """VAR, c_gt, c_eq and FLAG exactly; CVAR, TAIL_N and KL to 1e-11, CVAR_SE and ESS to 1e-9 (the bounds of test_cpu_worst_case.py for
    fixed-order sums of this length)."""
    J = costs_of(K)
    got = tail_risk(J, ALPHAS)
    for i, al in enumerate(ALPHAS):
        ref = direct(J, al)
        assert got["flag"][i] == ref["flag"], (K, al)
        assert got["var"][i] == ref["var"] and got["c_gt"][i] == ref["c_gt"] and got["c_eq"][i] == ref["c_eq"], (K, al)
        assert got["var"][i] == np.sort(J)[ref["k"] - 1]
        for key in ("cvar", "tail_n", "kl"):
            assert close(got[key][i], ref[key], 1e-11), (K, al, key, got[key][i], ref[key])
        if ref["flag"] == SATURATED:
            assert got["var"][i] == got["cvar"][i] == J.max() and np.isnan(got["cvar_se"][i]) and got["ess"][i] == ref["ess"]
            continue
        assert close(got["ess"][i], ref["ess"], 1e-9), (K, al, got["ess"][i], ref["ess"])
        if K >= 2:
            assert close(got["cvar_se"][i], ref["cvar_se"], 1e-9), (K, al, got["cvar_se"][i], ref["cvar_se"])
        else:
            assert np.isnan(got["cvar_se"][i]) and np.isnan(ref["cvar_se"])
    # which (K, alpha) are not saturated: n - n alpha >= 1
    assert (got["flag"] == OK).sum() == {1: 1, 2: 2, 3: 2, 257: 4, 5000: 4}[K]


def test_keys_are_monotone_and_the_select_skips_the_common_prefix():
    v = np.array([-np.inf, -1e300, -2.5, -5e-324, -0.0, 0.0, 5e-324, 1e-310, 2.5, np.nextafter(2.5, 3), 1e300, np.inf])
    k = key_of(v)
    assert k[4] == k[5] and np.all(np.diff(k.astype(object)) >= 0) and np.all(np.diff(k.astype(object))[[0, 1, 2, 3, 5, 6, 7, 8, 9, 10]] > 0)
    assert [value_of(q) for q in k] == [x + 0.0 for x in v.tolist()]
    # costs in [3, 4) share sign, exponent and the top mantissa bit: the first byte and half the second; all-equal costs need no sweep
    rng = np.random.default_rng(4)
    assert tail_risk(3.0 + rng.random(1000), (0.5,))["sweeps"] == 7
    assert tail_risk(3.0 + 2.0 ** -30 * rng.random(1000), (0.5,))["sweeps"] == 3
    assert tail_risk(np.full(300, 2.5), (0.0, 0.5))["sweeps"] == 0
    assert tail_risk(rng.standard_normal(1000), (0.5,))["sweeps"] == 8          # mixed signs: from the first digit


# ---- 2. identities ------------------------------------------------------------------------------------------------------------------
def test_identities_of_the_quantile_and_the_cvar():
    J = costs_of(5000)
    al = np.concatenate([[0.0], np.linspace(0.05, 0.95, 10), [0.99, 0.999, 0.9998]])
    r = tail_risk(J, al)
    assert np.all(r["flag"] == OK)
    assert r["var"][0] == J.min() and close(r["cvar"][0], J.mean(), 1e-13) and r["kl"][0] == 0.0 and r["ess"][0] == 5000 and r["tail_n"][0] == 5000
    assert close(r["cvar_se"][0], J.std(ddof=1) / np.sqrt(5000), 1e-12)
    assert np.all(np.diff(r["cvar"]) >= 0) and np.all(np.diff(r["var"]) >= 0) and np.all(r["cvar"] >= r["var"]) and r["cvar"][-1] <= J.max()
    assert np.all(np.diff(r["kl"]) > 0) and np.all(np.diff(r["ess"]) < 0)
    for a in (0.0, 0.5, 0.9, 0.99, 0.99991):                         # the last: n alpha = 4999.55 is no integer, the atom at v is split
        g = tail_risk(J, (a,), want_weights=True)
        w = g["weights"]
        assert abs(w.sum() - 1.0) <= 1e-14 and close(w @ J, g["cvar"][0], 1e-12), a
        assert close(1.0 / (w * w).sum(), g["ess"][0], 1e-12) and np.all(w[J < g["var"][0]] == 0.0)
        pos = w > 0
        assert abs((w[pos] * np.log(5000 * w[pos])).sum() - g["kl"][0]) <= 1e-12 * max(g["kl"][0], 1e-3)
        assert np.allclose(w, direct(J, a)["weights"], rtol=1e-12, atol=0.0)


def test_heavy_ties_the_ru_form_equals_the_sorted_form():
    """Costs rounded to one decimal: some forty distinct values among 5000.  The Rockafellar-Uryasev form v + sum (J - v)^+ / (n - a) needs
    no special case for the ties at v or the fractional atom; the sorted form is direct's."""
    J = np.round(costs_of(5000), 1)
    assert np.unique(J).size < 300
    split = 0
    for al in (0.0, 0.1, 0.5, 0.777, 0.9, 0.99, 0.9993, 1.0 - 1e-12):
        g, ref = tail_risk(J, (al,), want_weights=True), direct(J, al)
        assert g["flag"][0] == ref["flag"] and g["var"][0] == ref["var"] and g["c_eq"][0] == ref["c_eq"] and g["c_gt"][0] == ref["c_gt"], al
        assert close(g["cvar"][0], ref["cvar"], 1e-11) and close(g["kl"][0], ref["kl"], 1e-11) and close(g["ess"][0], ref["ess"], 1e-9), al
        assert abs(g["weights"].sum() - 1.0) <= 1e-14 and close(g["weights"] @ J, g["cvar"][0], 1e-12), al
        if ref["flag"] == OK:
            r = g["tail_n"][0] - g["c_gt"][0]
            assert 0.0 <= r <= g["c_eq"][0]
            split += 0.0 < r < g["c_eq"][0]
    assert split >= 4                                                # the atom at v is split at most levels


@pytest.mark.parametrize("K", [257, 5000])
def test_cvar_is_below_the_worst_case_over_its_own_kl_ball(K):
    """CVaR is the worst-case expectation over the densities dp/dq <= 1 / (1 - alpha); the tail distribution attains it and has
    KL(p || q) = KL, so the KL-ball bound at that radius cannot be below it."""
    J = costs_of(K)
    r = tail_risk(J, ALPHAS)
    for i, al in enumerate(ALPHAS):
        b = worst_case(J, kl_bounds=[r["kl"][i]])["bounds"]["bound"][0]
        assert r["cvar"][i] <= b * (1.0 + 1e-11), (K, al, r["cvar"][i], b)
        assert r["kl"][i] >= 0.0


# ---- 3. flags ------------------------------------------------------------------------------------------------------------------------
def test_saturation_empty_and_nonfinite():
    """K = 10: at alpha = 0.9 the tail is one rollout, the row is OK and CVaR is the maximum; at 0.95 n - a = 0.5 < 1 and the row is SATURATED
    by the flag's definition (CVaR is the maximum there too)."""
    J = costs_of(10)
    r = tail_risk(J, (0.9, 0.95, 0.90000001), want_weights=True)
    assert r["flag"].tolist() == [OK, SATURATED, SATURATED]
    assert r["var"][0] == np.sort(J)[8] and close(r["cvar"][0], J.max(), 1e-15) and close(r["ess"][0], 1.0, 1e-12)   # n - a = 1: the maximum alone
    for i in (1, 2):
        assert r["var"][i] == r["cvar"][i] == J.max() and np.isnan(r["cvar_se"][i]) and r["ess"][i] == 1.0 and close(r["kl"][i], np.log(10.0), 1e-15)
    assert r["tail_n"][1] == 10 - 10 * 0.95 and r["tail_n"][1] < 1.0
    T = np.array([1.0, 5.0, 2.0, np.nan, 5.0, 5.0, 0.5])
    s = tail_risk(T, (0.9,), want_weights=True)
    assert s["flag"][0] == SATURATED and s["var"][0] == 5.0 and s["ess"][0] == 3.0 and close(s["kl"][0], np.log(2.0), 1e-15)
    assert np.array_equal(s["weights"], np.where(T == 5.0, 1.0 / 3.0, 0.0))
    e = tail_risk(np.full(7, np.nan), (0.0, 0.5), want_weights=True)
    assert np.all(e["flag"] == EMPTY) and all(np.all(np.isnan(e[k])) for k in SLOTS if k not in ("flag", "alpha")) and np.all(e["weights"] == 0.0)
    assert direct(np.full(7, np.nan), 0.5)["flag"] == EMPTY
    for inf in (np.inf, -np.inf):
        Ji = costs_of(300); Ji[17] = inf
        f = tail_risk(Ji, (0.0, 0.5))
        assert np.all(f["flag"] == NONFINITE) and all(np.all(np.isnan(f[k])) for k in SLOTS if k not in ("flag", "alpha"))
        assert direct(Ji, 0.5)["flag"] == NONFINITE
    same = tail_risk(np.full(300, 2.5), (0.0, 0.5, 0.999))
    assert same["flag"].tolist() == [OK, OK, SATURATED] and same["var"].tolist() == [2.5] * 3 and same["cvar"].tolist() == [2.5] * 3
    assert same["ess"].tolist() == [300, 300, 300] and np.all(np.abs(same["kl"]) <= 1e-15)
    z = tail_risk(np.array([-1.0, -0.0, 0.0, 0.0, 2.0]), (0.3, 0.5))  # -0.0 counts as +0.0: three ties at zero
    assert z["var"].tolist() == [0.0, 0.0] and z["c_eq"].tolist() == [3.0, 3.0] and not np.signbit(z["var"]).any()


# ---- 4. the library without a device ------------------------------------------------------------------------------------------------
def test_symbol_header_mirrors_and_refusals():
    """Fails on a tree without the feature: the symbol, its declarations and the wrappers."""
    L = nv.lib()
    assert hasattr(L, "rat_policy_tail_risk") and "rat_policy_tail_risk" in nv.EXPORTS
    assert re.search(r"rat_rc\s+rat_policy_tail_risk\s*\(\s*rat_handle h,\s*const double \*cost,\s*int64_t K,\s*const double \*alpha,\s*int32_t n_alpha,"
                     r"\s*double \*rows_out,\s*double \*weights_out\)", HEADER)
    for i, name in enumerate(("ALPHA", "VAR", "CVAR", "CVAR_SE", "TAIL_N", "ESS", "KL", "FLAG")):
        assert re.search(rf"#define RAT_TR_{name}\s+{i}\b", HEADER), name
        assert nv.TR_SLOTS[i] == name.lower() == SLOTS[i]
    for name, val in (("NSTAT", 8), ("OK", 0), ("SATURATED", 1), ("EMPTY", 2), ("NONFINITE", 3)):
        assert re.search(rf"#define RAT_TR_{name}\s+{val}\b", HEADER), name
        assert getattr(nv, "TR_" + name) == val
    assert (OK, SATURATED, EMPTY, NONFINITE) == (nv.TR_OK, nv.TR_SATURATED, nv.TR_EMPTY, nv.TR_NONFINITE)
    al, out, J = np.array([0.5]), np.zeros(8), np.ones(4)
    rc = L.rat_policy_tail_risk(None, nv.P(J), C.c_int64(4), nv.P(al), C.c_int32(1), nv.P(out), None)
    assert rc == 1 and "null handle" in L.rat_last_error().decode()
    assert callable(rat.Context.policy_tail_risk)
    from ratilqr.jl_amd.generic import GenericContext
    assert "policy_tail_risk" in vars(GenericContext)
    jl = open(os.path.join(ROOT, "julia", "RATiLQRAMD.jl")).read()
    assert "(:rat_policy_tail_risk, LIB)" in jl and re.search(r"export[^\n]*(\n[^\n]*)*policy_tail_risk", jl)
    assert "policy_tail_risk(" in open(os.path.join(ROOT, "julia", "runtests.jl")).read()


def test_argument_refusals_need_no_device():
    """What the arguments alone decide is refused before the handle is looked at: alpha, n_alpha, the outputs, K with host costs.  The
    refusals that need a handle's state (cost == NULL) are in test_gpu_tail_risk.py."""
    L = nv.lib()
    out, J = np.zeros(16 * 8), np.ones(4)

    def call(al, n=None, cost=J, K=4, rows=out):
        al = None if al is None else np.asarray(al, dtype=np.float64)
        rc = L.rat_policy_tail_risk(None, nv.P(cost), C.c_int64(K), nv.P(al), C.c_int32(len(al) if n is None else n), nv.P(rows), None)
        return rc, L.rat_last_error().decode()
    for al in ([np.nan], [-0.1], [1.0], [1.5], [0.5, np.inf], [0.5, -1e-300]):
        rc, msg = call(al)
        assert rc == 1 and "alpha must be in [0, 1)" in msg, al
    for n in (0, 17, -1):
        rc, msg = call(np.full(17, 0.5), n=n)
        assert rc == 1 and "n_alpha must be in 1 .. 16" in msg, n
    for kw in (dict(al=None, n=1), dict(al=[0.5], rows=None)):
        rc, msg = call(**kw)
        assert rc == 1 and "null alpha / rows_out" in msg
    rc, msg = call([0.5], K=0)
    assert rc == 1 and "K must be positive" in msg
    rc, msg = call([0.5], K=(1 << 27) + 1)
    assert rc == 1 and "2^27" in msg
    for kw in (dict(), dict(cost=None, K=0)):                        # nothing left to refuse but the handle
        rc, msg = call([0.0, 0.5], **kw)
        assert rc == 1 and "null handle" in msg
    assert out.tolist() == [0.0] * 128                               # no refusal wrote a row
