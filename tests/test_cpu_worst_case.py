"""rat_policy_worst_case without a device: the NumPy model of the device's search and sums (worst_case_model.py) against an independent
extended-precision bisection, the limits and flags of the dual, and the symbol, its declarations and its argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ratilqr.jl_amd as rat
from ratilqr.jl_amd import _native as nv
from worst_case_model import EMPTY, NONFINITE, OK, SATURATED, direct, kl_of, worst_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ratilqr.h")).read()
DS = (0.0, 1e-6, 0.1, 1.0, 3.0)


def close(a, b, rtol):
    return abs(a - b) <= rtol * abs(b)


def costs_of(K, seed=None):
    rng = np.random.default_rng(K if seed is None else seed)
    return 3.0 + 2.0 * rng.standard_normal(K) ** 2                   # chi-square-like: a heavy right tail


# ---- 1. the model against the independent answer ----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 257, 5000])
def test_model_agrees_with_the_bisection(K):
    """theta* to 1e-9 relative; BOUND, TILT_MEAN, KL to 1e-11 (the bound of tests/test_gpu_policy_mc.py for fixed-order sums of this
    length: the bound is flat to first order at theta*, so the theta error enters squared).  TILT_VAR and ESS to 1e-9: they are first
    order in the theta error.  BOUND == TILT_MEAN to 1e-11 on every unsaturated row."""
    J = costs_of(K)
    got = worst_case(J, kl_bounds=DS)["bounds"]
    for i, d in enumerate(DS):
        ref = direct(J, d)
        assert got["flag"][i] == ref["flag"], (K, d)
        if ref["flag"] == SATURATED:
            assert got["theta"][i] == np.inf and got["bound"][i] == got["tilt_mean"][i] == J.max() and got["tilt_var"][i] == 0.0
            assert np.isnan(got["bound_se"][i]) and got["ess"][i] == (J == J.max()).sum()
            assert close(got["kl"][i], ref["kl"], 1e-15) or got["kl"][i] == ref["kl"]
            continue
        assert ref["flag"] == OK
        if d == 0.0:
            assert got["theta"][i] == 0.0 and got["kl"][i] == 0.0 and got["bound"][i] == got["tilt_mean"][i] and got["ess"][i] == K
            assert close(got["bound"][i], J.mean(), 1e-14)
            if K >= 2:
                assert close(got["bound_se"][i], J.std(ddof=1) / np.sqrt(K), 1e-12) and close(got["tilt_var"][i], J.var(), 1e-12)
            continue
        assert close(got["theta"][i], ref["theta"], 1e-9), (K, d, got["theta"][i], ref["theta"])
        for key in ("bound", "tilt_mean", "kl"):
            assert close(got[key][i], ref[key], 1e-11), (K, d, key, got[key][i], ref[key])
        for key in ("tilt_var", "ess"):
            assert close(got[key][i], ref[key], 1e-9), (K, d, key, got[key][i], ref[key])
        assert close(got["bound"][i], got["tilt_mean"][i], 1e-11)
        assert close(got["kl"][i], d, 1e-11)
        assert J.mean() < got["bound"][i] < J.max() and 1.0 <= got["ess"][i] < K and got["bound_se"][i] > 0
    # which (K, d) are searched at all: K = 1 never (n_max = n), K = 2, 3 below log 2 / log 3 only
    assert (got["flag"] == OK).sum() == {1: 1, 2: 3, 3: 4, 257: 5, 5000: 5}[K]


def test_bound_is_the_minimum_of_the_dual_and_grows_with_d():
    J = costs_of(5000)
    ds = (1e-3, 0.1, 1.0, 3.0)
    got = worst_case(J, kl_bounds=ds)["bounds"]
    assert np.all(np.diff(got["bound"]) > 0) and np.all(np.diff(got["theta"]) > 0) and np.all(np.diff(got["ess"]) < 0)
    for i, d in enumerate(ds):
        ts = got["theta"][i] * np.linspace(0.5, 1.5, 201)              # brute force: risk(theta) + d / theta on a grid around theta*
        Jl = J.astype(np.longdouble)
        dual = [float(J.max() + np.log(np.exp(np.longdouble(t) * (Jl - Jl.max())).mean()) / t + d / t) for t in ts]
        assert min(dual) >= got["bound"][i] * (1 - 1e-12) and close(dual[100], got["bound"][i], 1e-12)


def test_theta_rows_and_kl_is_non_decreasing():
    J = costs_of(5000)
    ths = np.concatenate([[0.0], np.logspace(-4, 2.5, 15)])
    r = worst_case(J, thetas=ths)["thetas"]
    assert np.array_equal(r["theta"], ths) and np.all(r["flag"] == OK)
    assert r["kl"][0] == 0.0 and np.all(np.diff(r["kl"]) >= 0.0) and r["kl"][-1] <= np.log(5000)
    for i, t in enumerate(ths[1:], 1):
        assert close(r["kl"][i], kl_of(J, t), 1e-11), t
        assert close(r["bound"][i], r["tilt_mean"][i], 1e-12)         # a theta row's d is its own KL
        Jl, tl = J.astype(np.longdouble), np.longdouble(t)
        yl = np.exp(tl * (Jl - Jl.max()))
        ml = (yl * Jl).sum() / yl.sum()
        assert close(r["tilt_mean"][i], float(ml), 1e-12) and close(r["tilt_var"][i], float((yl * (Jl - ml) ** 2).sum() / yl.sum()), 1e-11), t
    assert r["bound"][0] == r["tilt_mean"][0] and r["ess"][0] == 5000 and close(r["bound"][0], J.mean(), 1e-14)
    # a theta row at a bound row's theta* reproduces that row
    b = worst_case(J, kl_bounds=(0.1,))["bounds"]
    t = worst_case(J, thetas=(b["theta"][0],))["thetas"]
    for key in ("theta", "kl", "tilt_mean", "tilt_var", "ess", "bound_se"):
        assert t[key][0] == b[key][0], key
    assert close(t["bound"][0], b["bound"][0], 1e-12)


@pytest.mark.parametrize("J", [[1, 2, 2.5, 3, 3.5, 4, 4.25, 5], [1, 2, 5, 5]])
def test_saturation_edge_of_the_handcrafted_vectors(J):
    J = np.array(J, dtype=np.float64)
    n, nmax = J.size, int((J == J.max()).sum())
    edge = float(np.log(n / nmax))
    got = worst_case(J, kl_bounds=(edge - 1e-3, edge, np.inf), want_weights=True)
    b = got["bounds"]
    ref = direct(J, edge - 1e-3)
    assert b["flag"][0] == OK == ref["flag"] and close(b["theta"][0], ref["theta"], 1e-9)
    for key in ("bound", "tilt_mean", "kl"):
        assert close(b[key][0], ref[key], 1e-11), key
    assert b["bound"][0] < 5.0 and nmax < b["ess"][0] < nmax + 0.1
    assert close(got["weights"].sum(), 1.0, 1e-14) and close(got["weights"] @ J, b["tilt_mean"][0], 1e-14)
    for i in (1, 2):
        assert b["flag"][i] == SATURATED and b["theta"][i] == np.inf and b["kl"][i] == edge
        assert b["bound"][i] == b["tilt_mean"][i] == 5.0 and b["tilt_var"][i] == 0.0 and b["ess"][i] == nmax and np.isnan(b["bound_se"][i])
    w = worst_case(J, kl_bounds=(edge,), want_weights=True)["weights"]
    assert np.array_equal(w, np.where(J == 5.0, 1.0 / nmax, 0.0))


def test_all_costs_equal_nan_entries_and_an_infinity():
    same = worst_case(np.full(300, 2.5), kl_bounds=(0.0, 0.1), thetas=(0.0, 3.0))
    b, t = same["bounds"], same["thetas"]
    assert b["flag"].tolist() == [OK, SATURATED] and b["bound"].tolist() == [2.5, 2.5] and b["ess"].tolist() == [300, 300]
    assert b["theta"][0] == 0.0 and b["theta"][1] == np.inf and b["kl"].tolist() == [0.0, 0.0]
    assert t["flag"].tolist() == [OK, OK] and t["kl"].tolist() == [0.0, 0.0] and t["bound"].tolist() == [2.5, 2.5] and t["ess"].tolist() == [300, 300]
    # NaN entries are DomainError rollouts: left out, weight 0
    rng = np.random.default_rng(9)
    J = costs_of(3000)
    bad = rng.random(3000) < 0.3
    Jn = np.where(bad, np.nan, J)
    a, c = worst_case(Jn, kl_bounds=(0.1,), thetas=(0.4,), want_weights=True), worst_case(J[~bad], kl_bounds=(0.1,), thetas=(0.4,), want_weights=True)
    ref = direct(J[~bad], 0.1)
    for key in ("theta", "bound", "tilt_mean", "kl", "ess"):
        assert close(a["bounds"][key][0], c["bounds"][key][0], 1e-11) and close(a["thetas"][key][0], c["thetas"][key][0], 1e-11), key
    assert close(a["bounds"]["bound"][0], ref["bound"], 1e-11) and direct(Jn, 0.1)["bound"] == ref["bound"]
    assert np.all(a["weights"][bad] == 0.0) and np.all(a["weights"][~bad] > 0.0) and close(a["weights"].sum(), 1.0, 1e-13)
    none = worst_case(np.full(10, np.nan), kl_bounds=(0.0, 0.1), thetas=(0.0, 1.0), want_weights=True)
    for rows in (none["bounds"], none["thetas"]):
        assert np.all(rows["flag"] == EMPTY) and all(np.all(np.isnan(rows[k])) for k in rows if k != "flag")
    assert np.all(none["weights"] == 0.0) and direct(np.full(10, np.nan), 0.1)["flag"] == EMPTY
    for inf in (np.inf, -np.inf):
        Ji = J.copy(); Ji[17] = inf
        r = worst_case(Ji, kl_bounds=(0.0, 0.1, np.inf), thetas=(0.0, 1.0))
        for rows in (r["bounds"], r["thetas"]):
            assert np.all(rows["flag"] == NONFINITE) and all(np.all(np.isnan(rows[k])) for k in rows if k != "flag")
        assert direct(Ji, 0.1)["flag"] == NONFINITE


def test_tilted_variance_where_the_tilted_mean_sits_on_the_maximum():
    """Two costs, theta (Jmax - Jmin) = 19: the sums are centred about the mean, m is within 1e-9 of Jmax, and E (J - mean)^2 - (m - mean)^2
    would cancel seven digits.  Taken about the nearer centre, Jmax, it does not."""
    J = 3.0 + 2.0 * np.random.default_rng(2).standard_normal(2) ** 2
    t = worst_case(J, thetas=(40.0,))["thetas"]
    Jl = J.astype(np.longdouble)
    yl = np.exp(np.longdouble(40.0) * (Jl - Jl.max()))
    ml = (yl * Jl).sum() / yl.sum()
    assert 40.0 * (J.max() - J.mean()) < 32.0
    assert close(t["tilt_var"][0], float((yl * (Jl - ml) ** 2).sum() / yl.sum()), 1e-12)
    assert close(t["ess"][0], float(yl.sum() ** 2 / (yl * yl).sum()), 1e-12)


def test_top_of_the_search_and_large_theta_do_not_overflow():
    """d within 1e-9 of log(n / n_max) on a sample whose two largest costs nearly tie needs a theta beyond theta_top = 65536 theta_0: the
    documented saturated flag.  A theta row at theta (Jmax - Jmin) = 2000 takes the sums about Jmax and stays finite."""
    J = np.array([0.0, 1.0, 2.0, 3.0, 3.0 + 1e-7])
    r = worst_case(J, kl_bounds=(np.log(5.0) - 1e-9,))["bounds"]
    assert r["flag"][0] == SATURATED and r["bound"][0] == J.max() and direct(J, np.log(5.0) - 1e-9)["flag"] == OK
    U = np.random.default_rng(6).uniform(0.0, 1.0, 4096)
    U[0], U[1] = 0.0, 1.0
    t = worst_case(U, thetas=(2000.0,))["thetas"]
    assert t["flag"][0] == OK and all(np.isfinite(t[k][0]) for k in t)
    assert close(t["kl"][0], kl_of(U, 2000.0), 1e-11) and close(t["bound"][0], t["tilt_mean"][0], 1e-12) and t["tilt_mean"][0] <= 1.0


# ---- 2. the library without a device ------------------------------------------------------------------------------------------------
def test_symbol_header_mirrors_and_null_handle():
    """Fails on a tree without the feature: the symbol, its declarations and the wrappers."""
    L = nv.lib()
    assert hasattr(L, "rat_policy_worst_case") and "rat_policy_worst_case" in nv.EXPORTS
    assert re.search(r"rat_rc\s+rat_policy_worst_case\s*\(\s*rat_handle h,\s*const double \*cost,\s*int64_t K,", HEADER)
    for i, name in enumerate(("THETA", "KL", "BOUND", "BOUND_SE", "TILT_MEAN", "TILT_VAR", "ESS", "FLAG")):
        assert re.search(rf"#define RAT_WC_{name}\s+{i}\b", HEADER), name
        assert nv.WC_SLOTS[i] == name.lower()
    for name, val in (("NSTAT", 8), ("OK", 0), ("SATURATED", 1), ("EMPTY", 2), ("NONFINITE", 3)):
        assert re.search(rf"#define RAT_WC_{name}\s+{val}\b", HEADER), name
        assert getattr(nv, "WC_" + name) == val
    assert (OK, SATURATED, EMPTY, NONFINITE) == (nv.WC_OK, nv.WC_SATURATED, nv.WC_EMPTY, nv.WC_NONFINITE)
    assert "RAT_VERSION 600" in HEADER and L.rat_version() == 600
    d, out = np.array([0.1]), np.zeros(8)
    J = np.ones(4)
    rc = L.rat_policy_worst_case(None, nv.P(J), C.c_int64(4), nv.P(d), C.c_int32(1), None, C.c_int32(0), nv.P(out), None, None)
    assert rc == 1 and "null handle" in L.rat_last_error().decode()
    assert callable(rat.Context.policy_worst_case)
    from ratilqr.jl_amd.generic import GenericContext
    assert "policy_worst_case" in vars(GenericContext)
    jl = open(os.path.join(ROOT, "julia", "RATiLQRAMD.jl")).read()
    assert "(:rat_policy_worst_case, LIB)" in jl and re.search(r"export[^\n]*(\n[^\n]*)*policy_worst_case", jl)
