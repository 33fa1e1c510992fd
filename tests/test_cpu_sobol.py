"""rat_policy_sobol without a device: the exported symbols and their prototypes, the compile-only check (gfx950) with its refusals, the
SobolGroup masks and the host-side refusals, and the NumPy model of the whole call (tests/sobol_model.py) against two closed forms.

Closed forms (sobol_model.CLOSED; n = m = 1, N = 4, groups {z0}, {z1}, {xi}) at K = 2^14:
  additive     Var J = 5,  S = T = (0.288, 0.512, 0.2)
  interaction  Var J = 20, S = (0, 0, 0.2), T = (0.8, 0.8, 0.2)
Every index must lie within 4 of its own reported standard errors of the closed form, and the reported standard error within a factor 1.5
of the spread (sample standard deviation) of the estimate over 16 disjoint seed pairs (seed_a, seed_b) = (SEED0 + 2 k, SEED0 + 2 k + 1),
k = 0 .. 15; the reported one is pair 0's, the pair the device tests use.  The spread of 16 estimates is itself known to about
1 / sqrt(30) = 18 %, so the factor is a condition on the seeds, confirmed here.  Seeds tried: SEED0 = 1000 (the first choice) passed both
conditions for all twelve indices of both forms; no other was tried."""
import ctypes as C
import inspect

import numpy as np
import pytest

import ratilqr.jl_amd as rat
import sobol_model as sm
import user_params_model as pm
from ratilqr.jl_amd import _native as nv
from test_cpu_julia_shim import PROTOS
from test_cpu_rare_event_params import ALL_P, NPAR

ARG, UNSUPPORTED = 1, 2
SEED0 = 1000
N_PAIRS = 16


def _check_rc(src, n, m, npar, npn, npu, ppn, ppu):
    return nv.lib().rat_policy_sobol_check(src.encode(), n, m, npar, npn, npu, ppn, ppu)


# ---- 1. exports, the check and its refusals -----------------------------------------------------------------------------------------------
def test_the_library_exports_both_symbols_with_the_declared_prototypes():
    lib = nv.lib()
    canon = {C.c_void_p: "p:void", C.c_char_p: "cstr", nv._dp: "p:f64", nv._up: "p:u64", C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64"}
    for name in ("rat_policy_sobol", "rat_policy_sobol_check"):
        assert name in nv.EXPORTS and hasattr(lib, name) and name in PROTOS, name
        ret, args = PROTOS[name]
        assert ret == "i32" and [canon[t] for t in getattr(lib, name).argtypes] == args, name
    assert len(PROTOS["rat_policy_sobol"][1]) == 14 and len(PROTOS["rat_policy_sobol_check"][1]) == 8
    # no device: a null handle is an argument error, as for the other calls
    assert lib.rat_policy_sobol(None, None, None, None, 64, 1, 0, None, 1, 1, 2, None, None, None) == ARG


def test_the_check_compiles_the_all_hooks_source():
    assert _check_rc(ALL_P, 2, 1, NPAR, 2, 0, 2, 1) == 0, nv.lib().rat_last_error().decode()       # parameter sampling on
    assert _check_rc(ALL_P, 2, 1, 0, 2, 0, 0, 0) == 0, nv.lib().rat_last_error().decode()          # ... and off
    rat.policy_sobol_check(ALL_P, 2, 1, n_params=NPAR, normals_per_step=2, param_normals=2, param_uniforms=1)


@pytest.mark.parametrize("name", ["pend", "lq12"])
def test_the_check_compiles_the_cases(name):
    c = pm.case(name)
    assert _check_rc(c.source("scale"), c.n, c.m, len(c.p), c.npn, c.npu, 2, 1) == 0, nv.lib().rat_last_error().decode()


def test_the_check_refuses_what_the_call_refuses():
    c = pm.case("pend")
    np_ = len(c.p)
    last = lambda: nv.lib().rat_last_error().decode()
    no_sampler = c.source("scale").split("#define RAT_USER_NOISE")[0]
    assert _check_rc(no_sampler, c.n, c.m, 0, c.npn, c.npu, 0, 0) == UNSUPPORTED and "does not define RAT_USER_NOISE" in last()
    assert _check_rc(c.source(None), c.n, c.m, np_, c.npn, c.npu, 2, 1) == ARG and "does not define RAT_USER_PARAMS" in last()    # no hook
    assert _check_rc(c.source(None), c.n, c.m, 0, c.npn, c.npu, 0, 0) == 0                          # ... which sampling off does not need
    assert _check_rc(c.source("scale"), c.n, c.m, 0, c.npn, c.npu, 2, 1) == ARG                     # parameter draws without parameters
    assert _check_rc(c.source("scale"), c.n, c.m, np_, 65, c.npu, 2, 1) == UNSUPPORTED and "above 64" in last()
    assert _check_rc(c.source("scale"), c.n, c.m, np_, c.npn, 65, 2, 1) == UNSUPPORTED
    assert _check_rc(c.source("scale"), c.n, c.m, np_, c.npn, c.npu, 65, 1) == UNSUPPORTED
    assert _check_rc(c.source("scale"), c.n, c.m, np_, c.npn, c.npu, 2, 65) == UNSUPPORTED
    assert _check_rc(c.source("scale"), 13, c.m, np_, c.npn, c.npu, 2, 1) == UNSUPPORTED
    assert _check_rc(c.source("scale"), c.n, 5, np_, c.npn, c.npu, 2, 1) == UNSUPPORTED
    assert _check_rc(c.source("scale"), c.n, c.m, np_, -1, c.npu, 2, 1) == ARG
    assert _check_rc(c.source("scale"), c.n, c.m, 33, c.npn, c.npu, 2, 1) == UNSUPPORTED            # rat_user_params_check's cap
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_UNSUPPORTED.*does not define RAT_USER_NOISE"):
        rat.policy_sobol_check(no_sampler, c.n, c.m, normals_per_step=c.npn)


# ---- 2. the groups on the host ----------------------------------------------------------------------------------------------------------------
def test_sobol_group_masks():
    g = rat.SobolGroup(param_normals=(0, 3), param_uniforms=1, step_normals=range(5), step_uniforms=(63,), name="g")
    assert g.words == (0b1001, 0b10, 0b11111, 1 << 63) and g.name == "g"
    assert rat.SobolGroup().words == (0, 0, 0, 0) and rat.SobolGroup().name is None
    for bad in (64, -1):
        with pytest.raises(ValueError, match="outside 0 .. 63"):
            rat.SobolGroup(step_normals=(bad,))
    words = rat.SobolGroup.check_groups([g, rat.SobolGroup(param_normals=(1,))], 5, 64, 4, 2)
    assert words.dtype == np.uint64 and words.shape == (2, 4) and words[0, 3] == np.uint64(1 << 63) and words[1, 0] == 2


def test_the_host_refuses_overlap_and_out_of_range():
    G = rat.SobolGroup
    with pytest.raises(ValueError, match="group 1 overlaps"):
        G.check_groups([G(step_normals=(0, 1)), G(step_normals=(1,))], 3, 0)
    with pytest.raises(ValueError, match="group 1 overlaps"):
        G.check_groups([G(param_uniforms=(0,)), G(param_uniforms=(0,))], 3, 0, 2, 1)
    G.check_groups([G(step_normals=(1,)), G(step_uniforms=(1,)), G(param_normals=(1,)), G(param_uniforms=(1,))], 2, 2, 2, 2)   # one index, four kinds
    with pytest.raises(ValueError, match=r"group 0 names a draw at or beyond the declared count \(3\)"):
        G.check_groups([G(step_normals=(3,))], 3, 0)
    with pytest.raises(ValueError, match=r"beyond the declared count \(0\)"):
        G.check_groups([G(param_normals=(0,))], 3, 0)                 # parameter sampling off: no parameter draw to name
    with pytest.raises(ValueError, match="1 .. 16 groups"):
        G.check_groups([], 3, 0)
    with pytest.raises(ValueError, match="1 .. 16 groups"):
        G.check_groups([G()] * 17, 3, 0)
    assert G.check_groups([G()] * 16, 3, 0).shape == (16, 4)          # empty groups overlap nothing


def test_the_python_surface():
    sig = inspect.signature(rat.Context.policy_sobol)
    for k in ("x_nom", "l", "L", "noise", "groups", "K", "seed_a", "seed_b", "want_costs"):
        assert k in sig.parameters, k
    assert sig.parameters["want_costs"].default is False and sig.parameters["L"].default is None
    from ratilqr.jl_amd import generic                                # the refusal of the general-size carrier
    assert any("policy_sobol" in getattr(v, "__dict__", {}) for v in vars(generic).values() if inspect.isclass(v))


# ---- 3. the model against the closed forms -------------------------------------------------------------------------------------------------
def test_the_estimator_on_rows_written_out():
    """five base samples by hand: a NaN in any row drops the sample; an AB row equal to A gives S = T = 0 exactly, one equal to B gives
    T = mean((a - b)^2) / (2 V)"""
    a = np.array([1.0, 2.0, 4.0, 0.5, 3.0])
    b = np.array([2.0, 0.0, 1.0, 9.0, 5.0])
    Y = np.array([a, b, a, b, np.array([1.0, 2.0, np.nan, 0.5, 3.0])])
    r = sm.estimator(Y)
    ok = np.array([True, True, False, True, True])
    mu = (a[ok].sum() + b[ok].sum()) / 8
    V = (((a[ok] - mu) ** 2 + (b[ok] - mu) ** 2) / 2).mean()
    assert r["n_ok"] == 4 and r["flag"] == 0 and abs(r["mean"] - mu) < 1e-15 and abs(r["var"] - V) < 1e-14
    assert r["S"][0] == 0.0 and r["T"][0] == 0.0 and r["S_se"][0] == 0.0 and r["T_se"][0] == 0.0
    assert abs(r["T"][1] - ((a[ok] - b[ok]) ** 2).mean() / (2 * V)) < 1e-14
    assert abs(r["S"][1] - ((b[ok] - mu) * (b[ok] - a[ok])).mean() / V) < 1e-14
    flat = sm.estimator(np.ones((3, 8)))
    assert flat["flag"] == sm.DEGENERATE and np.isnan(flat["S"]).all() and flat["var"] == 0.0
    assert sm.estimator(np.full((3, 4), np.nan))["n_ok"] == 0


@pytest.fixture(scope="module", params=sorted(sm.CLOSED))
def closed_runs(request):
    which = request.param
    runs = [sm.estimator(sm.closed_costs(which, sm.CLOSED_K, SEED0 + 2 * k, SEED0 + 2 * k + 1)) for k in range(N_PAIRS)]
    return which, runs


def test_the_model_meets_the_closed_form_within_four_standard_errors(closed_runs):
    which, runs = closed_runs
    m, r = sm.CLOSED[which], runs[0]
    print(f"{which}: Var {r['var']:.4f} +- {r['var_se']:.4f} (exact {m['var']})")
    assert r["n_ok"] == sm.CLOSED_K and r["flag"] == 0
    assert abs(r["var"] - m["var"]) <= 4.0 * r["var_se"]
    for key in ("S", "T"):
        for i in range(3):
            dev = abs(r[key][i] - m[key][i]) / r[key + "_se"][i]
            print(f"{which}: {key}[{i}] {r[key][i]:+.4f} +- {r[key + '_se'][i]:.4f} (exact {m[key][i]}): {dev:.2f} sigma")
            assert dev <= 4.0


def test_the_reported_standard_error_is_the_spread_over_seed_pairs(closed_runs):
    which, runs = closed_runs
    for key in ("S", "T"):
        est = np.array([r[key] for r in runs])
        spread = est.std(axis=0, ddof=1)
        for i in range(3):
            ratio = runs[0][key + "_se"][i] / spread[i]
            print(f"{which}: {key}[{i}] reported SE {runs[0][key + '_se'][i]:.5f}, spread over {N_PAIRS} seed pairs {spread[i]:.5f}: ratio {ratio:.2f}")
            assert 1 / 1.5 <= ratio <= 1.5
