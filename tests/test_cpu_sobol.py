"""rat_policy_sobol without a device: the exported symbols and their prototypes, the compile-only check (gfx950) with its refusals, the
SobolGroup masks and the host-side refusals, and the NumPy model of the whole call (tests/sobol_model.py) against two closed forms.

Closed forms (sobol_model.CLOSED; n = m = 1, N = 4, groups {z0}, {z1}, {xi}) at K = 2^14:
  additive     Var J = 5,  S = T = (0.288, 0.512, 0.2)
  interaction  Var J = 20, S = (0, 0, 0.2), T = (0.8, 0.8, 0.2)
Every index must lie within 4 of its own reported standard errors of the closed form, and the reported standard error within a factor 1.5
of the spread (sample standard deviation) of the estimate over 16 disjoint seed pairs (seed_a, seed_b) = (SEED0 + 2 k, SEED0 + 2 k + 1),
k = 0 .. 15; the reported one is pair 0's, the pair the device tests use.  The spread of 16 estimates is itself known to about
1 / sqrt(30) = 18 %, so the factor is a condition on the seeds, confirmed here.  Seeds tried: SEED0 = 1000 (the first choice) passed both
conditions for all twelve indices of both forms; no other was tried.

The wide closed form (sobol_model.WIDE_*: 64 draws of each of the four kinds, 32 parameters, N = 2) with the sixteen groups of
sobol_model.wide_groups() is pinned here before the device is compared with it: the fsum estimator at K = 2^14 under (SEED0, SEED0 + 1)
within 4 of its own standard errors of the exact shares, and "teeth": for every mask bit those groups single out, the model's row under
each wrong reading of that bit (the other half of the word, the Box-Muller neighbour, the bit below, the word cut to 32 bits) is another
row.  The masks at their edges -- bit 63, a count of exactly 64, a count of 65 -- are held on SobolGroup and on the compile-only check."""
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


# ---- 4. the wide closed form: 64 draws of every kind, sixteen groups ----------------------------------------------------------------------
WIDE_K = 1 << 14
TEETH_K = 256


def test_the_wide_model_meets_its_exact_shares_within_four_standard_errors():
    groups = sm.wide_groups()
    assert len(groups) == 16 and rat.SobolGroup.check_groups(groups, 64, 64, 64, 64).shape == (16, 4)
    var, exact = sm.wide_exact(groups)
    r = sm.estimator(sm.wide_model(WIDE_K, SEED0, SEED0 + 1))
    print(f"wide: Var {r['var']:.3f} +- {r['var_se']:.3f} (exact {var})")
    assert r["n_ok"] == WIDE_K and r["flag"] == 0 and abs(r["var"] - var) <= 4.0 * r["var_se"]
    assert exact[15] == 0.0 and np.all(exact[:15] > 0.0) and abs(sm.wide_exact([rat.SobolGroup(*[range(64)] * 4)])[1][0] - 1.0) < 1e-15
    for key in ("S", "T"):
        assert r[key][15] == 0.0 and r[key + "_se"][15] == 0.0       # the empty group: row A itself
        for i in range(15):
            dev = abs(r[key][i] - exact[i]) / r[key + "_se"][i]
            print(f"wide: {key}[{i}] {groups[i].name} {r[key][i]:+.5f} +- {r[key + '_se'][i]:.5f} (exact {exact[i]:.5f}): {dev:.2f} sigma")
            assert dev <= 4.0


def wrong_readings(mask, i):
    """what a wrong reading of bit i makes of the mask: bit i moved to the same place of the word's other half (i - 32 modulo 64: a 32-bit
    shift count), to its Box-Muller neighbour i ^ 1, to the bit below (the spare rule's i - 1), and the word cut to 32 bits (dropped where
    that is the mask itself)"""
    moved = {f"bit {i} read at {j}": (mask & ~(1 << i)) | (1 << j) for j in ((i - 32) % 64, i ^ 1, i - 1)}
    cut = {f"bit {i}, the word cut to 32 bits": mask & 0xFFFFFFFF} if mask >> 32 else {}
    return {**moved, **cut}


def test_every_wrong_reading_of_a_singled_out_bit_is_another_row():
    A, B = sm.wide_streams(TEETH_K, SEED0, SEED0 + 1)
    n_read, least = 0, np.inf
    for g in sm.wide_groups()[:15]:
        right = sm.wide_row(A, B, g.words)
        for k in range(4):
            for i in (b for b in range(64) if (g.words[k] >> b) & 1):
                for label, mask in wrong_readings(g.words[k], i).items():
                    assert mask != g.words[k], (g.name, label)
                    wrong = sm.wide_row(A, B, g.words[:k] + (mask,) + g.words[k + 1:])
                    gap = float(np.abs(wrong - right).max() / np.abs(right).max())
                    n_read, least = n_read + 1, min(least, gap)
                    assert gap > 1e-6, (g.name, k, label, gap)
    print(f"wide: {n_read} wrong readings, the nearest row {least:.2e} of the row's largest entry away")
    # an odd bit's neighbour is the bit below (two moves, not three); the cut counts where the mask has a high half: per word 2 (bit 31)
    # + 4 (bit 32) + 3 (bit 63); 3 for each lone 33; the run 4 x 4 (24, 26, 28, 30) + 3 x 3 (25, 27, 29) + 2 x 3 (33, 35) + 2 x 4 (34, 36)
    assert n_read == 4 * 9 + 2 * 3 + 39


def test_the_check_compiles_the_wide_source_at_sixty_four_draws_of_every_kind():
    assert _check_rc(sm.wide_source(), 1, 1, sm.WIDE_NPAR, 64, 64, 64, 64) == 0, nv.lib().rat_last_error().decode()


@pytest.mark.parametrize("which", range(4))
def test_the_check_refuses_sixty_five_in_any_one_count(which):
    counts = [64, 64, 64, 64]
    counts[which] = 65
    assert _check_rc(sm.wide_source(), 1, 1, sm.WIDE_NPAR, *counts) == UNSUPPORTED and "above 64" in nv.lib().rat_last_error().decode()
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*above 64"):
        rat.policy_sobol_check(sm.wide_source(), 1, 1, n_params=sm.WIDE_NPAR, **dict(zip(
            ("normals_per_step", "uniforms_per_step", "param_normals", "param_uniforms"), counts)))


def test_the_python_mirror_at_the_edges_of_a_word():
    G = rat.SobolGroup
    for kind in range(4):
        args = [()] * 4
        args[kind] = (63,)
        assert G(*args).words[kind] == 1 << 63 and sum(G(*args).words) == 1 << 63
        args[kind] = (64,)
        with pytest.raises(ValueError, match="index 64 is outside 0 .. 63"):
            G(*args)
        args[kind] = (31, 32)
        assert G(*args).words[kind] == 0x180000000
    assert G(step_normals=range(64)).words[2] == (1 << 64) - 1
    top, counts = [G(*[(63,)] * 4)], lambda k, c: [c if j == k else 64 for j in (2, 3, 0, 1)]    # (check_groups takes the step counts first)
    words = G.check_groups(top, 64, 64, 64, 64)                       # a count of 64 accepts bit 63 ...
    assert words.dtype == np.uint64 and [int(w) for w in words[0]] == [1 << 63] * 4
    for k in range(4):
        with pytest.raises(ValueError, match=r"group 0 names a draw at or beyond the declared count \(63\)"):
            G.check_groups(top, *counts(k, 63))                       # ... one of 63 does not
        args = [()] * 4
        args[k] = (40,)
        with pytest.raises(ValueError, match=r"group 0 names a draw at or beyond the declared count \(40\)"):
            G.check_groups([G(*args)], *counts(k, 40))
        args[k] = (39,)
        assert int(G.check_groups([G(*args)], *counts(k, 40))[0, k]) == 1 << 39
        args[k] = (63,)
        with pytest.raises(ValueError, match="group 1 overlaps"):
            G.check_groups([G(*args), G(*args)], 64, 64, 64, 64)
        args[k] = (0, 63)
        with pytest.raises(ValueError, match="group 2 overlaps"):
            G.check_groups([G(), G(*args), G(*[(63,)] * 4)], 64, 64, 64, 64)
    full = G(*[range(64)] * 4)
    assert [int(w) for w in G.check_groups([full], 64, 64, 64, 64)[0]] == [(1 << 64) - 1] * 4


# ---- 5. the aids of the device tests at K = 65536 + 5 and about a large mean ----------------------------------------------------------------
def test_the_vectorised_pendulum_is_the_per_sample_model():
    """sobol_model.pend_costs rolls a whole row out at once (the device test at K = 65536 + 5); on the leading base samples it is
    case_costs, NaN for NaN.  The operations are the same; only the feedback product goes through another matmul, an ulp a step over
    eight steps: 1e-13 relative."""
    c = pm.case("pend")
    G = rat.SobolGroup
    groups = [G(step_normals=(0, 2), param_normals=(0,)), G(step_normals=(1,), param_normals=(1,)), G(param_uniforms=(0,))]
    p = c.p.copy()
    p[c.idx["pnan"]] = 1.2
    for hook in ("scale", "nan"):
        one = sm.case_costs(c, hook, True, groups, 96, 41, 42, p=p)
        vec = sm.pend_costs(c, hook, groups, 300, 41, 42, p=p)[:, :96]
        assert np.array_equal(np.isnan(one), np.isnan(vec)) and np.isnan(one).any() == (hook == "nan")
        err = float(np.nanmax(np.abs(vec / one - 1)))
        print(f"{hook}: the vectorised pendulum against the per-sample model {err:.2e}")
        assert err <= 1e-13
    bad = np.isnan(sm.pend_costs(c, "nan", groups, 300, 41, 42, p=p)).any(axis=0)
    assert np.array_equal(bad, sm.nan_thresholds(c, 300, 41, 42) > 1.2)


# |mean| / sd = 1e4 of the additive form (sd = sqrt 5): the first choice, and both figures below hold at it
OFFSET = 22360.0
_FIGURES = []


def large_mean_figures():
    """(the largest |S_se of the uncentred float64 estimator - fsum's|, the largest |S or S_se of the centred float64 estimator - fsum's|,
    the model's rows) of the additive form about OFFSET at K = 2^14: what gives the device's 1e-9 against fsum its room on both sides"""
    if not _FIGURES:
        Y = sm.offset_costs(OFFSET, sm.CLOSED_K, SEED0, SEED0 + 1)
        Y.setflags(write=False)
        ref, un, ce = sm.estimator(Y), sm.plain_estimator(Y, centred=False), sm.plain_estimator(Y, centred=True)
        _FIGURES.append((float(np.abs(un["S_se"] - ref["S_se"]).max()),
                         max(float(np.abs(ce[k] - ref[k]).max()) for k in ("S", "S_se")), Y))
    return _FIGURES[0]


def test_only_a_centred_estimator_survives_a_large_mean():
    uncentred, centred, Y = large_mean_figures()
    ref = sm.estimator(Y)
    print(f"offset {OFFSET}: |mean| / sd {abs(ref['mean']) / np.sqrt(ref['var']):.1f}; S_se uncentred float64 against fsum {uncentred:.3e}, "
          f"S, S_se centred float64 against fsum {centred:.3e}")
    assert 0.9e4 <= abs(ref["mean"]) / np.sqrt(ref["var"]) <= 1.1e4
    assert uncentred > 1e-6 and centred <= 1e-10
    ref0 = sm.estimator(sm.closed_costs("additive", sm.CLOSED_K, SEED0, SEED0 + 1))
    for key in ("S", "T"):                                            # the rows differ by the constant to rounding: the same indices
        assert float(np.abs(ref[key] - ref0[key]).max()) <= 1e-9, key
