"""Sobol indices of a policy's cost on the GPU (rat_policy_sobol, include/ratilqr.h "which uncertainty drives the cost";
csrc/source_sobol.h, sb_pass1 / sb_pass2 / sb_final of csrc/policy_mc.hip) against the NumPy restatement of tests/sobol_model.py.

Shapes (tests/user_params_model.Case): the pendulum 2 x 1 at N = 8, K = 256 with three normals a step; the LQ + cubic source 12 x 4 at
N = 4, K = 128 with twelve normals and a uniform per step; the same source at 5 x 3, K = 65 (padding lanes, a ragged last wave); d = 3
groups, open and closed loop, parameter sampling on (two parameter normals, one uniform) unless a test says otherwise.  The groups of
SPLIT put the two normals of every Box-Muller block -- the parameters' and each step's -- into different groups, so every AB_i row takes
the two outputs of a block from different streams (the spare rule).

Held: rows A and B bit for bit against rat_policy_evaluate_noise under seed_a / seed_b (the project's replay rule); an empty group's row
bit for bit row A with S = T = 0 exactly; an all-draws group's row bit for bit row B; every row against the model to 1e-12 relative (what
tests/test_gpu_user_params.py holds under the generator); indices, standard errors and summary against the model's math.fsum estimator
on the device's own rows to 1e-9 absolute (the project's parity bound; the indices are O(1)); a shorter call returns the leading columns
bit for bit; the closed forms of tests/test_cpu_sobol.py within 4 reported standard errors; every refusal of the header with its code.

Beyond those sizes (sections 9 .. 11; the bounds are the same 1e-12, 1e-9 and 4 standard errors):
  9   the wide closed form of tests/sobol_model.py -- 64 draws of each of the four kinds, 32 parameters, N = 2 -- at K = 2^14 with the
      sixteen groups of sobol_model.wide_groups(): bits 31, 32 and 63 of every word alone, Box-Muller block 16 of the step and of the
      parameter normals cut in two, one mask with bits in both halves, the empty group at index 15 (variant 17); one group of all 256
      bits; a 40-draw instantiation that refuses bit 40 and serves bit 39.  tests/test_cpu_sobol.py shows that each wrong reading of one of
      those bits gives the model another row, at least 4e-2 of the row's largest entry away.
  10  K = 65536 + 5, past the stride 256 x 256 of the reduction grid: the additive closed form, its calls at 65535 and 65536, and the
      pendulum's "nan" hook with dropped base samples and survivors on both sides of 65536 (the model: sobol_model.pend_costs).
  11  the "nan" hook at K = 64 with thresholds that leave 0, 1 and 2 base samples; the additive form about a mean of 10^4 standard
      deviations (sobol_model.OFFSET_SOURCE), where test_cpu_sobol.large_mean_figures shows that an uncentred estimator is 8e+1 away from
      fsum in S_se and a centred float64 one agrees with it."""
import ctypes as C

import numpy as np
import pytest

import ratilqr.jl_amd as rat
import sobol_model as sm
import user_params_model as pm
import user_policy_model as up
from ratilqr.jl_amd import _native as nv
from test_cpu_sobol import SEED0

pytestmark = pytest.mark.gpu
SEED_A, SEED_B = 41, 42
G = rat.SobolGroup
_CTX, _RUN = {}, {}


def split_groups(c, sampling=True):
    """three groups that cut through every Box-Muller block: even step normals | odd step normals | the uniforms, with one parameter
    normal each for the first two"""
    ev, od = tuple(range(0, c.npn, 2)), tuple(range(1, c.npn, 2))
    if not sampling:
        return [G(step_normals=ev, name="even"), G(step_normals=od, name="odd"), G(step_uniforms=tuple(range(c.npu)), name="uniforms")]
    return [G(step_normals=ev, param_normals=(0,), name="even"), G(step_normals=od, param_normals=(1,), name="odd"),
            G(step_uniforms=tuple(range(c.npu)), param_uniforms=(0,), name="uniforms")]


def context(name, hook):
    if (name, hook) not in _CTX:
        _CTX[name, hook] = rat.Context(pm.case(name).problem(hook), max_batch=64)
    ctx = _CTX[name, hook]
    ctx.set_params(pm.case(name).p)
    ctx.set_param_sampling(None)
    return ctx


def run(name, closed):
    """the shared call of a case: sampling on, SPLIT groups, all rows (computed once, left unchanged)"""
    if (name, closed) not in _RUN:
        c = pm.case(name)
        ctx = context(name, "scale")
        ctx.set_param_sampling(c.sampling(injected=False))
        groups = split_groups(c)
        r = ctx.policy_sobol(*c.args(closed), noise=c.user_noise(), groups=groups, K=c.K, seed_a=SEED_A, seed_b=SEED_B, want_costs=True)
        model = sm.case_costs(c, "scale", closed, groups, c.K, SEED_A, SEED_B)
        for v in (r["y"], model):
            v.setflags(write=False)
        _RUN[name, closed] = (r, model)
    return _RUN[name, closed]


def against_estimator(r, label):
    """indices, standard errors and summary against the model's fsum on the device's own rows: 1e-9 absolute"""
    ref = sm.estimator(r["y"])
    assert r["n_ok"] == ref["n_ok"] and r["flag"] == ref["flag"], label
    for key in ("S", "S_se", "T", "T_se"):
        err = float(np.abs(r[key] - ref[key]).max())
        print(f"{label}: {key} {np.round(r[key], 4)} against fsum {err:.2e}")
        assert err <= 1e-9, (label, key)
    for key in ("mean", "var", "var_se"):
        print(f"{label}: {key} {r[key]:.6g} against fsum {abs(r[key] - ref[key]):.2e}")
        assert abs(r[key] - ref[key]) <= 1e-9 * max(1.0, abs(ref[key])), (label, key)


# ---- 1. rows A and B are the plain evaluations -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("name", pm.CASE_NAMES)
def test_rows_a_and_b_are_the_evaluations_under_the_two_seeds_bit_for_bit(name, closed):
    c = pm.case(name)
    r, _ = run(name, closed)
    ctx = context(name, "scale")
    ctx.set_param_sampling(c.sampling(injected=False))
    for row, seed in ((0, SEED_A), (1, SEED_B)):
        e = ctx.policy_evaluate_noise(*c.args(closed), noise=c.user_noise(seed=seed), K=c.K, want_costs=True)
        assert np.array_equal(r["y"][row], e["costs"]), (name, closed, row)
    assert not np.array_equal(r["y"][0], r["y"][1]) and r["n_ok"] == c.K and r["flag"] == 0


# ---- 2. every row against the model, the estimator against fsum ------------------------------------------------------------------------------
@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("name", pm.CASE_NAMES)
def test_every_row_against_the_model(name, closed):
    r, model = run(name, closed)
    err = float(np.abs(r["y"] / model - 1).max())
    print(f"{name} closed={closed}: rows against the model {err:.2e}")
    assert r["y"].shape == model.shape and err <= 1e-12
    for i in range(2, 5):                                             # the mixed rows are neither stream's
        assert not np.array_equal(r["y"][i], r["y"][0]) and not np.array_equal(r["y"][i], r["y"][1])
    against_estimator(r, f"{name} closed={closed}")
    assert r["names"] == ["even", "odd", "uniforms"] and np.all(r["T"] >= 0) and np.all(r["S_se"] > 0)


# ---- 3. the empty group and the group of everything ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pm.CASE_NAMES)
def test_an_empty_group_is_row_a_and_a_full_group_is_row_b(name):
    c = pm.case(name)
    ctx = context(name, "scale")
    ctx.set_param_sampling(c.sampling(injected=False))
    full = G(param_normals=range(pm.PARAM_NORMALS), param_uniforms=range(pm.PARAM_UNIFORMS), step_normals=range(c.npn), step_uniforms=range(c.npu))
    r = ctx.policy_sobol(*c.args(True), noise=c.user_noise(), groups=[G(), full, G()], K=c.K, seed_a=SEED_A, seed_b=SEED_B, want_costs=True)
    base, _ = run(name, True)
    assert np.array_equal(r["y"][0], base["y"][0]) and np.array_equal(r["y"][1], base["y"][1])
    assert np.array_equal(r["y"][2], r["y"][0]) and np.array_equal(r["y"][4], r["y"][0]) and np.array_equal(r["y"][3], r["y"][1])
    for i in (0, 2):
        assert r["S"][i] == 0.0 and r["T"][i] == 0.0 and r["S_se"][i] == 0.0 and r["T_se"][i] == 0.0
    assert r["T"][1] > 0.0 and r["flag"] == 0                         # (everything frozen at once: T estimates 1)
    against_estimator(r, name)


# ---- 4. how K is cut does not show ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pm.CASE_NAMES)
def test_a_shorter_call_returns_the_leading_columns_and_a_repeat_the_same_bits(name):
    c = pm.case(name)
    r, _ = run(name, True)
    ctx = context(name, "scale")
    ctx.set_param_sampling(c.sampling(injected=False))
    kw = dict(noise=c.user_noise(), groups=split_groups(c), seed_a=SEED_A, seed_b=SEED_B, want_costs=True)
    K2 = c.K // 2 + 1
    short = ctx.policy_sobol(*c.args(True), K=K2, **kw)
    assert np.array_equal(short["y"], r["y"][:, :K2])
    again = ctx.policy_sobol(*c.args(True), K=c.K, **kw)
    for key in ("y", "S", "S_se", "T", "T_se"):
        assert np.array_equal(again[key], r[key]), key
    assert (again["mean"], again["var"], again["var_se"]) == (r["mean"], r["var"], r["var_se"])
    quiet = ctx.policy_sobol(*c.args(True), K=c.K, **{**kw, "want_costs": False})
    assert quiet["y"] is None and np.array_equal(quiet["S"], r["S"]) and np.array_equal(quiet["T_se"], r["T_se"])


# ---- 5. sampling off, the policy hook, a DomainError, the overdraw ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pend", "lq5"])
def test_parameter_sampling_off_with_step_groups_only(name):
    c = pm.case(name)
    ctx = context(name, "scale")                                      # (the hook is in the source; sampling is off)
    groups = split_groups(c, sampling=False)
    r = ctx.policy_sobol(*c.args(True), noise=c.user_noise(), groups=groups, K=c.K, seed_a=SEED_A, seed_b=SEED_B, want_costs=True)
    model = sm.case_costs(c, None, True, groups, c.K, SEED_A, SEED_B)
    assert float(np.abs(r["y"] / model - 1).max()) <= 1e-12
    e = ctx.policy_evaluate_noise(*c.args(True), noise=c.user_noise(seed=SEED_A), K=c.K, want_costs=True)
    assert np.array_equal(r["y"][0], e["costs"])
    against_estimator(r, f"{name} sampling off")
    if c.npu == 0:                                                    # the pendulum draws no uniform: an empty group
        assert r["S"][2] == 0.0 and r["T"][2] == 0.0
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*parameter sampling is off"):
        raw(ctx, c, [(1, 0, 0, 0)])


def test_the_policy_hook_applies():
    c = up.case("pend")
    ctx = rat.Context(c.problem("clamp"), max_batch=64)
    x_nom, l, L = c.args(True)
    groups = [G(step_normals=(0,)), G(step_normals=(1,)), G(step_normals=(2,))]
    r = ctx.policy_sobol(x_nom, l, L, noise=c.user_noise(), groups=groups, K=c.K, seed_a=SEED_A, seed_b=SEED_B, want_costs=True)
    e = ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=SEED_A), K=c.K, want_costs=True)
    assert np.array_equal(r["y"][0], e["costs"])
    A, B = (sm.streams(s, c.K, c.N, c.npn, 0, 0, 0) for s in (SEED_A, SEED_B))
    f, cc, h, noise = c.fns
    for row, words in enumerate(sm.variants(groups)):
        zn = sm.mixed(A, B, words)["sn"].ravel()
        ref = up.np_rollouts(f, cc, h, noise, c.params(), x_nom, l, L, c.K, zn, None, c.npn, 0, hook=up.np_hook("clamp"), q=c.q)[0]
        assert float(np.abs(r["y"][row] / ref - 1).max()) <= 1e-12, row
    hookless = rat.Context(c.problem(None), max_batch=64).policy_sobol(x_nom, l, L, noise=c.user_noise(), groups=groups, K=c.K, seed_a=SEED_A,
                                                                        seed_b=SEED_B, want_costs=True)
    assert not np.allclose(hookless["y"], r["y"], rtol=1e-6, atol=0.0)
    against_estimator(r, "clamp hook")


def test_a_domain_error_drops_the_base_sample():
    c = pm.case("pend")
    ctx = context("pend", "nan")
    p = c.p.copy()
    p[c.idx["pnan"]] = 1.2                                            # the first parameter normal beyond 1.2: about one stream draw in nine
    ctx.set_params(p)
    ctx.set_param_sampling(c.sampling(injected=False))
    groups = split_groups(c)
    r = ctx.policy_sobol(*c.args(True), noise=c.user_noise(), groups=groups, K=c.K, seed_a=SEED_A, seed_b=SEED_B, want_costs=True)
    model = sm.case_costs(c, "nan", True, groups, c.K, SEED_A, SEED_B, p=p)
    bad = np.isnan(model).any(axis=0)
    assert 10 < bad.sum() < c.K // 2 and np.array_equal(np.isnan(r["y"]), np.isnan(model))
    assert np.array_equal(np.isnan(r["y"][0]), np.isnan(r["y"][3])) and not np.array_equal(np.isnan(r["y"][0]), np.isnan(r["y"][1]))
    assert r["n_ok"] == c.K - bad.sum() and r["flag"] == 0
    against_estimator(r, "nan hook")


def test_an_overdraw_is_refused_with_its_bits():
    c = pm.case("pend")
    ctx = context("pend", "over")                                     # the hook draws three normals, two are declared
    ctx.set_param_sampling(c.sampling(injected=False))
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*rat_user_params drew more.*param_normals = 2, param_uniforms = 1"):
        ctx.policy_sobol(*c.args(True), noise=c.user_noise(), groups=split_groups(c), K=c.K, seed_a=SEED_A, seed_b=SEED_B)
    rc, index, summary = raw(ctx, c, [g.words for g in split_groups(c)], check=False)
    assert rc == 1 and int(summary[nv.SB_FLAG]) & 4                   # the hook's normals: bit 2
    ok = context("pend", "scale")
    ok.set_param_sampling(c.sampling(injected=False))
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*a step drew more.*normals_per_step = 2"):
        ok.policy_sobol(*c.args(True), noise=rat.UserNoise(2, 0), groups=[G(step_normals=(0,))], K=c.K, seed_a=SEED_A, seed_b=SEED_B)
    assert ok.policy_sobol(*c.args(True), noise=c.user_noise(), groups=[G(step_normals=(0,))], K=c.K, seed_a=SEED_A, seed_b=SEED_B)["flag"] == 0


# ---- 6. the closed forms on the device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(sm.CLOSED))
def test_the_closed_forms_within_four_standard_errors(which):
    m = sm.CLOSED[which]
    ctx = rat.Context(sm.closed_problem(which))
    ctx.set_param_sampling(rat.ParamSampling(2, 0))
    x, l, L = sm.closed_policy()
    r = ctx.policy_sobol(x, l, L, noise=rat.UserNoise(1, 0), groups=sm.closed_groups(), K=sm.CLOSED_K, seed_a=SEED0, seed_b=SEED0 + 1, want_costs=True)
    model = sm.closed_costs(which, sm.CLOSED_K, SEED0, SEED0 + 1)
    print(f"{which}: rows against the model {float(np.abs(r['y'] - model).max()):.2e}; Var {r['var']:.4f} +- {r['var_se']:.4f} (exact {m['var']})")
    assert float(np.abs(r["y"] - model).max()) <= 1e-12 * float(np.abs(model).max())
    assert r["n_ok"] == sm.CLOSED_K and r["flag"] == 0 and abs(r["var"] - m["var"]) <= 4.0 * r["var_se"]
    for key in ("S", "T"):
        for i in range(3):
            dev = abs(r[key][i] - m[key][i]) / r[key + "_se"][i]
            print(f"{which}: {key}[{i}] {r[key][i]:+.4f} +- {r[key + '_se'][i]:.4f} (exact {m[key][i]}): {dev:.2f} sigma")
            assert dev <= 4.0
    against_estimator(r, which)


def test_a_cost_that_does_not_vary_is_flagged():
    c = pm.case("pend")
    ctx = context("pend", "scale")
    p = c.p.copy()
    p[1] = p[2] = 0.0                                                 # the sampler's two scales: no disturbance, one cost
    ctx.set_params(p)
    r = ctx.policy_sobol(*c.args(True), noise=c.user_noise(), groups=[G(step_normals=(0,))], K=64, seed_a=SEED_A, seed_b=SEED_B, want_costs=True)
    assert np.unique(r["y"]).size == 1 and r["var"] == 0.0 and r["flag"] == nv.SB_DEGENERATE and r["n_ok"] == 64
    assert np.isnan(r["S"]).all() and np.isnan(r["T_se"]).all()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------
def raw(ctx, c, words, K=None, npn=None, npu=None, seeds=(SEED_A, SEED_B), n_groups=None, check=True):
    """rat_policy_sobol itself, past the checks of the Python mirror"""
    x_nom, l, L = c.args(True)
    w = np.array(words, dtype=np.uint64).reshape(-1, 4)
    d = len(w) if n_groups is None else n_groups
    index, summary = np.zeros((max(len(w), 1), 4)), np.zeros(nv.SB_NSTAT)
    rc = nv.lib().rat_policy_sobol(ctx.h, nv.P(nv.f64(x_nom)), nv.P(nv.f64(l)), nv.P(nv.cm3(L)), C.c_int64(c.K if K is None else K),
                                   C.c_int32(c.npn if npn is None else npn), C.c_int32(c.npu if npu is None else npu),
                                   w.ctypes.data_as(nv._up), C.c_int32(d), C.c_uint64(seeds[0]), C.c_uint64(seeds[1]), nv.P(index), nv.P(summary), None)
    if check:
        nv.check(rc)
    return rc, index, summary


def test_refusals_and_the_handle_goes_on():
    c = pm.case("pend")
    ctx = context("pend", "scale")
    ctx.set_param_sampling(c.sampling(injected=False))
    one = [(0, 0, 1, 0)]
    arg = lambda **kw: pytest.raises(rat.RatError, match="RAT_ERR_ARG" + kw.get("m", ""))
    with arg(m=".*n_groups must be in 1 .. 16"):
        raw(ctx, c, one, n_groups=0)
    with arg(m=".*n_groups must be in 1 .. 16"):
        raw(ctx, c, [(0, 0, 0, 0)] * 17)
    with arg(m=".*K must be at least 2"):
        raw(ctx, c, one, K=1)
    with arg(m=".*must be at most 2\\^28"):
        raw(ctx, c, one, K=1 << 27)
    with arg(m=".*seed_a and seed_b must differ"):
        raw(ctx, c, one, seeds=(7, 7))
    with arg(m=".*overlaps an earlier group"):
        raw(ctx, c, [(0, 0, 3, 0), (1, 0, 2, 0)])
    with arg(m=".*at or beyond the declared count \\(3\\)"):
        raw(ctx, c, [(0, 0, 8, 0)])
    with arg(m=".*at or beyond the declared count \\(0\\)"):
        raw(ctx, c, [(0, 0, 0, 1)])                                   # the pendulum declares no step uniform
    with arg(m=".*at or beyond the declared count \\(2\\)"):
        raw(ctx, c, [(4, 0, 0, 0)])
    with arg(m=".*must not be negative"):
        raw(ctx, c, one, npn=-1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*above 64"):
        raw(ctx, c, one, npn=65)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*above 64"):
        raw(ctx, c, one, npu=65)
    ctx.set_param_sampling(c.sampling())                              # injected parameter streams
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*injected parameter draws"):
        raw(ctx, c, one)
    ctx.set_param_sampling(c.sampling(injected=False))
    with pytest.raises(ValueError, match="no injected streams"):
        ctx.policy_sobol(*c.args(True), noise=c.user_noise(zn=c.zn), groups=[G(step_normals=(0,))], K=c.K)
    assert raw(ctx, c, one)[0] == 0                                   # the handle goes on
    # a source without the sampler, a family, a general size
    plain = rat.Context(rat.DeviceSourceProblem(pm.um.PEND_PLAIN, 2, 1, c.N, c.W, params=c.p))
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_UNSUPPORTED.*does not define RAT_USER_NOISE"):
        raw(plain, c, one)
    for n in (2, 13):                                                 # n = 13: beyond the 12 + 4 tile
        fam = rat.Context(rat.LQRiskSensitiveProblem(0.9 * np.eye(n), np.ones((n, 1)), Q=np.eye(n), R=np.eye(1), N=c.N, W=1e-2 * np.eye(n), Qf=np.eye(n)))
        x = np.zeros((c.N + 1, n))
        index, summary, w = np.zeros((1, 4)), np.zeros(nv.SB_NSTAT), np.array(one, dtype=np.uint64)
        rc = nv.lib().rat_policy_sobol(fam.h, nv.P(x), nv.P(np.zeros((c.N, 1))), None, C.c_int64(64), C.c_int32(1), C.c_int32(0), w.ctypes.data_as(nv._up),
                                       C.c_int32(1), C.c_uint64(1), C.c_uint64(2), nv.P(index), nv.P(summary), None)
        assert rc == 2 and "not a source model" in nv.lib().rat_last_error().decode(), n


# ---- 8. the recorded evaluation is left alone -----------------------------------------------------------------------------------------------------
def test_the_recorded_evaluation_survives_the_call():
    c = pm.case("pend")
    ctx = context("pend", "scale")
    ctx.set_param_sampling(c.sampling(injected=False))
    e = ctx.policy_evaluate_noise(*c.args(True), noise=c.user_noise(seed=5), K=c.K, want_costs=True)
    before_t = ctx.policy_worst_case_trajectory(thetas=(0.0, 0.3))
    before_w = ctx.policy_worst_case(kl_bounds=(0.1,), want_weights=True)
    r = ctx.policy_sobol(*c.args(False), noise=c.user_noise(), groups=split_groups(c), K=c.K // 2, seed_a=SEED_A, seed_b=SEED_B, want_costs=True)
    assert r["n_ok"] == c.K // 2 and not np.array_equal(r["y"][0], e["costs"][:c.K // 2])
    after_w = ctx.policy_worst_case(kl_bounds=(0.1,), want_weights=True)       # the stored costs
    after_t = ctx.policy_worst_case_trajectory(thetas=(0.0, 0.3))              # the replay record: the closed-loop evaluation under seed 5

    def same(a, b):
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
        if isinstance(a, np.ndarray):
            return np.array_equal(a, b, equal_nan=True)
        return a == b or (a != a and b != b)
    assert same(before_w, after_w) and same(before_t, after_t)


# ---- 9. masks past bit 31: sixteen groups over all four words at 64 draws each ------------------------------------------------------------------
WIDE_K = 1 << 14
_WIDE = {}


def wide_context(nd=sm.WIDE_D):
    if nd not in _WIDE:
        _WIDE[nd] = rat.Context(sm.wide_problem(nd))
        _WIDE[nd].set_param_sampling(rat.ParamSampling(nd, nd))
    return _WIDE[nd]


def wide_run():
    """the shared call of the wide closed form: the sixteen groups of sobol_model.wide_groups(), all rows (computed once, left unchanged)"""
    if "run" not in _WIDE:
        x, l, L = sm.wide_policy()
        r = wide_context().policy_sobol(x, l, L, noise=rat.UserNoise(64, 64), groups=sm.wide_groups(), K=WIDE_K, seed_a=SEED0, seed_b=SEED0 + 1,
                                        want_costs=True)
        r["y"].setflags(write=False)
        _WIDE["run"] = (r, sm.wide_model(WIDE_K, SEED0, SEED0 + 1))
    return _WIDE["run"]


def test_wide_rows_a_and_b_are_the_evaluations_with_every_bit_of_row_b_live():
    r, _ = wide_run()
    x, l, L = sm.wide_policy()
    for row, seed in ((0, SEED0), (1, SEED0 + 1)):
        e = wide_context().policy_evaluate_noise(x, l, L, noise=rat.UserNoise(64, 64, seed=seed), K=WIDE_K, want_costs=True)
        assert np.array_equal(r["y"][row], e["costs"]), row
    assert not np.array_equal(r["y"][0], r["y"][1])


def test_wide_sixteen_groups_over_both_halves_of_all_four_words():
    r, model = wide_run()
    groups = sm.wide_groups()
    var, exact = sm.wide_exact(groups)
    scale = float(np.abs(model).max())
    err = np.abs(r["y"] - model).max(axis=1) / scale
    print(f"wide: rows against the model, the largest {err.max():.2e} of max |model| = {scale:.1f} (row {int(err.argmax())}); per row {np.array2string(err, precision=1)}")
    assert r["y"].shape == model.shape == (18, WIDE_K) and err.max() <= 1e-12
    assert np.array_equal(r["y"][17], r["y"][0])                      # the empty group, index 15: row A bit for bit
    for key in ("S", "S_se", "T", "T_se"):
        assert r[key][15] == 0.0, key
    for i in range(17):                                               # A, B and the fifteen groups that hold a draw: seventeen different rows
        for j in range(i):
            assert not np.array_equal(r["y"][i], r["y"][j]), (i, j)
    against_estimator(r, "wide")
    assert r["names"] == [g.name for g in groups] and r["names"][0] == "pn31" and r["names"][15] == "empty"
    assert r["n_ok"] == WIDE_K and r["flag"] == 0 and abs(r["var"] - var) <= 4.0 * r["var_se"]
    worst = 0.0
    for key in ("S", "T"):
        for i in range(15):
            dev = abs(r[key][i] - exact[i]) / r[key + "_se"][i]
            worst = max(worst, dev)
            print(f"wide: {key}[{i}] {groups[i].name} {r[key][i]:+.5f} +- {r[key + '_se'][i]:.5f} (exact {exact[i]:.5f}): {dev:.2f} sigma")
            assert dev <= 4.0, (key, i)
    print(f"wide: Var {r['var']:.3f} +- {r['var_se']:.3f} (exact {var}); the largest deviation {worst:.2f} sigma")


def test_wide_one_group_of_all_two_hundred_and_fifty_six_bits_is_row_b():
    base, _ = wide_run()
    x, l, L = sm.wide_policy()
    full = G(*[range(64)] * 4, name="all")
    assert full.words == (sm.ALL,) * 4
    r = wide_context().policy_sobol(x, l, L, noise=rat.UserNoise(64, 64), groups=[full], K=WIDE_K, seed_a=SEED0, seed_b=SEED0 + 1, want_costs=True)
    assert np.array_equal(r["y"][0], base["y"][0]) and np.array_equal(r["y"][1], base["y"][1]) and np.array_equal(r["y"][2], r["y"][1])
    against_estimator(r, "wide, one group of everything")
    for key in ("S", "T"):                                            # everything frozen at once: both estimate 1
        dev = abs(r[key][0] - 1.0) / r[key + "_se"][0]
        print(f"wide, one group of everything: {key} {r[key][0]:.5f} +- {r[key + '_se'][0]:.5f}: {dev:.2f} sigma from 1")
        assert dev <= 4.0 and r[key + "_se"][0] > 0.0
    assert r["flag"] == 0 and r["names"] == ["all"]


def test_a_count_of_forty_refuses_bit_forty_and_serves_bit_thirty_nine():
    from types import SimpleNamespace
    K, N = 256, sm.WIDE_N
    ctx = wide_context(40)
    c = SimpleNamespace(args=lambda closed: (np.zeros((N + 1, 1)), np.zeros((N, 1)), np.zeros((N, 1, 1))), K=K, npn=40, npu=40)
    for k in range(4):
        word = lambda b: tuple((1 << b) if j == k else 0 for j in range(4))
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*group 0 names a draw at or beyond the declared count \\(40\\)"):
            raw(ctx, c, [word(40)], seeds=(SEED0, SEED0 + 1))
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*group 1 names a draw at or beyond the declared count \\(40\\)"):
            raw(ctx, c, [word(39), word(63)], seeds=(SEED0, SEED0 + 1))
        rc, index, summary = raw(ctx, c, [word(39)], seeds=(SEED0, SEED0 + 1))
        assert rc == 0 and int(summary[nv.SB_FLAG]) == 0 and int(summary[nv.SB_N_OK]) == K and index[0, nv.SB_T] > 0.0, k
    groups = [G(param_normals=(39,)), G(param_uniforms=(39,)), G(step_normals=(39,)), G(step_uniforms=(39,))]
    x, l, L = sm.wide_policy()
    r = ctx.policy_sobol(x, l, L, noise=rat.UserNoise(40, 40), groups=groups, K=K, seed_a=SEED0, seed_b=SEED0 + 1, want_costs=True)
    model = sm.wide_costs(groups, K, SEED0, SEED0 + 1, nd=40)
    err = float(np.abs(r["y"] - model).max() / np.abs(model).max())
    print(f"wide at 40 draws: rows against the model {err:.2e}")
    assert err <= 1e-12 and np.unique(r["y"], axis=0).shape[0] == 6
    index = raw(ctx, c, [g.words for g in groups], seeds=(SEED0, SEED0 + 1))[1]      # (L = 0 under raw(): the same controls, the same bits)
    assert np.array_equal(index, np.stack([r[k] for k in ("S", "S_se", "T", "T_se")], axis=1))
    against_estimator(r, "wide at 40 draws")


# ---- 10. K across the stride of the reduction grid (256 blocks of 256 lanes) ----------------------------------------------------------------------
LONG_K = 65536 + 5
_LONG = {}


def long_run():
    """the additive closed form at K = 65536 + 5: lanes 0 .. 4 of the first block of sb_pass1 / sb_pass2 take a second trip"""
    if not _LONG:
        ctx = rat.Context(sm.closed_problem("additive"))
        ctx.set_param_sampling(rat.ParamSampling(2, 0))
        x, l, L = sm.closed_policy()
        call = lambda K: ctx.policy_sobol(x, l, L, noise=rat.UserNoise(1, 0), groups=sm.closed_groups(), K=K, seed_a=SEED0, seed_b=SEED0 + 1,
                                          want_costs=True)
        model = sm.closed_costs("additive", LONG_K, SEED0, SEED0 + 1)
        r = call(LONG_K)
        for v in (r["y"], model):
            v.setflags(write=False)
        _LONG.update(ctx=ctx, call=call, r=r, model=model)
    return _LONG


def test_the_additive_form_across_the_reduction_grid():
    run = long_run()
    r, model, m = run["r"], run["model"], sm.CLOSED["additive"]
    err = float(np.abs(r["y"] - model).max())
    print(f"additive at K = {LONG_K}: rows against the model {err:.2e}, in the second trip {float(np.abs(r['y'][:, 65536:] - model[:, 65536:]).max()):.2e}")
    assert r["y"].shape == (5, LONG_K) and err <= 1e-12 * float(np.abs(model).max())
    x, l, L = sm.closed_policy()
    for row, seed in ((0, SEED0), (1, SEED0 + 1)):
        e = run["ctx"].policy_evaluate_noise(x, l, L, noise=rat.UserNoise(1, 0, seed=seed), K=LONG_K, want_costs=True)
        assert np.array_equal(r["y"][row], e["costs"]), row
    against_estimator(r, f"additive at K = {LONG_K}")
    assert r["n_ok"] == LONG_K and r["flag"] == 0 and abs(r["var"] - m["var"]) <= 4.0 * r["var_se"]
    for key in ("S", "T"):
        for i in range(3):
            dev = abs(r[key][i] - m[key][i]) / r[key + "_se"][i]
            print(f"additive at K = {LONG_K}: {key}[{i}] {r[key][i]:+.5f} +- {r[key + '_se'][i]:.5f} (exact {m[key][i]}): {dev:.2f} sigma")
            assert dev <= 4.0


@pytest.mark.parametrize("K", [65535, 65536])
def test_a_call_that_ends_at_the_stride_returns_the_leading_columns(K):
    run = long_run()
    short = run["call"](K)
    assert np.array_equal(short["y"], run["r"]["y"][:, :K]) and short["n_ok"] == K
    against_estimator(short, f"additive at K = {K}")


def test_dropped_base_samples_on_both_sides_of_the_stride():
    c = pm.case("pend")
    groups = split_groups(c)
    m = sm.nan_thresholds(c, LONG_K, SEED_A, SEED_B)
    tail = np.sort(m[65536:])
    p = c.p.copy()
    p[c.idx["pnan"]] = 0.5 * (tail[3] + tail[4])                      # four of the five base samples of the second trip survive, one drops
    model = sm.pend_costs(c, "nan", groups, LONG_K, SEED_A, SEED_B, p=p)
    bad = np.isnan(model).any(axis=0)
    print(f"nan hook at K = {LONG_K}: threshold {p[c.idx['pnan']]:.4f}, dropped {int(bad.sum())}, of them at or beyond 65536: {int(bad[65536:].sum())}")
    assert bad[65536:].sum() == 1 and (~bad[65536:]).sum() == 4 and bad[:65536].any() and (~bad[:65536]).any()
    assert np.array_equal(bad, m > p[c.idx["pnan"]])
    ctx = context("pend", "nan")
    ctx.set_params(p)
    ctx.set_param_sampling(c.sampling(injected=False))
    r = ctx.policy_sobol(*c.args(True), noise=c.user_noise(), groups=groups, K=LONG_K, seed_a=SEED_A, seed_b=SEED_B, want_costs=True)
    assert np.array_equal(np.isnan(r["y"]), np.isnan(model))
    assert r["n_ok"] == LONG_K - bad.sum() and r["flag"] == 0
    err = float(np.nanmax(np.abs(r["y"] / model - 1)))
    print(f"nan hook at K = {LONG_K}: rows against the model {err:.2e}")
    assert err <= 1e-12
    against_estimator(r, f"nan hook at K = {LONG_K}")


# ---- 11. few survivors, and a mean that is large against the spread -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_left", [0, 1, 2])
def test_few_survivors(n_left):
    c = pm.case("pend")
    groups = split_groups(c)
    ms = np.sort(sm.nan_thresholds(c, 64, SEED_A, SEED_B))
    p = c.p.copy()
    p[c.idx["pnan"]] = ms[0] - 0.5 if n_left == 0 else 0.5 * (ms[n_left - 1] + ms[n_left])
    model = sm.case_costs(c, "nan", True, groups, 64, SEED_A, SEED_B, p=p)
    alive = ~np.isnan(model).any(axis=0)
    ref = sm.estimator(model)
    assert alive.sum() == n_left and ref["n_ok"] == n_left and np.array_equal(alive, sm.nan_thresholds(c, 64, SEED_A, SEED_B) <= p[c.idx["pnan"]])
    assert not np.isnan(model[:, alive]).any()                        # the survivors are whole in all five rows
    ctx = context("pend", "nan")
    ctx.set_params(p)
    ctx.set_param_sampling(c.sampling(injected=False))
    r = ctx.policy_sobol(*c.args(True), noise=c.user_noise(), groups=groups, K=64, seed_a=SEED_A, seed_b=SEED_B, want_costs=True)   # rc: RAT_OK
    assert np.array_equal(np.isnan(r["y"]), np.isnan(model)) and r["n_ok"] == n_left
    if n_left == 2:
        assert r["flag"] == 0
        against_estimator(r, "two survivors")
        return
    assert r["flag"] == nv.SB_DEGENERATE and ref["flag"] == sm.DEGENERATE and np.isnan(r["var_se"])
    for key in ("S", "S_se", "T", "T_se"):
        assert np.isnan(r[key]).all(), key
    if n_left == 0:
        assert np.isnan(r["mean"]) and np.isnan(r["var"])
    else:
        print(f"one survivor: mean {r['mean']:.6g} against fsum {abs(r['mean'] - ref['mean']):.2e}, var {r['var']:.6g} against fsum {abs(r['var'] - ref['var']):.2e}")
        assert np.isfinite(r["mean"]) and np.isfinite(r["var"]) and r["var"] > 0.0
        assert abs(r["mean"] - ref["mean"]) <= 1e-9 * max(1.0, abs(ref["mean"])) and abs(r["var"] - ref["var"]) <= 1e-9 * max(1.0, abs(ref["var"]))


def test_a_mean_ten_thousand_spreads_away():
    from test_cpu_sobol import OFFSET, large_mean_figures
    uncentred, centred, Y = large_mean_figures()                      # on the model's rows, before the device is touched
    assert uncentred > 1e-6 and centred <= 1e-10
    ctx = rat.Context(sm.offset_problem())
    ctx.set_param_sampling(rat.ParamSampling(2, 0))
    x, l, L = sm.closed_policy()
    kw = dict(noise=rat.UserNoise(1, 0), groups=sm.closed_groups(), K=sm.CLOSED_K, seed_a=SEED0, seed_b=SEED0 + 1, want_costs=True)
    ctx.set_params([0.0, 0.0, OFFSET])
    r = ctx.policy_sobol(x, l, L, **kw)
    err = float(np.abs(r["y"] - Y).max())
    print(f"offset {OFFSET}: rows against the model {err:.2e}; mean {r['mean']:.4f}, sd {np.sqrt(r['var']):.4f}, |mean| / sd {abs(r['mean']) / np.sqrt(r['var']):.1f}")
    assert err <= 1e-12 * float(np.abs(Y).max()) and 0.9e4 <= abs(r["mean"]) / np.sqrt(r["var"]) <= 1.1e4
    against_estimator(r, f"offset {OFFSET}")
    ctx.set_params([0.0, 0.0, 0.0])
    r0 = ctx.policy_sobol(x, l, L, **kw)
    Y0 = sm.closed_costs("additive", sm.CLOSED_K, SEED0, SEED0 + 1)
    assert float(np.abs(r0["y"] - Y0).max()) <= 1e-12 * float(np.abs(Y0).max())
    for key in ("S", "T"):
        gap = float(np.abs(r[key] - r0[key]).max())
        print(f"offset {OFFSET}: {key} {np.round(r[key], 5)} against offset 0 {gap:.2e}")
        assert gap <= 1e-9, key
