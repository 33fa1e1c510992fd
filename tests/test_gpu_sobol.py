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
bit for bit; the closed forms of tests/test_cpu_sobol.py within 4 reported standard errors; every refusal of the header with its code."""
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
