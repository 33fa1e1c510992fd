"""Model parameters drawn per rollout without a GPU (rat_user_params, include/ratilqr.h "source models"): rat_user_params_check compiles the
cases of tests/user_params_model.py for gfx950 and refuses what the header says it refuses, every new export exists, the NumPy model
agrees with itself when K is cut into chunks, the generator's keying is a function of the global rollout index, and one closed form."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
import user_params_model as pm
from ratilqr.jl_amd import _native as nv


def test_every_export_exists():
    L = nv.lib()
    for name in ("rat_policy_params_sampling", "rat_user_params_check", "rat_policy_params_sample"):
        assert name in nv.EXPORTS and getattr(L, name) is not None
    assert rat.ParamSampling(2, 1).param_normals == 2 and callable(rat.user_params_check)
    assert hasattr(rat.Context, "set_param_sampling") and hasattr(rat.Context, "sample_params")


@pytest.mark.parametrize("hook", ["scale", "identity", "nan"])
@pytest.mark.parametrize("name", pm.CASE_NAMES)
def test_the_cases_compile_for_gfx950(name, hook):
    c = pm.case(name)
    rat.user_params_check(c.source(hook), c.n, c.m, c.p.size, c.npn, c.npu, pm.PARAM_NORMALS, pm.PARAM_UNIFORMS)
    # with the user's event behind it, and under the other kinds' checks (sampling off: the hook is not compiled in)
    rat.user_event_check(c.source(hook, event=True), c.n, c.m, n_event=1)
    rat.native.user_noise_check(c.source(hook), c.n, c.m, c.npn, c.npu)


def test_refusals():
    c = pm.case("pend")
    args = (c.n, c.m, c.p.size, c.npn, c.npu, pm.PARAM_NORMALS, pm.PARAM_UNIFORMS)
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_ARG.*does not define RAT_USER_PARAMS"):
        rat.user_params_check(c.source(None), *args)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*above 32"):
        rat.user_params_check(c.source("scale"), c.n, c.m, 33, c.npn, c.npu, 2, 1)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no parameters"):
        rat.user_params_check(c.source("scale"), c.n, c.m, 0, c.npn, c.npu, 2, 1)
    for pn, pu in ((-1, 1), (2, -1)):
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*must not be negative"):
            rat.user_params_check(c.source("scale"), c.n, c.m, c.p.size, c.npn, c.npu, pn, pu)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*must not be negative"):
        rat.user_params_check(c.source("scale"), c.n, c.m, c.p.size, -1, 0, 2, 1)
    # a hook that draws is a template over the generator: a wrong signature does not compile
    bad = c.source("scale").replace("R &rng, const double *p, double *q", "R &rng, double *q")
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_ARG.*rat_user_params"):
        rat.user_params_check(bad, *args)


@pytest.mark.parametrize("name", pm.CASE_NAMES)
def test_the_model_agrees_with_itself_across_chunks(name):
    """rollout j reads row j of the parameter draws and its own step draws wherever a chunk starts"""
    c = pm.case(name)
    cost, xs, us = c.model("scale", True)
    cut = c.K // 3 + 1
    parts = [c.model("scale", True, K=min(cut, c.K - j0), j0=j0) for j0 in range(0, c.K, cut)]
    for i, ref in enumerate((cost, xs, us)):
        assert np.array_equal(np.concatenate([p[i] for p in parts]), ref)
    free, _, _ = c.model(None, True)
    assert not np.allclose(cost, free, rtol=1e-3)                     # the drawn parameters move the costs
    same, _, _ = c.model("identity", True)
    assert np.array_equal(same, free)


def test_the_generator_is_keyed_by_the_global_rollout_index():
    zn, zu = pm.gen_draws(0x1234567890ABCDEF, 300, 3, 2)
    for j0, K in ((0, 7), (100, 200), (299, 1)):
        a, b = pm.gen_draws(0x1234567890ABCDEF, K, 3, 2, j0=j0)
        assert np.array_equal(a, zn[j0:j0 + K]) and np.array_equal(b, zu[j0:j0 + K])
    assert np.array_equal(pm.gen_draws(0x1234567890ABCDEF, 300, 1, 1)[0][:, 0], zn[:, 0])      # a draw does not depend on the count
    assert np.all((zu >= 0) & (zu < 1)) and abs(zn.mean()) < 0.2 and abs(zn.std() - 1) < 0.2
    assert not np.array_equal(pm.gen_draws(2, 300, 3, 2)[0], zn)


def test_the_scalar_closed_form():
    """x+ = a x, cost sum_{t <= N} x_t^2, a ~ N(a0, s^2): the model's mean over 2^14 rollouts under the generator's draws for this seed lies
    within 4 of its standard errors of sum_t E a^(2t) x_0^2 (the GPU test holds the device to the same seed)."""
    a0, s, x0, N, K, seed = 0.9, 0.05, 1.5, 6, 1 << 14, 2024
    zpn, _ = pm.gen_draws(seed, K, 1, 0)
    a = a0 + s * zpn[:, 0]
    cost = x0 * x0 * sum(a ** (2 * t) for t in range(N + 1))
    ref = pm.scalar_mean_cost(a0, s, x0, N)
    se = cost.std(ddof=1) / np.sqrt(K)
    print(f"closed form {ref:.6f}, model mean {cost.mean():.6f}, se {se:.2e}: {abs(cost.mean() - ref) / se:.2f} sigma")
    assert abs(cost.mean() - ref) <= 4.0 * se
    assert np.isclose(pm.normal_moment(0.0, 2.0, 4), 3 * 16.0) and np.isclose(pm.normal_moment(1.0, 0.0, 5), 1.0)
