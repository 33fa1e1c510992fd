"""Monte-Carlo evaluation of a source model under user-written process noise (rat_policy_evaluate_noise, csrc/source_user_noise.h): what
can be checked without a device -- the compile-only entry point rat_user_noise_check (hiprtc for gfx950), the exports and their mirrors,
and the NumPy model the GPU tests compare against."""
import os
import re

import numpy as np

import ratilqr.jl_amd as rat
from ratilqr.jl_amd import _native as nv
import user_noise_model as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = open(os.path.join(ROOT, "julia", "RATiLQRAMD.jl")).read()


def check(src, n, m, npn, npu):
    rc = nv.lib().rat_user_noise_check(src.encode(), n, m, npn, npu)
    return rc, nv.lib().rat_last_error().decode()


def test_the_two_test_sources_compile():
    d = um.PEND_STATE_DIMS
    assert check(um.PEND_STATE, d["n"], d["m"], d["normals_per_step"], d["uniforms_per_step"])[0] == 0
    assert check(um.LQ_MIX, 12, 4, 12, 1)[0] == 0
    nv.user_noise_check(um.PEND_MIX, 2, 1, 2, 1)                      # the Python mirror raises on failure
    # a source with a sampler still compiles as an ordinary source model
    assert nv.lib().rat_source_check(um.PEND_STATE.encode(), 2, 1) == 0


def test_a_typo_in_the_sampler_is_reported_by_line():
    bad = um.PEND_STATE.replace("fabs(x[1])", "fabz(x[1])")
    rc, msg = check(bad, 2, 1, 3, 0)
    assert rc == 1 and "fabz" in msg
    line = bad[:bad.index("fabz")].count("\n") + 1
    assert f"model.hip:{line}" in msg, msg


def test_refusals():
    rc, msg = check(um.PEND_PLAIN, 2, 1, 2, 0)
    assert rc == 1 and "RAT_USER_NOISE" in msg and "does not define" in msg
    assert check(um.PEND_STATE, 13, 1, 3, 0)[0] == 2                 # RAT_ERR_UNSUPPORTED: beyond the 12 + 4 tile
    assert check(um.PEND_STATE, 2, 5, 3, 0)[0] == 2
    assert check(um.PEND_STATE, 2, 1, -1, 0)[0] == 1 and check(um.PEND_STATE, 2, 1, 3, -1)[0] == 1
    assert check(um.PEND_STATE, 0, 1, 3, 0)[0] == 1
    assert nv.lib().rat_user_noise_check(None, 2, 1, 3, 0) == 1


def test_exports_and_mirrors():
    lib = nv.lib()
    for name in ("rat_policy_evaluate_noise", "rat_user_noise_check"):
        assert hasattr(lib, name) and name in nv.EXPORTS
        assert re.search(r"ccall\(\(:" + name + r", LIB\)", JL), name
    assert callable(rat.Context.policy_evaluate_noise) and callable(nv.user_noise_check)
    n = rat.UserNoise(3, 1, zn=np.zeros((2, 4, 3)), seed=5)
    assert (n.normals_per_step, n.uniforms_per_step, n.seed, n.zu) == (3, 1, 5, None) and n.zn.dtype == np.float64
    for name in ("UserNoise", "user_noise_check"):
        assert re.search(r"\nexport\b.*[\s,]" + name + r"[,\n]", JL, flags=re.S), name
    assert re.search(r"function evaluate_policy\([^)]*noise::", JL)


def test_numpy_model_reads_the_slot_layout_and_marks_domain_errors():
    K, N = 3, 4
    rng = np.random.default_rng(0)
    zn = rng.standard_normal((K, N, 3))
    x0, l = np.array([0.4, -0.3]), 0.1 * rng.standard_normal((N, 1))
    cost, xs, us = um.np_rollouts(um.pend_f, um.pend_c, um.pend_h, um.pend_state_noise, um.PEND_STATE_P, x0, l, None, K, zn.ravel(), None, 3, 0)
    p = um.PEND_STATE_P
    x = x0.copy()                                                     # rollout 1, step by step
    for t in range(N):
        assert np.array_equal(xs[1, t], x) and np.array_equal(us[1, t], l[t])
        z = zn[1, t]
        x = um.pend_f(x, l[t], p) + np.array([p[1] * abs(x[0]) * z[0], p[1] * abs(x[1]) * z[1] + p[2] * z[2]])
    assert np.array_equal(xs[1, N], x) and np.all(np.isfinite(cost))
    z1 = np.zeros((K, N, 1)); z1[2, 1, 0] = 3.5
    cost, _, _ = um.np_rollouts(um.pend_f, um.pend_c, um.pend_h, um.pend_nan_noise, [0.1, 0.05], x0, l, None, K, z1.ravel(), None, 1, 0)
    assert np.array_equal(np.isnan(cost), [False, False, True])


def test_the_numpy_generator_run_is_stable_at_the_statistical_tests_margin():
    """tests/test_gpu_user_noise.py holds the device generator's mean at K = 20 000 within 5 standard errors of this run's mean: two
    NumPy runs with different seeds must agree at that margin themselves (the difference of two independent means has a standard
    deviation of sqrt(2) standard errors: 5 of them are 3.5 sigma)."""
    N, K = 10, 20000
    x_nom, l, L = um.pend_policy(N)
    a = um.np_pend_state_costs(um.PEND_STATE_P, x_nom, l, L, K, seed=101)
    b = um.np_pend_state_costs(um.PEND_STATE_P, x_nom, l, L, K, seed=202)
    se = a.std(ddof=1) / np.sqrt(K)
    assert se > 0 and abs(a.mean() - b.mean()) <= 5.0 * se
    # the vectorised run is the per-rollout model: the same injected draws, the same costs
    zn = np.random.default_rng(3).standard_normal((4, N, 3))
    c1, _, _ = um.np_rollouts(um.pend_f, um.pend_c, um.pend_h, um.pend_state_noise, um.PEND_STATE_P, x_nom, l, L, 4, zn.ravel(), None, 3, 0)

    class Fixed:
        def __init__(self):
            self.t, self.i = 0, 0

        def normal(self):
            v = zn[:, self.i // 3, self.i % 3]
            self.i += 1
            return v

    real = um.GenRng
    um.GenRng = lambda seed, K: Fixed()
    try:
        c2 = um.np_pend_state_costs(um.PEND_STATE_P, x_nom, l, L, 4, seed=0)
    finally:
        um.GenRng = real
    assert np.allclose(c1, c2, rtol=1e-13, atol=0.0)

