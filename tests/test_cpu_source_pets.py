"""Generative source models (PETS, rat_pets_problem_set_source) without a device: rat_pets_source_check (hiprtc through dlopen, gfx950)
and the Python helpers."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
from ratilqr.jl_amd import pets
from source_pets_models import DOCS, DOCS_DIMS, LQ, PENDULUM, PENDULUM_DIMS, REF_TEST, REF_TEST_DIMS


def check(src, n=2, m=2, npn=2, npu=1):
    L = rat.native.lib()
    rc = L.rat_pets_source_check(src.encode(), n, m, npn, npu)
    return rc, L.rat_last_error().decode()


def dims(d):
    return d["n"], d["m"], d["normals_per_step"], d["uniforms_per_step"]


def test_source_check_accepts_the_docs_example_the_pendulum_and_the_reference_test():
    for src, d in ((DOCS, DOCS_DIMS), (PENDULUM, PENDULUM_DIMS), (REF_TEST, REF_TEST_DIMS)):
        rc, log = check(src, *dims(d))
        assert rc == 0, log
    rc, log = check(LQ, 12, 4, 12, 1)                                 # BASELINE config 5's shape
    assert rc == 0, log


def test_source_check_reports_a_syntax_error_with_its_line():
    bad = PENDULUM.replace("xn[0] = x[0] + dt * x[1];", "xn[0] = x[0] + * dt x[1];")
    rc, log = check(bad, *dims(PENDULUM_DIMS))
    assert rc == 1 and "model.hip:4:" in log and "error" in log, log


@pytest.mark.parametrize("name", ["rat_user_f_stochastic", "rat_user_h"])
def test_source_check_refuses_a_source_without_f_stochastic_or_h(name):
    head, tail = PENDULUM.split("__device__ void rat_user_f_stochastic") if name == "rat_user_f_stochastic" else \
        PENDULUM.split("template <class T> __device__ T rat_user_h")
    src = head + ("template <class T> __device__ T rat_user_c" + tail.split("template <class T> __device__ T rat_user_c")[1]
                  if name == "rat_user_f_stochastic" else "")
    assert name not in src
    rc, log = check(src, *dims(PENDULUM_DIMS))
    assert rc == 1 and name in log, log


def test_a_generative_source_needs_no_rat_user_f_and_a_source_with_all_four_serves_both():
    assert "rat_user_f(" not in PENDULUM and check(PENDULUM, *dims(PENDULUM_DIMS))[0] == 0
    both = PENDULUM + r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) {
    xn[0] = x[0] + p[0] * x[1];
    xn[1] = x[1] + p[0] * (-sin(x[0]) - p[1] * x[1] + u[0]);
}
"""
    assert check(both, *dims(PENDULUM_DIMS))[0] == 0
    L = rat.native.lib()
    assert L.rat_source_check(both.encode(), 2, 1) == 0, L.rat_last_error().decode()


def test_source_check_refuses_sizes_beyond_the_tile_and_negative_counts():
    assert check(PENDULUM, 13, 1, 1, 0)[0] == 2
    assert check(PENDULUM, 2, 5, 1, 0)[0] == 2
    assert check(PENDULUM, 2, 1, -1, 0)[0] == 1
    assert check(PENDULUM, 2, 1, 1, -2)[0] == 1


def test_the_draw_counts_are_compile_time_constants():
    src = PENDULUM.replace("const double dt = p[0];", "static_assert(RAT_PETS_NORMALS == 1 && RAT_PETS_UNIFORMS == 3, \"counts\");\n"
                           "    const double dt = p[0];")
    assert check(src, 2, 1, 1, 3)[0] == 0
    rc, log = check(src, 2, 1, 1, 0)
    assert rc == 1 and "counts" in log, log


def test_python_helper_raises_with_the_log():
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG"):
        rat.native.pets_source_check(PENDULUM.replace("sin(", "sine("), 2, 1, 1, 0)
    rat.native.pets_source_check(PENDULUM, 2, 1, 1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED"):
        rat.native.pets_source_check(PENDULUM, 13, 1)


def test_draw_noise_shapes_for_source_problems():
    rng = np.random.default_rng(0)
    S, K, N = 3, 5, 7
    docs = rat.DeviceGenerativeSourceProblem(DOCS, 2, 2, N, params=[10.0], normals_per_step=2, uniforms_per_step=1)
    zn, zu = pets.draw_noise(docs, rng, S, K, use_true_model=True)
    assert zn.shape == (S * K * N * 2,) and zu.shape == (S * K * N,)
    assert np.all((zu >= 0) & (zu < 1))
    ref = rat.DeviceGenerativeSourceProblem(REF_TEST, 2, 2, N, normals_per_step=0, uniforms_per_step=2)
    zn, zu = pets.draw_noise(ref, rng, S, K)
    assert zn is None and zu.shape == (S * K * N * 2,)
    pend = rat.DeviceGenerativeSourceProblem(PENDULUM, 2, 1, N, params=[0.1, 0.1, 0.05], normals_per_step=1)
    zn, zu = pets.draw_noise(pend, rng, S, K)
    assert zn.shape == (S * K * N,) and zu is None
    dflt = rat.DeviceGenerativeSourceProblem(PENDULUM, 2, 1, N)
    assert dflt.normals_per_step == 2 and dflt.uniforms_per_step == 0 and dflt.params.size == 0
    assert isinstance(dflt, rat.problems.FiniteHorizonGenerativeOptimalControlProblem)
