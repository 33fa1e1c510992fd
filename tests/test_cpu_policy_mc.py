"""rat_policy_evaluate without a device: the symbol and its declarations, the source models' Monte-Carlo rollout kernel compiled for
gfx950, the argument checks that come before the handle is touched, and the NumPy model of the device reduction (policy_mc_model.py)
against an extended-precision evaluation."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ratilqr.jl_amd as rat
from ratilqr.jl_amd import _native as nv
from policy_mc_model import direct, reduce_costs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ratilqr.h")).read()

PENDULUM = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) {
    const double dt = p[0];
    xn[0] = x[0] + dt * x[1];
    xn[1] = x[1] + dt * (-sin(x[0]) - 0.1 * x[1] + u[0]);
}
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) {
    return 0.5 * (x[0] * x[0] + x[1] * x[1]) + 0.05 * (u[0] * u[0]) + 0.01 * k * x[0];
}
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return 2.0 * (x[0] * x[0] + x[1] * x[1]); }
"""


def test_symbol_header_and_exports():
    assert hasattr(nv.lib(), "rat_policy_evaluate")
    assert "rat_policy_evaluate" in nv.EXPORTS
    assert re.search(r"rat_rc\s+rat_policy_evaluate\s*\(\s*rat_handle h,", HEADER)
    for name, val in (("N_OK", 0), ("N_DOMAIN", 1), ("MEAN", 2), ("VAR", 3), ("MIN", 4), ("MAX", 5), ("SE_MEAN", 6), ("NSTAT", 8)):
        assert re.search(rf"#define RAT_MC_{name}\s+{val}\b", HEADER), name
        assert getattr(nv, "MC_" + name) == val
    assert "RAT_VERSION 600" in HEADER
    assert callable(rat.evaluate_policy) and callable(rat.Context.policy_evaluate)
    # the refusal of rat_rollout_noisy stays, and the header names the way round it
    assert "rat_policy_evaluate with cost_out" in HEADER


def test_julia_binds_the_symbol():
    jl = open(os.path.join(ROOT, "julia", "RATiLQRAMD.jl")).read()
    assert "(:rat_policy_evaluate, LIB)" in jl and re.search(r"export[^\n]*(\n[^\n]*)*evaluate_policy", jl)


def _compile_noisy(src, n, m, tmp_path):
    """The Monte-Carlo kernel's translation unit as the library assembles it for hiprtc (source_model.cpp), through hipcc for gfx950."""
    csrc = os.path.join(ROOT, "ratilqr.jl_amd", "csrc")
    unit = tmp_path / f"noisy_{n}_{m}.hip"
    unit.write_text('#include <hip/hip_runtime.h>\n#include "source_args.h"\n#include "rat_ad.h"\n#include "rat_rng.h"\n' + src +
                    '\n#include "source_noisy.h"\n')
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", f"-DRAT_N={n}", f"-DRAT_M={m}",
                           "-DRAT_PETS_NORMALS=0", "-DRAT_PETS_UNIFORMS=0", "-I", csrc, "-c", str(unit), "-o", str(tmp_path / "noisy.o")],
                          capture_output=True, text=True)


def test_source_modules_compile_for_gfx950(tmp_path):
    """The model kernels' module is what it was (rat_source_check; the Monte-Carlo kernel is a module of its own, compiled by the first
    rat_policy_evaluate of a source problem), and that kernel compiles for gfx950 behind the pendulum and at the widest size."""
    L = nv.lib()
    assert L.rat_source_check(PENDULUM.encode(), 2, 1) == 0, L.rat_last_error().decode()
    assert "rat_src_noisy_rollout" not in open(os.path.join(ROOT, "ratilqr.jl_amd", "csrc", "source_kernels.h")).read()
    src = open(os.path.join(ROOT, "ratilqr.jl_amd", "csrc", "source_noisy.h")).read()
    assert 'extern "C" __global__ __launch_bounds__(64) void rat_src_noisy_rollout(SrcNoisyArgs a)' in src
    assert "source_noisy.h" in open(os.path.join(ROOT, "ratilqr.jl_amd", "csrc", "Makefile")).read()       # embedded in the library
    r = _compile_noisy(PENDULUM, 2, 1, tmp_path)
    assert r.returncode == 0, r.stderr
    wide = PENDULUM.replace("xn[1] = x[1]", "for (int i = 2; i < RAT_N; ++i) xn[i] = 0.5 * x[i] + u[i & 3];\n    xn[1] = x[1]")
    r = _compile_noisy(wide, 12, 4, tmp_path)
    assert r.returncode == 0, r.stderr
    assert L.rat_source_check(wide.encode(), 12, 4) == 0, L.rat_last_error().decode()


def _call(K=4, thetas=(0.5,), h=None):
    th = nv.f64(np.asarray(thetas, dtype=np.float64))
    x, l, stats = np.zeros(4), np.zeros(4), np.zeros(8)
    L = nv.lib()
    rc = L.rat_policy_evaluate(h, nv.P(x), nv.P(l), None, C.c_int64(K), None, C.c_uint64(0), nv.P(th), C.c_int32(th.size), nv.P(stats),
                               None, None, None)
    return rc, L.rat_last_error().decode()


def test_argument_checks_come_before_the_handle():
    """n_theta, theta and K are checked first: the message names them even without a handle (a null handle alone is RAT_ERR_ARG "null")."""
    rc, msg = _call(thetas=np.zeros(17))
    assert rc == 1 and "n_theta" in msg
    rc, msg = _call(thetas=(0.1, -0.5))
    assert rc == 1 and "theta must be >= 0" in msg
    rc, msg = _call(thetas=(float("nan"),))
    assert rc == 1 and "theta must be >= 0" in msg
    rc, msg = _call(K=0)
    assert rc == 1 and "K must be positive" in msg
    rc, msg = _call(K=(1 << 27) + 1)
    assert rc == 1 and "2^27" in msg
    rc, msg = _call()
    assert rc == 1 and msg == "null"


# ---- the model of the reduction --------------------------------------------------------------------------------------------------
def _extended(J, thetas):
    """float128 / math.fsum evaluation of the definitions."""
    J = np.asarray(J, dtype=np.float64)
    J = J[~np.isnan(J)]
    n = J.size
    mean = math.fsum(J) / n
    Jl = J.astype(np.longdouble)
    var = float(math.fsum(((Jl - np.longdouble(mean)) ** 2).astype(np.float64))) / (n - 1)
    mx = J.max()
    risk, se = [], []
    for t in thetas:
        if t == 0.0:
            risk.append(mean); se.append(math.sqrt(var / n))
            continue
        y = np.exp(np.longdouble(t) * (Jl - np.longdouble(mx)))
        ybar = y.sum() / n
        vy = ((y - ybar) ** 2).sum() / (n - 1)
        risk.append(float(mx + np.log(ybar) / t))
        se.append(float(np.sqrt(vy) / (ybar * t * np.sqrt(np.longdouble(n)))))
    return dict(mean=mean, var=var, min=J.min(), max=mx, se_mean=math.sqrt(var / n), risk=np.array(risk), risk_se=np.array(se))


@pytest.mark.parametrize("K", [1, 2, 37, 5000, 70001])
def test_model_agrees_with_extended_precision(K):
    rng = np.random.default_rng(K)
    J = 3.0 + 2.0 * rng.standard_normal(K) ** 2
    thetas = (0.0, 1e-4, 0.1, 1.0, 7.0)
    got = reduce_costs(J, thetas)
    assert got["n_ok"] == K and got["n_domain"] == 0
    if K == 1:
        assert got["mean"] == J[0] == got["min"] == got["max"] and np.isnan(got["var"]) and np.isnan(got["se_mean"])
        assert np.allclose(got["risk"], J[0], rtol=1e-15) and np.all(np.isnan(got["risk_se"][1:]))
        return
    ref = _extended(J, thetas)
    for key in ("mean", "var", "se_mean", "risk", "risk_se"):
        assert np.allclose(got[key], ref[key], rtol=1e-12, atol=0.0), key
    assert got["min"] == ref["min"] and got["max"] == ref["max"]
    assert got["risk"][0] == got["mean"] and got["risk_se"][0] == got["se_mean"]           # theta = 0: the mean and its error
    d = direct(J, thetas)
    for key in ("mean", "var", "se_mean", "risk"):
        assert np.allclose(got[key], d[key], rtol=1e-11, atol=0.0), key


def test_model_leaves_nan_costs_out():
    rng = np.random.default_rng(5)
    J = rng.standard_normal(3000)
    bad = rng.random(3000) < 0.3
    Jn = np.where(bad, np.nan, J)
    got, ref = reduce_costs(Jn, (0.0, 0.5)), reduce_costs(J[~bad], (0.0, 0.5))
    assert got["n_ok"] == int((~bad).sum()) and got["n_domain"] == int(bad.sum()) and got["n_ok"] + got["n_domain"] == 3000
    ext = _extended(J[~bad], (0.0, 0.5))
    for key in ("mean", "var", "risk", "risk_se"):
        assert np.allclose(got[key], ext[key], rtol=1e-12, atol=0.0) and np.allclose(ref[key], ext[key], rtol=1e-12, atol=0.0), key
    none = reduce_costs(np.full(10, np.nan), (0.0, 1.0))
    assert none["n_ok"] == 0 and none["n_domain"] == 10
    assert all(np.isnan(none[k]) for k in ("mean", "var", "min", "max", "se_mean")) and np.all(np.isnan(none["risk"])) and np.all(np.isnan(none["risk_se"]))


def test_model_does_not_overflow_at_theta_range_2000():
    rng = np.random.default_rng(6)
    J = rng.uniform(0.0, 1.0, 4096)
    J[0], J[1] = 0.0, 1.0
    theta = 2000.0                                                       # theta (max - min) = 2000: exp(theta J) itself overflows
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(theta * J)).any()
    got = reduce_costs(J, (theta,))
    ref = _extended(J, (theta,))
    assert np.isfinite(got["risk"][0]) and np.isfinite(got["risk_se"][0])
    assert np.allclose(got["risk"], ref["risk"], rtol=1e-12) and np.allclose(got["risk_se"], ref["risk_se"], rtol=1e-12)
    assert got["max"] - math.log(4096) / theta <= got["risk"][0] <= got["max"]
