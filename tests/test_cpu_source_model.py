"""Source models (RAT_MODEL_SOURCE) without a device: rat_source_check (hiprtc through dlopen, gfx950) and the forward-mode AD header
(csrc/rat_ad.h) compiled for the host and checked against closed-form derivatives."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import ratilqr.jl_amd as rat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AD_H = os.path.join(ROOT, "ratilqr.jl_amd", "csrc", "rat_ad.h")

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


def check(src, n=2, m=1):
    L = rat.native.lib()
    rc = L.rat_source_check(src.encode(), n, m)
    return rc, L.rat_last_error().decode()


def test_source_check_accepts_the_pendulum():
    assert check(PENDULUM) == (0, check(PENDULUM)[1])
    assert check(PENDULUM)[0] == 0


def test_source_check_reports_a_syntax_error_with_its_line():
    bad = PENDULUM.replace("xn[0] = x[0] + dt * x[1];", "xn[0] = x[0] + * dt x[1];")
    rc, log = check(bad)
    assert rc == 1 and "model.hip:4:" in log and "error" in log, log


def test_source_check_refuses_a_source_without_h():
    rc, log = check(PENDULUM.split("template <class T> __device__ T rat_user_h")[0])
    assert rc == 1 and "rat_user_h" in log, log


def test_source_check_refuses_sizes_beyond_the_tile():
    assert check(PENDULUM, n=13, m=1)[0] == 2
    assert check(PENDULUM, n=2, m=5)[0] == 2


def test_python_helper_raises_with_the_log():
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG"):
        rat.native.source_check(PENDULUM.replace("sin(", "sine("), 2, 1)


AD_TEST = r"""
#include "rat_ad.h"
#include <cstdio>
#include <cmath>
static double worst = 0.0;
static void cmp(double got, double want, const char *what) {
    const double e = std::fabs(got - want) / std::fmax(1.0, std::fabs(want));
    if (!(e <= worst)) worst = e;
    if (!(e < 1e-13)) std::printf("MISMATCH %s %.17g %.17g\n", what, got, want);
}
// g evaluated on a hyper-dual seeded in both directions (second derivative) and a dual (first derivative)
template <class F> static void one(const char *name, double a, F g, double v, double d1, double d2) {
    rat_hdual h = g(rat_hdual(a, 1.0, 1.0, 0.0));
    rat_dual d = g(rat_dual(a, 1.0));
    cmp(h.v, v, name); cmp(h.e1, d1, name); cmp(h.e2, d1, name); cmp(h.e12, d2, name);
    cmp(d.v, v, name); cmp(d.d, d1, name);
}
int main() {
    const double a = 0.7;
    one("sin", a, [](auto x) { return sin(x); }, std::sin(a), std::cos(a), -std::sin(a));
    one("cos", a, [](auto x) { return cos(x); }, std::cos(a), -std::sin(a), -std::cos(a));
    { const double t = std::tan(a); one("tan", a, [](auto x) { return tan(x); }, t, 1 + t * t, 2 * t * (1 + t * t)); }
    one("exp", a, [](auto x) { return exp(x); }, std::exp(a), std::exp(a), std::exp(a));
    one("log", a, [](auto x) { return log(x); }, std::log(a), 1 / a, -1 / (a * a));
    one("sqrt", a, [](auto x) { return sqrt(x); }, std::sqrt(a), 0.5 / std::sqrt(a), -0.25 / (a * std::sqrt(a)));
    one("pow", a, [](auto x) { return pow(x, 2.5); }, std::pow(a, 2.5), 2.5 * std::pow(a, 1.5), 3.75 * std::pow(a, 0.5));
    one("powTT", a, [](auto x) { return pow(x, x); }, std::pow(a, a), std::pow(a, a) * (std::log(a) + 1),
        std::pow(a, a) * ((std::log(a) + 1) * (std::log(a) + 1) + 1 / a));
    { const double t = std::tanh(a); one("tanh", a, [](auto x) { return tanh(x); }, t, 1 - t * t, -2 * t * (1 - t * t)); }
    one("atan", a, [](auto x) { return atan(x); }, std::atan(a), 1 / (1 + a * a), -2 * a / ((1 + a * a) * (1 + a * a)));
    // atan2(y, x) along y = x^2, x = -a (second quadrant, |y| < |x|) and y = 2, x = a (|y| > |x|)
    { auto g = [](auto x) { return atan2(x * x, -x); };            // d/dx atan2(x^2, -x) = -1 / (1 + x^2) ... closed form below
      const double v = std::atan2(a * a, -a), r = 1 + a * a; one("atan2", a, g, v, -1 / r, 2 * a / (r * r)); }
    { auto g = [](auto x) { return atan2(2.0, x); };
      const double r = 4 + a * a; one("atan2b", a, g, std::atan2(2.0, a), -2 / r, 4 * a / (r * r)); }
    one("fabs", -a, [](auto x) { return fabs(x); }, a, -1, 0);
    one("fmin", a, [](auto x) { return fmin(x * x, x); }, a * a, 2 * a, 2);
    one("fmax", a, [](auto x) { return fmax(x * x, 3.0 * x); }, 3 * a, 3, 0);
    // products and quotients
    one("prod", a, [](auto x) { return (x * x) * sin(x); }, a * a * std::sin(a), 2 * a * std::sin(a) + a * a * std::cos(a),
        2 * std::sin(a) + 4 * a * std::cos(a) - a * a * std::sin(a));
    one("quot", a, [](auto x) { return sin(x) / (1.0 + x * x); }, std::sin(a) / (1 + a * a),
        std::cos(a) / (1 + a * a) - 2 * a * std::sin(a) / ((1 + a * a) * (1 + a * a)),
        -std::sin(a) / (1 + a * a) - 4 * a * std::cos(a) / ((1 + a * a) * (1 + a * a))
            + std::sin(a) * (6 * a * a - 2) / ((1 + a * a) * (1 + a * a) * (1 + a * a)));
    one("rdiv", a, [](auto x) { return 2.0 / x - x / 4.0; }, 2 / a - a / 4, -2 / (a * a) - 0.25, 4 / (a * a * a));
    // a mixed second partial: f(x, y) = x^2 y^3 at (a, b), e1 on x, e2 on y
    { const double b = 1.3;
      rat_hdual x(a, 1.0, 0.0, 0.0), y(b, 0.0, 1.0, 0.0);
      rat_hdual f = (x * x) * (y * y * y);
      cmp(f.v, a * a * b * b * b, "mixed"); cmp(f.e1, 2 * a * b * b * b, "mixed"); cmp(f.e2, 3 * a * a * b * b, "mixed");
      cmp(f.e12, 6 * a * b * b, "mixed");
      rat_hdual g = y; g += x; g *= 2.0; g -= 1.0; g /= y;             // (2 (x + y) - 1) / y
      cmp(g.e12, -2.0 / (b * b), "compound"); }
    // comparisons look at the value
    if (!(rat_hdual(1.0, 5.0, 0, 0) < 2.0) || rat_dual(3.0, -1.0) < rat_dual(2.0, 9.0)) std::printf("MISMATCH compare\n");
    std::printf("worst %.3e\n", worst);
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("c++") is None, reason="no host C++ compiler")
def test_ad_header_on_the_host_matches_closed_forms(tmp_path):
    src = tmp_path / "ad_test.cpp"
    src.write_text(AD_TEST)
    exe = tmp_path / "ad_test"
    subprocess.run(["c++", "-std=c++17", "-O2", "-I", os.path.dirname(AD_H), str(src), "-o", str(exe)], check=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout
    assert "MISMATCH" not in out, out
    assert float(out.split("worst")[1]) < 1e-13, out
