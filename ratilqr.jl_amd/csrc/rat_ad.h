// rat_ad.h -- forward-mode automatic differentiation for runtime-compiled models (the device analogue of ForwardDiff, ileqg.jl:265-273).
//
//   rat_dual    a + b e,                      e^2 = 0              one directional derivative: a Jacobian column of f
//   rat_hdual   a + b e1 + c e2 + d e1 e2,    e1^2 = e2^2 = 0      value, the two first partials and the mixed second partial: the
//                                                                  Hessian entry (i, j) of c or h when e1 seeds z_i and e2 seeds z_j
//
// Every elementary function g is applied by the chain rule on its value g(a), slope g'(a) and (hyper-dual) curvature g''(a):
//   g(a + b e1 + c e2 + d e1 e2) = g(a) + g'(a) b e1 + g'(a) c e2 + (g'(a) d + g''(a) b c) e1 e2
// Comparisons, fmin / fmax and fabs's branch look at the value only.  No fast-math: NaN in a value is how a model signals a domain
// error, and it has to survive.
//
// At singular points (tests/ad_edge_cases.py, profiles/ad_edges.md) the derivatives are what plain IEEE evaluation of the chain rule gives:
// sqrt at 0 has slope Inf and curvature NaN, log and 1 / x at 0 have infinite partials, and a non-finite slope times the zero seed of
// another variable is NaN in that variable's partial.  One exception: pow(T, double) returns exactly 0 for a partial whose coefficient
// (p, or p (p - 1)) is 0.  pow with a dual exponent differentiates through exp(b log a), so its partials are NaN for a base <= 0 even
// where the value is fine.  fabs has slope +1 at +-0; fmin and fmax return the first argument at a tie and the other one beside a NaN.
// Division differs between the types: rat_dual uses (a' - q b') / b, rat_hdual multiplies by 1 / b, whose curvature 2 / b^3 leaves the
// double range for |b| outside about [1e-102, 1e102]; the two agree for denominators in [1e-100, 1e100] and need not beyond.
//
// The header compiles as device code under hiprtc (the JIT of the source-model family) and as plain host C++ (its unit test).
#pragma once

#if defined(__HIPCC_RTC__) || defined(__HIP__)
#define RAT_AD_FN __device__ __host__ inline
#else
#include <cmath>
#define RAT_AD_FN inline
using std::sin; using std::cos; using std::tan; using std::exp; using std::log; using std::sqrt; using std::pow; using std::tanh;
using std::atan; using std::atan2; using std::fabs; using std::fmin; using std::fmax;
#endif

struct rat_dual {
    double v, d;
    RAT_AD_FN rat_dual() : v(0.0), d(0.0) {}
    RAT_AD_FN rat_dual(double a) : v(a), d(0.0) {}
    RAT_AD_FN rat_dual(double a, double b) : v(a), d(b) {}
};
struct rat_hdual {
    double v, e1, e2, e12;
    RAT_AD_FN rat_hdual() : v(0.0), e1(0.0), e2(0.0), e12(0.0) {}
    RAT_AD_FN rat_hdual(double a) : v(a), e1(0.0), e2(0.0), e12(0.0) {}
    RAT_AD_FN rat_hdual(double a, double b, double c, double d) : v(a), e1(b), e2(c), e12(d) {}
};

RAT_AD_FN double rat_value(double a) { return a; }
RAT_AD_FN double rat_value(const rat_dual &a) { return a.v; }
RAT_AD_FN double rat_value(const rat_hdual &a) { return a.v; }

// chain rule with value g, slope g1 and curvature g2 at a's value
RAT_AD_FN rat_dual rat_chain(const rat_dual &a, double g, double g1, double) { return rat_dual(g, g1 * a.d); }
RAT_AD_FN rat_hdual rat_chain(const rat_hdual &a, double g, double g1, double g2) {
    return rat_hdual(g, g1 * a.e1, g1 * a.e2, g1 * a.e12 + g2 * (a.e1 * a.e2));
}

// ---- arithmetic --------------------------------------------------------------------------------------------------------------------
RAT_AD_FN rat_dual operator+(const rat_dual &a, const rat_dual &b) { return rat_dual(a.v + b.v, a.d + b.d); }
RAT_AD_FN rat_dual operator-(const rat_dual &a, const rat_dual &b) { return rat_dual(a.v - b.v, a.d - b.d); }
RAT_AD_FN rat_dual operator-(const rat_dual &a) { return rat_dual(-a.v, -a.d); }
RAT_AD_FN rat_dual operator+(const rat_dual &a) { return a; }
RAT_AD_FN rat_dual operator*(const rat_dual &a, const rat_dual &b) { return rat_dual(a.v * b.v, a.d * b.v + a.v * b.d); }
RAT_AD_FN rat_dual operator/(const rat_dual &a, const rat_dual &b) {
    const double q = a.v / b.v;
    return rat_dual(q, (a.d - q * b.d) / b.v);
}
RAT_AD_FN rat_dual operator+(const rat_dual &a, double b) { return rat_dual(a.v + b, a.d); }
RAT_AD_FN rat_dual operator+(double a, const rat_dual &b) { return rat_dual(a + b.v, b.d); }
RAT_AD_FN rat_dual operator-(const rat_dual &a, double b) { return rat_dual(a.v - b, a.d); }
RAT_AD_FN rat_dual operator-(double a, const rat_dual &b) { return rat_dual(a - b.v, -b.d); }
RAT_AD_FN rat_dual operator*(const rat_dual &a, double b) { return rat_dual(a.v * b, a.d * b); }
RAT_AD_FN rat_dual operator*(double a, const rat_dual &b) { return rat_dual(a * b.v, a * b.d); }
RAT_AD_FN rat_dual operator/(const rat_dual &a, double b) { return rat_dual(a.v / b, a.d / b); }
RAT_AD_FN rat_dual operator/(double a, const rat_dual &b) { return rat_dual(a) / b; }

RAT_AD_FN rat_hdual operator+(const rat_hdual &a, const rat_hdual &b) { return rat_hdual(a.v + b.v, a.e1 + b.e1, a.e2 + b.e2, a.e12 + b.e12); }
RAT_AD_FN rat_hdual operator-(const rat_hdual &a, const rat_hdual &b) { return rat_hdual(a.v - b.v, a.e1 - b.e1, a.e2 - b.e2, a.e12 - b.e12); }
RAT_AD_FN rat_hdual operator-(const rat_hdual &a) { return rat_hdual(-a.v, -a.e1, -a.e2, -a.e12); }
RAT_AD_FN rat_hdual operator+(const rat_hdual &a) { return a; }
RAT_AD_FN rat_hdual operator*(const rat_hdual &a, const rat_hdual &b) {
    return rat_hdual(a.v * b.v, a.e1 * b.v + a.v * b.e1, a.e2 * b.v + a.v * b.e2, ((a.e12 * b.v + a.v * b.e12) + (a.e1 * b.e2 + a.e2 * b.e1)));
}
RAT_AD_FN rat_hdual operator/(const rat_hdual &a, const rat_hdual &b) {      // a * (1 / b)
    const double r = 1.0 / b.v;
    return a * rat_chain(b, r, -r * r, 2.0 * r * r * r);
}
RAT_AD_FN rat_hdual operator+(const rat_hdual &a, double b) { return rat_hdual(a.v + b, a.e1, a.e2, a.e12); }
RAT_AD_FN rat_hdual operator+(double a, const rat_hdual &b) { return rat_hdual(a + b.v, b.e1, b.e2, b.e12); }
RAT_AD_FN rat_hdual operator-(const rat_hdual &a, double b) { return rat_hdual(a.v - b, a.e1, a.e2, a.e12); }
RAT_AD_FN rat_hdual operator-(double a, const rat_hdual &b) { return rat_hdual(a - b.v, -b.e1, -b.e2, -b.e12); }
RAT_AD_FN rat_hdual operator*(const rat_hdual &a, double b) { return rat_hdual(a.v * b, a.e1 * b, a.e2 * b, a.e12 * b); }
RAT_AD_FN rat_hdual operator*(double a, const rat_hdual &b) { return rat_hdual(a * b.v, a * b.e1, a * b.e2, a * b.e12); }
RAT_AD_FN rat_hdual operator/(const rat_hdual &a, double b) { return rat_hdual(a.v / b, a.e1 / b, a.e2 / b, a.e12 / b); }
RAT_AD_FN rat_hdual operator/(double a, const rat_hdual &b) { return rat_hdual(a) / b; }

#define RAT_AD_COMPOUND(T)                                                                       \
    RAT_AD_FN T &operator+=(T &a, const T &b) { a = a + b; return a; }                            \
    RAT_AD_FN T &operator-=(T &a, const T &b) { a = a - b; return a; }                            \
    RAT_AD_FN T &operator*=(T &a, const T &b) { a = a * b; return a; }                            \
    RAT_AD_FN T &operator/=(T &a, const T &b) { a = a / b; return a; }                            \
    RAT_AD_FN T &operator+=(T &a, double b) { a = a + b; return a; }                              \
    RAT_AD_FN T &operator-=(T &a, double b) { a = a - b; return a; }                              \
    RAT_AD_FN T &operator*=(T &a, double b) { a = a * b; return a; }                              \
    RAT_AD_FN T &operator/=(T &a, double b) { a = a / b; return a; }                              \
    RAT_AD_FN bool operator<(const T &a, const T &b) { return a.v < b.v; }                        \
    RAT_AD_FN bool operator>(const T &a, const T &b) { return a.v > b.v; }                        \
    RAT_AD_FN bool operator<=(const T &a, const T &b) { return a.v <= b.v; }                      \
    RAT_AD_FN bool operator>=(const T &a, const T &b) { return a.v >= b.v; }                      \
    RAT_AD_FN bool operator==(const T &a, const T &b) { return a.v == b.v; }                      \
    RAT_AD_FN bool operator!=(const T &a, const T &b) { return a.v != b.v; }                      \
    RAT_AD_FN bool operator<(const T &a, double b) { return a.v < b; }                            \
    RAT_AD_FN bool operator>(const T &a, double b) { return a.v > b; }                            \
    RAT_AD_FN bool operator<=(const T &a, double b) { return a.v <= b; }                          \
    RAT_AD_FN bool operator>=(const T &a, double b) { return a.v >= b; }                          \
    RAT_AD_FN bool operator<(double a, const T &b) { return a < b.v; }                            \
    RAT_AD_FN bool operator>(double a, const T &b) { return a > b.v; }                            \
    RAT_AD_FN bool operator<=(double a, const T &b) { return a <= b.v; }                          \
    RAT_AD_FN bool operator>=(double a, const T &b) { return a >= b.v; }                          \
    /* elementary functions: value, slope, curvature */                                           \
    RAT_AD_FN T sin(const T &a) { const double s = sin(a.v), c = cos(a.v); return rat_chain(a, s, c, -s); }      \
    RAT_AD_FN T cos(const T &a) { const double s = sin(a.v), c = cos(a.v); return rat_chain(a, c, -s, -c); }     \
    RAT_AD_FN T tan(const T &a) { const double t = tan(a.v), s = 1.0 + t * t; return rat_chain(a, t, s, 2.0 * t * s); } \
    RAT_AD_FN T exp(const T &a) { const double e = exp(a.v); return rat_chain(a, e, e, e); }                     \
    RAT_AD_FN T log(const T &a) { const double r = 1.0 / a.v; return rat_chain(a, log(a.v), r, -r * r); }         \
    RAT_AD_FN T sqrt(const T &a) { const double s = sqrt(a.v), d1 = 0.5 / s; return rat_chain(a, s, d1, -0.5 * d1 / a.v); } \
    RAT_AD_FN T tanh(const T &a) { const double t = tanh(a.v), s = 1.0 - t * t; return rat_chain(a, t, s, -2.0 * t * s); } \
    RAT_AD_FN T atan(const T &a) { const double r = 1.0 / (1.0 + a.v * a.v); return rat_chain(a, atan(a.v), r, -2.0 * a.v * r * r); } \
    RAT_AD_FN T pow(const T &a, double p) {      /* a zero coefficient is a zero partial: pow(x, 1.0) and pow(x, 0.0) at x = 0 */ \
        const double c1 = p, c2 = p * (p - 1.0);                                                  \
        return rat_chain(a, pow(a.v, p), c1 == 0.0 ? 0.0 : c1 * pow(a.v, p - 1.0), c2 == 0.0 ? 0.0 : c2 * pow(a.v, p - 2.0)); } \
    RAT_AD_FN T pow(const T &a, const T &b) {                                                     \
        T r = exp(b * log(a)); r.v = pow(a.v, b.v); return r; }                                   \
    RAT_AD_FN T pow(double a, const T &b) { T r = exp(b * log(a)); r.v = pow(a, b.v); return r; } \
    RAT_AD_FN T fabs(const T &a) { return a.v < 0.0 ? -a : a; }                                  \
    RAT_AD_FN T fmin(const T &a, const T &b) { return (b.v < a.v || a.v != a.v) ? b : a; }        \
    RAT_AD_FN T fmax(const T &a, const T &b) { return (b.v > a.v || a.v != a.v) ? b : a; }        \
    RAT_AD_FN T fmin(const T &a, double b) { return fmin(a, T(b)); }                              \
    RAT_AD_FN T fmin(double a, const T &b) { return fmin(T(a), b); }                              \
    RAT_AD_FN T fmax(const T &a, double b) { return fmax(a, T(b)); }                              \
    RAT_AD_FN T fmax(double a, const T &b) { return fmax(T(a), b); }                              \
    /* atan2: the derivatives of atan(y / x) (or of -atan(x / y) where |y| > |x|), the value of atan2 */           \
    RAT_AD_FN T atan2(const T &y, const T &x) {                                                   \
        T r = (fabs(x.v) >= fabs(y.v)) ? atan(y / x) : -atan(x / y);                              \
        r.v = atan2(y.v, x.v); return r; }                                                        \
    RAT_AD_FN T atan2(const T &y, double x) { return atan2(y, T(x)); }                            \
    RAT_AD_FN T atan2(double y, const T &x) { return atan2(T(y), x); }

RAT_AD_COMPOUND(rat_dual)
RAT_AD_COMPOUND(rat_hdual)
#undef RAT_AD_COMPOUND
