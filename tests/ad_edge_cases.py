"""The case table of the AD header's edge tests (tests/test_cpu_ad_edges.py on the host, tests/test_gpu_ad_edges.py on the device).

A case is a function G of the three scalars (x[0], x[1], u[0]) -- written X, Y, U below -- as device code (`body`, the statements of a
function returning T) and, for regular points, as an mpmath function (`ref`) written without any reference to the header's chain rule.
A point is (X, Y, U) with a kind:

  regular    every partial up to second order exists and is finite.  Value, gradient and Hessian are compared with mpmath.diff at 1100
             bits, rounded once to double, by |got - want| / max(1, |want|): 1e-13 on the host, 1e-12 on the device.  `edge` marks the
             regular points that sit next to a domain edge, a kink, a tie, a branch switch or at an extreme scale.
  singular   the table states the class of every output: a finite number (compared at the same bound), inf, -inf or nan; `ref` where a
             finite output is compared with mpmath although the point is ill-conditioned (no longer a regular point by the rule of
             test_regular_points_are_finite_and_well_conditioned); `fin` where only finiteness is asserted and the number is reported.

The rule behind the classes of the singular points:
  * the value is what IEEE libm gives;
  * a partial of pow(T, double) whose chain-rule coefficient (p for the slope, p (p - 1) for the curvature) is exactly zero is zero;
  * every other partial is what plain IEEE evaluation of the header's chain rule gives today, pinned: g(a)' * seed with Inf * 0 = NaN,
    so a non-finite slope makes the partials of the *other* variables NaN too;
  * the first partials of rat_dual agree in class with those of rat_hdual, except where `dual` states otherwise (x / x below 1e-100, where
    rat_hdual's a * (1 / b) overflows in r * r and rat_dual's (a' - q b') / b does not: documented, not asserted to agree).

An expectation is "v ; G_X G_Y G_U ; H_XX H_XY H_XU H_YY H_YU H_UU ; unused", `unused` being the first partial with respect to a variable the
function does not read (every seed zero): the columns of the other states and controls in [f_x | f_u]."""
import math
import operator

import mpmath as mp
import numpy as np

PREC = 1100                                                               # bits at which mpmath.diff is asked for its result
HOST_BOUND, DEVICE_BOUND = 1e-13, 1e-12
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))                  # the (i <= j) pairs of z = (x_0, x_1, u_0), row by row
SAFE = (0.7, 1.3, -0.4)                                                   # inside every domain the table uses a safe point for
NAN = float("nan")


def up(a):
    return float(np.nextafter(a, np.inf))


def dn(a):
    return float(np.nextafter(a, -np.inf))


class Point:
    def __init__(self, z, kind="regular", edge=False, expect=None, dual=None, safe=SAFE):
        self.z, self.kind, self.edge, self.expect, self.dual, self.safe = tuple(float(a) for a in z), kind, edge, expect, dual, safe
        assert kind in ("regular", "singular") and (kind == "singular") == (expect is not None)


def reg(*z):
    return Point(z)


def edge(*z):
    return Point(z, edge=True)


def sing(z, expect, dual=None, safe=SAFE):
    return Point(z, "singular", expect=expect, dual=dual, safe=safe)


class Case:
    def __init__(self, name, fams, body, ref, points, fn=None):
        self.name, self.fams, self.ref, self.points = name, tuple(fams), ref, tuple(points)
        self.fn = fn or name.split("@")[0]                                # the function the error report files the case under
        self.body = body if "return" in body else f"return {body};"

    def device_body(self):
        return self.body.replace("X", "x[0]").replace("Y", "x[1]").replace("U", "u[0]")


YU = 1.75                                                                  # Y + U at the points of the one-argument functions
CASES = []


def case(*a, **k):
    CASES.append(Case(*a, **k))


def one(name, fam, expr, ref, xs, edges, **k):
    """g(X) * (Y + U): value, slope and curvature of g all show, and the mixed partials are live."""
    case(name, [fam], f"({expr}) * (Y + U)", lambda X, Y, U: ref(X) * (Y + U),
         [reg(a, 1.25, 0.5) for a in xs] + [edge(a, 1.25, 0.5) for a in edges], **k)


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------------
case("add", ["operator+:TT", "operator+:Td", "operator+:dT"], "(X + Y) + (X + 2.5) + (1.5 + U)", lambda X, Y, U: 2 * X + Y + U + 4,
     [reg(0.7, 1.3, -0.4), edge(1e100, -3e99, 1e-100)])
case("sub", ["operator-:TT", "operator-:Td", "operator-:dT", "operator*:TT"], "(X - Y) * (X - 2.5) * (1.5 - U)",
     lambda X, Y, U: (X - Y) * (X - 2.5) * (1.5 - U), [reg(0.7, 1.3, -0.4), edge(1e50, 3e49, -1e-50)])
case("mul", ["operator*:TT", "operator*:Td", "operator*:dT"], "(X * Y) * (U * 3.0) * (0.25 * X)", lambda X, Y, U: 0.75 * X * X * Y * U,
     [reg(0.7, 1.3, -0.4), edge(1e50, 1e-50, 3.0)])
case("div", ["operator/:TT", "operator/:Td", "operator/:dT"], "(X / Y) + (U / 4.0) + (2.0 / X)", lambda X, Y, U: X / Y + U / 4 + 2 / X,
     [reg(0.7, 1.3, -0.4), edge(1e-100, 1e100, 7.0), edge(3.0, 1e-100, 7.0), edge(-1e100, -3.0, 7.0)])
case("quot_mixed", ["operator/:TT", "operator*:TT"], "(X * U) / (Y * Y + X)", lambda X, Y, U: X * U / (Y * Y + X),
     [reg(0.7, 1.3, -0.4), edge(1e-8, 1e-3, 1e8), edge(3e99, 1e50, -2.0)])
case("neg", ["operator-:T", "operator+:T"], "-(X * Y) + (+U)", lambda X, Y, U: U - X * Y, [reg(0.7, 1.3, -0.4), edge(1e100, -1e100, 1e-100)])
case("compound", ["operator+=:TT", "operator-=:TT", "operator*=:TT", "operator/=:TT", "operator+=:Td", "operator-=:Td", "operator*=:Td",
                  "operator/=:Td"],
     "T a = X; a += Y; a -= U; a *= Y; a /= X; a += 1.5; a -= 0.25; a *= 3.0; a /= 7.0; return a;",
     lambda X, Y, U: ((X + Y - U) * Y / X + 1.25) * 3 / 7, [reg(0.7, 1.3, -0.4), edge(1e8, 1e-8, -3.0), edge(-1e-8, 1e8, 3.0)])
case("compound_aliased", ["operator+=:TT", "operator-=:TT", "operator*=:TT", "operator/=:TT"],
     "T a = X; a *= a; a += a; T b = Y * U; b /= b; T c = X; c -= c; return a * b + c + Y;", lambda X, Y, U: 2 * X * X + Y,
     [reg(0.7, 1.3, -0.4), edge(1e50, 1e-50, 1e50)])
case("self_quot", ["operator/:TT"], "(X / X) * (Y + U)", lambda X, Y, U: Y + U, [reg(0.7, 1.25, 0.5), reg(-3.0, 1.25, 0.5)])

_CMP = {"<": operator.lt, ">": operator.gt, "<=": operator.le, ">=": operator.ge, "==": operator.eq, "!=": operator.ne}


def _cmp_case(op, form):
    f = _CMP[op]
    cond, test, pts = {
        "TT": ("X OP Y", lambda X, Y: f(X, Y), [reg(0.7, 1.3, -0.4), edge(1.3 - 1e-9, 1.3, -0.4), edge(1.3 + 1e-9, 1.3, -0.4)]),
        "Td": ("X OP 1.0", lambda X, Y: f(X, 1.0), [reg(0.7, 1.3, -0.4), edge(1.0 - 1e-9, 1.3, -0.4), edge(1.0 + 1e-9, 1.3, -0.4)]),
        "dT": ("1.0 OP X", lambda X, Y: f(1.0, X), [reg(0.7, 1.3, -0.4), edge(1.0 - 1e-9, 1.3, -0.4), edge(1.0 + 1e-9, 1.3, -0.4)])}[form]
    if form == "TT":                                                      # the tie itself: the value decides, the branch taken is X * Y + U or X + Y * U
        tie = "2.19 ; 1.3 1.3 1 ; 0 1 0 0 0 0 ; 0" if f(1.0, 1.0) else "1.95 ; 1 0.5 1.3 ; 0 0 0 0 1 0 ; 0"
        pts = pts + [sing((1.3, 1.3, 0.5), tie)]
    case(f"cmp{op}{form}", [f"operator{op}:{form}"], f"return ({cond.replace('OP', op)}) ? X * Y + U : X + Y * U;",
         lambda X, Y, U: X * Y + U if test(X, Y) else X + Y * U, pts, fn="compare")


for _op in ("<", ">", "<=", ">="):
    for _form in ("TT", "Td", "dT"):
        _cmp_case(_op, _form)
_cmp_case("==", "TT")
_cmp_case("!=", "TT")

# ---- elementary functions at regular points -------------------------------------------------------------------------------------------------
HALF_PI = math.pi / 2
one("sin", "sin:T", "sin(X)", mp.sin, [0.7], [1e-8, math.pi, -30.0])
one("cos", "cos:T", "cos(X)", mp.cos, [0.7], [1e-8, HALF_PI, -30.0])
one("tan", "tan:T", "tan(X)", mp.tan, [0.7], [HALF_PI - 0.125, -(HALF_PI - 0.125)])   # pi/2 - 1e-6 is ill-conditioned: with the singular points
one("exp", "exp:T", "exp(X)", mp.exp, [0.7], [30.0, -30.0])
one("log", "log:T", "log(X)", mp.log, [0.7], [1e-8, 1e8])
one("sqrt", "sqrt:T", "sqrt(X)", mp.sqrt, [0.7], [1e-8, 1e8])
one("tanh", "tanh:T", "tanh(X)", mp.tanh, [0.7], [5.0, -5.0])
one("atan", "atan:T", "atan(X)", mp.atan, [0.7], [1e8, -1e-8])
one("recip", "operator/:dT", "1.0 / X", lambda X: 1 / X, [0.7], [1e-8, 1e8])
one("pow2.5", "pow:Td", "pow(X, 2.5)", lambda X: X ** mp.mpf(2.5), [0.7], [1e-8, 1e8], fn="pow_Td")
for _p in (-2.5, -1.0, 0.0, 0.5, 1.0, 2.0, 3.0):
    _int = _p == int(_p)
    # an integer exponent in mpmath keeps a negative base real; at 0 only the exponents whose three coefficients stay finite
    one(f"pow{_p}", "pow:Td", f"pow(X, {_p})", (lambda p: lambda X: X ** (int(p) if p == int(p) else mp.mpf(p)))(_p), [1.7],
        ([-1.5] if _int else []) + ([0.0] if _p in (2.0, 3.0) else []), fn="pow_Td")
case("pow_TT", ["pow:TT"], "pow(X, Y) * U", lambda X, Y, U: X ** Y * U,
     [reg(1.7, 2.3, 0.5), edge(1e-8, 0.5, 0.5), edge(1e8, -1.5, 0.5), edge(1.0 + 1e-9, 3.0, 0.5)])
one("pow_dT", "pow:dT", "pow(1.7, X)", lambda X: mp.mpf(1.7) ** X, [0.7], [30.0, -30.0])
one("fabs", "fabs:T", "fabs(X)", abs, [0.7, -0.7], [1e-9, -1e-9])
for _nm, _f in (("fmin", min), ("fmax", max)):
    one(f"{_nm}_TT", f"{_nm}:TT", f"{_nm}(X * X, 3.0 * X)", (lambda f: lambda X: f(X * X, 3 * X))(_f), [0.7], [3.0 - 1e-9, 3.0 + 1e-9, 1e-9, -1e-9],
        fn=_nm)
    one(f"{_nm}_Td", f"{_nm}:Td", f"{_nm}(X * X, 4.0)", (lambda f: lambda X: f(X * X, 4))(_f), [0.7], [2.0 - 1e-9, 2.0 + 1e-9], fn=_nm)
    one(f"{_nm}_dT", f"{_nm}:dT", f"{_nm}(4.0, X * X)", (lambda f: lambda X: f(4, X * X))(_f), [0.7], [2.0 - 1e-9, 2.0 + 1e-9], fn=_nm)

# atan2(y, x) with both arguments active.  Quadrants (both branches of the header), the four half-axes, one ulp either side of |y| = |x|
# on the four diagonals, and the two extreme scales.
_D = 1.3
case("atan2_TT", ["atan2:TT"], "atan2(Y, X) * U", lambda X, Y, U: mp.atan2(Y, X) * U,
     [reg(1.3, 0.4, 0.5), reg(-0.4, 1.3, 0.5), reg(-1.3, -0.4, 0.5), reg(0.4, -1.3, 0.5), reg(-1.3, 0.4, 0.5), reg(0.4, 1.3, 0.5)]
     + [edge(2.0, 0.0, 0.5), edge(0.0, 2.0, 0.5), edge(0.0, -2.0, 0.5)]
     # the negative x axis is the cut: one ulp below y = 0 the value is -pi, so the point is not regular by the conditioning rule; at
     # y = +0 every output is still the limit from above
     + [sing((-2.0, 0.0, 0.5), "ref ; ref ref ref ; ref ref ref ref ref ref ; 0")]
     + [edge(sx * _D, sy * y, 0.5) for sx in (1, -1) for sy in (1, -1) for y in (dn(_D), up(_D))]
     + [edge(sx * _D, sy * _D, 0.5) for sx in (1, -1) for sy in (1, -1)]
     + [edge(1e100, 3e99, 0.5), edge(-3e-100, 1e-100, 0.5)], fn="atan2")
one("atan2_Td", "atan2:Td", "atan2(X, 2.0)", lambda X: mp.atan2(X, 2), [0.7, -5.0], [dn(2.0), up(2.0), -dn(2.0), -up(2.0), 0.0], fn="atan2")
one("atan2_dT", "atan2:dT", "atan2(2.0, X)", lambda X: mp.atan2(2, X), [0.7, -5.0], [dn(2.0), up(2.0), -dn(2.0), -up(2.0), 0.0], fn="atan2")

# ---- singular points: G(X) alone, so the classes read off the chain rule directly --------------------------------------------------------------
S = lambda a: (a, 1.3, -0.4)
case("pow1@0", ["pow:Td"], "pow(X, 1.0)", None, [sing(S(0.0), "0 ; 1 0 0 ; 0 0 0 0 0 0 ; 0")], fn="pow_Td")
case("pow0@0", ["pow:Td"], "pow(X, 0.0)", None, [sing(S(0.0), "1 ; 0 0 0 ; 0 0 0 0 0 0 ; 0")], fn="pow_Td")
case("powT2@", ["pow:TT"], "pow(X, T(2.0))", None, [sing(S(-1.5), "2.25 ; nan nan nan ; nan nan nan nan nan nan ; nan"),
                                                     sing(S(0.0), "0 ; nan nan nan ; nan nan nan nan nan nan ; nan")], fn="pow_TT")
_NANS = "nan nan nan ; nan nan nan nan nan nan ; nan"


def _fin(v, d1, d2):
    """G(X) with finite slope and curvature: nothing reaches the other variables."""
    return f"{v} ; {d1} 0 0 ; {d2} 0 0 0 0 0 ; 0"


def _bad(v, d1):
    """G(X) with a non-finite slope or curvature: times the zero seeds of the other variables it is NaN everywhere else."""
    return f"{v} ; {d1} nan nan ; {_NANS.split(' ; ', 1)[1]}"


case("pow0T@", ["pow:dT"], "pow(0.0, X)", None, [sing(S(1.5), "0 ; " + _NANS)], fn="pow_dT")            # exp(b log a): log(0), log(-2)
case("powm2T@", ["pow:dT"], "pow(-2.0, X)", None, [sing(S(2.0), "4 ; " + _NANS, safe=(3.0, 1.3, -0.4))], fn="pow_dT")   # safe: a finite value
# x / x.  For denominators in [1e-100, 1e100] the two types agree in the value and in the first partial; rat_hdual's curvature at 1e-100 is
# the rounding residue of terms near 1e200 (pinned as finite, reported).  Below 1e-102 r * r overflows in rat_hdual alone, and at 0 the
# quotient is NaN: there, and for 1 / x at 0, the first partials of the two types differ and `dual` states rat_dual's.
case("xoverx@", ["operator/:TT"], "X / X", None,
     [sing(S(1e-100), "1 ; 0 0 0 ; fin 0 0 0 0 0 ; 0"), sing(S(1e100), _fin(1, 0, 0)),
      sing(S(1e-200), _bad(1, "-inf")[:-3] + "0", dual="1 ; 0 0 0 ; 0 0 0 0 0 0 ; 0"), sing(S(0.0), "nan ; " + _NANS)], fn="self_quot")
case("aliased_quot@", ["operator/=:TT"], "T a = X; a /= a; return a;", None, [sing(S(0.0), "nan ; " + _NANS)], fn="self_quot")
case("recip@", ["operator/:dT"], "1.0 / X", None, [sing(S(0.0), "inf ; " + _NANS, dual="inf ; -inf nan nan ; 0 0 0 0 0 0 ; nan")], fn="recip")
case("sqrt@", ["sqrt:T"], "sqrt(X)", None, [sing(S(0.0), _bad(0, "inf")), sing(S(-1.0), "nan ; " + _NANS)], fn="sqrt")
case("sqrtsq@", ["sqrt:T", "operator*:TT"], "sqrt(X * X)", None, [sing(S(0.0), "0 ; " + _NANS)], fn="sqrt")      # inf * 0
case("fabs@", ["fabs:T"], "fabs(X)", None, [sing(S(0.0), _fin(0, 1, 0)), sing(S(-0.0), _fin(0, 1, 0))], fn="fabs")   # -0 stays -0, slope +1
# saturated tails: 1 - t * t cancels to 0 where the true slope is 1.7e-17 (absolute error below the bound; the relative one is reported)
case("tanh@", ["tanh:T"], "tanh(X)", lambda X, Y, U: mp.tanh(X), [sing(S(20.0), _fin(1, 0, 0)), sing(S(-20.0), _fin(-1, 0, 0))], fn="tanh")
case("exp@", ["exp:T"], "exp(X)", None, [sing(S(710.0), _bad("inf", "inf")), sing(S(-750.0), _fin(0, 0, 0))], fn="exp")
# log(-1) is NaN in the value alone: 1 / a and -1 / a^2 are finite
case("log@", ["log:T"], "log(X)", None, [sing(S(0.0), _bad("-inf", "inf")), sing(S(-1.0), _fin("nan", -1, -1))], fn="log")
# one ulp of pi/2 - 1e-6 moves tan by 2e-10 of itself: not a regular point, yet libm's tan of that double is exact to an ulp
case("tan@", ["tan:T"], "tan(X)", lambda X, Y, U: mp.tan(X), [sing(S(HALF_PI - 1e-6), _fin("ref", "ref", "ref"))], fn="tan")
# arguments far beyond the period: the value of that very double
case("sin@", ["sin:T"], "sin(X)", lambda X, Y, U: mp.sin(X), [sing(S(1e300), _fin("ref", "ref", "ref"))], fn="sin")
case("cos@", ["cos:T"], "cos(X)", lambda X, Y, U: mp.cos(X), [sing(S(1e300), _fin("ref", "ref", "ref"))], fn="cos")
case("atan@", ["atan:T"], "atan(X)", None, [sing(S(1e200), _fin(HALF_PI, 0, 0))], fn="atan")              # 1 / (1 + inf) = 0
case("atan2@00", ["atan2:TT"], "atan2(Y, X)", None, [sing((0.0, 0.0, -0.4), "0 ; " + _NANS)], fn="atan2")  # atan(0 / 0)
case("atan2_Td@0", ["atan2:Td"], "atan2(X, 0.0)", None, [sing(S(0.0), "0 ; " + _NANS)], fn="atan2")
case("atan2_dT@0", ["atan2:dT"], "atan2(0.0, X)", None, [sing(S(0.0), "0 ; " + _NANS)], fn="atan2")
for _nm in ("fmin", "fmax"):
    # a tie with different slopes: the first argument wins.  A NaN operand on either side: the other operand wins
    case(f"{_nm}_tie@", [f"{_nm}:TT"], f"{_nm}(X * X, 3.0 * X)", None, [sing(S(3.0), _fin(9, 6, 2))], fn=_nm)
    case(f"{_nm}_tie_swapped@", [f"{_nm}:TT"], f"{_nm}(3.0 * X, X * X)", None, [sing(S(3.0), _fin(9, 3, 0))], fn=_nm)
    case(f"{_nm}_Td_nan@", [f"{_nm}:Td"], f'{_nm}(X, __builtin_nan(""))', None, [sing(S(0.7), _fin(0.7, 1, 0))], fn=_nm)
    case(f"{_nm}_dT_nan@", [f"{_nm}:dT"], f'{_nm}(__builtin_nan(""), X)', None, [sing(S(0.7), _fin(0.7, 1, 0))], fn=_nm)
    case(f"{_nm}_TT_nan_right@", [f"{_nm}:TT"], f"{_nm}(X * X, log(Y))", None, [sing((0.7, -1.0, -0.4), _fin(0.7 * 0.7, 1.4, 2))], fn=_nm)
    case(f"{_nm}_TT_nan_left@", [f"{_nm}:TT"], f"{_nm}(log(Y), X * X)", None, [sing((0.7, -1.0, -0.4), _fin(0.7 * 0.7, 1.4, 2))], fn=_nm)

ITEMS = tuple((c, p) for c in CASES for p in c.points)                    # what the tests run: one entry per (case, point)


# ---- expectations ------------------------------------------------------------------------------------------------------------------------
def parse_expect(text):
    """"v ; g ; H ; unused" -> dict(v=token, g=[3 tokens], H={(i, j): token}, unused=token); a token is a float or "ref" / "fin"."""
    def tok(s):
        return s if s in ("ref", "fin") else float(s)
    parts = [[tok(s) for s in part.split()] for part in text.split(";")]
    assert [len(p) for p in parts] == [1, 3, 6, 1], text
    return dict(v=parts[0][0], g=parts[1], H=dict(zip(PAIRS, parts[2])), unused=parts[3][0])


def same_class(a, b):
    """Two doubles of one class: both NaN, the same infinity, or both finite."""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return True


def err(got, want):
    """The project's metric, |got - want| / max(1, |want|); inf for a non-finite `got`."""
    got, want = float(got), float(want)
    return abs(got - want) / max(1.0, abs(want)) if math.isfinite(got) else math.inf


def check_token(got, token, want_ref, bound):
    """None if `got` meets the table's token, else a message."""
    if token == "fin":
        return None if math.isfinite(got) else f"{got} is not finite"
    want = want_ref if token == "ref" else token
    if not same_class(got, want):
        return f"{got} where the table says {want}"
    if math.isfinite(want) and not err(got, want) <= bound:
        return f"{got!r} against {want!r}: {err(got, want):.2e}"
    return None


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
def reference(ref, z):
    """Value, gradient (3) and Hessian (3 x 3) of the mpmath function `ref` at the doubles z, each rounded once to double.

    mpmath.diff at PREC bits with one-sided steps, so a step never crosses a kink, a tie or atan2's cut next to the point.  The step is
    2^-(PREC + 10), about 1e-334: small beside a point at 1e-100, and mpmath works at twice PREC and more while it differences, so a partial
    of 1e-100 beside a value of 1e100 keeps 60 digits and more."""
    with mp.workprec(PREC):
        zs = [mp.mpf(a) for a in z]
        d = lambda o: mp.diff(ref, zs, o, direction=1)
        unit = lambda *idx: tuple(sum(1 for k in idx if k == q) for q in range(3))
        v = float(ref(*zs))
        g = [float(d(unit(i))) for i in range(3)]
        H = np.zeros((3, 3))
        for i, j in PAIRS:
            H[i, j] = H[j, i] = float(d(unit(i, j)))
    return v, g, H


_REF = {}


def item_reference(k):
    """The reference of item k, computed once per process; None where the case has no mpmath form (singular points pinned by class)."""
    if k not in _REF:
        c, p = ITEMS[k]
        _REF[k] = None if c.ref is None else reference(c.ref, p.z)
    return _REF[k]


def expected(k):
    """dict(v, g, H, unused) of tokens for item k: the reference's doubles at a regular point, the table's classes at a singular one."""
    c, p = ITEMS[k]
    if p.kind == "regular":
        v, g, H = item_reference(k)
        return dict(v=v, g=list(g), H={ij: H[ij] for ij in PAIRS}, unused=0.0)
    return parse_expect(p.expect)


def expected_dual(k):
    """The first partials rat_dual must give: those of rat_hdual unless the point states its own."""
    c, p = ITEMS[k]
    return parse_expect(p.dual)["g"] if p.dual else expected(k)["g"]


def resolve(token, k, what, idx=None):
    """The double a token stands for (the mpmath number for "ref"), or None for "fin"."""
    if token == "fin":
        return None
    if token == "ref":
        v, g, H = item_reference(k)
        return v if what == "v" else g[idx] if what == "g" else H[idx]
    return token


def value_is_nan(k):
    c, p = ITEMS[k]
    return p.kind == "singular" and isinstance(parse_expect(p.expect)["v"], float) and math.isnan(parse_expect(p.expect)["v"])


# ---- the families the header declares ------------------------------------------------------------------------------------------------------
def declared_families(header_text):
    """{"operator+:TT", "sin:T", "pow:Td", ...}: every function and operator csrc/rat_ad.h declares on a dual type, by name and by which
    arguments are dual (T) or double (d), read from the declarations above RAT_AD_COMPOUND and inside it."""
    import re
    fams = set()
    for m in re.finditer(r"RAT_AD_FN\s+(?:rat_h?dual|T|bool)\s*&?\s*(operator[^\s(]+|[a-z]\w*)\s*\(([^)]*)\)", header_text):
        name, args = m.group(1), m.group(2)
        if name.startswith("rat_"):
            continue
        form = "".join("T" if re.search(r"\b(rat_h?dual|T)\b", a) else "d" for a in args.split(","))
        fams.add(f"{name}:{form}")
    return fams


# ---- device source -------------------------------------------------------------------------------------------------------------------------
def item_switch(ids):
    """ade_item<T>(id, x, u): the case of item `id` at (x[0], x[1], u[0]), for the items in `ids`; items of one case share a label list."""
    by_case = {}
    for k in ids:
        by_case.setdefault(ITEMS[k][0].name, []).append(k)
    out = ["template <class T> __device__ T ade_item(int id, const T *x, const T *u) {", "    switch (id) {"]
    for name, ks in by_case.items():
        body = ITEMS[ks[0]][0].device_body()
        out.append("    " + " ".join(f"case {k}:" for k in ks) + " { " + body + " }   // " + name)
    out += ["    }", "    return T(0.0);", "}"]
    return "\n".join(out) + "\n"


C_MODEL = r"""
// step k evaluates item LO + k; h evaluates item p[0] with u_0 = p[1]
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) { xn[0] = x[0]; xn[1] = x[1]; }
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) { return ade_item<T>(%(lo)d + k, x, u); }
template <class T> __device__ T rat_user_h(const T *x, const double *p) {
    T u[1];
    u[0] = p[1];
    return ade_item<T>((int)p[0], x, u);
}
"""

F_MODEL = r"""
// row (sel mod n) of x_next evaluates item base + sel on (x[0], x[1], u[0]); base = p[0], sel is the value of x[2] (negative: no row)
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) {
    const int sel = (int)rat_value(x[2]);
    T r = 0.0;
    if (sel >= 0) r = ade_item<T>((int)p[0] + sel, x, u);
    for (int i = 0; i < RAT_N; ++i) xn[i] = 0.0;
    if (sel >= 0) xn[sel % RAT_N] = r;
}
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) { return 0.5 * (x[3] * x[3]) + 0.5 * (u[1] * u[1]); }
template <class T> __device__ T rat_user_h(const T *x, const double *p) { return 0.5 * (x[3] * x[3]); }
"""

CHUNK = 48                                                                # steps per model of the c path, and per launch of the f path


def chunks():
    return [range(lo, min(lo + CHUNK, len(ITEMS))) for lo in range(0, len(ITEMS), CHUNK)]


def c_source(ids, extra=()):
    """Step k evaluates item ids[0] + k; `extra` names further items h may be pointed at."""
    return item_switch(list(ids) + [k for k in extra if k not in ids]) + C_MODEL % dict(lo=ids[0])


def f_source():
    return item_switch(range(len(ITEMS))) + F_MODEL


def host_program():
    """A stand-alone C++ program over csrc/rat_ad.h: one lambda per case, every item under rat_dual seeded on each variable in turn and on none,
    and under rat_hdual seeded on every pair (i <= j); every output printed as a hex float."""
    out = ['#include "rat_ad.h"', "#include <cstdio>", "#include <type_traits>",
           "template <class T> static T seeded(double a, int q, int i, int j);",
           "template <> rat_dual seeded<rat_dual>(double a, int q, int i, int) { return rat_dual(a, q == i ? 1.0 : 0.0); }",
           "template <> rat_hdual seeded<rat_hdual>(double a, int q, int i, int j) { return rat_hdual(a, q == i ? 1.0 : 0.0, q == j ? 1.0 : 0.0, 0.0); }",
           "template <class T, class G> static T at(G g, const double *z, int i, int j) {",
           "    T x[2] = {seeded<T>(z[0], 0, i, j), seeded<T>(z[1], 1, i, j)}, u[1] = {seeded<T>(z[2], 2, i, j)};",
           "    return g(x, u);", "}",
           "template <class G> static void run(int id, double z0, double z1, double z2, G g) {",
           "    const double z[3] = {z0, z1, z2};",
           "    for (int i = 0; i < 4; ++i) { rat_dual d = at<rat_dual>(g, z, i, i); std::printf(\"D %d %d %a %a\\n\", id, i, d.v, d.d); }",
           "    for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) {",
           "        rat_hdual h = at<rat_hdual>(g, z, i, j); std::printf(\"H %d %d %d %a %a %a %a\\n\", id, i, j, h.v, h.e1, h.e2, h.e12); }",
           "}", "int main() {"]
    for k, (c, p) in enumerate(ITEMS):
        z = ", ".join(float(a).hex() for a in p.z)
        out.append("    run(%d, %s, [](auto *x, auto *u) { using T = std::remove_cv_t<std::remove_pointer_t<decltype(x)>>; %s });   // %s"
                   % (k, z, c.device_body(), c.name))
    out += ["    return 0;", "}"]
    return "\n".join(out) + "\n"


def parse_host_output(text):
    """{item: dict(dual={i: (v, d)}, hd={(i, j): (v, e1, e2, e12)})}; dual[3] is the run with every seed zero."""
    res = {}
    for line in text.splitlines():
        w = line.split()
        r = res.setdefault(int(w[1]), dict(dual={}, hd={}))
        if w[0] == "D":
            r["dual"][int(w[2])] = tuple(float.fromhex(s) for s in w[3:])
        else:
            r["hd"][(int(w[2]), int(w[3]))] = tuple(float.fromhex(s) for s in w[4:])
    return res
