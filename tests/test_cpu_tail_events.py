"""tests/tail_events_model.py against closed forms, before the device is held to it (tests/test_gpu_tail_events.py), the two new symbols
against the header, and the user-event kernel's compile check -- no GPU.

The closed forms need no trajectory: an event's g is handed to `reduce` directly, one step, one event.  With the margin an increasing
function of the cost the violators are the most expensive rollouts, so the tail holds min(N_VIOL, TAIL_N) of them; with a decreasing one
they are the cheapest, and the tail holds what does not fit below it.  K a power of two makes every quotient by N_OK exact, so the
identities hold in every bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ratilqr.jl_amd as rat
import events_model as em
import tail_events_model as te
import user_event_model as ue
from ratilqr.jl_amd import _native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = [(None, None, None, 0, 0)]                                      # one event, watched at the one step
NEW = ("rat_policy_tail_events", "rat_policy_tail_events_user")
EPS = np.finfo(float).eps


def distinct_costs(K, seed):
    """K distinct finite costs in no order"""
    r = np.random.default_rng(seed)
    return r.permutation(np.arange(K, dtype=np.float64)) * 0.37 - 3.0 + 0.01 * r.random(K)


def one_event(M):
    return np.asarray(M, dtype=np.float64)[:, None, None]


@pytest.mark.parametrize("K,alpha", [(64, 0.75), (128, 0.5), (256, 0.9375)])
def test_monotone_case(K, alpha):
    """M = J - c: PROB = min(1, N_VIOL / TAIL_N) exactly, and PROB == PROB_ROBUST"""
    J = distinct_costs(K, K)
    tail = K * (1.0 - alpha)
    assert tail == int(tail)
    s = np.sort(J)
    for nv in (0, 1, int(tail) - 1, int(tail), int(tail) + 1, K - 1, K):
        c = s[K - nv - 1] + 1e-6 if nv < K else s[0] - 1.0           # nv costs lie above c
        out = te.reduce(one_event(J - c), ONE, J, (0.0, alpha))
        assert np.array_equal(out["flag"], [0, 0]) and out["tail_n"][1] == tail and np.all(out["n_viol"] == nv)
        assert out["prob"][1, 0] == min(1.0, nv / tail) == out["prob_robust"][1, 0], (nv, out["prob"][1], out["prob_robust"][1])
        assert out["prob"][0, 0] == nv / K == out["prob_robust"][0, 0]                       # alpha = 0: the whole sample
        assert np.all(out["prob"] <= out["prob_robust"])
        assert np.array_equal(out["prob"][:, 1], out["prob"][:, 0])                          # "any" of one event is that event


def test_monotone_case_where_the_quotients_round():
    """K = 100, alpha = 0.9: (1 - alpha) K is the integer 10, but N_VIOL / 100 rounds: PROB_ROBUST is the count ratio to 4 ulp"""
    K, alpha = 100, 0.9
    J = distinct_costs(K, 7)
    s = np.sort(J)
    for nv in (1, 3, 7, 10, 33):
        out = te.reduce(one_event(J - (s[K - nv - 1] + 1e-6)), ONE, J, (alpha,))
        want = min(1.0, nv / 10.0)
        assert out["tail_n"][0] == 10.0 and out["prob"][0, 0] == want
        assert abs(out["prob_robust"][0, 0] - want) <= 4 * EPS * want


@pytest.mark.parametrize("K,alpha", [(64, 0.75), (128, 0.5)])
def test_anti_monotone_case(K, alpha):
    """M = c - J: PROB = max(0, 1 - N_OK (1 - p) / TAIL_N), p = N_VIOL / N_OK"""
    J = distinct_costs(K, K + 1)
    tail = K * (1.0 - alpha)
    s = np.sort(J)
    for nv in (0, 1, K - int(tail), K - int(tail) + 1, K - 1, K):
        c = s[nv] - 1e-6 if nv < K else s[-1] + 1.0                   # nv costs lie below c
        out = te.reduce(one_event(c - J), ONE, J, (alpha,))
        p = nv / K
        assert out["n_viol"][0, 0] == nv
        assert out["prob"][0, 0] == max(0.0, 1.0 - K * (1.0 - p) / tail), (nv, out["prob"][0, 0])
        assert out["prob"][0, 0] <= out["prob_robust"][0, 0] == min(1.0, nv / tail)


def test_ties_at_var():
    """costs clamped at zero: at a low level hundreds of rollouts share VAR = 0; the weights sum to one and each tied rollout carries the
    fractional weight r / c_eq"""
    K, alpha = 1000, 0.25
    J = np.fmax(np.random.default_rng(3).standard_normal(K), 0.0)
    out = te.reduce(one_event(0.5 - J), ONE, J, (alpha,))
    tied, above = J == 0.0, J > 0.0
    c_eq, c_gt, tail = int(tied.sum()), int(above.sum()), out["tail_n"][0]
    assert out["var"][0] == 0.0 and c_eq > 400 and tail == 750.0
    y = out["y"][0]
    r = tail - c_gt
    assert np.all(y[above] == 1.0) and np.all(y[tied] == y[tied][0]) and abs(y[tied][0] - r / c_eq) <= 2 * EPS
    assert abs((y / tail).sum() - 1.0) <= 1e-13                       # the tail distribution sums to one
    between = int((above & (J < 0.5)).sum())                          # the event J < 0.5: the ties and the costs between 0 and 0.5
    assert abs(out["prob"][0, 0] - (r + between) / tail) <= 1e-13
    assert out["n_viol"][0, 0] == c_eq + between and out["prob"][0, 0] <= out["prob_robust"][0, 0] == (c_eq + between) / 1000.0 / (tail / 1000.0)
    only = te.reduce(one_event(1e-300 - J), ONE, J, (alpha,))         # the event J == 0: the atom alone
    assert abs(only["prob"][0, 0] - r / tail) <= 1e-13 and only["n_viol"][0, 0] == c_eq
    assert only["prob"][0, 0] <= only["prob_robust"][0, 0] == c_eq / 1000.0 / (tail / 1000.0)


def test_alpha_zero_is_the_plain_sample():
    """the alpha = 0 row against tests/events_model.events under y = 1: one reduction, the same bits"""
    r = np.random.default_rng(5)
    K, N = 300, 3
    x, u = r.standard_normal((K, N + 1, 2)), r.standard_normal((K, N, 1))
    J = (x ** 2).sum(axis=(1, 2))
    J[::17] = np.nan
    evs = [(np.eye(3), np.ones(3), -4.0, 0, N), (None, np.array([1.0, 0.0, 0.0]), -0.5, 2, 2)]
    got = te.tail_events(x, u, J, (0.0, 0.6), evs)
    want = em.events(x, u, J, np.ones((1, K)), np.zeros(1, dtype=bool), evs)
    for k in em.SLOT_NAMES + ("step",):
        assert np.array_equal(got[k][0], want[k][0], equal_nan=True), k
    assert np.array_equal(got["margins"], want["margins"], equal_nan=True) and np.array_equal(got["tau"], want["tau"])
    assert np.array_equal(got["prob_robust"][0], got["prob"][0])
    assert np.all(got["prob"] <= got["prob_robust"]) and np.all(got["margin_max"][0] == got["margin_max"][1])
    assert np.all(got["step"][:, 1, [0, 1, 3]] == 0.0)                # outside the single-step window


def test_flags_and_nan_handling():
    K = 40
    J = distinct_costs(K, 2)
    M = np.linspace(-1.0, 1.0, K)
    # a level thinner than one rollout: uniform on the maximum, which is one rollout here
    out = te.reduce(one_event(M), ONE, J, (0.0, 1.0 - 0.5 / K))
    top = int(np.argmax(J))
    assert np.array_equal(out["flag"], [0, 1]) and np.array_equal(out["event_flag"][1], [1, 1])
    assert out["prob"][1, 0] == float(M[top] > 0) and out["margin_mean"][1, 0] == M[top] and out["prob_robust"][1, 0] == 1.0
    assert out["margin_max"][1, 0] == out["margin_max"][0, 0] == 1.0 and out["n_viol"][1, 0] == out["n_viol"][0, 0]
    # an empty sample and one that holds Inf: NaN but for the flag
    for bad, flag in ((np.full(K, np.nan), te.EMPTY), (np.where(np.arange(K) == 3, np.inf, J), te.NONFINITE)):
        out = te.reduce(one_event(M), ONE, bad, (0.0, 0.5))
        assert np.all(out["flag"] == flag) and np.all(out["event_flag"] == flag)
        for k in te.SLOT_NAMES + ("step",):
            assert np.isnan(out[k]).all(), (flag, k)
    # DomainError rollouts carry no weight and are not counted
    Jd = J.copy()
    Jd[M > 0.5] = np.nan
    out = te.reduce(one_event(M), ONE, Jd, (0.0, 0.5))
    n_ok = int((~np.isnan(Jd)).sum())
    assert np.all(out["y"][:, np.isnan(Jd)] == 0.0) and out["tail_n"][0] == n_ok
    assert out["n_viol"][0, 0] == ((M > 0) & (M <= 0.5)).sum() and out["margin_max"][0, 0] <= 0.5 and np.isnan(out["margins"][0][np.isnan(Jd)]).all()
    assert out["prob"][0, 0] == out["n_viol"][0, 0] / n_ok
    # a NaN g is passed over: the margin is the largest of the others; a rollout whose every g is NaN has a NaN margin and never violates
    g = np.stack([M, -M, np.full(K, np.nan)], axis=1)[:, :, None]     # three steps
    g[0] = np.nan
    win = [(None, None, None, 0, 2)]
    out = te.reduce(g, win, J, (0.0, 0.5))
    assert np.array_equal(out["margins"][0][1:], np.abs(M)[1:]) and np.isnan(out["margins"][0][0]) and out["tau"][0][0] == -1
    assert out["n_viol"][0, 0] == K - 1
    # ... it spoils MARGIN_MEAN only on a row it has weight in: selected out of the others
    assert np.isnan(out["margin_mean"][0, 0])
    assert np.isfinite(out["margin_mean"][1, 0]) == (out["y"][1][0] == 0.0)
    Jl = J.copy()
    Jl[0] = J.min() - 1.0                                             # the cheapest rollout: outside every tail above alpha = 0
    out = te.reduce(g, win, Jl, (0.0, 0.5))
    assert np.isnan(out["margin_mean"][0, 0]) and np.isfinite(out["margin_mean"][1, 0]) and np.isfinite(out["prob"]).all()


def test_export_prototypes_and_the_event_kernel_still_compiles():
    """the library exports the two calls with the header's prototypes, the mirrors exist, and rat_user_event_check still compiles the
    user-event kernel both calls share"""
    lib = C.CDLL(nv.SO_PATH)
    hdr = open(os.path.join(ROOT, "include", "ratilqr.h")).read()
    ctype = {"rat_handle": C.c_void_p, "const double *": nv._dp, "double *": nv._dp, "const int32_t *": nv._ip, "int32_t": C.c_int32}
    for name in NEW:
        assert name in nv.EXPORTS and hasattr(lib, name), name
        args = re.search(r"rat_rc " + name + r"\(([^;]*)\);", hdr).group(1)
        want = [ctype[re.sub(r"\s*\w+$", "", " ".join(a.split())).replace(" *", " *").strip()] for a in args.split(",")]
        assert list(getattr(nv.lib(), name).argtypes) == want, name
    for meth in ("policy_tail_events", "policy_tail_events_user"):
        assert callable(getattr(rat.Context, meth))
    julia = open(os.path.join(ROOT, "julia", "RATiLQRAMD.jl")).read()
    for name in NEW:
        assert f"(:{name}, LIB)" in julia, name
    for which, n, m in ((ue.DI, 2, 1), (ue.WALK, 1, 1)):
        text = ue.source(which, "half", 3).encode()
        assert nv.lib().rat_user_event_check(text, n, m, 1) == 0, nv.lib().rat_last_error().decode()
