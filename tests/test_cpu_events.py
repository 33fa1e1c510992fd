"""The NumPy model of rat_policy_events' kernels (tests/events_model.py) against a direct np.longdouble answer, the host-only
rat_kl_event_bound through the loaded library, and the Python mirror of both entry points."""
import ctypes as C

import numpy as np
import pytest

import ratilqr.jl_amd as rat
from ratilqr.jl_amd import _native as nv
from events_model import between, deviation, direct, events, scales
from test_cpu_wc_trajectory import sample
from wc_trajectory_model import row_weights

# The deviation of the restated order from the extended-precision answer that test_model_against_longdouble measures (worst over its
# cases: events_model.deviation): the GPU tests allow the device ten times this.
CPU_DEV_PROB, CPU_DEV_MARGIN = 4.5e-16, 2.9e-16


def event_set(x, u, n, m, N, rng):
    """the nine kinds of tests/test_gpu_events.py on synthetic trajectories, sized from their spread"""
    ok = ~np.isnan(x).any(axis=(1, 2))
    xs, us = x[ok], u[ok]
    d = n + m
    A = rng.standard_normal((d, d))
    Qd = A + A.T
    z = np.concatenate([xs[:, :-1], us], axis=2) if N else np.zeros((1, 1, d))
    qz = np.einsum("kti,ij,ktj->kt", z, Qd, z)
    evs = [rat.halfspace(np.eye(n)[0], -between(xs[:, :, 0], 0.5)),
           rat.halfspace(np.concatenate([np.zeros(n), np.eye(m)[m - 1]]), -between(us[:, :, m - 1], 0.7)),
           rat.ball([0, 1], xs[:, -1, :2].mean(axis=0), 1.2 * xs[:, -1, :2].std()),
           rat.quadratic_event(Qd, rng.standard_normal(d), -between(qz, 0.5)),
           rat.halfspace(np.eye(n)[1], 1.0 - x[0, 0, 1], steps=0),
           rat.quadratic_event(np.eye(d), np.zeros(d), -between((xs[:, -1] ** 2).sum(axis=1), 0.5), steps=N),
           rat.halfspace(np.ones(d), -1e30),
           rat.halfspace(np.zeros(d), 1.0, steps=(min(1, N), N)),
           rat.quadratic_event(np.zeros((d, d)), np.zeros(d), 0.0)]
    return [e.dense(n, m, N) for e in evs]


@pytest.mark.parametrize("K,nan_every,n,m", [(K, e, 3, 2) for K in (1, 3, 5, 257) for e in (0, 3)] + [(65536 + 5, 7, 3, 2), (65, 0, 12, 4), (257, 3, 12, 4)])
def test_model_against_longdouble(K, nan_every, n, m):
    """Rows: the nominal distribution, a tilt, a searched radius and a saturated one.  Measured here, worst over the eleven cases:
    probabilities 4.4e-16 (K = 65541), margin means 2.8e-16 of the event's scale (K = 257, one rollout in three selected out); the 12 + 4
    cases, the shape of the GPU tests' largest problem, stay at 2.2e-16 and 1.4e-16.  CPU_DEV_* round these up; asserted, not only recorded."""
    N = 2 if K < 1000 else 1
    x, u, J, _, _ = sample(K, 10 * K + nan_every, n=n, m=m, N=N, nan_every=nan_every)
    evs = event_set(x, u, n, m, N, np.random.default_rng(K))
    y, dead, wc = row_weights(J, kl_bounds=(0.05, np.inf), thetas=(0.0, 0.7))
    got, ref = events(x, u, J, y, dead, evs), direct(x, u, J, y, dead, evs)
    sc = scales(x, u, J, evs)
    dp, dm = deviation(got, ref, sc, N)
    print(f"K={K} nan_every={nan_every} n={n} m={m}: probabilities {dp:.2e} margin means {dm:.2e}")
    assert dp <= CPU_DEV_PROB and dm <= CPU_DEV_MARGIN
    assert np.array_equal(got["tau"], ref["tau"]) and np.array_equal(got["n_viol"], ref["n_viol"])
    ok = ~np.isnan(J)
    assert np.all(np.abs(got["margins"][:, ok] - ref["margins"][:, ok].astype(float)) <= 1e-12 * sc[:, None])
    n_ok = ok.sum()
    # nobody, everybody (from its window's first step), the boundary
    assert np.all(got["prob"][:, 6] == 0.0) and np.isnan(got["first_mean"][:, 6]).all()
    assert np.all(got["prob"][:, 7] == 1.0) and np.all(got["first_mean"][:, 7] == min(1, N))
    assert np.all(got["prob"][:, 8] == 0.0) and np.all(got["margin_mean"][:, 8] == 0.0)
    # the union dominates, and the theta = 0 row counts
    assert np.all(got["prob"][:, -1:] >= got["prob"][:, :-1])
    assert np.array_equal(got["prob"][2], got["n_viol"][2] / n_ok)
    nv_ = got["n_viol"][2]
    assert np.allclose(got["prob_se"][2], np.sqrt(nv_ * (n_ok - nv_) / n_ok) / n_ok, rtol=1e-14, atol=0)     # sqrt(p (1 - p) / N_OK), from the counts
    # step sums stay inside the window
    assert np.all(got["step"][:, 4, 1:] == 0.0) and np.all(got["step"][:, 5, :N] == 0.0)


GRID_P = (1e-9, 1e-6, 1e-3, 0.01, 0.1, 0.3, 0.5, 0.9, 0.99, 0.999)
GRID_D = (1e-6, 1e-4, 1e-2, 0.1, 0.5, 1.0, 3.0, 10.0, 20.0)


def kl_ld(q, p):
    q, p = np.longdouble(q), np.longdouble(p)
    return q * np.log1p((q - p) / p) + (1 - q) * np.log1p(-(q - p) / (1 - p))


def test_kl_event_bound_fixed_points_and_refusals():
    assert rat.kl_event_bound(0.3, 0.0) == 0.3 and rat.kl_event_bound(0.0, 5.0) == 0.0 and rat.kl_event_bound(0.0, np.inf) == 0.0
    assert rat.kl_event_bound(1.0, 0.2) == 1.0 and rat.kl_event_bound(0.2, np.inf) == 1.0 and rat.kl_event_bound(1e-300, np.inf) == 1.0
    out = C.c_double()
    for p, d in ((np.nan, 0.1), (0.1, np.nan), (-0.1, 0.1), (1.1, 0.1), (0.5, -1e-9), (np.inf, 0.1)):
        assert nv.lib().rat_kl_event_bound(C.c_double(p), C.c_double(d), C.byref(out)) == 1
        assert b"rat_kl_event_bound" in nv.lib().rat_last_error()
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG"):
            rat.kl_event_bound(p, d)
    assert nv.lib().rat_kl_event_bound(C.c_double(0.5), C.c_double(0.1), None) == 1


@pytest.mark.parametrize("p", GRID_P)
def test_kl_event_bound_solves_the_equation(p):
    """KL(p' || p) = d to 1e-12 relative wherever p' < 1, and p' = 1 exactly where d >= log(1 / p).  The hardest point is p = 0.999,
    d = 1e-6, where KL of neighbouring doubles p' differs by 5.0e-12 d: the function returns the neighbour of the root nearer in KL."""
    worst = 0.0
    for d in GRID_D:
        q = rat.kl_event_bound(p, d)
        assert p <= q <= 1.0
        if d >= -np.log(p):
            assert q == 1.0, (p, d, q)
            continue
        rel = abs(float((kl_ld(q, p) - np.longdouble(d)) / np.longdouble(d)))
        worst = max(worst, rel)
        print(f"p={p:g} d={d:g}: p'={q!r} KL off by {rel:.2e}")
        assert rel <= 1e-12, (p, d, q, rel)
    print(f"worst {worst:.2e}")


def test_kl_event_bound_is_monotone():
    """Non-decreasing in both arguments: on the grid, and on steps of 1e-6 relative about random points (the bisection ends on
    neighbouring doubles and evaluates KL in double, so steps of an ulp are below what it resolves)."""
    tab = np.array([[rat.kl_event_bound(p, d) for d in (0.0,) + GRID_D + (np.inf,)] for p in (0.0,) + GRID_P + (1.0,)])
    assert np.all(np.diff(tab[1:], axis=1) >= 0) and np.all(np.diff(tab, axis=0) >= 0)
    rng = np.random.default_rng(0)
    for _ in range(200):
        p, d = rng.uniform(0, 1), 10.0 ** rng.uniform(-6, 1)
        q = rat.kl_event_bound(p, d)
        assert rat.kl_event_bound(min(p * (1 + 1e-6), 1.0), d) >= q and rat.kl_event_bound(p, d * (1 + 1e-6)) >= q


def test_constructors():
    e = rat.ball([0, 3], [1.0, -2.0], 0.5)
    Q, a, b, lo, hi = e.dense(3, 2, 7)
    z = np.array([1.2, 9.0, 9.0, -2.1, 4.0])
    assert np.isclose(z @ Q @ z + a @ z + b, 0.25 - 0.04 - 0.01) and (lo, hi) == (0, 7)
    Q, a, b, lo, hi = rat.halfspace([1.0, 0.0, 2.0], -1.0, steps=3).dense(3, 2, 7)
    assert Q is None and np.array_equal(a, [1, 0, 2, 0, 0]) and (b, lo, hi) == (-1.0, 3, 3)
    Q, a, b, lo, hi = rat.quadratic_event(np.eye(3), np.zeros(5), 0.0, steps=(1, 2)).dense(3, 2, 7)
    assert Q.shape == (5, 5) and Q[3, 3] == 0 and (lo, hi) == (1, 2)
    with pytest.raises(ValueError):
        rat.halfspace(np.ones(4), 0.0).dense(3, 2, 7)
    with pytest.raises(ValueError):
        rat.ball([5], [0.0], 1.0).dense(3, 2, 7)


def test_the_entry_points_are_exported_and_mirrored():
    assert {"rat_policy_events", "rat_kl_event_bound"} <= set(nv.EXPORTS) and hasattr(nv.lib(), "rat_policy_events")
    assert callable(rat.Context.policy_events) and callable(rat.GenericContext.policy_events)
    rc = nv.lib().rat_policy_events(None, 1, None, None, None, None, None, None, 0, None, 0, None, None, None, None)
    assert rc == 1 and b"rat_policy_events" in nv.lib().rat_last_error()
