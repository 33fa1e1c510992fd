"""rat_policy_margin_gradient without a device: the exports, the compile-only check and its refusals, the NumPy model
(tests/margin_gradient_model.py) against central differences of a margin with the disturbances frozen and against the structure the header
states, and the ground the GPU test stands on: on every case it runs, the float64 and the longdouble model take the same arg-max steps
and the same tail sets."""
import ctypes as C

import numpy as np
import pytest

import margin_gradient_model as mg
import policy_gradient_model as pg
import ratilqr.jl_amd as rat
import user_noise_model as un
from ratilqr.jl_amd import _native as nv

EPS = np.finfo(np.float64).eps
SEED = mg.SEED


def test_exports_and_prototypes():
    lib = nv.lib()
    for name in ("rat_policy_margin_gradient", "rat_policy_margin_gradient_check"):
        assert name in nv.EXPORTS and hasattr(lib, name)
    assert len(lib.rat_policy_margin_gradient.argtypes) == 14 and lib.rat_policy_margin_gradient.argtypes[-1] == C.POINTER(C.c_int64)
    assert len(lib.rat_policy_margin_gradient_check.argtypes) == 5


@pytest.mark.parametrize("case", [pg.ScalarLQ(), pg.LqCubic(12, 4, 3), pg.Pendulum(source=pg.PEND_JAC)],
                         ids=["scalar1x1", "lqcubic12x4", "pendulum_jacobian_hook"])
def test_check_compiles_the_kernel_for_gfx950(case):
    rat.policy_margin_gradient_check(case.source, **case.dims())


def test_check_refuses_with_the_documented_codes():
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_UNSUPPORTED.*defines RAT_USER_POLICY"):
        rat.policy_margin_gradient_check("#define RAT_USER_POLICY\n" + un.PEND_DIAG, 2, 1, 2, 0)
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_ARG.*does not define RAT_USER_NOISE"):
        rat.policy_margin_gradient_check(un.PEND_PLAIN, 2, 1, 0, 0)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*n <= 12"):
        rat.policy_margin_gradient_check(un.PEND_DIAG, 13, 1, 2, 0)


def disc(case, t):
    """being inside the disc of radius 0.8 about (0.4, 0.3) in the pendulum's state at step t: g = r^2 - |x - c|^2"""
    d = case.n + case.m
    Q, a = np.zeros((d, d)), np.zeros(d)
    Q[0, 0] = Q[1, 1] = -1.0
    a[:2] = 2.0 * np.array([0.4, 0.3])
    return (Q, a, 0.8 ** 2 - (0.4 ** 2 + 0.3 ** 2), t, t)


@pytest.mark.parametrize("t", [3, 2, 0], ids=["t=N", "t=N-1", "t=0"])
def test_model_matches_central_differences_of_the_margin(t):
    """The pendulum, a disc event with a window of one step (the arg-max cannot switch), w frozen: per rollout M_k(l, L) is smooth, and
    the model's gu and gu (x - x_nom)' are its derivatives.  The central difference is taken in np.longdouble and Richardson-extrapolated,
    D(h) = (4 d(h / 2) - d(h)) / 3 with h = 2^-8: truncation O(h^4) = 2e-10 times a fifth derivative of size <= 1 for this model over
    three steps of dt = 0.1, rounding 1e-19 / h = 3e-17.  Tolerance 1e-9 absolute on gradients of size 1: the truncation bound times 4,
    far above the float64 model's own rounding (1e-15)."""
    case, N, K = pg.Pendulum(), 3, 16
    x_nom, l, L = pg.policy(case, N)
    ev = [disc(case, t)]
    mod = mg.model(case, x_nom, l, L, K, SEED, ev, [0.0])
    z = pg.draws(case, SEED, K, N)

    def M(lq, Lq):
        J, xs, us = pg.rollout(case, x_nom, lq, Lq, z, np.longdouble)
        g, _ = mg.g_values(xs, us, ev)
        return g[:, t, 0]

    def d(arr, idx, h, which):
        a, b = arr.copy(), arr.copy()
        a[idx] += h; b[idx] -= h
        hi, lo = (M(a, L), M(b, L)) if which == "l" else (M(l, a), M(l, b))
        return (hi - lo) / (np.longdouble(a[idx]) - np.longdouble(b[idx]))
    h = 2.0 ** -8
    gu, x = mod["gu"][0], mod["x"]
    worst = 0.0
    for idx in np.ndindex(*l.shape):
        fd = (4 * d(l, idx, h / 2, "l") - d(l, idx, h, "l")) / 3
        worst = max(worst, float(np.abs(fd - gu[:, idx[0], idx[1]]).max()))
    for idx in np.ndindex(*L.shape):
        s, j, i = idx
        fd = (4 * d(L, idx, h / 2, "L") - d(L, idx, h, "L")) / 3
        worst = max(worst, float(np.abs(fd - gu[:, s, j] * (x[:, s, i] - x_nom[s, i])).max()))
    print(f"t* = {t}: largest difference from the extrapolated central difference {worst:.3e}")
    assert worst <= 1e-9
    assert np.all(gu[:, t:] == 0.0)                                   # (the disc reads x alone: nothing at t* either, and t > t* is exact 0)


def test_steps_above_the_argmax_are_exact_zeros_and_the_last_step_has_no_u_part():
    case, N, K = pg.LqCubic(5, 3, 2), 2, 33
    pol = pg.policy(case, N)
    evs = mg.four_events(case, N)
    mod = mg.model(case, *pol, K, SEED, evs, [0.0])
    seen_N = False
    for e in range(len(evs)):
        ts, gu = mod["tstar"][e], mod["gu"][e]
        for k in range(K):
            assert np.all(gu[k, ts[k] + 1:] == 0.0)                   # t > t*: exactly 0
            if ts[k] < N and evs[e][0] is None:
                assert np.array_equal(gu[k, ts[k]], evs[e][1][case.n:])   # a linear event at t*: gu is the u part of a
            seen_N = seen_N or ts[k] == N
    assert seen_N
    # t* = N: u_N is no variable, so the seed is the x part alone -- the u entries of a do not matter
    lin = mg.linear_event(case, N, 21, N)
    other = (None, np.concatenate([lin[1][:case.n], 7.0 + lin[1][case.n:]]), lin[2], N, N)
    a, b = (mg.model(case, *pol, K, SEED, [ev], [0.0]) for ev in (lin, other))
    assert np.array_equal(a["gu"][0], b["gu"][0]) and np.array_equal(a["grad_L"][0], b["grad_L"][0])


def test_the_first_argmax_wins_on_an_exact_tie_and_nan_is_passed_over():
    g = np.array([[[1.0], [3.0], [3.0], [np.nan]], [[np.nan], [np.nan], [-2.0], [-2.0]], [[np.nan], [np.nan], [np.nan], [np.nan]],
                  [[5.0], [4.0], [5.0], [1.0]]])
    M, ts = mg.margins(g, [(None, None, 0.0, 0, 3)], np.ones(4, dtype=bool))
    assert ts[0].tolist() == [1, 2, -1, 0] and np.array_equal(M[0], [3.0, -2.0, np.nan, 5.0], equal_nan=True)
    M, ts = mg.margins(g, [(None, None, 0.0, 2, 3)], np.array([True, True, True, False]))
    assert ts[0].tolist() == [2, 2, -1, -1] and np.isnan(M[0, 3])
    # an exact tie in a rollout: a linear event on a state the dynamics hold still (a = 1, b = 0, sigma = 0)
    case = pg.ScalarLQ([1.0, 0.0, 1.0, 0.2, 2.0, 0.0])
    mod = mg.model(case, np.array([0.7]), np.zeros((3, 1)), None, 4, SEED, [(None, np.array([1.0, 0.0]), 0.0, 1, 3)], [0.0])
    assert np.all(mod["tstar"][0] == 1) and np.all(mod["M"][0] == 0.7)


def test_alpha_zero_is_the_plain_mean_of_the_per_rollout_gradients():
    case, N, K = pg.Pendulum(), 3, 200
    x_nom, l, L = pg.policy(case, N)
    evs = [disc(case, N), mg.quadratic_event(case, N, 22)]
    mod = mg.model(case, x_nom, l, L, K, SEED, evs, [0.0, 0.9])
    for e in range(2):
        gu = mod["gu"][e]
        want_l = gu.mean(axis=0)
        want_L = (gu[:, :, :, None] * (mod["x"][:, :N] - x_nom[None, :N])[:, :, None, :]).mean(axis=0)
        assert np.abs(mod["grad_l"][e][0] - want_l).max() <= 64 * EPS * np.abs(want_l).max()
        assert np.abs(mod["grad_L"][e][0] - want_L).max() <= 64 * EPS * np.abs(want_L).max()
        tail = mod["y"][e][1] > 0                                     # alpha = 0.9 at K = 200: the 20 largest margins, weight 1 each
        assert tail.sum() == 20 and np.array_equal(np.sort(np.argsort(mod["M"][e])[-20:]), np.flatnonzero(tail))
        assert np.abs(mod["grad_l"][e][1] - gu[tail].mean(axis=0)).max() <= 64 * EPS * np.abs(gu[tail]).max()


def test_nonfinite_sensitivities_are_left_out():
    case, pol = mg.sqrt_dyn_setup()
    ev = [(None, np.array([1.0, 0.0]), -0.3, 2, 2)]
    mod = mg.model(case, *pol, 64, SEED, ev, [0.0])
    bad = ~mod["fin"][0]
    assert 0 < mod["n_nonfinite"][0] == bad.sum() < 64 and np.isfinite(mod["M"][0]).all()
    assert np.array_equal(bad, mod["u"][:, 1, 0] == 0.0)
    assert np.allclose(mod["grad_l"][0][0], mod["gu"][0][~bad].mean(axis=0), rtol=1e-13, atol=0)


@pytest.mark.parametrize("closed", [True, False], ids=["closed", "open"])
@pytest.mark.parametrize("name,make,N", mg.CASES, ids=[c[0] for c in mg.CASES])
def test_float64_and_longdouble_models_select_the_same_rollouts_and_steps(name, make, N, closed):
    """What lets the GPU test hold the device within a multiple of the two models' distance without skipping a case: under the seed the
    tests use, no margin sits within a rounding of a tail's cut and no two steps tie within a rounding."""
    case = make()
    pol = pg.policy(case, N, closed)
    evs = mg.four_events(case, N)
    for K in mg.KS:
        m64, mld = mg.reference((name, closed, K), case, pol, K, evs)
        assert mg.same_selection(m64, mld), (name, closed, K)


def test_the_other_gpu_cases_select_the_same_too():
    case, N = pg.Lin2(), 2
    m64, mld = mg.reference(("chunk",), case, pg.policy(case, N), 65536 + 5, [mg.linear_event(case, N, 21, N)])
    assert mg.same_selection(m64, mld)
    case, N = pg.Pendulum(source=pg.PEND_JAC), 3
    m64, mld = mg.reference(("jac",), case, pg.policy(case, N), 65, mg.four_events(case, N))
    assert mg.same_selection(m64, mld)
