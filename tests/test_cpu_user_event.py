"""rat_user_event on the host: tests/user_event_model.py pinned on hand-made three-step trajectories, the compile-only checks of the two
kernels (rat_user_event_check: rat_src_user_events of csrc/source_events.h; rat_rare_event_user_check: rat_src_rare_rollout of
csrc/source_rare.h under RAT_RARE_USER_EVENT), the four new symbols against the header, and the closed form the GPU test holds
rat_policy_rare_event_user to -- no GPU.

The closed form.  WALK is x_{k+1} = x_k + s z_k from x_0: x_N is N(x_0, N s^2), so the event x_N - c > 0 with c = x_0 + q s sqrt(N) has
P = Phi(-q), 1e-6 at q = 4.7534.  The event's g is one subtraction, and the quadratic path forms 1 x_0 plus exact zeros plus b, the same
bits: tests/rare_event_noise_model.py with the half-space (a = e_0, b = -c, step N) is the reference estimator of the user call.
SEED_WALK was fixed here, on that model alone, before the device ran: the first seed tried (tests/test_cpu_rare_event_noise.py's); the
figure it gives is in test_closed_form_reference_estimator's output."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ratilqr.jl_amd as rat
import rare_event_model as rm
import rare_event_noise_model as nm
import user_event_model as ue
import user_noise_model as um
from ratilqr.jl_amd import _native as nv
from test_cpu_rare_event import K_CLOSED, N_ITER_CLOSED, QUANTILES, RHO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED = 0, 1, 2
SEED_WALK = 20261019
N_WALK = 8
NAN = np.nan


# ---- the model on hand-made trajectories ---------------------------------------------------------------------------------------------------
def hand():
    """four rollouts of (2, 1) over three steps (N = 2); rollout 3 is a DomainError whose trajectory holds NaN"""
    x = np.array([[[0.0, 0.0], [1.0, 0.0], [2.0, 0.0]],               # crosses 1.0 only at the last step; sits ON it at step 1
                  [[3.0, 0.0], [0.0, 0.0], [0.5, 0.0]],               # violates at the first step
                  [[0.0, 0.0], [0.5, 0.0], [0.75, 0.0]],              # never
                  [[5.0, 0.0], [NAN, NAN], [NAN, NAN]]])
    u = np.array([[[0.5], [2.0]], [[0.0], [0.0]], [[-1.0], [-1.0]], [[0.0], [NAN]]])
    return x, u, np.array([1.0, 2.0, 3.0, NAN])


def test_a_tie_at_zero_is_not_violated_and_the_first_step_is_kept():
    x, u, costs = hand()
    M, tau, viol = ue.per_rollout(ue.g_user("half", x, u, [1.0]), costs)
    assert np.array_equal(M[0], [1.0, 2.0, -0.25, NAN], equal_nan=True)
    assert list(tau[0]) == [2, 0, -1, -1]                             # g == 0 at step 1 of rollout 0: not violated
    assert np.array_equal(viol[:, :, 0], [[False, False, True], [True, False, False], [False] * 3, [False] * 3])
    assert np.array_equal(M[1], M[0], equal_nan=True) and np.array_equal(tau[1], tau[0])      # "any" of one event is the event


def test_an_entry_left_alone_is_passed_over():
    """half_at writes g[0] at one step alone: M is that step's g, not a maximum with NaN; an event that is never written has a NaN margin
    on every rollout, never violates and does not disturb "any" """
    x, u, costs = hand()
    g = ue.g_user("half_at", x, u, [0.25, 1.0])
    assert np.isnan(g[:, [0, 2], 0]).all() and np.array_equal(g[:3, 1, 0], [0.75, -0.25, 0.25])
    M, tau, viol = ue.per_rollout(g, costs)
    assert np.array_equal(M[0], [0.75, -0.25, 0.25, NAN], equal_nan=True) and list(tau[0]) == [1, -1, 1, -1]
    g16 = ue.g_user("16", x, u, np.concatenate([np.full(14, 10.0), [0.25]]))
    M, tau, viol = ue.per_rollout(g16, costs)
    assert np.isnan(M[15]).all() and np.all(tau[15] == -1) and not viol[:, :, 15].any()
    # entry 14 is on u[0]: watched at k = N with u = 0, so every margin is at least 0 - 0.25
    assert np.array_equal(M[14], [1.75, -0.25, -0.25, NAN], equal_nan=True) and list(tau[14]) == [0, -1, -1, -1]
    # "any": the largest margin and the earliest step over the events that have one
    assert np.array_equal(M[16], [1.75, -0.25, -0.25, NAN], equal_nan=True) and np.array_equal(tau[16], tau[14])


def test_a_window_and_an_intersection():
    x, u, costs = hand()
    assert np.isnan(ue.g_user("window", x, u, [0.0])).all()           # three steps: 3 <= k <= 5 never comes
    xs = np.zeros((1, 7, 2))
    xs[0, :, 0] = [9.0, 9.0, 9.0, 0.0, 1.0, 0.5, 9.0]
    M, tau, _ = ue.per_rollout(ue.g_user("window", xs, np.zeros((1, 6, 1)), [0.75]), [0.0])
    assert M[0, 0] == 0.25 and tau[0, 0] == 4                         # the 9s outside the window are not seen
    # inside the box [0, 2] x [-1, 1]: rollout 0 at steps 1 (on the edge: g == ... > 0 only strictly inside) and 2 (on the other edge)
    g = ue.g_user("box", x, u, [0.0, 2.0, -1.0, 1.0])[:, :, 0]
    assert np.array_equal(g[0], [0.0, 1.0, 0.0]) and np.array_equal(g[1], [-1.0, 0.0, 0.5]) and np.isnan(g[3, 1:]).all()
    M, tau, _ = ue.per_rollout(g[:, :, None], costs)
    assert list(tau[0]) == [1, 2, 1, -1] and np.isnan(M[0, 3])        # the DomainError rollout: selected out though x_0 = (5, 0) has a g
    # a moving square of half-width 0.5 whose centre follows rollout 0: inside at every step, the others only where they meet it
    q = np.concatenate([[0.5], x[0].ravel()])
    M, tau, _ = ue.per_rollout(ue.g_user("moving", x, u, q), costs)
    assert M[0, 0] == 0.5 and tau[0, 0] == 0 and tau[0, 1] == -1 and tau[0, 2] == 0


def test_the_reduction_is_the_quadratic_models():
    """`reduce` on the half-space's g against events_model.events on the same half-space as (Q = None, a = e_0, b = -c): one reduction, so
    every slot agrees in bits wherever 1 x_0 + 0 + b is x_0 - c, which is everywhere"""
    import events_model as em
    r = np.random.default_rng(0)
    K, N = 300, 4
    x, u = r.standard_normal((K, N + 1, 2)), r.standard_normal((K, N, 1))
    costs = r.standard_normal(K)
    costs[::7] = NAN
    y = np.abs(r.standard_normal((2, K)))
    dead = np.array([False, False])
    got = ue.reduce(ue.g_user("half", x, u, [0.3]), costs, y, dead)
    want = em.events(x, u, costs, y, dead, [(None, np.array([1.0, 0.0, 0.0]), -0.3, 0, N)])
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert 0 < got["n_viol"][0, 0] < K


# ---- the kernels compile without a device ----------------------------------------------------------------------------------------------------
def sources():
    """every test event on both sizes: (text, n, m, n_event)"""
    out = []
    for name, (_, ne) in ue.BODIES.items():
        out.append((ue.source(ue.DI, name, len(ue.DI_P)), 2, 1, ne))
        out.append((ue.source(um.LQ_GAUSS, name, 400), 12, 4, ne))
    return out


def last_error():
    return nv.lib().rat_last_error().decode()


def test_both_kernels_compile_for_every_test_event():
    ev, re_ = nv.lib().rat_user_event_check, nv.lib().rat_rare_event_user_check
    for text, n, m, ne in sources():
        assert ev(text.encode(), n, m, ne) == OK, last_error()
        assert re_(text.encode(), n, m, n, 0, ne) == OK, last_error()


def test_what_the_checks_refuse():
    ev, re_ = nv.lib().rat_user_event_check, nv.lib().rat_rare_event_user_check
    good = ue.source(ue.DI, "half", 3).encode()
    # a source without the event: the message says what to define
    assert ev(ue.DI.encode(), 2, 1, 1) == ARG and "RAT_USER_EVENT" in last_error() and "rat_user_event(k, x, u, g, p)" in last_error()
    assert re_(ue.DI.encode(), 2, 1, 2, 0, 1) == ARG and "RAT_USER_EVENT" in last_error()
    # a syntax error inside the event: the compiler names the line of the user's text
    bad = ue.source(ue.DI, "half", 3, body=ue.SYNTAX_ERROR)
    line = bad[:bad.index(ue.SYNTAX_ERROR)].count("\n") + 1
    for rc in (ev(bad.encode(), 2, 1, 1), re_(bad.encode(), 2, 1, 2, 0, 1)):
        assert rc == ARG and re.search(rf"model\.hip:{line}:", last_error()), last_error()
    for ne in (0, 17, -1):
        assert ev(good, 2, 1, ne) == ARG and "n_event" in last_error()
        assert re_(good, 2, 1, 2, 0, ne) == ARG and "n_event" in last_error()
    big = ue.source(um.LQ_GAUSS, "half", 400).encode()
    assert ev(big, 13, 4, 1) == UNSUPPORTED and re_(big, 13, 4, 12, 0, 1) == UNSUPPORTED
    assert ev(good, 2, 5, 1) == UNSUPPORTED
    # the rare-event kernel keeps rat_rare_event_noise_check's refusals: nothing to shift, more than twelve normals, a source without a sampler
    assert re_(good, 2, 1, 0, 0, 1) == ARG and re_(good, 2, 1, 13, 0, 1) == UNSUPPORTED and re_(good, 2, 1, 2, -1, 1) == ARG
    no_noise = um.PEND_PLAIN + "#define EVOFF 1\n" + ue.EVENT_HEAD + ue.BODIES["half"][0] + "}\n"
    assert ev(no_noise.encode(), 2, 1, 1) == OK, last_error()         # the events kernel draws nothing
    assert re_(no_noise.encode(), 2, 1, 2, 0, 1) == ARG and "RAT_USER_NOISE" in last_error()
    # the Python wrappers raise on a refusal
    rat.user_event_check(good.decode(), 2, 1, 1)
    rat.rare_event_user_check(good.decode(), 2, 1, 2, 0, 1)
    with pytest.raises(rat.RatError, match="RAT_USER_EVENT"):
        rat.user_event_check(ue.DI, 2, 1, 1)
    with pytest.raises(rat.RatError, match="RAT_USER_EVENT"):
        rat.rare_event_user_check(ue.DI, 2, 1, 2, 0, 1)


def test_a_source_with_an_event_still_compiles_as_every_other_kind():
    text = ue.source(ue.DI, "16", 3).encode()
    assert nv.lib().rat_source_check(text, 2, 1) == OK, last_error()
    assert nv.lib().rat_user_noise_check(text, 2, 1, 2, 0) == OK, last_error()
    assert nv.lib().rat_rare_event_noise_check(text, 2, 1, 2, 0) == OK, last_error()


def test_abi_export_and_prototype():
    lib = C.CDLL(nv.SO_PATH)
    hdr = open(os.path.join(ROOT, "include", "ratilqr.h")).read()
    ctype = {"rat_handle": C.c_void_p, "const double *": nv._dp, "double *": nv._dp, "int64_t": C.c_int64, "int32_t": C.c_int32,
             "uint64_t": C.c_uint64, "double": C.c_double, "const char *": C.c_char_p}
    for name in ("rat_policy_events_user", "rat_user_event_check", "rat_policy_rare_event_user", "rat_rare_event_user_check"):
        assert name in nv.EXPORTS and hasattr(lib, name)
        args = re.search(r"rat_rc " + name + r"\(([^;]*)\);", hdr).group(1)
        want = [ctype[re.sub(r"\s*\w+$", "", " ".join(a.split())).replace(" *", " *").strip()] for a in args.split(",")]
        assert list(getattr(nv.lib(), name).argtypes) == want, name
    for meth in ("policy_events_user", "policy_rare_event_user"):
        assert callable(getattr(rat.Context, meth))
    julia = open(os.path.join(ROOT, "julia", "RATiLQRAMD.jl")).read()
    for name in ("rat_policy_events_user", "rat_user_event_check", "rat_policy_rare_event_user", "rat_rare_event_user_check"):
        assert f"(:{name}, LIB)" in julia, name


# ---- the closed form's reference estimator ----------------------------------------------------------------------------------------------------
def walk_case():
    """(Model, x_nom, l, threshold c, exact p): the random walk from x_0 = 0.5, open loop with l = 0, N_WALK steps"""
    q = QUANTILES[1e-6]
    x0, s = 0.5, ue.WALK_P[1]
    f = lambda x, u, p: x + p[0] * u
    noise = lambda k, x, u, rng, p: (p[1] * rng.normal())[:, None]
    mod = nm.Model(f, noise, ue.WALK_P, 1, 1, N_WALK, 1)
    return mod, np.array([x0]), np.zeros((N_WALK, 1)), x0 + q * s * math.sqrt(N_WALK), 0.5 * math.erfc(q / math.sqrt(2.0))


def test_closed_form_reference_estimator():
    mod, x0, l, c, exact = walk_case()
    r = nm.rare_event_noise(mod, x0, l, None, rat.halfspace([1.0, 0.0], -c, steps=N_WALK), K_CLOSED, seed=SEED_WALK, n_iter=N_ITER_CLOSED, rho=RHO)
    print(f"p = {exact:.6e}: PROB {r['prob']:.6e} SE {r['prob_se']:.3e} ({abs(r['prob'] - exact) / r['prob_se']:.2f} sigma), "
          f"{r['n_iter']} iterations, ESS {r['ess']:.0f}")
    assert r["flag"] == rm.OK
    assert abs(r["prob"] - exact) <= 5.0 * r["prob_se"]
