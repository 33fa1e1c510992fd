"""The lazily compiled kernels of a source problem share one handle (csrc/driver.cpp: SrcSlot, src_kernel, src_drop_slots): a context that
walks through every kind and back answers as a fresh context that made only that call, and setting the problem again drops every kernel
of the previous one.

The double integrator of tests/user_event_model.py with the event "half", N = 4, K = 65 (a full wavefront and one rollout).  Everything is
compared with np.array_equal: the same kernel on the same inputs at the same seed."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
import user_event_model as ue

pytestmark = pytest.mark.gpu
N, K = 4, 65
Q_HALF = [0.62]                                                       # (x_0 = 0.602 on every rollout: the margin peaks later on some)
THETAS = (0.0, 0.5)
NOISE = dict(normals_per_step=2, uniforms_per_step=0, seed=21)
# the same n, m, N and parameter count, other dynamics: a kernel kept from the first source gives a wrong number, not a bad access
DI_2 = ue.DI.replace("xn[0] = x[0] + p[0] * x[1];", "xn[0] = x[0] + 2.0 * p[0] * x[1];")


def problem(base):
    return rat.DeviceSourceProblem(ue.source(base, "half", len(ue.DI_P)), 2, 1, N, 1e-3 * np.eye(2), params=np.concatenate([ue.DI_P, Q_HALF]))


EVENT = rat.halfspace(np.eye(2)[0], -Q_HALF[0])
_policy = []


def policy():
    """(x_nom, l, L) of user_event_model.di_case"""
    if not _policy:
        _policy.extend(ue.di_case("half", N, Q_HALF)[1:4])
    return _policy


def noise():
    return rat.UserNoise(**NOISE)


# the calls; CALLS says which of them replay the evaluation before them
def evaluate_noise(ctx):
    return ctx.policy_evaluate_noise(*policy(), noise=noise(), K=K, thetas=THETAS, want_costs=True)


def evaluate(ctx):
    return ctx.policy_evaluate(*policy(), K=K, seed=3, thetas=THETAS, want_costs=True)


def events_user(n_event):
    return lambda ctx: ctx.policy_events_user(n_event, thetas=THETAS, want_margins=True)


def rare_noise(ctx):
    return ctx.policy_rare_event_noise(*policy(), EVENT, K, noise=noise(), n_iter=0, want_margins=True, want_logw=True)


def rare_user(ctx):
    return ctx.policy_rare_event_user(*policy(), 1, 0, K, noise=noise(), n_iter=0, want_margins=True, want_logw=True)


CALLS = {"evaluate_noise": (evaluate_noise, False), "events_user_1": (events_user(1), True), "rare_noise": (rare_noise, False),
         "rare_user": (rare_user, False), "evaluate": (evaluate, False), "events_user_2": (events_user(2), True)}


def flat(r):
    """a result (dict, RareEventResult, array, number, None) as a list of arrays"""
    if r is None:
        return []
    if isinstance(r, dict) or hasattr(r, "__dict__"):
        d = r if isinstance(r, dict) else vars(r)
        return [a for k in sorted(d) for a in flat(d[k])]
    return [np.asarray(r)]


def same(a, b):
    a, b = flat(a), flat(b)
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(a, b))


_fresh = {}


def fresh(base):
    """every call on a context of its own that made only that call, behind the evaluation it replays; computed once per source"""
    if base not in _fresh:
        out = {}
        for name, (call, replays) in CALLS.items():
            ctx = rat.Context(problem(base))
            if replays:
                evaluate_noise(ctx)
            out[name] = call(ctx)
        _fresh[base] = out
    return _fresh[base]


def test_one_handle_walks_through_every_lazy_kind_and_back():
    want = fresh(ue.DI)
    assert want["evaluate_noise"]["costs"].shape == (K,) and want["events_user_1"]["margins"].shape == (1, K)
    assert np.unique(want["events_user_1"]["margins"]).size > K // 8  # the event tells rollouts apart
    ctx = rat.Context(problem(ue.DI))
    assert ctx.debug_get("src_un_loads") == 0
    for step, name in enumerate(("evaluate_noise", "events_user_1", "rare_noise", "rare_user", "evaluate", "evaluate_noise", "events_user_2",
                                 "events_user_1")):
        assert same(CALLS[name][0](ctx), want[name]), (step, name)
    assert ctx.debug_get("src_un_loads") == 1


def test_a_problem_set_again_drops_every_kernel_of_the_previous_one():
    first, second = fresh(ue.DI), fresh(DI_2)
    order = ("evaluate_noise", "events_user_1", "rare_noise", "rare_user", "evaluate")
    for name in order:
        assert not same(first[name], second[name]), name              # the two sources differ in every call
    ctx = rat.Context(problem(ue.DI))
    for visit, (base, want) in enumerate(((ue.DI, first), (DI_2, second), (ue.DI, first))):
        if visit:
            ctx.set_problem(problem(base))
        for name in order:
            assert same(CALLS[name][0](ctx), want[name]), (visit, name)
