"""csrc/rat_ad.h on the device at domain edges, kinks, ties, branch switches and extreme scales: the table of tests/ad_edge_cases.py through
rat_src_linearize, against mpmath at the regular points and the table's classes at the singular ones (tests/test_cpu_ad_edges.py does the
same on the host).

rat_hdual: models at (n, m) = (2, 1), the smallest shape with x-x, x-u and u-u pairs.  rat_user_c(k, ...) evaluates item lo + k at the
point in row k of a hand-built trajectory, rat_user_h evaluates the item named in p at the last row: one approximate_model call returns value,
gradient and Hessian of up to 48 items.  rat_dual: one model at (12, 4) whose x_next has the item p[0] + sel in row sel mod 12, sel being the
value of x[2] at that step (f has no step index; the selector is read, never differentiated), compared through A_array and B_array."""
import math

import numpy as np
import pytest

import ratilqr.jl_amd as rat

import ad_edge_cases as T

pytestmark = pytest.mark.gpu

ARRAYS = ("q_array", "q_vec_array", "Q_array", "r_array", "R_array", "P_array", "A_array", "B_array")
REPORT = {}                                                            # function -> [worst project metric, worst error relative to |want|]


def point(k, clean=False):
    """The point of item k; with `clean`, a singular item's safe point instead."""
    c, p = T.ITEMS[k]
    return p.safe if clean and p.kind == "singular" else p.z


def note(k, got, what, idx):
    """File one finite device output under its function for the report (against mpmath wherever the case has a reference)."""
    ref = T.item_reference(k)
    if ref is None or not math.isfinite(got):
        return
    m = float(ref[0] if what == "v" else ref[1][idx] if what == "g" else ref[2][idx])
    w = REPORT.setdefault(T.ITEMS[k][0].fn, [0.0, 0.0])
    w[0] = max(w[0], T.err(got, m))
    if m != 0:
        w[1] = max(w[1], abs(got - m) / abs(m))


def check(k, bad, outputs, dual=False):
    """outputs: (what, idx, got) triples of item k against the table, at the device bound."""
    c, p = T.ITEMS[k]
    want = T.expected(k)
    for what, idx, got in outputs:
        got = float(got)
        token = T.expected_dual(k)[idx] if dual and what == "g" else want[what] if idx is None else want[what][idx]
        msg = T.check_token(got, token, T.resolve(token, k, what, idx), T.DEVICE_BOUND)
        if msg:
            bad.append(f"{c.name} at {p.z} {'dual ' if dual else ''}{what}{'' if idx is None else idx}: {msg}")
        if what != "unused":
            note(k, got, what, idx)


def step_outputs(ap, t, terminal=False):
    """The hyper-dual outputs the kernel wrote for step t: value, gradient and (mirrored) Hessian."""
    yield "v", None, ap.q_array[t]
    Q = ap.Q_array[t]
    yield from (("g", i, ap.q_vec_array[t][i]) for i in range(2))
    yield from (("H", (0, 0), Q[0, 0]), ("H", (0, 1), Q[0, 1]), ("H", (0, 1), Q[1, 0]), ("H", (1, 1), Q[1, 1]))
    if not terminal:
        yield "g", 2, ap.r_array[t][0]
        yield from (("H", (0, 2), ap.P_array[t][0, 0]), ("H", (1, 2), ap.P_array[t][0, 1]), ("H", (2, 2), ap.R_array[t][0, 0]))


def trajectory(ids, h_item, clean=(), nan_ok=()):
    """x (N + 1, 2) and u (N, 1): row k holds the point of item ids[k] (its safe point for the items in `clean`), the last row the point
    of h's item.  An item with a NaN value is at its safe point unless named in `nan_ok`."""
    N = len(ids)
    x, u = np.zeros((N + 1, 2)), np.zeros((N, 1))
    for t, k in enumerate(ids):
        z = point(k, clean=k in clean or (T.value_is_nan(k) and k not in nan_ok))
        x[t], u[t, 0] = z[:2], z[2]
    z = point(h_item, clean=h_item in clean or (T.value_is_nan(h_item) and h_item not in nan_ok))
    x[N] = z[:2]
    return x, u, [float(h_item), z[2]]


@pytest.mark.parametrize("chunk", range(len(T.chunks())))
def test_hyper_dual_outputs_of_the_cost_over_the_table(chunk):
    ids = list(T.chunks()[chunk])
    N = len(ids)
    singular = [k for k in ids if T.ITEMS[k][1].kind == "singular"]
    finite_value = [k for k in singular if not T.value_is_nan(k)]
    h_regular = next((k for k in ids if T.ITEMS[k][1].kind == "regular"), 0)      # the last chunk is singular throughout: item 0 for h
    h_singular = finite_value[0] if finite_value else h_regular
    prob = rat.DeviceSourceProblem(T.c_source(ids, extra=[h_regular]), 2, 1, N, 1e-3 * np.eye(2), params=[float(h_regular), 0.0])
    ctx = rat.Context(prob)

    def run(h_item, **kw):
        x, u, p = trajectory(ids, h_item, **kw)
        ctx.set_params(p)
        return ctx.approximate_model(u, x)

    # every point of the table at once: a non-finite partial beside a finite (or infinite) value raises nothing
    ap = run(h_singular)
    bad, ran = [], 0
    for t, k in enumerate(ids):
        if not T.value_is_nan(k):
            check(k, bad, step_outputs(ap, t))
            ran += 1
    check(h_singular, bad, step_outputs(ap, N, terminal=True))
    # the same trajectory with every singular point replaced by a regular one: the other steps do not change by a bit
    ap_clean = run(h_regular, clean=set(singular))
    check(h_regular, bad, step_outputs(ap_clean, N, terminal=True))
    keep = np.array([k not in singular for k in ids])
    for name in ARRAYS:
        a, b = getattr(ap, name)[:N][keep], getattr(ap_clean, name)[:N][keep]
        assert np.all(np.isfinite(b)) and np.array_equal(a, b), name
    # a NaN value is the DomainError it always was: in c at that step alone, and in h
    for k in singular:
        if T.value_is_nan(k):
            with pytest.raises(ArithmeticError):
                run(h_regular, clean=set(singular) - {k}, nan_ok={k})
            with pytest.raises(ArithmeticError):
                run_h_nan(ctx, ids, k, singular)
            ran += 1
    assert ran == N
    assert not bad, "\n".join(bad)


def run_h_nan(ctx, ids, k, singular):
    """Every step at a regular point, h on the NaN-valued item k."""
    x, u, _ = trajectory(ids, k, clean=set(singular))
    z = T.ITEMS[k][1].z
    x[len(ids)] = z[:2]
    ctx.set_params([float(k), z[2]])
    return ctx.approximate_model(u, x)


def test_dual_outputs_of_the_dynamics_over_the_table():
    n, m, N = 12, 4, T.CHUNK
    prob = rat.DeviceSourceProblem(T.f_source(), n, m, N, 1e-3 * np.eye(n), params=[0.0])
    ctx = rat.Context(prob)
    bad, ran = [], 0
    for ids in T.chunks():
        x, u = np.zeros((N + 1, n)), np.zeros((N, m))
        x[:, 2] = -1.0                                                 # no row
        for t, k in enumerate(ids):
            if not T.value_is_nan(k):
                z = T.ITEMS[k][1].z
                x[t, :2], x[t, 2], u[t, 0] = z[:2], t, z[2]
        ctx.set_params([float(ids[0])])
        ap = ctx.approximate_model(u, x)
        for t in range(N):
            row = t % n
            J = np.hstack([ap.A_array[t], ap.B_array[t]])
            other = np.delete(J, row, axis=0)
            assert np.all(other == 0), t                               # the rows no item writes
            if t >= len(ids) or T.value_is_nan(ids[t]):
                assert np.all(J == 0), t
                continue
            k = ids[t]
            check(k, bad, [("g", 0, J[row, 0]), ("g", 1, J[row, 1]), ("g", 2, J[row, n])], dual=True)
            unused = np.delete(J[row], [0, 1, n])
            if T.ITEMS[k][1].kind == "regular":
                assert np.all(unused == 0), (T.ITEMS[k][0].name, t)    # the columns of the variables the item does not read: exactly zero
            for g in unused:
                check(k, bad, [("unused", None, g)], dual=True)
            ran += 1
    assert ran == sum(not T.value_is_nan(k) for k in range(len(T.ITEMS)))
    assert not bad, "\n".join(bad)


def test_report():
    """Printed, not asserted: per function the worst device error in the project's metric and relative to |want| alone (the saturated
    tails of tanh, the curvature of x / x at 1e-100)."""
    print("function            worst |err| / max(1, |want|)   worst |err| / |want|   (device)")
    for fn in sorted(REPORT):
        print(f"{fn:18s}  {REPORT[fn][0]:.2e}                       {REPORT[fn][1]:.2e}")
