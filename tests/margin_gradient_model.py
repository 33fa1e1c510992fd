"""NumPy model of rat_policy_margin_gradient (csrc/source_margin_adjoint.h, the arg-max sibling of ev_eval, tlt_weights on a sample of
margins, pg_moments and pg_final of csrc/policy_mc.hip) -- test aid, shared by tests/test_cpu_margin_gradient.py,
tests/test_gpu_margin_gradient.py and tools/policy_margin_gradient_bench.py.

Built on tests/policy_gradient_model.py: its cases (ScalarLQ, Pendulum, LqCubic, Lin2 with their hand-written Jacobians), its rollout on
the device generator's draws and its `gradient` (the self-normalised sums, the standard error, the rollouts left out), and on the tail
weights of tests/tail_scenarios_model.py.  What is new is the seed of the adjoint: per rollout k and event i

    M_ik = max over the window of g_i(t, z_t),  g_i(t, z) = z' Q_i z + a_i' z + b_i,  z = (x_t, u_t), u_N = 0
    t*   = the first step of the window that attains it (a NaN g is passed over: only a strictly greater value replaces the running one)
    at t*:   g_z = (Q_i + Q_i') z + a_i;   t* < N: gu_t* = its u part, lambda_t* = its x part + L_t*' gu_t*;   t* = N: lambda_N = its x part
    t > t*:  gu_t = 0
    t < t*:  g_t = f_z' lambda_{t+1};   gu_t = its u part;   lambda_t = its x part + L_t' gu_t   (open loop: the x part alone)

An event is (Q or None, a, b, t_lo, t_hi) over the d = n + m coordinates, as Event.dense returns it.  dtype = np.longdouble runs the
rollout, g, the adjoint and the sums in extended precision on the same draws; the tail's cut comes from the margins rounded to float64
(as policy_gradient_model takes it from the float64 costs), so the two runs put the weight on the same rollouts unless a margin sits
within a rounding of the cut -- `same_selection` says whether they did, and the tests choose seeds for which they do."""
import numpy as np

import policy_gradient_model as pg
from tail_scenarios_model import tail_weights


def g_values(xs, us, events):
    """g [K, N+1, E] in xs.dtype, and z [K, N+1, d]"""
    K, T, n = xs.shape
    m = us.shape[2]
    z = np.zeros((K, T, n + m), dtype=xs.dtype)
    z[:, :, :n] = xs
    z[:, :T - 1, n:] = us
    g = np.zeros((K, T, len(events)), dtype=xs.dtype)
    with np.errstate(all="ignore"):
        for e, (Q, a, b, lo, hi) in enumerate(events):
            g[:, :, e] = (z * np.asarray(a, float).astype(xs.dtype)).sum(axis=2) + xs.dtype.type(b)
            if Q is not None:
                Qd = np.asarray(Q, float).astype(xs.dtype)
                g[:, :, e] = g[:, :, e] + ((z @ Qd.T) * z).sum(axis=2)
    return g, z


def margins(g, events, ok):
    """(M [E, K], tstar [E, K]): ev_eval's rule -- M starts NaN; g replaces it if g > M or M is NaN; t* moves when a number comes in.
    A rollout that is not ok: NaN, -1"""
    K, T, E = g.shape
    M = np.full((E, K), np.nan, dtype=g.dtype)
    ts = np.full((E, K), -1, dtype=np.int64)
    with np.errstate(all="ignore"):
        for e, (Q, a, b, lo, hi) in enumerate(events):
            for t in range(int(lo), int(hi) + 1):
                gv = g[:, t, e]
                rep = (gv > M[e]) | np.isnan(M[e])
                ts[e] = np.where(rep & ~np.isnan(gv), t, ts[e])
                M[e] = np.where(rep, gv, M[e])
    M[:, ~ok] = np.nan
    ts[:, ~ok] = -1
    return M, ts


def adjoint(case, xs, us, z, L, event, tstar):
    """(gu (K, N, m), finite (K,)) of one event: dM_k / du_t with the loop closed downstream, and whether g_z at t* and every g_t below
    it are finite; a rollout with tstar = -1 is all zeros and finite"""
    K, N, n = us.shape[0], us.shape[1], xs.shape[2]
    dt = xs.dtype
    Q, a = event[0], np.asarray(event[1], float).astype(dt)
    Lq = None if L is None else np.asarray(L, float).astype(dt)
    gu = np.zeros((K, N, case.m), dtype=dt)
    fin = np.ones(K, dtype=bool)
    lam = np.zeros((K, n), dtype=dt)
    has = tstar >= 0
    zs = z[np.arange(K), np.where(has, tstar, 0)]                     # z at t*
    with np.errstate(all="ignore"):
        gz = np.broadcast_to(a, zs.shape).copy()
        if Q is not None:
            Qd = np.asarray(Q, float).astype(dt)
            gz = gz + zs @ (Qd + Qd.T).T
        at_N = has & (tstar == N)
        fin &= ~has | (np.isfinite(gz[:, :n]).all(axis=1) & (at_N | np.isfinite(gz[:, n:]).all(axis=1)))
        lam = np.where(at_N[:, None], gz[:, :n], lam)
        for t in range(N - 1, -1, -1):
            x, u = xs[:, t], us[:, t]
            below, here = has & (t < tstar), has & (t == tstar)
            gx = (case.fx(x, u) * lam[:, :, None]).sum(axis=1)
            g_u = (case.fu(x, u) * lam[:, :, None]).sum(axis=1)
            gx = np.where(below[:, None], gx, np.where(here[:, None], gz[:, :n], 0))
            g_u = np.where(below[:, None], g_u, np.where(here[:, None], gz[:, n:], 0))
            fin &= np.isfinite(gx).all(axis=1) & np.isfinite(g_u).all(axis=1)
            gu[:, t] = g_u
            lam = gx if L is None else gx + g_u @ Lq[t]
    return gu, fin


def model(case, x_nom, l, L, K, seed, events, alphas, dtype=np.float64, tstar=None):
    """The whole call: dict(J, x, u, M (E, K), tstar (E, K), and per event i lists gu, fin, y, dead, info, grad_l, grad_L, grad_l_se,
    n_nonfinite, se_scale).  tstar (E, K): take these arg-max steps instead of the run's own (the device's, say)"""
    N = np.asarray(l).shape[0]
    zd = pg.draws(case, seed, K, N)
    J, xs, us = pg.rollout(case, x_nom, l, L, zd, dtype)
    ok = ~np.isnan(np.asarray(J, float))
    g, z = g_values(xs, us, events)
    M, ts = margins(g, events, ok)
    if tstar is not None:
        ts = np.asarray(tstar)
    out = dict(J=J, x=xs, u=us, g=g, M=M, tstar=ts, gu=[], fin=[], y=[], dead=[], info=[], grad_l=[], grad_L=[], grad_l_se=[], n_nonfinite=[],
               se_scale=[])
    for e, ev in enumerate(events):
        gu, fin = adjoint(case, xs, us, z, L, ev, ts[e])
        y, dead, info = tail_weights(M[e].astype(np.float64), alphas, dtype=dtype)
        gl, gL, se, nf, sc = pg.gradient(gu, fin, xs, x_nom, L, y, dead, M[e])
        for k, v in (("gu", gu), ("fin", fin), ("y", y), ("dead", dead), ("info", info), ("grad_l", gl), ("grad_L", gL), ("grad_l_se", se),
                     ("n_nonfinite", nf), ("se_scale", sc)):
            out[k].append(v)
    return out


def same_selection(m64, mld):
    """whether two runs of `model` took the same arg-max steps and put weight on the same rollouts, in every event and level"""
    if not np.array_equal(m64["tstar"], mld["tstar"]):
        return False
    return all(np.array_equal(a != 0, b != 0) for a, b in zip(m64["y"], mld["y"]))


# ---- the events the tests use, in the coordinates of a case ---------------------------------------------------------------------------------
def linear_event(case, N, seed, t):
    """a half-space with a window of one step"""
    r = np.random.default_rng(seed)
    return (None, r.standard_normal(case.n + case.m), float(r.standard_normal()), t, t)


def quadratic_event(case, N, seed, lo=0, hi=None):
    """z' Q z + a' z + b with a Q that is not symmetric, over lo .. hi (the whole horizon by default)"""
    r = np.random.default_rng(seed)
    d = case.n + case.m
    Q = 0.3 * r.standard_normal((d, d))
    return (Q, 0.5 * r.standard_normal(d), float(0.2 * r.standard_normal()), lo, N if hi is None else hi)


def four_events(case, N):
    """two linear and two quadratic events, windows of one step and longer ones"""
    return [linear_event(case, N, 21, N), quadratic_event(case, N, 22), linear_event(case, N, 23, 0) if N < 2 else
            (None,) + linear_event(case, N, 23, 0)[1:3] + (0, N - 1), quadratic_event(case, N, 24, lo=min(1, N), hi=N)]


def to_rat(rat, ev):
    """the model's event as Context.policy_events takes it"""
    Q, a, b, lo, hi = ev
    return rat.halfspace(a, b, (lo, hi)) if Q is None else rat.quadratic_event(Q, a, b, (lo, hi))


# ---- a source whose f has an infinite derivative at u == 0 and a finite value: x+ = a x + b u + sqrt(|u|) / 8 + w -----------------------
SQRT_DYN = pg.SCALAR_LQ.replace("xn[0] = p[0] * x[0] + p[1] * u[0];", "xn[0] = p[0] * x[0] + p[1] * u[0] + 0.125 * sqrt(fabs(u[0]));").replace(
    "w[0] = p[5] * rng.normal();", "const double z = rng.normal();\n    w[0] = (z > 0.0) ? p[5] * z : 0.0;")


class SqrtDyn(pg.ScalarLQ):
    source = SQRT_DYN

    def f(self, x, u): return self.p[0] * x + self.p[1] * u + 0.125 * np.sqrt(np.abs(u))

    def fu(self, x, u):
        with np.errstate(all="ignore"):
            return (self.p[1] + 0.125 * np.where(np.signbit(u), -1.0, 1.0) * (0.5 / np.sqrt(np.abs(u))))[:, :, None]

    def noise(self, z): return np.where(z > 0.0, self.p[5] * z, 0.0)


def sqrt_dyn_setup():
    """(case, policy): half of the rollouts draw w_0 = 0, reach x_1 = x_nom_1 exactly and apply u_1 = 0, where f_u is Inf"""
    case = SqrtDyn([0.5, 0.5, 0.0, 0.0, 1.0, 0.3])
    pol = (np.array([[1.0], [1.125], [0.0]]), np.array([[1.0], [0.0]]), np.array([[[0.5]], [[0.5]]]))
    return case, pol


# ---- the cases tests/test_gpu_margin_gradient.py holds the device against; tests/test_cpu_margin_gradient.py checks, without a device,
# that on every one of them the float64 and the longdouble model take the same arg-max steps and the same tail sets -------------------------
SEED, ALPHAS, KS = 11, [0.0, 0.9], (1, 3, 4, 5, 63, 64, 65)
CASES = [("scalar", lambda: pg.ScalarLQ(), 1), ("pend3", lambda: pg.Pendulum(), 3), ("lq5x3", lambda: pg.LqCubic(5, 3, 2), 2),
         ("lq12x4", lambda: pg.LqCubic(12, 4, 3), 3)]
_cache = {}


def reference(key, case, pol, K, events, alphas=ALPHAS, seed=SEED):
    """the float64 and the longdouble model of one case, computed once per process"""
    if key not in _cache:
        _cache[key] = tuple(model(case, *pol, K, seed, events, alphas, dtype=dt) for dt in (np.float64, np.longdouble))
    return _cache[key]
