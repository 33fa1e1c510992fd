"""Host-side mirror of the reference's ``src/ileqg.jl`` API over the C ABI (include/ratilqr.h).

Same names as the reference's exports (src/RATiLQR.jl:20-53); Julia's ``f!`` becomes ``f_``.
Greek keyword arguments are spelled out (``mu_min`` for μ_min, ``Delta_0`` for Δ_0, ``lam`` for λ,
``eps_init`` for ϵ_init ...).  Array conventions on the Python side: a ``Vector{Vector}`` is a 2-D
array ``[t, i]``, a ``Vector{Matrix}`` a 3-D array ``[t, row, col]``.

All numerics run in libratilqr_hip.so on the GPU.  ``solve_`` / batched solves use the fused device
state machine; ``initialize_`` / ``step_`` / ``line_search_`` compose the operator entry points exactly
as the reference composes its functions, so the unit tests of test/ileqg_test.jl can be restated 1:1.
"""
from __future__ import annotations

import ctypes as C
import weakref
from dataclasses import dataclass

import numpy as np

from . import _native as nv
from .problems import MODEL_SOURCE, FiniteHorizonRiskSensitiveOptimalControlProblem

SQRT_EPS = 1.4901161193847656e-8


class UserNoise:
    """The disturbance of Context.policy_evaluate_noise / evaluate_policy(..., noise=): what the source's rat_user_noise draws per step
    (normals_per_step, uniforms_per_step: the most rng.normal() / rng.uniform() calls of one step) and where the draws come from --
    injected streams zn (K, N, normals_per_step) and zu (K, N, uniforms_per_step), every declared one, or the device generator keyed
    by seed."""

    def __init__(self, normals_per_step, uniforms_per_step=0, zn=None, zu=None, seed=0):
        self.normals_per_step, self.uniforms_per_step = int(normals_per_step), int(uniforms_per_step)
        self.zn = None if zn is None else nv.f64(zn)
        self.zu = None if zu is None else nv.f64(zu)
        self.seed = int(seed)


class ParamSampling:
    """Model parameters drawn per rollout (Context.set_param_sampling, rat_policy_params_sampling): what the source's rat_user_params
    draws for one rollout (param_normals, param_uniforms: the most rng.normal() / rng.uniform() calls of the hook) and where the draws
    come from -- injected streams zpn (K, param_normals) and zpu (K, param_uniforms), every declared one, rollout j reading row j
    whatever K a later call has (no more than the streams hold), or the device generator keyed by each call's seed."""

    def __init__(self, param_normals, param_uniforms=0, zpn=None, zpu=None):
        self.param_normals, self.param_uniforms = int(param_normals), int(param_uniforms)
        self.zpn = None if zpn is None else nv.f64(zpn)
        self.zpu = None if zpu is None else nv.f64(zpu)


class SobolGroup:
    """One group of random inputs of Context.policy_sobol (rat_policy_sobol): the draw indices it holds -- param_normals /
    param_uniforms: the i-th rng.normal() / rng.uniform() of the source's rat_user_params; step_normals / step_uniforms: the i-th
    rng.normal() / rng.uniform() of rat_user_noise at every step -- as four 64-bit masks (`words`, in the order of the C ABI's
    RAT_SB_G_*).  Indices are 0 .. 63; groups of one call must be disjoint (check_groups)."""

    def __init__(self, param_normals=(), param_uniforms=(), step_normals=(), step_uniforms=(), name=None):
        self.name = name
        self.words = tuple(self._mask(ix, what) for ix, what in ((param_normals, "param_normals"), (param_uniforms, "param_uniforms"),
                                                                  (step_normals, "step_normals"), (step_uniforms, "step_uniforms")))

    @staticmethod
    def _mask(indices, what):
        mask = 0
        for i in np.atleast_1d(np.asarray(indices, dtype=np.int64)).ravel():
            if not 0 <= int(i) < 64:
                raise ValueError(f"SobolGroup: {what} index {int(i)} is outside 0 .. 63")
            mask |= 1 << int(i)
        return mask

    @staticmethod
    def check_groups(groups, normals_per_step, uniforms_per_step, param_normals=0, param_uniforms=0):
        """What rat_policy_sobol asks of the groups, on the host: 1 .. 16 of them, no index at or beyond its declared count, no draw in
        two groups.  Raises ValueError naming the group."""
        groups = list(groups)
        if not 1 <= len(groups) <= nv.SB_MAX_GROUPS:
            raise ValueError("policy_sobol takes 1 .. 16 groups")
        counts, seen = (param_normals, param_uniforms, normals_per_step, uniforms_per_step), [0, 0, 0, 0]
        for gi, g in enumerate(groups):
            for k in range(4):
                if g.words[k] >> int(counts[k]):
                    raise ValueError(f"policy_sobol: group {gi} names a draw at or beyond the declared count ({int(counts[k])})")
                if g.words[k] & seen[k]:
                    raise ValueError(f"policy_sobol: group {gi} overlaps an earlier group: groups must be disjoint")
                seen[k] |= g.words[k]
        return np.array([g.words for g in groups], dtype=np.uint64)


def explained_share(cov_q, cov_qJ, tilt_var):
    """The linear share of the cost's variance that each parameter explains under a row's distribution, from the outputs of
    Context.policy_worst_case_params: cov_qJ[i]^2 / (cov_q[i, i] tilt_var) -- the squared correlation of q_i with J.  cov_q (R, P, P),
    cov_qJ (R, P), tilt_var (R,); (R, P), NaN where a parameter or the cost does not vary."""
    cov_q, cov_qJ, tilt_var = np.asarray(cov_q, float), np.asarray(cov_qJ, float), np.asarray(tilt_var, float)
    with np.errstate(all="ignore"):
        share = cov_qJ ** 2 / (np.diagonal(cov_q, axis1=-2, axis2=-1) * tilt_var[..., None])
    return np.where(np.isfinite(share), share, np.nan)


class Event:
    """A safety event of Context.policy_events: g(t, z) = z' Q z + a' z + b of z = (x_t, u_t), violated where g > 0 at a step of the window.
    Build one with halfspace, ball or quadratic_event.  Q (or None: linear) and a are given over (x, u) -- n + m entries -- or over x
    alone; steps is None (the whole horizon 0 .. N), one step t, or (t_lo, t_hi)."""

    def __init__(self, Q, a, b, steps=None):
        self.Q = None if Q is None else np.asarray(Q, dtype=np.float64)
        self.a = np.atleast_1d(np.asarray(a, dtype=np.float64)).ravel()
        self.b = float(b)
        self.steps = steps

    def dense(self, n, m, N):
        """(Q (d, d) or None, a (d,), b, t_lo, t_hi) over d = n + m coordinates"""
        d = n + m
        if self.a.size not in (n, d):
            raise ValueError(f"an event's a has {self.a.size} entries: n = {n} or n + m = {d} are served")
        a = np.zeros(d)
        a[:self.a.size] = self.a
        Q = None
        if self.Q is not None:
            if self.Q.shape not in ((n, n), (d, d)):
                raise ValueError(f"an event's Q is {self.Q.shape}: ({n}, {n}) or ({d}, {d}) are served")
            Q = np.zeros((d, d))
            Q[:self.Q.shape[0], :self.Q.shape[1]] = self.Q
        if self.steps is None:
            lo, hi = 0, N
        elif np.ndim(self.steps) == 0:
            lo = hi = int(self.steps)
        else:
            lo, hi = (int(v) for v in self.steps)
        return Q, a, self.b, lo, hi


def halfspace(a, b, steps=None):
    """The event a' z + b > 0 (a lane edge, an actuator limit): a over (x, u) or over x alone."""
    return Event(None, a, b, steps)


def quadratic_event(Q, a, b, steps=None):
    """The event z' Q z + a' z + b > 0; Q is used as given (not symmetrised), over (x, u) or over x alone."""
    return Event(Q, a, b, steps)


def ball(idx, centre, radius, steps=None):
    """The event of being INSIDE the ball of that radius about `centre` in the coordinates idx of (x, u) -- a circular obstacle:
    g = radius^2 - |z[idx] - centre|^2."""
    idx = [int(i) for i in np.atleast_1d(idx)]
    c = np.atleast_1d(np.asarray(centre, dtype=np.float64)).ravel()
    if c.size != len(idx):
        raise ValueError("ball: one centre entry per index")
    d = max(idx) + 1
    Q, a = np.zeros((d, d)), np.zeros(d)
    for i, ci in zip(idx, c):
        Q[i, i] = -1.0
        a[i] = 2.0 * ci
    return _BallEvent(Q, a, float(radius) ** 2 - float(c @ c), steps)


class _BallEvent(Event):
    """ball's event: Q and a reach as far as the largest index, and are padded to n + m whatever that is"""

    def dense(self, n, m, N):
        d, k = n + m, self.a.size
        if k > d:
            raise ValueError(f"ball: index {k - 1} is beyond the {d} coordinates of (x, u)")
        Q, a = np.zeros((d, d)), np.zeros(d)
        Q[:k, :k], a[:k] = self.Q, self.a
        return Event(Q, a, self.b, self.steps).dense(n, m, N)


def kl_event_bound(p, d):
    """rat_kl_event_bound: the largest probability an event of probability p can have within KL radius d of the sampling distribution
    (host only: no GPU needed)."""
    out = C.c_double()
    nv.check(nv.lib().rat_kl_event_bound(C.c_double(float(p)), C.c_double(float(d)), C.byref(out)))
    return out.value


@dataclass
class RareEventResult:
    """What Context.policy_rare_event / policy_rare_event_noise return: the RAT_RE_* slots of the header as fields (flag: 0 OK, 1 the level
    never reached 0, 2 no OK rollout, 3 non-finite), the shift (N, n) -- (N, normals_per_step) under user noise -- the final pass ran under, the trace (n_iter, 4) -- level, elite count, elite effective sample
    size, |shift| per adaptation iteration, NaN where none ran -- and, on request, the margins and log-weights (K,) of the final pass."""
    prob: float
    prob_se: float
    ess: float
    n_viol: int
    n_ok: int
    n_domain: int
    logw_max: float
    logw_min: float
    flag: int
    n_iter: int
    level: float
    shift: np.ndarray
    trace: np.ndarray
    margins: np.ndarray | None = None
    logw: np.ndarray | None = None
    param_shift: np.ndarray | None = None                             # policy_rare_event_params alone: (param_normals,)
    param_trace: np.ndarray | None = None                             # ... and (n_iter,): |param_shift| after every iteration that updated


class Context:
    """One rat_handle bound to one problem (device buffers sized for max_batch samples x spec_eps step sizes)."""

    def __init__(self, problem, opts: nv.IleqgOpts | None = None, max_batch=1, spec_eps=1, device=0):
        """problem None: a handle without an iLEQG problem (PETS on a generative source model sets its own)."""
        L = nv.lib()
        self.problem = problem
        self.n, self.m, self.N = (problem.n, problem.m, problem.N) if problem is not None else (0, 0, 0)
        self.max_batch, self.spec_eps, self.device = int(max_batch), int(spec_eps), int(device)
        self.h = C.c_void_p()
        nv.check(L.rat_create(C.byref(opts) if opts is not None else None, self.max_batch, self.spec_eps,
                              self.device, C.byref(self.h)))
        self._fin = weakref.finalize(self, L.rat_destroy, self.h)
        self._param_normals = 0                                       # param_normals of the handle's parameter sampling (0: off)
        self._param_uniforms = 0
        self._keep = self._upload(problem) if problem is not None else None

    def _upload(self, problem):
        self._param_normals = self._param_uniforms = 0                # (rat_problem_set_source switches parameter sampling off)
        if getattr(problem, "model", 0) == MODEL_SOURCE:            # user-written f, c, h: compiled at run time (rat_problem_set_source)
            keep = nv.set_source(self.h, problem)
            self.params = keep["params"].copy()                       # what this handle's kernels read (set_params changes it)
            return keep
        desc, keep = nv.make_desc(problem)
        nv.check(nv.lib().rat_problem_set(self.h, C.byref(desc)))
        return keep

    def set_opts(self, opts):
        nv.check(nv.lib().rat_set_ileqg_opts(self.h, C.byref(opts)))

    def set_problem(self, problem):
        """Re-bind the handle to another problem of the same model families (rat_problem_set on the live handle: device buffers are
        kept when n, m, N are unchanged -- the receding-horizon pattern of re-setting the tables every control step)."""
        keep = self._upload(problem)
        self.problem, self._keep = problem, keep
        self.n, self.m, self.N = problem.n, problem.m, problem.N

    def set_params(self, params):
        """New parameter values of this handle's source problem (rat_problem_set_params: the same count, no recompilation).  They hold for
        this handle only: the problem object keeps its own `params`, which every other handle -- and this one, when the problem is set
        again -- uploads."""
        p = nv.f64(np.atleast_1d(params))
        nv.check(nv.lib().rat_problem_set_params(self.h, nv.P(p) if p.size else None, C.c_int64(p.size)))
        self.params = p.copy()

    def set_param_sampling(self, ps):
        """Switch per-rollout model parameters on (a ParamSampling) or off (None, the default) for this handle
        (rat_policy_params_sampling): with sampling on, policy_evaluate_noise, the rare-event calls under user noise and the replays
        behind policy_evaluate_noise call the source's rat_user_params once per rollout.  Injected streams are copied by the call."""
        if ps is None:
            nv.check(nv.lib().rat_policy_params_sampling(self.h, C.c_int32(0), C.c_int32(0), None, None, C.c_int64(0)))
            self._param_normals = self._param_uniforms = 0
            return
        if not isinstance(ps, ParamSampling):
            raise TypeError("set_param_sampling needs a ParamSampling or None")
        pn, pu, K = ps.param_normals, ps.param_uniforms, 0
        for z, per, name in ((ps.zpn, pn, "zpn"), (ps.zpu, pu, "zpu")):
            if z is not None and per > 0:
                if z.size % per:
                    raise ValueError(f"{name} holds {z.size} draws: no multiple of {per}")
                if K and z.size // per != K:
                    raise ValueError("zpn and zpu hold different numbers of rollouts")
                K = z.size // per
        nv.check(nv.lib().rat_policy_params_sampling(self.h, C.c_int32(pn), C.c_int32(pu), nv.P(ps.zpn), nv.P(ps.zpu), C.c_int64(K)))
        self._param_normals, self._param_uniforms = pn, pu

    def sample_params(self, K, seed=0):
        """The parameters rat_user_params draws for rollouts 0 .. K - 1 under `seed` (or the injected draws): (K, n_params), row j behind
        costs[j] of policy_evaluate_noise with that seed (rat_policy_params_sample)."""
        K = int(K)
        np_ = getattr(self, "params", np.zeros(0)).size
        q = np.zeros((max(K, 0), np_))
        nv.check(nv.lib().rat_policy_params_sample(self.h, C.c_int64(K), C.c_uint64(int(seed)), nv.P(q)))
        return q

    # ---- operator forms --------------------------------------------------------------------------
    def rollout_open(self, x0, u):
        x = np.zeros((self.N + 1, self.n))
        dom = C.c_int32()
        nv.check(nv.lib().rat_rollout_open(self.h, nv.P(nv.f64(x0)), nv.P(nv.f64(u)), nv.P(x), C.byref(dom)))
        if dom.value:
            raise ArithmeticError("DomainError in simulate_dynamics")
        return x

    def rollout_feedback(self, xbar, l, L):
        xn, un = np.zeros((self.N + 1, self.n)), np.zeros((self.N, self.m))
        dom = C.c_int32()
        nv.check(nv.lib().rat_rollout_feedback(self.h, nv.P(nv.f64(xbar)), nv.P(nv.f64(l)), nv.P(nv.cm3(L)),
                                               nv.P(xn), nv.P(un), C.byref(dom)))
        if dom.value:
            raise ArithmeticError("DomainError in simulate_dynamics")
        return xn, un

    def rollout_noisy(self, x_nom, l, L=None, K=None, z=None, seed=0, want_x=True, want_u=True):
        """K Monte-Carlo rollouts under process noise w ~ N(0, W(k)) (ileqg.jl:44-55 open loop with L=None and x_nom = x_0,
        :94-109 under the affine policy).  z: injected N(0,1) draws of shape (K, N, n), or None for the device generator.
        Returns x (K, N+1, n), u (K, N, m), cost (K,) -- x/u are None when not wanted."""
        if z is not None:
            z = nv.f64(z)
            K = z.shape[0]
        K = int(K)
        x = np.zeros((K, self.N + 1, self.n)) if want_x else None
        u = np.zeros((K, self.N, self.m)) if want_u else None
        cost = np.zeros(K)
        dom = C.c_int32()
        nv.check(nv.lib().rat_rollout_noisy(self.h, nv.P(nv.f64(x_nom)), nv.P(nv.f64(l)), nv.P(nv.cm3(L)) if L is not None else None,
                                            C.c_int64(K), nv.P(z), C.c_uint64(int(seed)), nv.P(x), nv.P(u), nv.P(cost), C.byref(dom)))
        return x, u, cost, bool(dom.value)

    def policy_evaluate(self, x_nom, l, L=None, thetas=(), K=None, z=None, seed=0, want_costs=False):
        """Monte-Carlo evaluation of a policy (rat_policy_evaluate): the K rollouts of rollout_noisy -- open loop with L=None and
        x_nom = x_0, or under u = l + L (x - x_nom) -- for a problem of any model kind, source models included, with the statistics of
        the K costs formed on the device.  thetas: up to 16 risk parameters >= 0.  Returns a dict: n_ok, n_domain (rollouts that hit a
        DomainError: left out of every statistic), mean, var (unbiased), min, max, se_mean, risk[i] = (1/theta_i) log mean exp(theta_i J)
        (the mean at theta_i = 0), risk_se[i] (delta method), costs ((K,), NaN for a DomainError rollout; None unless want_costs)."""
        if z is not None:
            z = nv.f64(z)
            K = z.shape[0]
        if K is None:
            raise ValueError("policy_evaluate needs K= or z=")
        K = int(K)
        th = nv.f64(np.atleast_1d(np.asarray(thetas, dtype=np.float64))).ravel()
        stats, risk, se = np.zeros(nv.MC_NSTAT), np.zeros(th.size), np.zeros(th.size)
        costs = np.zeros(max(K, 0)) if want_costs else None
        nv.check(nv.lib().rat_policy_evaluate(self.h, nv.P(nv.f64(x_nom)), nv.P(nv.f64(l)), nv.P(nv.cm3(L)) if L is not None else None,
                                              C.c_int64(K), nv.P(z), C.c_uint64(int(seed)), nv.P(th) if th.size else None,
                                              C.c_int32(th.size), nv.P(stats), nv.P(risk) if th.size else None,
                                              nv.P(se) if th.size else None, nv.P(costs)))
        return dict(n_ok=int(stats[nv.MC_N_OK]), n_domain=int(stats[nv.MC_N_DOMAIN]), mean=float(stats[nv.MC_MEAN]),
                    var=float(stats[nv.MC_VAR]), min=float(stats[nv.MC_MIN]), max=float(stats[nv.MC_MAX]),
                    se_mean=float(stats[nv.MC_SE_MEAN]), risk=risk, risk_se=se, costs=costs)

    def policy_evaluate_noise(self, x_nom, l, L=None, noise=None, thetas=(), K=None, want_costs=False, want_trajectories=False):
        """policy_evaluate for a source problem under the disturbance its own rat_user_noise draws (rat_policy_evaluate_noise): noise is
        a UserNoise.  K defaults to the rollouts an injected stream holds.  The same dict, and with want_trajectories x (K, N+1, n) and
        u (K, N, m), rollout index first (None otherwise)."""
        if not isinstance(noise, UserNoise):
            raise TypeError("policy_evaluate_noise needs noise=UserNoise(...)")
        npn, npu = noise.normals_per_step, noise.uniforms_per_step
        if K is None:
            for z, per in ((noise.zn, npn), (noise.zu, npu)):
                if z is not None and per > 0 and self.N > 0:
                    K = z.size // (self.N * per)
                    break
        if K is None:
            raise ValueError("policy_evaluate_noise needs K= or an injected stream")
        K = int(K)
        for z, per, name in ((noise.zn, npn, "zn"), (noise.zu, npu, "zu")):
            if z is not None and per > 0 and z.size != K * self.N * per:
                raise ValueError(f"{name} holds {z.size} draws, K N per-step = {K * self.N * per}")
        th = nv.f64(np.atleast_1d(np.asarray(thetas, dtype=np.float64))).ravel()
        stats, risk, se = np.zeros(nv.MC_NSTAT), np.zeros(th.size), np.zeros(th.size)
        costs = np.zeros(max(K, 0)) if want_costs else None
        x = np.zeros((max(K, 0), self.N + 1, self.n)) if want_trajectories else None
        u = np.zeros((max(K, 0), self.N, self.m)) if want_trajectories else None
        nv.check(nv.lib().rat_policy_evaluate_noise(self.h, nv.P(nv.f64(x_nom)), nv.P(nv.f64(l)), nv.P(nv.cm3(L)) if L is not None else None,
                                                    C.c_int64(K), C.c_int32(npn), C.c_int32(npu), nv.P(noise.zn), nv.P(noise.zu),
                                                    C.c_uint64(noise.seed), nv.P(th) if th.size else None, C.c_int32(th.size), nv.P(stats),
                                                    nv.P(risk) if th.size else None, nv.P(se) if th.size else None, nv.P(costs), nv.P(x),
                                                    nv.P(u)))
        self._noise_open_loop = L is None                             # (policy_gradient returns grad_L None for it)
        return dict(n_ok=int(stats[nv.MC_N_OK]), n_domain=int(stats[nv.MC_N_DOMAIN]), mean=float(stats[nv.MC_MEAN]),
                    var=float(stats[nv.MC_VAR]), min=float(stats[nv.MC_MIN]), max=float(stats[nv.MC_MAX]),
                    se_mean=float(stats[nv.MC_SE_MEAN]), risk=risk, risk_se=se, costs=costs, x=x, u=u)

    def policy_worst_case(self, kl_bounds=(), thetas=(), costs=None, want_weights=False):
        """The worst-case expected cost sup { E_p[J] : KL(p || q) <= d } of a sample of Monte-Carlo costs (rat_policy_worst_case), by its
        one-dimensional dual searched on the device.  costs None: the costs the last policy_evaluate / policy_evaluate_noise on this
        context left on the device (or the ones an earlier call uploaded); otherwise K host values (NaN = DomainError rollout, left out).  kl_bounds: up to 16 radii d >= 0;
        thetas: up to 16 tilts >= 0.  Returns {"bounds": rows, "thetas": rows, "weights": (K,) or None}; rows is a dict of arrays keyed
        theta, kl, bound, bound_se, tilt_mean, tilt_var, ess, flag (int: 0 OK, 1 saturated, 2 empty, 3 non-finite), one entry per
        kl_bound / per theta.  weights: y_k / sum y at kl_bounds[0]'s theta* (thetas[0] without bounds), 0 at a DomainError rollout."""
        d = nv.f64(np.atleast_1d(np.asarray(kl_bounds, dtype=np.float64))).ravel()
        th = nv.f64(np.atleast_1d(np.asarray(thetas, dtype=np.float64))).ravel()
        K = 0
        if costs is not None:
            costs = nv.f64(costs).ravel()
            K = costs.size
        ob, ot = np.zeros((d.size, nv.WC_NSTAT)), np.zeros((th.size, nv.WC_NSTAT))
        w = None
        if want_weights:
            kw = K if costs is not None else int(self.debug_get("mc_cost_K"))
            w = np.zeros(max(kw, 1))
        nv.check(nv.lib().rat_policy_worst_case(self.h, nv.P(costs), C.c_int64(K), nv.P(d) if d.size else None, C.c_int32(d.size),
                                                nv.P(th) if th.size else None, C.c_int32(th.size), nv.P(ob) if d.size else None,
                                                nv.P(ot) if th.size else None, nv.P(w)))

        def rows(o):
            r = {k: o[:, i].copy() for i, k in enumerate(nv.WC_SLOTS)}
            r["flag"] = r["flag"].astype(np.int64)
            return r
        if w is not None and costs is None:
            w = w[:int(self.debug_get("mc_cost_K"))]
        return dict(bounds=rows(ob), thetas=rows(ot), weights=w)

    def policy_tail_risk(self, alphas, costs=None, want_weights=False):
        """The tail risk of a sample of Monte-Carlo costs (rat_policy_tail_risk): per level alpha in [0, 1) the alpha-quantile of the cost
        (value at risk) and the conditional value at risk, the mean of the worst (1 - alpha) share of the rollouts, by a radix select on
        the device.  costs None: the costs the last policy_evaluate / policy_evaluate_noise on this context left on the device (or the
        ones an earlier call of this method or of policy_worst_case uploaded); otherwise K host values (NaN = DomainError rollout, left
        out).  alphas: 1 to 16 levels.  Returns a dict of arrays, one entry per level: alpha, var, cvar, cvar_se, tail_n (= n - n alpha),
        ess, kl (of the tail distribution from the sample: cvar <= policy_worst_case(kl_bounds=[kl]) bound), flag (int: 0 OK, 1 saturated:
        the tail is thinner than one rollout, 2 empty, 3 non-finite); and weights: the tail distribution at alphas[0] ((K,), summing to
        one, 0 at a DomainError rollout; None unless want_weights)."""
        al = nv.f64(np.atleast_1d(np.asarray(alphas, dtype=np.float64))).ravel()
        K = 0
        if costs is not None:
            costs = nv.f64(costs).ravel()
            K = costs.size
        rows = np.zeros((al.size, nv.TR_NSTAT))
        w = None
        if want_weights:
            kw = K if costs is not None else int(self.debug_get("mc_cost_K"))
            w = np.zeros(max(kw, 1))
        nv.check(nv.lib().rat_policy_tail_risk(self.h, nv.P(costs), C.c_int64(K), nv.P(al) if al.size else None, C.c_int32(al.size),
                                               nv.P(rows), nv.P(w)))
        r = {k: rows[:, i].copy() for i, k in enumerate(nv.TR_SLOTS)}
        r["flag"] = r["flag"].astype(np.int64)
        if w is not None:
            w = w[:K if costs is not None else int(self.debug_get("mc_cost_K"))]
        r["weights"] = w
        return r

    def policy_worst_case_trajectory(self, kl_bounds=(), thetas=()):
        """What the worst case looks like (rat_policy_worst_case_trajectory): the mean and covariance of the state and the control at every
        step under the worst-case distribution p* ~ exp(theta* J) q of each KL radius -- and under the tilt of each given theta; theta = 0 is
        the nominal distribution q -- formed on the device by replaying the last policy_evaluate / policy_evaluate_noise of this context
        (device generator only).  Returns {"bounds": part, "thetas": part}; a part carries policy_worst_case's row keys and, with R rows,
        mean_x (R, N+1, n), cov_x (R, N+1, n, n), mean_u (R, N, m), cov_u (R, N, m, m), cov_xu (R, N, n, m).  Covariances are the
        population form (weights sum to one).  A saturated row holds the moments of the rollouts attaining the maximum; an empty or
        non-finite sample gives NaN."""
        d = nv.f64(np.atleast_1d(np.asarray(kl_bounds, dtype=np.float64))).ravel()
        th = nv.f64(np.atleast_1d(np.asarray(thetas, dtype=np.float64))).ravel()
        n, m, N, R = self.n, self.m, self.N, d.size + th.size
        rows, mean, cov = np.zeros((R, nv.WC_NSTAT)), np.zeros((R, N + 1, n + m)), np.zeros((R, N + 1, n + m, n + m))
        nv.check(nv.lib().rat_policy_worst_case_trajectory(self.h, nv.P(d) if d.size else None, C.c_int32(d.size), nv.P(th) if th.size else None,
                                                           C.c_int32(th.size), nv.P(rows), nv.P(mean), nv.P(cov)))
        return self._wc_parts(rows, d.size, lambda sl, r: self._unpack_trajectory(mean[sl], cov[sl]))

    def policy_worst_case_disturbance(self, kl_bounds=(), thetas=(), cross=True):
        """What the adversary does to the noise (rat_policy_worst_case_disturbance): the mean and covariance of the disturbance w_t at every
        step, and its covariance with the state and the control it acts on, under the worst-case distribution p* ~ exp(theta* J) q of each
        KL radius -- and under the tilt of each given theta; theta = 0 is the nominal distribution q -- formed on the device by replaying
        the last policy_evaluate / policy_evaluate_noise of this context like policy_worst_case_trajectory.  Returns {"bounds": part,
        "thetas": part}; a part carries policy_worst_case's row keys and, with R rows, mean_w (R, N, n), cov_w (R, N, n, n) and, with
        cross, cov_wx (R, N, n, n) and cov_wu (R, N, n, m): entry [i, j] is Cov(w_t[i], x_t[j]).  Population covariances.
        cov_wx[r, t] @ pinv(policy_worst_case_trajectory's cov_x[r, t]) is the adversary's feedback gain at step t."""
        d = nv.f64(np.atleast_1d(np.asarray(kl_bounds, dtype=np.float64))).ravel()
        th = nv.f64(np.atleast_1d(np.asarray(thetas, dtype=np.float64))).ravel()
        n, m, N, R = self.n, self.m, self.N, d.size + th.size
        rows, mean, cov = np.zeros((R, nv.WC_NSTAT)), np.zeros((R, N, n)), np.zeros((R, N, n, n))
        wz = np.zeros((R, N, n + m, n)) if cross else None
        nv.check(nv.lib().rat_policy_worst_case_disturbance(self.h, nv.P(d) if d.size else None, C.c_int32(d.size), nv.P(th) if th.size else None,
                                                            C.c_int32(th.size), nv.P(rows), nv.P(mean), nv.P(cov), nv.P(wz)))
        return self._wc_parts(rows, d.size, lambda sl, r: self._unpack_disturbance(mean[sl], cov[sl], wz[sl] if cross else None))

    def policy_worst_case_params(self, kl_bounds=(), thetas=(), cost=True):
        """What the adversary picks among the uncertain parameters (rat_policy_worst_case_params): the mean and covariance of the
        parameters q that the source's rat_user_params drew for the rollouts, and their covariance with the rollout's cost, under the
        worst-case distribution p* ~ exp(theta* J) q of each KL radius -- and under the tilt of each given theta; theta = 0 is the nominal
        distribution -- formed on the device by replaying the last policy_evaluate_noise of this context (parameter sampling on, device
        generator for the noise) like policy_worst_case_trajectory.  Returns {"bounds": part, "thetas": part}; a part carries
        policy_worst_case's row keys and, with R rows and P = n_params, mean_q (R, P), cov_q (R, P, P) (population form, exactly
        symmetric) and, with cost, cov_qJ (R, P) -- dE[q] / dtheta at the row's tilt -- and the derived explained_share (R, P):
        cov_qJ[i]^2 / (cov_q[i, i] tilt_var), the linear share of the cost's variance that parameter i explains (NaN where a parameter or
        the cost does not vary)."""
        d = nv.f64(np.atleast_1d(np.asarray(kl_bounds, dtype=np.float64))).ravel()
        th = nv.f64(np.atleast_1d(np.asarray(thetas, dtype=np.float64))).ravel()
        P, R = getattr(self, "params", np.zeros(0)).size, d.size + th.size
        rows, mean, cov = np.zeros((R, nv.WC_NSTAT)), np.zeros((R, P)), np.zeros((R, P, P))
        qJ = np.zeros((R, P)) if cost else None
        nv.check(nv.lib().rat_policy_worst_case_params(self.h, nv.P(d) if d.size else None, C.c_int32(d.size), nv.P(th) if th.size else None,
                                                       C.c_int32(th.size), nv.P(rows), nv.P(mean), nv.P(cov), nv.P(qJ)))

        def moments(sl, r):
            out = self._unpack_params(mean[sl], cov[sl], qJ[sl] if cost else None)
            if cost:
                out.update(explained_share=explained_share(out["cov_q"], out["cov_qJ"], r["tilt_var"]))
            return out
        return self._wc_parts(rows, d.size, moments)

    # What a moment replay's worst-case call and its tail sibling share: the family's moments out of the C ABI's buffers (column-major
    # blocks, the 12 + 4 layout's (x, u) split), as fresh arrays
    @staticmethod
    def _wc_parts(rows, n_bound, moments):
        """{"bounds": part, "thetas": part} of a worst-case replay: policy_worst_case's row keys and moments(slice, rows so far)"""
        def part(sl):
            r = {k: rows[sl, i].copy() for i, k in enumerate(nv.WC_SLOTS)}
            r["flag"] = r["flag"].astype(np.int64)
            r.update(moments(sl, r))
            return r
        return dict(bounds=part(slice(0, n_bound)), thetas=part(slice(n_bound, rows.shape[0])))

    def _unpack_trajectory(self, mean, cov):
        n, N = self.n, self.N
        cov = cov.transpose(0, 1, 3, 2)
        return dict(mean_x=mean[:, :, :n].copy(), cov_x=cov[:, :, :n, :n].copy(), mean_u=mean[:, :N, n:].copy(),
                    cov_u=cov[:, :N, n:, n:].copy(), cov_xu=cov[:, :N, :n, n:].copy())

    def _unpack_disturbance(self, mean, cov, wz):
        n = self.n
        out = dict(mean_w=mean.copy(), cov_w=cov.transpose(0, 1, 3, 2).copy())
        if wz is not None:
            wz = wz.transpose(0, 1, 3, 2)                             # [R, N, n, n+m]
            out.update(cov_wx=wz[:, :, :, :n].copy(), cov_wu=wz[:, :, :, n:].copy())
        return out

    @staticmethod
    def _unpack_params(mean, cov, qJ):
        out = dict(mean_q=mean.copy(), cov_q=cov.transpose(0, 2, 1).copy())
        if qJ is not None:
            out.update(cov_qJ=qJ.copy())
        return out

    def _tail_rows(self, alphas):
        al = nv.f64(np.atleast_1d(np.asarray(alphas, dtype=np.float64))).ravel()
        return al, np.zeros((al.size, nv.TR_NSTAT))

    @staticmethod
    def _tail_part(rows):
        r = {k: rows[:, i].copy() for i, k in enumerate(nv.TR_SLOTS)}
        r["flag"] = r["flag"].astype(np.int64)
        return r

    def policy_tail_trajectory(self, alphas):
        """What the tail looks like (rat_policy_tail_trajectory): the mean and covariance of the state and the control at every step over
        the worst (1 - alpha) share of the rollouts -- the tail distribution of policy_tail_risk, the CVaR adversary's -- per level alpha in
        [0, 1) (1 to 16 levels; alpha = 0 is the nominal distribution), formed on the device by replaying the last policy_evaluate /
        policy_evaluate_noise of this context like policy_worst_case_trajectory.  Returns one dict: policy_tail_risk's row keys (alpha, var,
        cvar, ..., flag) and, with R levels, mean_x (R, N+1, n), cov_x (R, N+1, n, n), mean_u (R, N, m), cov_u (R, N, m, m), cov_xu
        (R, N, n, m), population form.  A saturated level holds the moments of the rollouts attaining the maximum; an empty or non-finite
        sample gives NaN."""
        al, rows = self._tail_rows(alphas)
        n, m, N, R = self.n, self.m, self.N, al.size
        mean, cov = np.zeros((R, N + 1, n + m)), np.zeros((R, N + 1, n + m, n + m))
        nv.check(nv.lib().rat_policy_tail_trajectory(self.h, nv.P(al) if al.size else None, C.c_int32(al.size), nv.P(rows), nv.P(mean), nv.P(cov)))
        r = self._tail_part(rows)
        r.update(self._unpack_trajectory(mean, cov))
        return r

    def _gradient_out(self, R):
        n, m, N = self.n, self.m, self.N
        return np.zeros((R, N, m)), np.zeros((R, N, n, m)), np.zeros((R, N, m)), C.c_int64(0)

    def _gradient_part(self, gl, gL, se, nf):
        open_loop = getattr(self, "_noise_open_loop", False)
        return dict(grad_l=gl, grad_L=None if open_loop else gL.transpose(0, 1, 3, 2).copy(), grad_l_se=se, n_nonfinite=int(nf.value))

    def policy_gradient(self, kl_bounds=(), thetas=()):
        """Which way to move the policy (rat_policy_gradient): the gradient with respect to l and L of the mean cost (theta = 0), of the
        entropic risk of each theta and of the KL-robust bound of each radius (at its theta*, envelope theorem), by adjoint replay of the
        last policy_evaluate_noise of this context on the device (source problems, device generator, the affine law).  Returns
        {"bounds": part, "thetas": part}; a part carries policy_worst_case's row keys and, with R rows, grad_l (R, N, m), grad_L
        (R, N, m, n) (None after an open-loop evaluation), grad_l_se (R, N, m), the self-normalised standard error of grad_l, and
        n_nonfinite, the rollouts left out because their sensitivities hold a NaN or Inf.  The disturbances are held fixed (a sampler that
        reads x or u is not differentiated through), x_nom is not differentiated, a saturated row is a subgradient."""
        d = nv.f64(np.atleast_1d(np.asarray(kl_bounds, dtype=np.float64))).ravel()
        th = nv.f64(np.atleast_1d(np.asarray(thetas, dtype=np.float64))).ravel()
        R = d.size + th.size
        rows = np.zeros((R, nv.WC_NSTAT))
        gl, gL, se, nf = self._gradient_out(R)
        nv.check(nv.lib().rat_policy_gradient(self.h, nv.P(d) if d.size else None, C.c_int32(d.size), nv.P(th) if th.size else None,
                                              C.c_int32(th.size), nv.P(rows), nv.P(gl), nv.P(gL), nv.P(se), C.byref(nf)))
        full = self._gradient_part(gl, gL, se, nf)

        def moments(sl, r):
            return {k: (v[sl].copy() if isinstance(v, np.ndarray) else v) for k, v in full.items()}
        return self._wc_parts(rows, d.size, moments)

    def policy_tail_gradient(self, alphas):
        """The gradient of CVaR_alpha with respect to l and L per level (rat_policy_tail_gradient): policy_gradient under the tail
        distribution of policy_tail_risk (alpha = 0 is the mean).  Returns one dict: policy_tail_risk's row keys and grad_l, grad_L,
        grad_l_se, n_nonfinite as policy_gradient's parts carry them."""
        al, rows = self._tail_rows(alphas)
        gl, gL, se, nf = self._gradient_out(al.size)
        nv.check(nv.lib().rat_policy_tail_gradient(self.h, nv.P(al) if al.size else None, C.c_int32(al.size), nv.P(rows), nv.P(gl), nv.P(gL),
                                                   nv.P(se), C.byref(nf)))
        r = self._tail_part(rows)
        r.update(self._gradient_part(gl, gL, se, nf))
        return r

    def policy_margin_gradient(self, events, alphas):
        """Which way to move the policy to clear a safety event (rat_policy_margin_gradient): for each of 1 to 4 events (halfspace, ball,
        quadratic_event) and each level alpha in [0, 1) (1 to 16), the gradient with respect to l and L of the tail mean of the event's
        margin M = max over its window of g -- alpha = 0: the mean margin; otherwise CVaR_alpha(M), whose being <= 0 implies
        P(M > 0) <= 1 - alpha -- by adjoint replay of the last policy_evaluate_noise of this context (source problems, device generator,
        the affine law).  Returns a list with one dict per event: policy_tail_risk's row keys on that event's margins (bit for bit
        policy_tail_risk(costs=margins[i])) and grad_l (R, N, m), grad_L (R, N, m, n) (None after an open-loop evaluation), grad_l_se,
        n_nonfinite as policy_tail_gradient carries them.  The disturbances are held fixed, x_nom and the value at risk are not
        differentiated; a tie of the arg-max step or of the tail's membership, and a saturated level, give a subgradient."""
        al, _ = self._tail_rows(alphas)
        E, Q, a, b, lo, hi = self._events_dense(events)
        A, Ea = al.size, min(max(E, 1), 4)                            # (the arrays of a call that the library refuses)
        rows = np.zeros((Ea * max(A, 1), nv.TR_NSTAT))
        gl, gL, se, _ = self._gradient_out(Ea * max(A, 1))
        nf = np.zeros(max(E, 1), dtype=np.int64)
        nv.check(nv.lib().rat_policy_margin_gradient(self.h, C.c_int32(E), nv.P(Q), nv.P(a), nv.P(b), nv.PI(lo), nv.PI(hi),
                                                     nv.P(al) if A else None, C.c_int32(A), nv.P(rows), nv.P(gl), nv.P(gL), nv.P(se),
                                                     nf.ctypes.data_as(C.POINTER(C.c_int64))))
        out = []
        for i in range(E):
            sl = slice(i * A, (i + 1) * A)
            r = self._tail_part(rows[sl])
            r.update(self._gradient_part(gl[sl].copy(), gL[sl], se[sl].copy(), C.c_int64(int(nf[i]))))
            out.append(r)
        return out

    def _param_gradient_out(self, R):
        P = getattr(self, "params", np.zeros(0)).size
        return np.zeros((R, P)), np.zeros((R, P)), np.zeros((R, self.n)), np.zeros((R, self.n)), C.c_int64(0)

    def policy_param_gradient(self, kl_bounds=(), thetas=()):
        """How a risk reacts to the model (rat_policy_param_gradient): the gradient with respect to the source problem's parameters p and
        to the initial state x_0 of the mean cost (theta = 0), of the entropic risk of each theta and of the KL-robust bound of each
        radius (at its theta*), by adjoint replay of the last policy_evaluate_noise of this context on the device.  The source defines
        RAT_USER_PARAMS_AD (rat_user_f, rat_user_c, rat_user_h templated on the parameters' type).  Returns {"bounds": part, "thetas":
        part}; a part carries policy_worst_case's row keys and, with R rows, grad_p and grad_p_se (R, n_params), grad_x0 and grad_x0_se
        (R, n), and n_nonfinite.  Noise and controller are frozen (a sampler that scales with a parameter is not differentiated through;
        x_nom and the law are constants), theta* is not differentiated, and with parameter sampling on every rollout is differentiated at
        its own drawn q."""
        d = nv.f64(np.atleast_1d(np.asarray(kl_bounds, dtype=np.float64))).ravel()
        th = nv.f64(np.atleast_1d(np.asarray(thetas, dtype=np.float64))).ravel()
        R = d.size + th.size
        rows = np.zeros((R, nv.WC_NSTAT))
        gp, gps, gx, gxs, nf = self._param_gradient_out(R)
        has_p = gp.shape[1] > 0                                       # (no parameters: grad_x0 alone)
        nv.check(nv.lib().rat_policy_param_gradient(self.h, nv.P(d) if d.size else None, C.c_int32(d.size), nv.P(th) if th.size else None,
                                                    C.c_int32(th.size), nv.P(rows), nv.P(gp) if has_p else None,
                                                    nv.P(gps) if has_p else None, nv.P(gx), nv.P(gxs), C.byref(nf)))
        full = dict(grad_p=gp, grad_p_se=gps, grad_x0=gx, grad_x0_se=gxs, n_nonfinite=int(nf.value))

        def moments(sl, r):
            return {k: (v[sl].copy() if isinstance(v, np.ndarray) else v) for k, v in full.items()}
        return self._wc_parts(rows, d.size, moments)

    def policy_tail_param_gradient(self, alphas):
        """The gradient of CVaR_alpha with respect to p and x_0 per level (rat_policy_tail_param_gradient): policy_param_gradient under the
        tail distribution of policy_tail_risk (alpha = 0 is the mean).  Returns one dict: policy_tail_risk's row keys and grad_p,
        grad_p_se, grad_x0, grad_x0_se, n_nonfinite as policy_param_gradient's parts carry them."""
        al, rows = self._tail_rows(alphas)
        gp, gps, gx, gxs, nf = self._param_gradient_out(al.size)
        has_p = gp.shape[1] > 0
        nv.check(nv.lib().rat_policy_tail_param_gradient(self.h, nv.P(al) if al.size else None, C.c_int32(al.size), nv.P(rows),
                                                         nv.P(gp) if has_p else None, nv.P(gps) if has_p else None, nv.P(gx), nv.P(gxs),
                                                         C.byref(nf)))
        r = self._tail_part(rows)
        r.update(dict(grad_p=gp, grad_p_se=gps, grad_x0=gx, grad_x0_se=gxs, n_nonfinite=int(nf.value)))
        return r

    def policy_tail_disturbance(self, alphas, cross=True):
        """What the noise of the tail looks like (rat_policy_tail_disturbance): policy_worst_case_disturbance's moments over the worst
        (1 - alpha) share of the rollouts per level.  Returns one dict: policy_tail_risk's row keys and, with R levels, mean_w (R, N, n),
        cov_w (R, N, n, n) and, with cross, cov_wx (R, N, n, n) and cov_wu (R, N, n, m)."""
        al, rows = self._tail_rows(alphas)
        n, m, N, R = self.n, self.m, self.N, al.size
        mean, cov = np.zeros((R, N, n)), np.zeros((R, N, n, n))
        wz = np.zeros((R, N, n + m, n)) if cross else None
        nv.check(nv.lib().rat_policy_tail_disturbance(self.h, nv.P(al) if al.size else None, C.c_int32(al.size), nv.P(rows), nv.P(mean), nv.P(cov),
                                                      nv.P(wz)))
        r = self._tail_part(rows)
        r.update(self._unpack_disturbance(mean, cov, wz))
        return r

    def policy_tail_params(self, alphas, cost=True):
        """Which parameters the tail drew (rat_policy_tail_params): policy_worst_case_params' moments over the worst (1 - alpha) share of
        the rollouts per level.  Returns one dict: policy_tail_risk's row keys and, with R levels and P = n_params, mean_q (R, P), cov_q
        (R, P, P) and, with cost, cov_qJ (R, P)."""
        al, rows = self._tail_rows(alphas)
        P, R = getattr(self, "params", np.zeros(0)).size, al.size
        mean, cov = np.zeros((R, P)), np.zeros((R, P, P))
        qJ = np.zeros((R, P)) if cost else None
        nv.check(nv.lib().rat_policy_tail_params(self.h, nv.P(al) if al.size else None, C.c_int32(al.size), nv.P(rows), nv.P(mean), nv.P(cov),
                                                 nv.P(qJ)))
        r = self._tail_part(rows)
        r.update(self._unpack_params(mean, cov, qJ))
        return r

    def _events_dense(self, events):
        """The events of policy_events / policy_tail_events as the C call takes them: n_event, Q (column-major, or None: all linear), a, b,
        t_lo, t_hi."""
        n, m, N = self.n, self.m, self.N
        dense = [e.dense(n, m, N) for e in events]
        E = len(dense)
        quad = any(q[0] is not None for q in dense)
        Q = nv.f64(np.stack([(np.zeros((n + m, n + m)) if q[0] is None else q[0]).T for q in dense])) if quad and E else None   # column-major
        a = nv.f64(np.stack([q[1] for q in dense])) if E else None
        b = nv.f64(np.array([q[2] for q in dense])) if E else None
        lo = np.ascontiguousarray([q[3] for q in dense], dtype=np.int32) if E else None
        hi = np.ascontiguousarray([q[4] for q in dense], dtype=np.int32) if E else None
        return E, Q, a, b, lo, hi

    @staticmethod
    def _events_part(row_slots, rows, ev, step, sl):
        """The rows sl of an events call as a dict: the row keys (row_slots), the RAT_EV_* arrays, event_flag and, with step, step."""
        r = {k: rows[sl, i].copy() for i, k in enumerate(row_slots)}
        r["flag"] = r["flag"].astype(np.int64)
        r.update({k: ev[sl, :, i].copy() for i, k in enumerate(nv.EV_SLOTS) if k != "flag"})
        r["event_flag"] = ev[sl, :, nv.EV_SLOTS.index("flag")].astype(np.int64)
        if step is not None:
            r["step"] = step[sl].copy()
        return r

    def policy_events(self, events, kl_bounds=(), thetas=(), want_steps=False, want_margins=False):
        """How often the policy violates safety events (rat_policy_events): per event (halfspace, ball, quadratic_event; 1 to 16) and per
        row -- the worst-case distribution of each KL radius, the tilt of each theta; theta = 0 is the nominal distribution -- the
        probability that a rollout violates it, formed on the device by replaying the last policy_evaluate / policy_evaluate_noise of this
        context like policy_worst_case_trajectory.  Returns {"bounds": part, "thetas": part, "margins": (n_event, K) or None}; a part
        carries policy_worst_case's row keys and, with R rows, arrays (R, n_event + 1) -- the last column is "any", the union --
        prob, prob_se, margin_mean, margin_max, first_mean, n_viol, prob_robust, event_flag, and with want_steps step (R, n_event + 1, N+1):
        the probability of a violation at each step.  margins[i] (want_margins) is the margin of every rollout for event i, NaN for a
        DomainError rollout: a sample to hand to policy_tail_risk(costs=) or policy_worst_case(costs=)."""
        d = nv.f64(np.atleast_1d(np.asarray(kl_bounds, dtype=np.float64))).ravel()
        th = nv.f64(np.atleast_1d(np.asarray(thetas, dtype=np.float64))).ravel()
        E, Q, a, b, lo, hi = self._events_dense(events)
        N, R = self.N, d.size + th.size
        rows, ev = np.zeros((R, nv.WC_NSTAT)), np.zeros((R, E + 1, nv.EV_NSTAT))
        step = np.zeros((R, E + 1, N + 1)) if want_steps else None
        margins = np.zeros((max(E, 1), max(int(self.debug_get("mc_cost_K")), 1))) if want_margins else None
        nv.check(nv.lib().rat_policy_events(self.h, C.c_int32(E), nv.P(Q), nv.P(a), nv.P(b), nv.PI(lo), nv.PI(hi), nv.P(d) if d.size else None,
                                            C.c_int32(d.size), nv.P(th) if th.size else None, C.c_int32(th.size), nv.P(rows), nv.P(ev),
                                            nv.P(step), nv.P(margins)))

        def part(sl):
            return self._events_part(nv.WC_SLOTS, rows, ev, step, sl)
        return dict(bounds=part(slice(0, d.size)), thetas=part(slice(d.size, R)), margins=margins)

    def policy_events_user(self, n_event, kl_bounds=(), thetas=(), want_steps=False, want_margins=False):
        """policy_events for the events the source problem's own rat_user_event writes (rat_policy_events_user): n_event in 1 .. 16 is the
        number of entries of g the function may write; an entry it leaves alone at a step is not watched there.  A moving obstacle, a box
        (a min of half-spaces), any function of (k, x, u, p).  It replays the last policy_evaluate_noise of this context (device generator
        only) and returns policy_events' dict: the last column of every array is "any", margins is (n_event, K) or None."""
        d = nv.f64(np.atleast_1d(np.asarray(kl_bounds, dtype=np.float64))).ravel()
        th = nv.f64(np.atleast_1d(np.asarray(thetas, dtype=np.float64))).ravel()
        N, R, E = self.N, d.size + th.size, int(n_event)
        Ea = min(max(E, 1), 16)                                       # (the arrays of a call that the library refuses)
        rows, ev = np.zeros((R, nv.WC_NSTAT)), np.zeros((R, Ea + 1, nv.EV_NSTAT))
        step = np.zeros((R, Ea + 1, N + 1)) if want_steps else None
        margins = np.zeros((Ea, max(int(self.debug_get("mc_cost_K")), 1))) if want_margins else None
        nv.check(nv.lib().rat_policy_events_user(self.h, C.c_int32(E), nv.P(d) if d.size else None, C.c_int32(d.size),
                                                 nv.P(th) if th.size else None, C.c_int32(th.size), nv.P(rows), nv.P(ev), nv.P(step),
                                                 nv.P(margins)))

        def part(sl):
            return self._events_part(nv.WC_SLOTS, rows, ev, step, sl)
        return dict(bounds=part(slice(0, d.size)), thetas=part(slice(d.size, R)), margins=margins)

    def policy_tail_events(self, events, alphas, want_steps=False, want_margins=False):
        """Safety events under the CVaR adversary (rat_policy_tail_events): policy_events with one row per level alpha in [0, 1) (1 to 16
        levels; alpha = 0 is the nominal distribution) -- among the worst (1 - alpha) share of the rollouts, the tail distribution of
        policy_tail_risk, how often each event is violated, where in the horizon and by how much.  Replays the last policy_evaluate /
        policy_evaluate_noise of this context.  Returns {"levels": part, "margins": (n_event, K) or None}; the part carries
        policy_tail_risk's row keys (alpha, var, cvar, ..., flag) and policy_events' arrays (R, n_event + 1) -- the last column is "any" --
        and, with want_steps, step (R, n_event + 1, N+1).  prob_robust is min(1, (n_viol / N_OK) / (tail_n / N_OK)): the largest
        probability of the event under any p with dp/dq <= N_OK / tail_n; event_flag is the level's flag."""
        al, rows = self._tail_rows(alphas)
        E, Q, a, b, lo, hi = self._events_dense(events)
        N, R = self.N, al.size
        ev = np.zeros((R, E + 1, nv.EV_NSTAT))
        step = np.zeros((R, E + 1, N + 1)) if want_steps else None
        margins = np.zeros((max(E, 1), max(int(self.debug_get("mc_cost_K")), 1))) if want_margins else None
        nv.check(nv.lib().rat_policy_tail_events(self.h, C.c_int32(E), nv.P(Q), nv.P(a), nv.P(b), nv.PI(lo), nv.PI(hi), nv.P(al) if al.size else None,
                                                 C.c_int32(al.size), nv.P(rows), nv.P(ev), nv.P(step), nv.P(margins)))
        return dict(levels=self._events_part(nv.TR_SLOTS, rows, ev, step, slice(0, R)), margins=margins)

    def policy_tail_events_user(self, n_event, alphas, want_steps=False, want_margins=False):
        """policy_tail_events for the events the source problem's own rat_user_event writes (rat_policy_tail_events_user): n_event as
        policy_events_user takes it; returns policy_tail_events' dict."""
        al, rows = self._tail_rows(alphas)
        N, R, E = self.N, al.size, int(n_event)
        Ea = min(max(E, 1), 16)                                       # (the arrays of a call that the library refuses)
        ev = np.zeros((R, Ea + 1, nv.EV_NSTAT))
        step = np.zeros((R, Ea + 1, N + 1)) if want_steps else None
        margins = np.zeros((Ea, max(int(self.debug_get("mc_cost_K")), 1))) if want_margins else None
        nv.check(nv.lib().rat_policy_tail_events_user(self.h, C.c_int32(E), nv.P(al) if al.size else None, C.c_int32(al.size), nv.P(rows),
                                                      nv.P(ev), nv.P(step), nv.P(margins)))
        return dict(levels=self._events_part(nv.TR_SLOTS, rows, ev, step, slice(0, R)), margins=margins)

    def policy_rare_event(self, x_nom, l, L, event, K, seed=0, shift=None, n_iter=8, rho=0.1, want_margins=False, want_logw=False):
        """The probability of a rare safety event under the policy (x_nom, l, L) -- as policy_evaluate takes it -- by adaptive importance
        sampling on the device (rat_policy_rare_event): the process noise is drawn from a proposal shifted by s (N, n), every rollout
        carries its likelihood ratio, and up to n_iter multilevel cross-entropy iterations (elite share rho) move the shift towards the
        event before the final pass estimates.  One event (halfspace, ball, quadratic_event).  shift: where the adaptation starts (None:
        0); hand a result's shift back with n_iter=0 to estimate again at another K or seed.  LQ and power-law families, n <= 12, m <= 4.
        Returns a RareEventResult."""
        n, m, N = self.n, self.m, self.N
        Q, a, b, lo, hi = event.dense(n, m, N)
        Qc = nv.f64(Q.T) if Q is not None else None                   # column-major
        a = nv.f64(a)
        s_in = None
        if shift is not None:
            s_in = nv.f64(shift)
            if s_in.shape != (N, n):
                raise ValueError(f"policy_rare_event: the shift is {s_in.shape}, (N, n) = ({N}, {n}) is served")
        K, n_iter = int(K), int(n_iter)
        stats, s_out, trace = np.zeros(nv.RE_NSTAT), np.zeros((N, n)), np.zeros((max(n_iter, 0), nv.RE_NTRACE))
        margins = np.zeros(max(K, 1)) if want_margins else None
        logw = np.zeros(max(K, 1)) if want_logw else None
        nv.check(nv.lib().rat_policy_rare_event(self.h, nv.P(nv.f64(x_nom)), nv.P(nv.f64(l)), nv.P(nv.cm3(L)) if L is not None else None,
                                                C.c_int64(K), C.c_uint64(int(seed)), nv.P(Qc), nv.P(a), C.c_double(b), C.c_int32(lo), C.c_int32(hi),
                                                nv.P(s_in), C.c_int32(n_iter), C.c_double(float(rho)), nv.P(stats), nv.P(s_out),
                                                nv.P(trace) if n_iter > 0 else None, nv.P(margins), nv.P(logw)))
        r = {k: float(stats[i]) for i, k in enumerate(nv.RE_SLOTS)}
        for k in ("n_viol", "n_ok", "n_domain", "flag", "n_iter"):
            r[k] = int(r[k])
        return RareEventResult(shift=s_out, trace=trace, margins=margins, logw=logw, **r)

    def policy_rare_event_noise(self, x_nom, l, L, event, K, noise=None, seed=None, shift=None, n_iter=8, rho=0.1, want_margins=False,
                                want_logw=False):
        """policy_rare_event for a source problem under the disturbance its own rat_user_noise draws (rat_policy_rare_event_noise): noise
        is a UserNoise without injected streams (the device generator only); the proposal shifts the normals the sampler draws -- the
        i-th rng.normal() of step t returns shift[t, i] + xi -- so the shift is (N, P), P = noise.normals_per_step in 1 .. 12.
        rng.uniform() is not shifted: an event that a uniform drives cannot be made likelier by this call.  seed None: the UserNoise's.
        With n_iter=0 and no shift the margins are policy_events' behind policy_evaluate_noise at the same seed, bit for bit.
        Returns a RareEventResult."""
        if not isinstance(noise, UserNoise):
            raise TypeError("policy_rare_event_noise needs noise=UserNoise(...)")
        if noise.zn is not None or noise.zu is not None:
            raise ValueError("policy_rare_event_noise draws from the device generator only: no injected streams")
        n, m, N, npn, npu = self.n, self.m, self.N, noise.normals_per_step, noise.uniforms_per_step
        Q, a, b, lo, hi = event.dense(n, m, N)
        Qc = nv.f64(Q.T) if Q is not None else None                   # column-major
        a = nv.f64(a)
        s_in = None
        if shift is not None:
            s_in = nv.f64(shift)
            if s_in.shape != (N, npn):
                raise ValueError(f"policy_rare_event_noise: the shift is {s_in.shape}, (N, normals_per_step) = ({N}, {npn}) is served")
        K, n_iter = int(K), int(n_iter)
        seed = noise.seed if seed is None else int(seed)
        stats, s_out, trace = np.zeros(nv.RE_NSTAT), np.zeros((N, max(npn, 1))), np.zeros((max(n_iter, 0), nv.RE_NTRACE))
        margins = np.zeros(max(K, 1)) if want_margins else None
        logw = np.zeros(max(K, 1)) if want_logw else None
        nv.check(nv.lib().rat_policy_rare_event_noise(self.h, nv.P(nv.f64(x_nom)), nv.P(nv.f64(l)), nv.P(nv.cm3(L)) if L is not None else None,
                                                      C.c_int64(K), C.c_int32(npn), C.c_int32(npu), C.c_uint64(seed), nv.P(Qc), nv.P(a),
                                                      C.c_double(b), C.c_int32(lo), C.c_int32(hi), nv.P(s_in), C.c_int32(n_iter),
                                                      C.c_double(float(rho)), nv.P(stats), nv.P(s_out), nv.P(trace) if n_iter > 0 else None,
                                                      nv.P(margins), nv.P(logw)))
        r = {k: float(stats[i]) for i, k in enumerate(nv.RE_SLOTS)}
        for k in ("n_viol", "n_ok", "n_domain", "flag", "n_iter"):
            r[k] = int(r[k])
        return RareEventResult(shift=s_out, trace=trace, margins=margins, logw=logw, **r)

    def policy_rare_event_user(self, x_nom, l, L, n_event, event, K, noise=None, seed=None, shift=None, n_iter=8, rho=0.1, want_margins=False,
                               want_logw=False):
        """policy_rare_event_noise with entry `event` (0 .. n_event - 1) of the source's own rat_user_event in place of the quadratic event
        (rat_policy_rare_event_user): the margin is the largest g[event] over the steps at which the function wrote it.  With n_iter=0
        and no shift the margins are row `event` of policy_events_user's behind policy_evaluate_noise at the same seed, bit for bit.
        Returns a RareEventResult."""
        if not isinstance(noise, UserNoise):
            raise TypeError("policy_rare_event_user needs noise=UserNoise(...)")
        if noise.zn is not None or noise.zu is not None:
            raise ValueError("policy_rare_event_user draws from the device generator only: no injected streams")
        N, npn, npu = self.N, noise.normals_per_step, noise.uniforms_per_step
        s_in = None
        if shift is not None:
            s_in = nv.f64(shift)
            if s_in.shape != (N, npn):
                raise ValueError(f"policy_rare_event_user: the shift is {s_in.shape}, (N, normals_per_step) = ({N}, {npn}) is served")
        K, n_iter = int(K), int(n_iter)
        seed = noise.seed if seed is None else int(seed)
        stats, s_out, trace = np.zeros(nv.RE_NSTAT), np.zeros((N, max(npn, 1))), np.zeros((max(n_iter, 0), nv.RE_NTRACE))
        margins = np.zeros(max(K, 1)) if want_margins else None
        logw = np.zeros(max(K, 1)) if want_logw else None
        nv.check(nv.lib().rat_policy_rare_event_user(self.h, nv.P(nv.f64(x_nom)), nv.P(nv.f64(l)), nv.P(nv.cm3(L)) if L is not None else None,
                                                     C.c_int64(K), C.c_int32(npn), C.c_int32(npu), C.c_uint64(seed), C.c_int32(int(n_event)),
                                                     C.c_int32(int(event)), nv.P(s_in), C.c_int32(n_iter), C.c_double(float(rho)),
                                                     nv.P(stats), nv.P(s_out), nv.P(trace) if n_iter > 0 else None, nv.P(margins),
                                                     nv.P(logw)))
        r = {k: float(stats[i]) for i, k in enumerate(nv.RE_SLOTS)}
        for k in ("n_viol", "n_ok", "n_domain", "flag", "n_iter"):
            r[k] = int(r[k])
        return RareEventResult(shift=s_out, trace=trace, margins=margins, logw=logw, **r)

    def policy_rare_event_params(self, x_nom, l, L, event, K, noise=None, seed=None, shift=None, param_shift=None, adapt="both", n_iter=8,
                                 rho=0.1, n_event=0, want_margins=False, want_logw=False):
        """policy_rare_event_noise (n_event=0: event is an Event) or policy_rare_event_user (n_event in 1 .. 16: event is the entry of
        rat_user_event) for an event that an uncertain parameter drives (rat_policy_rare_event_params): with parameter sampling on
        (set_param_sampling, the device generator) the i-th rng.normal() of the source's rat_user_params returns param_shift[i] + xi and
        its likelihood ratio is part of every rollout's logw.  adapt: "both", "step" or "params" -- the part that is not adapted stays
        at the shift handed in (0 for None), is still applied and still counted; "params" is the choice for an event that the
        parameters alone drive.  A model without process noise declares one normal per step and multiplies it by 0.
        Returns a RareEventResult with param_shift (param_normals,) and param_trace (n_iter,)."""
        if not isinstance(noise, UserNoise):
            raise TypeError("policy_rare_event_params needs noise=UserNoise(...)")
        if noise.zn is not None or noise.zu is not None:
            raise ValueError("policy_rare_event_params draws from the device generator only: no injected streams")
        if adapt not in ("both", "step", "params"):
            raise ValueError('policy_rare_event_params: adapt is "both", "step" or "params"')
        n, m, N, npn, npu, pn = self.n, self.m, self.N, noise.normals_per_step, noise.uniforms_per_step, self._param_normals
        n_event = int(n_event)
        Qc, a, b, lo, hi, ev = None, None, 0.0, 0, 0, 0
        if n_event == 0:
            Q, a, b, lo, hi = event.dense(n, m, N)
            Qc = nv.f64(Q.T) if Q is not None else None               # column-major
            a = nv.f64(a)
        else:
            ev = int(event)
        s_in = ps_in = None
        if shift is not None:
            s_in = nv.f64(shift)
            if s_in.shape != (N, npn):
                raise ValueError(f"policy_rare_event_params: the shift is {s_in.shape}, (N, normals_per_step) = ({N}, {npn}) is served")
        if param_shift is not None:
            ps_in = nv.f64(param_shift)
            if ps_in.shape != (pn,):
                raise ValueError(f"policy_rare_event_params: the parameter shift is {ps_in.shape}, (param_normals,) = ({pn},) is served")
        K, n_iter = int(K), int(n_iter)
        seed = noise.seed if seed is None else int(seed)
        stats, s_out, trace = np.zeros(nv.RE_NSTAT), np.zeros((N, max(npn, 1))), np.zeros((max(n_iter, 0), nv.RE_NTRACE))
        ps_out, ptrace = np.zeros(max(pn, 1)), np.zeros(max(n_iter, 0))
        margins = np.zeros(max(K, 1)) if want_margins else None
        logw = np.zeros(max(K, 1)) if want_logw else None
        nv.check(nv.lib().rat_policy_rare_event_params(self.h, nv.P(nv.f64(x_nom)), nv.P(nv.f64(l)), nv.P(nv.cm3(L)) if L is not None else None,
                                                       C.c_int64(K), C.c_int32(npn), C.c_int32(npu), C.c_uint64(seed), C.c_int32(n_event),
                                                       C.c_int32(ev), nv.P(Qc), nv.P(a), C.c_double(b), C.c_int32(lo), C.c_int32(hi),
                                                       nv.P(s_in), nv.P(ps_in), C.c_int32({"step": 1, "params": 2, "both": 3}[adapt]),
                                                       C.c_int32(n_iter), C.c_double(float(rho)), nv.P(stats), nv.P(s_out), nv.P(ps_out),
                                                       nv.P(trace) if n_iter > 0 else None, nv.P(ptrace) if n_iter > 0 else None,
                                                       nv.P(margins), nv.P(logw)))
        r = {k: float(stats[i]) for i, k in enumerate(nv.RE_SLOTS)}
        for k in ("n_viol", "n_ok", "n_domain", "flag", "n_iter"):
            r[k] = int(r[k])
        return RareEventResult(shift=s_out, trace=trace, margins=margins, logw=logw, param_shift=ps_out[:pn], param_trace=ptrace, **r)

    def policy_sobol(self, x_nom, l, L=None, noise=None, groups=(), K=None, seed_a=1, seed_b=2, want_costs=False):
        """Which uncertainty drives the cost (rat_policy_sobol): the first-order and total Sobol indices of the Monte-Carlo cost of the
        policy (x_nom, l, L) for the groups of draws `groups` (SobolGroup), from K base samples of d + 2 pick-freeze rollouts each on the
        device generator -- stream A under seed_a, stream B under seed_b.  noise: a UserNoise without injected streams (its seed is not
        read).  Parameter sampling may be on (the device generator) or off.  Returns a dict: S, S_se, T, T_se (arrays over the groups),
        names, n_ok, mean, var, var_se, flag, and with want_costs y (d + 2, K): rows A, B, then the groups (None otherwise)."""
        if not isinstance(noise, UserNoise):
            raise TypeError("policy_sobol needs noise=UserNoise(...)")
        if noise.zn is not None or noise.zu is not None:
            raise ValueError("policy_sobol draws from the device generator only: no injected streams")
        if K is None:
            raise ValueError("policy_sobol needs K=")
        groups = list(groups)
        words = SobolGroup.check_groups(groups, noise.normals_per_step, noise.uniforms_per_step, self._param_normals, self._param_uniforms)
        K, d = int(K), len(groups)
        index, summary = np.zeros((d, nv.SB_NINDEX)), np.zeros(nv.SB_NSTAT)
        y = np.zeros((d + 2, max(K, 1))) if want_costs else None
        nv.check(nv.lib().rat_policy_sobol(self.h, nv.P(nv.f64(x_nom)), nv.P(nv.f64(l)), nv.P(nv.cm3(L)) if L is not None else None,
                                           C.c_int64(K), C.c_int32(noise.normals_per_step), C.c_int32(noise.uniforms_per_step),
                                           words.ctypes.data_as(nv._up), C.c_int32(d), C.c_uint64(int(seed_a)), C.c_uint64(int(seed_b)),
                                           nv.P(index), nv.P(summary), nv.P(y)))
        return dict(S=index[:, nv.SB_S].copy(), S_se=index[:, nv.SB_S_SE].copy(), T=index[:, nv.SB_T].copy(), T_se=index[:, nv.SB_T_SE].copy(),
                    names=[g.name for g in groups], n_ok=int(summary[nv.SB_N_OK]), mean=float(summary[nv.SB_MEAN]),
                    var=float(summary[nv.SB_VAR]), var_se=float(summary[nv.SB_VAR_SE]), flag=int(summary[nv.SB_FLAG]), y=y)

    def integrate_cost(self, x, u):
        out = C.c_double()
        nv.check(nv.lib().rat_integrate_cost(self.h, nv.P(nv.f64(x)), nv.P(nv.f64(u)), C.byref(out)))
        return out.value

    def approximate_model(self, u, x):
        n, m, N = self.n, self.m, self.N
        b = dict(q=np.zeros(N + 1), qv=np.zeros(n * (N + 1)), Q=np.zeros(n * n * (N + 1)), r=np.zeros(m * N),
                 R=np.zeros(m * m * N), P=np.zeros(m * n * N), A=np.zeros(n * n * N), B=np.zeros(n * m * N),
                 W=np.zeros(n * n * N))
        dom = C.c_int32()
        nv.check(nv.lib().rat_approximate_model(self.h, nv.P(nv.f64(u)), nv.P(nv.f64(x)), *[nv.P(b[k]) for k in
                                                ("q", "qv", "Q", "r", "R", "P", "A", "B", "W")], C.byref(dom)))
        if dom.value:
            raise ArithmeticError("DomainError in approximate_model")
        return ApproximationResult(
            q_array=b["q"], q_vec_array=b["qv"].reshape(N + 1, n), Q_array=nv.from_cm3(b["Q"], N + 1, n, n),
            r_array=b["r"].reshape(N, m), R_array=nv.from_cm3(b["R"], N, m, m), P_array=nv.from_cm3(b["P"], N, m, n),
            A_array=nv.from_cm3(b["A"], N, n, n), B_array=nv.from_cm3(b["B"], N, n, m),
            W_array=nv.from_cm3(b["W"], N, n, n))

    def _approx_ptrs(self, ap):
        bufs = [nv.f64(ap.q_array), nv.f64(ap.q_vec_array), nv.cm3(ap.Q_array), nv.f64(ap.r_array), nv.cm3(ap.R_array),
                nv.cm3(ap.P_array), nv.cm3(ap.A_array), nv.cm3(ap.B_array)]
        return bufs, [nv.P(b) for b in bufs]

    def _dp_out(self):
        n, m, N = self.n, self.m, self.N
        return dict(s=np.zeros(N + 1), sv=np.zeros(n * (N + 1)), S=np.zeros(n * n * (N + 1)), g=np.zeros(m * N),
                    G=np.zeros(m * n * N), H=np.zeros(m * m * N))

    def _dp_result(self, o):
        n, m, N = self.n, self.m, self.N
        return DynamicProgrammingResult(
            s_array=o["s"], s_vec_array=o["sv"].reshape(N + 1, n), S_array=nv.from_cm3(o["S"], N + 1, n, n),
            g_array=o["g"].reshape(N, m), G_array=nv.from_cm3(o["G"], N, m, n), H_array=nv.from_cm3(o["H"], N, m, m))

    def dp_gain_sweep(self, ap, theta, mu, delta):
        n, m, N = self.n, self.m, self.N
        keep, ptrs = self._approx_ptrs(ap)
        mu_c, de_c, st = C.c_double(mu), C.c_double(delta), C.c_int32()
        Lb, dl, o = np.zeros(m * n * N), np.zeros((N, m)), self._dp_out()
        nv.check(nv.lib().rat_dp_gain_sweep(self.h, *ptrs, C.c_double(theta), C.byref(mu_c), C.byref(de_c), nv.P(Lb),
                                            nv.P(dl), C.byref(st), *[nv.P(o[k]) for k in ("s", "sv", "S", "g", "G", "H")]))
        return st.value, nv.from_cm3(Lb, N, m, n), dl, self._dp_result(o), mu_c.value, de_c.value

    def dp_policy_eval(self, ap, L, dl, theta, mu):
        keep, ptrs = self._approx_ptrs(ap)
        st, o = C.c_int32(), self._dp_out()
        Lc = nv.cm3(L)
        dlc = None if dl is None else nv.f64(dl)
        nv.check(nv.lib().rat_dp_policy_eval(self.h, *ptrs, nv.P(Lc), nv.P(dlc), C.c_double(theta), C.c_double(mu),
                                             C.byref(st), *[nv.P(o[k]) for k in ("s", "sv", "S", "g", "G", "H")]))
        return st.value, self._dp_result(o)

    # ---- fused solves ----------------------------------------------------------------------------
    def solve(self, x0, u, theta, hist_cap=4096):
        n, m, N = self.n, self.m, self.N
        x, l, Lb = np.zeros((N + 1, n)), np.zeros((N, m)), np.zeros(m * n * N)
        val, st, it, hn = C.c_double(), C.c_int32(), C.c_int32(), C.c_int64()
        while True:           # eps_history is unbounded in the reference (ileqg.jl:537): when it did not fit, grow and re-run (deterministic)
            hist = np.zeros((hist_cap, 2))
            nv.check(nv.lib().rat_ileqg_solve(self.h, nv.P(nv.f64(x0)), nv.P(nv.f64(u)), C.c_double(theta), nv.P(x), nv.P(l),
                                              nv.P(Lb), C.byref(val), C.byref(st), C.byref(it), nv.P(hist),
                                              C.c_int64(hist_cap), C.byref(hn)))
            if hn.value <= hist_cap:
                break
            hist_cap = int(hn.value)
        return dict(x=x, l=l, L=nv.from_cm3(Lb, N, m, n), value=val.value, status=st.value, iters=it.value,
                    eps_history=hist[: min(hn.value, hist_cap)].copy(), hist_n=hn.value)

    def solve_batch(self, x0, u, theta):
        theta = nv.f64(theta)
        B = theta.size
        value, status = np.zeros(B), np.zeros(B, np.int32)
        iters, ls = np.zeros(B, np.int32), np.zeros(B, np.int32)
        nv.check(nv.lib().rat_ileqg_solve_batch(self.h, nv.P(nv.f64(x0)), nv.P(nv.f64(u)), nv.P(theta), C.c_int64(B),
                                                nv.P(value), nv.PI(status), nv.PI(iters), nv.PI(ls)))
        return value, status, iters, ls

    def set_initial(self, x0, u):
        nv.check(nv.lib().rat_set_initial(self.h, nv.P(nv.f64(x0)), nv.P(nv.f64(u))))

    def solve_batch_dev(self, theta_ptr, B, value_ptr, status_ptr=None, iters_ptr=None, ls_ptr=None):
        """Device-pointer form (ints): inputs/outputs stay in HBM."""
        nv.check(nv.lib().rat_ileqg_solve_batch_dev(self.h, C.c_void_p(theta_ptr), C.c_int64(B), C.c_void_p(value_ptr),
                                                    C.c_void_p(status_ptr), C.c_void_p(iters_ptr), C.c_void_p(ls_ptr)))

    def compute_cost_dev(self, theta_ptr, B, kl_bound, cost_ptr):
        """compute_cost (cross_entropy...jl:173-195), device-pointer form: cost = value + kl_bound / theta stays in HBM."""
        nv.check(nv.lib().rat_ce_compute_cost_dev(self.h, C.c_void_p(theta_ptr), C.c_int64(B), C.c_double(kl_bound),
                                                  C.c_void_p(cost_ptr)))

    def compute_cost_enqueue(self, theta_ptr, B, kl_bound, cost_ptr):
        """Stream-ordered compute_cost_dev: returns once the batch is enqueued on ``self.stream`` (hipStream_t as int)."""
        nv.check(nv.lib().rat_ce_compute_cost_enqueue(self.h, C.c_void_p(theta_ptr), C.c_int64(B), C.c_double(kl_bound),
                                                      C.c_void_p(cost_ptr)))

    def compute_cost_enqueue_ex(self, theta_ptr, B, kl_bound, cost_ptr, status_ptr=None, iters_ptr=None, ls_ptr=None):
        """compute_cost_enqueue with the per-sample status / iteration / line-search counts written beside the costs."""
        nv.check(nv.lib().rat_ce_compute_cost_enqueue_ex(self.h, C.c_void_p(theta_ptr), C.c_int64(B), C.c_double(kl_bound), C.c_void_p(cost_ptr),
                                                         C.c_void_p(status_ptr), C.c_void_p(iters_ptr), C.c_void_p(ls_ptr)))

    # ---- execution path (include/ratilqr.h RAT_PATH_*; results are identical on all of them) -------
    PATHS = {"auto": 0, "rounds": 1, "fused": 2, "block": 3}

    def set_path(self, path):
        """Fix the execution path of this handle's batched solves: "auto" | "rounds" | "fused" | "block" (rat_set_path).  Moving between
        the single-launch E = 1 kernels and the round-based path re-lays the state: the initial trajectory must be given again."""
        nv.check(nv.lib().rat_set_path(self.h, C.c_int32(self.PATHS[path] if isinstance(path, str) else int(path))))

    def debug_set(self, key, value):
        """An execution switch of the handle (rat_debug_set; keys in include/ratilqr.h): tests, A/B tools, bench.py's contract leg."""
        nv.check(nv.lib().rat_debug_set(self.h, key.encode(), C.c_int64(int(value))))

    def debug_get(self, key):
        v = C.c_int64(0)
        nv.check(nv.lib().rat_debug_get(self.h, key.encode(), C.byref(v)))
        return int(v.value)

    def get_path(self, B):
        """Which path a batch of B samples takes: "rounds" | "fused" | "block" | "wide"."""
        r = int(nv.lib().rat_get_path(self.h, C.c_int64(int(B))))
        return {1: "rounds", 2: "fused", 3: "block", 4: "wide"}.get(r)

    @property
    def stream(self):
        """The handle's HIP stream (hipStream_t) as an integer, e.g. for ``torch.cuda.ExternalStream``."""
        return int(nv.lib().rat_stream(self.h) or 0)

    # ---- measurement -----------------------------------------------------------------------------
    def profile(self, on=True, kinds=None):
        """HIP-event timing of kernel launches; ``kinds`` (names from _native.K_NAMES) restricts what is recorded."""
        flag = int(bool(on))
        if on and kinds is not None:
            mask = 0
            for k in kinds:
                mask |= 1 << nv.K_NAMES.index(k)
            flag = (mask << 1) | 1
        nv.check(nv.lib().rat_profile_enable(self.h, flag))

    def profile_reset(self):
        nv.check(nv.lib().rat_profile_reset(self.h))

    def profile_get(self):
        nk = len(nv.K_NAMES)
        la = (C.c_int64 * nk)(); tr = (C.c_int64 * nk)(); ms = (C.c_double * nk)()
        nv.check(nv.lib().rat_profile_get(self.h, la, tr, ms))
        return {nv.K_NAMES[k]: dict(launches=la[k], trajectories=tr[k], ms=ms[k]) for k in range(nk)}

    def layout_info(self):
        v = [C.c_int64() for _ in range(4)]
        nv.check(nv.lib().rat_layout_info(self.h, *[C.byref(x) for x in v]))
        return dict(tile_bytes=v[0].value, L_bytes=v[1].value, x_bytes=v[2].value, u_bytes=v[3].value)


@dataclass
class ApproximationResult:                 # ileqg.jl:242-252
    q_array: np.ndarray
    q_vec_array: np.ndarray
    Q_array: np.ndarray
    r_array: np.ndarray
    R_array: np.ndarray
    P_array: np.ndarray
    A_array: np.ndarray
    B_array: np.ndarray
    W_array: np.ndarray


@dataclass
class DynamicProgrammingResult:            # ileqg.jl:328-335
    s_array: np.ndarray
    s_vec_array: np.ndarray
    S_array: np.ndarray
    g_array: np.ndarray
    G_array: np.ndarray
    H_array: np.ndarray


_ctx_cache: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _ctx(problem) -> Context:
    """Default context of a problem for the stateless reference functions (simulate_dynamics, ...)."""
    c = _ctx_cache.get(problem)
    if c is None:
        c = make_context(problem)
        _ctx_cache[problem] = c
    return c


def make_context(problem, opts=None, max_batch=1, spec_eps=1, device=0) -> Context:
    """Context of a device model family, or the host-closure context of a generic problem (generic.py)."""
    if getattr(problem, "model", 0) == 0:
        from .generic import GenericContext
        return GenericContext(problem, opts, max_batch=max_batch, spec_eps=spec_eps, device=device)
    return Context(problem, opts, max_batch=max_batch, spec_eps=spec_eps, device=device)


def make_opts(mu_min=1e-6, Delta_0=2.0, lam=0.5, d=1e-2, iter_max=100, eps_init=1.0, adaptive_eps_init=False,
              eps_min=1e-6) -> nv.IleqgOpts:
    # the @assert block of ileqg.jl:195-201
    assert 0 < lam < 1, "λ has to be in (0, 1)"
    assert d > 0, "d > 0 is necessary"
    assert mu_min > 0, "μ_min > 0 is necessary"
    assert Delta_0 > 0, "Δ_0 > 0 is necessary"
    assert 0 < eps_init <= 1, "ϵ_init has to be in (0, 1]"
    assert eps_init > eps_min, "ϵ_init > ϵ_min is necessary"
    assert 0 < eps_min < 1, "ϵ_min has to be in (0, 1)"
    o = nv.IleqgOpts()
    o.mu_min, o.delta_0, o.lam, o.d, o.iter_max = mu_min, Delta_0, lam, d, int(iter_max)
    o.eps_init, o.eps_min, o.adaptive_eps_init = eps_init, eps_min, int(bool(adaptive_eps_init))
    return o


class ILEQGSolver:
    """ILEQGSolver(problem; kwargs...)  (ileqg.jl:164-208)."""

    def __init__(self, problem: FiniteHorizonRiskSensitiveOptimalControlProblem, mu_min=1e-6, Delta_0=2.0, lam=0.5,
                 d=1e-2, iter_max=100, eps_init=1.0, adaptive_eps_init=False, eps_min=1e-6, f_returns_jacobian=False,
                 max_batch=1, spec_eps=1, device=0):
        self.opts = make_opts(mu_min, Delta_0, lam, d, iter_max, eps_init, adaptive_eps_init, eps_min)
        self.mu_min, self.mu, self.Delta_0, self.Delta = mu_min, mu_min, Delta_0, Delta_0      # :206
        self.lam, self.d, self.iter_max = lam, d, int(iter_max)
        self.eps_init_auto, self.eps_init, self.eps_min = bool(adaptive_eps_init), eps_init, eps_min
        self.f_returns_jacobian = f_returns_jacobian    # analytic Jacobians are always used on the device
        self.x_array = self.l_array = self.L_array = None
        self.A_array = self.B_array = None
        self.value_current, self.iter_current, self.d_current = np.inf, 0, np.inf
        self.eps_history = []
        self.eps_init_init = eps_init
        self.status = None
        self._ctx_args = dict(max_batch=max_batch, spec_eps=spec_eps, device=device)
        self.ctx = make_context(problem, self.opts, **self._ctx_args)

    def context(self, problem) -> "Context":
        """The device context of `problem`.  The reference's solve!/initialize!/step!/line_search! take every table from their
        `problem` argument (ileqg.jl:214, 494, 598, 635), so a solver built on one problem and called with another must follow the
        argument: the context (device tables) is rebuilt when the problem object differs from the one it was made for."""
        bound = getattr(self.ctx, "generic", None) or self.ctx.problem
        if problem is not bound:
            self.ctx = make_context(problem, self.opts, **self._ctx_args)
        return self.ctx


# ---- the reference's free functions ----------------------------------------------------------------
def simulate_dynamics(problem, a, b, c=None, f_returns_jacobian=False):
    """simulate_dynamics(problem, x_0, u_array) (ileqg.jl:18-38) or
    simulate_dynamics(problem, x_array, l_array, L_array) (ileqg.jl:62-87)."""
    ctx = _ctx(problem)
    if c is None:
        return ctx.rollout_open(a, b)
    return ctx.rollout_feedback(a, b, c)


def simulate_dynamics_noisy(problem, a, b, c=None, K=1, z=None, seed=0):
    """The rng methods of simulate_dynamics, K rollouts at once: simulate_dynamics(problem, x_0, u_array, rng) (ileqg.jl:44-55)
    or simulate_dynamics(problem, x_array, l_array, L_array, rng) (ileqg.jl:94-109).  The rng is an injected standard-normal
    array z of shape (K, N, n) or a seed of the device generator.  Returns (x, cost) or (x, u, cost), rollout index first."""
    ctx = _ctx(problem)
    x, u, cost, dom = ctx.rollout_noisy(a, b, c, K=K, z=z, seed=seed)
    if dom:
        raise ArithmeticError("DomainError in simulate_dynamics")
    return (x, cost) if c is None else (x, u, cost)


def evaluate_policy(problem, x, l, L=None, thetas=(), K=None, z=None, seed=0, want_costs=False, noise=None, want_trajectories=False):
    """Monte-Carlo evaluation of the policy (x, l, L) that solve_ returned -- or of an open-loop plan (x_0, u_array) with L=None -- under
    the problem's process noise: Context.policy_evaluate on the problem's default context.  DeviceSourceProblem included.  With
    noise=UserNoise(...) the disturbance is the one the source's rat_user_noise draws (Context.policy_evaluate_noise; z and seed are then
    the UserNoise's own), and want_trajectories returns the rollouts' x and u as well."""
    if noise is not None:
        if z is not None:
            raise ValueError("evaluate_policy: with noise= the injected draws are noise.zn / noise.zu, not z")
        return _ctx(problem).policy_evaluate_noise(x, l, L, noise=noise, thetas=thetas, K=K, want_costs=want_costs,
                                                   want_trajectories=want_trajectories)
    if want_trajectories:
        raise ValueError("evaluate_policy: trajectories come with noise=UserNoise(...) only (rollout_noisy returns them for the families)")
    return _ctx(problem).policy_evaluate(x, l, L, thetas=thetas, K=K, z=z, seed=seed, want_costs=want_costs)


def rare_event_probability(problem, x, l, L, event, K=1 << 16, seed=0, shift=None, n_iter=8, rho=0.1, want_margins=False, want_logw=False):
    """The probability that the policy (x, l, L) violates `event`, however rare, by adaptive importance sampling on the device:
    Context.policy_rare_event on the problem's default context.  Where policy_events counts no violation among K rollouts this still
    returns an estimate with its standard error."""
    return _ctx(problem).policy_rare_event(x, l, L, event, K, seed=seed, shift=shift, n_iter=n_iter, rho=rho, want_margins=want_margins,
                                           want_logw=want_logw)


def rare_event_probability_noise(problem, x, l, L, event, noise, K=1 << 16, seed=None, shift=None, n_iter=8, rho=0.1, want_margins=False,
                                 want_logw=False):
    """rare_event_probability for a source problem under the disturbance its own rat_user_noise draws: Context.policy_rare_event_noise on
    the problem's default context.  noise is a UserNoise (the device generator only); the shift is (N, noise.normals_per_step)."""
    return _ctx(problem).policy_rare_event_noise(x, l, L, event, K, noise=noise, seed=seed, shift=shift, n_iter=n_iter, rho=rho,
                                                 want_margins=want_margins, want_logw=want_logw)


def rare_event_probability_params(problem, x, l, L, event, noise, sampling, K=1 << 16, seed=None, shift=None, param_shift=None, adapt="both",
                                  n_iter=8, rho=0.1, n_event=0, want_margins=False, want_logw=False):
    """rare_event_probability_noise for an event that an uncertain parameter drives: Context.policy_rare_event_params on the problem's
    default context, with parameter sampling switched on as `sampling` (a ParamSampling on the device generator) says."""
    ctx = _ctx(problem)
    ctx.set_param_sampling(sampling)
    return ctx.policy_rare_event_params(x, l, L, event, K, noise=noise, seed=seed, shift=shift, param_shift=param_shift, adapt=adapt,
                                        n_iter=n_iter, rho=rho, n_event=n_event, want_margins=want_margins, want_logw=want_logw)


def integrate_cost(problem, x_array, u_array):          # ileqg.jl:115-124
    return _ctx(problem).integrate_cost(x_array, u_array)


def approximate_model(problem, u_array, x_array, A_array_input=None, B_array_input=None):   # ileqg.jl:258-322
    return _ctx(problem).approximate_model(u_array, x_array)


def initialize_(ileqg: ILEQGSolver, problem, x_0, u_array, theta):          # initialize!  ileqg.jl:214-236
    ctx = ileqg.context(problem)
    ileqg.mu, ileqg.Delta = 0.0, ileqg.Delta_0
    ileqg.d_current, ileqg.iter_current = np.inf, 0
    ileqg.eps_init = ileqg.eps_init_init
    ileqg.eps_history = []
    ileqg.x_array = ctx.rollout_open(x_0, u_array)
    ileqg.l_array = np.array(u_array, dtype=np.float64)
    ileqg.L_array = np.zeros((problem.N, problem.m, problem.n))
    ap = ctx.approximate_model(ileqg.l_array, ileqg.x_array)
    st, dp = ctx.dp_policy_eval(ap, ileqg.L_array, None, theta, ileqg.mu)
    assert st == 0, "M: (inv(W) - θ*S) is not PSD"                            # the @assert at :440
    ileqg.value_current = dp.s_array[0]


def solve_approximate_dp_(ileqg: ILEQGSolver, approx_result, verbose=False, theta=0.0):   # solve_approximate_dp!  :341-406
    st, L, dl, dp, mu, delta = ileqg.ctx.dp_gain_sweep(approx_result, theta, ileqg.mu, ileqg.Delta)
    ileqg.mu, ileqg.Delta = mu, delta
    assert st != nv.ST_M_NOT_PD_GAIN, "M: (inv(W) - θ*S) is not PSD"           # the @assert at :366
    if st != 0:
        raise ArithmeticError(f"solve_approximate_dp!: status {st}")
    ileqg.L_array = L
    return dp, dl


def solve_approximate_dp(approx_result, L_array, dl_array=None, theta=0.0, mu=0.0, ctx: Context | None = None,
                         problem=None):                                         # ileqg.jl:412-465
    if ctx is None:
        if problem is None:
            raise ValueError("solve_approximate_dp needs ctx= or problem= (the W(k) tables live in the problem)")
        ctx = _ctx(problem)
    st, dp = ctx.dp_policy_eval(approx_result, L_array, dl_array, theta, mu)
    assert st == 0, "M: (inv(W) - θ*S) is not PSD"
    return dp


def increase_mu_and_delta_(ileqg: ILEQGSolver):            # increase_μ_and_Δ!  ileqg.jl:471-474
    ileqg.Delta = max(ileqg.Delta_0, ileqg.Delta * ileqg.Delta_0)
    ileqg.mu = max(ileqg.mu_min, ileqg.mu * ileqg.Delta)


def decrease_mu_and_delta_(ileqg: ILEQGSolver):            # decrease_μ_and_Δ!  ileqg.jl:480-488
    ileqg.Delta = min(1 / ileqg.Delta_0, ileqg.Delta / ileqg.Delta_0)
    cand = ileqg.mu * ileqg.Delta
    ileqg.mu = cand if cand >= ileqg.mu_min else 0.0


def _isapprox(x, y):
    if x == y:
        return True
    if not (np.isfinite(x) and np.isfinite(y)):
        return False
    return abs(x - y) <= SQRT_EPS * max(abs(x), abs(y))


def line_search_(ileqg: ILEQGSolver, problem, dl_array_new, theta, verbose=False):      # line_search!  ileqg.jl:494-592
    ctx = ileqg.context(problem)
    cur = ileqg.value_current
    eps = ileqg.eps_init
    count = 0
    dl_array_new = np.asarray(dl_array_new, dtype=np.float64)
    while True:
        count += 1
        l_new = ileqg.l_array + eps * dl_array_new                                            # :509
        x_new, u_new = ctx.rollout_feedback(ileqg.x_array, l_new, ileqg.L_array)             # :517
        ap_new = ctx.approximate_model(u_new, x_new)                                           # :520
        st, dp_new = ctx.dp_policy_eval(ap_new, ileqg.L_array, None, theta, ileqg.mu)          # :522-528
        if st != 0:
            eps *= ileqg.lam                                                                   # :529-535
            continue
        new = dp_new.s_array[0]
        ileqg.eps_history.append((eps, new - cur))                                             # :537
        accept = _isapprox(new, cur) or new < cur                                              # :538
        if not accept:
            eps *= ileqg.lam                                                                   # :557
            if not eps < ileqg.eps_min:
                continue
        ileqg.d_current = float(np.max(np.linalg.norm(ileqg.l_array - u_new, axis=1)))        # :539 / :559
        ileqg.value_current = new
        ileqg.x_array, ileqg.l_array = x_new, u_new
        break
    if ileqg.eps_init_auto:                                                                    # :582-591
        if count == 1:
            ileqg.eps_init = min(ileqg.eps_init_init, eps / ileqg.lam)
        else:
            while eps < ileqg.eps_min:
                eps = eps / ileqg.lam
            ileqg.eps_init = eps


def step_(ileqg: ILEQGSolver, problem, theta, verbose=False):                 # step!  ileqg.jl:598-613
    ileqg.iter_current += 1
    ap = ileqg.context(problem).approximate_model(ileqg.l_array, ileqg.x_array)            # :604
    _, dl = solve_approximate_dp_(ileqg, ap, verbose, theta=theta)            # :610-611
    line_search_(ileqg, problem, dl, theta, verbose)                          # :612


def solve_(ileqg: ILEQGSolver, problem, x_0, u_array, theta, verbose=False):
    """solve!(ileqg, problem, x_0, u_array; θ)  (ileqg.jl:635-659) on the fused device state machine.

    Returns (x_array, l_array, L_array, value, ϵ_history).  Raises where the reference throws."""
    if getattr(problem, "model", 0) == 0:            # generic closures: host rollouts + linearisation, device sweeps
        return solve_stepwise_(ileqg, problem, x_0, u_array, theta)
    r = ileqg.context(problem).solve(x_0, u_array, theta)
    ileqg.status = r["status"]
    ileqg.iter_current = r["iters"]
    ileqg.eps_history = [tuple(p) for p in r["eps_history"]]
    if r["status"] in (nv.ST_M_NOT_PD_INIT, nv.ST_M_NOT_PD_GAIN):
        raise AssertionError("M: (inv(W) - θ*S) is not PSD")
    if r["status"] not in (nv.ST_OK, nv.ST_ITER_MAX):
        raise ArithmeticError(f"iLEQG solve failed with status {r['status']}")
    ileqg.x_array, ileqg.l_array, ileqg.L_array, ileqg.value_current = r["x"], r["l"], r["L"], r["value"]
    return r["x"].copy(), r["l"].copy(), r["L"].copy(), r["value"], list(ileqg.eps_history)


def solve_stepwise_(ileqg: ILEQGSolver, problem, x_0, u_array, theta):
    """The same solve!, composed from initialize_/step_ through the operator entry points (test aid)."""
    initialize_(ileqg, problem, x_0, u_array, theta)
    while True:
        step_(ileqg, problem, theta)
        if ileqg.d > ileqg.d_current and ileqg.mu <= ileqg.mu_min:
            break
        elif ileqg.iter_current == ileqg.iter_max:
            break
    return ileqg.x_array.copy(), ileqg.l_array.copy(), ileqg.L_array.copy(), ileqg.value_current, list(ileqg.eps_history)
