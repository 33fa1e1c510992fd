"""Record / replay of the Riccati matrices in solve_fused_kernel (switch lq_replay, csrc/sweep_dual.h: replay_dual_body).

For the LQ family with kappa = 0 and a diagonal time-invariant W, every full paired gain sweep of the one-wavefront-per-sample solve records
its Riccati matrices, and a later pair -- the evaluation of the gains it solved beside the gain sweep at the same mu -- runs only the vector
half of both recursions over that record.  The outputs must be the bits the full sweeps give: the same batches with the switch on and off, on workloads that hit
every way out of a replay (a gain sweep restarted with a raised mu, a line search that rejects candidates, M not PD, theta = 0, a
trajectory whose x^2 overflows)."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
from test_gpu_parity import stress_problem

pytestmark = pytest.mark.gpu


def _draw_theta(B, seed):          # positive samples of N(1, 2): the headline's batch (bench.py)
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < B:
        z = 1.0 + 2.0 * rng.standard_normal(B)
        out.extend(z[z > 0.0].tolist())
    return np.array(out[:B])


def _overflow_problem():
    """kappa = 0 LQ problem whose open-loop trajectory overflows: x_t = (1e60 Q)^t x_0 is Inf from t = 6 on."""
    prob, x0, u = rat.synthetic_lq_problem()
    big = rat.LQRiskSensitiveProblem(1e60 * prob.A, prob.B, Q=np.eye(12), R=0.1 * np.eye(4), N=prob.N, W=1e-3 * np.eye(12),
                                     Qf=np.eye(12))
    return big, x0, u


def _workloads():
    lq, x0, u = rat.synthetic_lq_problem()
    th_lq = np.concatenate([[0.0], np.linspace(0.01, 14.0, 30), [50.0, 300.0, 1e4]])     # the last ones: M not PD (status 1)
    stress = [stress_problem(i, kappa=0.0) for i in (1, 2)]                               # indefinite Q: H not PD, mu restarts, iter_max
    th_s = np.array([0.0, 0.3, 1.0, 4.0])
    # more indefinite: the line search rejects up to ~150 candidates per solve at theta = 4, 8
    back = stress_problem(2, kappa=0.0, qs=-1.0)
    th_b = np.array([0.0, 1.0, 4.0, 8.0])
    return (lq, x0, u, th_lq), stress, th_s, (back, th_b), _overflow_problem()


def _run(replay):
    (lq, x0, u, th_lq), stress, th_s, ((back, bkx0, bku), th_b), (big, bx0, bu) = _workloads()
    it8 = rat.ileqg.make_opts(iter_max=8)

    def ctx(prob, opts=None, B=1):
        c = rat.Context(prob, opts, max_batch=B)
        c.debug_set("lq_replay", replay)
        return c

    out = []
    c = ctx(lq, B=th_lq.size)
    out += c.solve_batch(x0, u, th_lq)
    counts = [c.debug_get("lq_replay_count")]
    for sp, sx, su in stress:
        c = ctx(sp, it8, B=th_s.size)
        out += c.solve_batch(sx, su, th_s)
        counts.append(c.debug_get("lq_replay_count"))
    c = ctx(back, it8, B=th_b.size)
    out += c.solve_batch(bkx0, bku, th_b)
    counts.append(c.debug_get("lq_replay_count"))
    c = ctx(big, B=4)
    out += c.solve_batch(bx0, bu, np.array([0.0, 0.5, 2.0, 5.0]))
    counts.append(c.debug_get("lq_replay_count"))
    for prob, sx, su, opts, th in ((lq, x0, u, None, 3.0), (back, bkx0, bku, it8, 4.0), (stress[0][0], stress[0][1], stress[0][2], it8, 1.0)):
        r = ctx(prob, opts).solve(sx, su, th)
        out += [r["x"], r["l"], r["L"], np.array([r["value"], r["status"], r["iters"]]), np.asarray(r["eps_history"], dtype=float)]
    return out, counts


def test_replay_on_and_off_are_bit_identical(monkeypatch):
    monkeypatch.setenv("RATILQR_BLOCK", "0")                   # the fused kernel at every batch size
    on, n_on = _run(1)
    off, n_off = _run(0)
    assert len(on) == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), k
    assert all(n == 0 for n in n_off)
    assert n_on[0] > 0                                         # the replay did run
    # the workloads reach what they are there for
    v, st, it, ls = on[0:4]
    assert (st == 1).any() and (st == 0).any()                 # M not PD on the largest theta
    vb, sb, ib, lb = on[12:16]
    assert (lb > ib).any()                                     # rejected line-search candidates
    for q in (1, 2):
        assert np.all(on[4 * q + 1] == 3)                      # mu restarts keep the stress problems at iter_max
    vo, so, io, lo = on[16:20]
    assert not np.isfinite(vo).all() or (so != 0).any()        # the overflowing trajectory


def test_replay_count_on_the_headline_batch(monkeypatch):
    """B = 1024, theta ~ N(1, 2) > 0: every sample pairs the evaluation of the first gains with the second gain sweep, and that pair
    replays the record of the first gain sweep (paired with initialize!'s evaluation): two replayed sweeps per sample, identical outputs.
    (The evaluation that ends the solve runs sweep_body, whose compilation of the V update rounds differently from the pair's on some
    samples: it does not replay a record of the pair.)"""
    monkeypatch.setenv("RATILQR_BLOCK", "0")
    prob, x0, u = rat.synthetic_lq_problem()
    theta = _draw_theta(1024, seed=1000)
    res = {}
    for replay in (1, 0):
        ctx = rat.Context(prob, max_batch=theta.size)
        ctx.debug_set("lq_replay", replay)
        assert ctx.get_path(theta.size) == "fused"
        res[replay] = ctx.solve_batch(x0, u, theta)
        assert ctx.debug_get("lq_replay_count") == (2 * theta.size if replay else 0)
        ctx.debug_set("lq_replay_count", 0)
        assert ctx.debug_get("lq_replay_count") == 0
    for a, b in zip(res[1], res[0]):
        assert np.array_equal(a, b)


def test_no_replay_outside_its_problem_class(monkeypatch):
    monkeypatch.setenv("RATILQR_BLOCK", "0")
    cub, x0, u = rat.synthetic_lq_problem(kappa=0.03)
    ctx = rat.Context(cub, max_batch=8)
    ctx.solve_batch(x0, u, np.linspace(0.0, 4.0, 8))
    assert ctx.debug_get("lq_replay") == 1 and ctx.debug_get("lq_replay_count") == 0
    pl = rat.PowerLawRiskSensitiveProblem(2, 10, 0.01 * np.eye(2), a=1.3, b=1.5, p=2.5, hconst=1.0)
    ctx = rat.Context(pl, max_batch=3)
    ctx.solve_batch(np.zeros(2), 0.1 * np.ones((10, 2)), np.array([0.0, 0.5, 2.0]))
    assert ctx.debug_get("lq_replay_count") == 0
