"""Replay of the evaluation that ends a fused LQ solve (switch lq_replay_last, csrc/sweep_dual.h: replay_eval_body).

The one-wavefront-per-sample solve of the LQ family (kappa = 0, diagonal time-invariant W and cost) ends on a plain policy evaluation of the
candidate whose acceptance ends it.  Where the gains that candidate ran under were solved from the Riccati-matrix record (lq_replay), the
evaluation runs only its vector half over the record -- the evaluation half of the replayed pair alone.  The replay is exact: outputs with
the switch on and off are the same bits on every workload of test_gpu_lq_replay.py, the round-based path (which runs the full sweep_body)
still agrees bit for bit with the fused one, and lq_replay_count keeps counting pairs only."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
from test_gpu_lq_replay import _draw_theta, _workloads

pytestmark = pytest.mark.gpu


def _run(last):
    """The workloads of test_gpu_lq_replay._run (lq_replay on) with lq_replay_last = last; outputs and the two counters per handle."""
    (lq, x0, u, th_lq), stress, th_s, ((back, bkx0, bku), th_b), (big, bx0, bu) = _workloads()
    it8 = rat.ileqg.make_opts(iter_max=8)

    def ctx(prob, opts=None, B=1):
        c = rat.Context(prob, opts, max_batch=B)
        c.debug_set("lq_replay_last", last)
        return c

    out, pairs, lasts = [], [], []

    def batch(c, *args):
        out.extend(c.solve_batch(*args))
        pairs.append(c.debug_get("lq_replay_count"))
        lasts.append(c.debug_get("lq_replay_last_count"))

    batch(ctx(lq, B=th_lq.size), x0, u, th_lq)
    for sp, sx, su in stress:
        batch(ctx(sp, it8, B=th_s.size), sx, su, th_s)
    batch(ctx(back, it8, B=th_b.size), bkx0, bku, th_b)
    batch(ctx(big, B=4), bx0, bu, np.array([0.0, 0.5, 2.0, 5.0]))
    for prob, sx, su, opts, th in ((lq, x0, u, None, 3.0), (back, bkx0, bku, it8, 4.0), (stress[0][0], stress[0][1], stress[0][2], it8, 1.0)):
        r = ctx(prob, opts).solve(sx, su, th)
        out += [r["x"], r["l"], r["L"], np.array([r["value"], r["status"], r["iters"]]), np.asarray(r["eps_history"], dtype=float)]
    return out, pairs, lasts


def test_last_evaluation_replayed_and_full_are_bit_identical(monkeypatch):
    monkeypatch.setenv("RATILQR_BLOCK", "0")                   # the fused kernel at every batch size
    on, p_on, l_on = _run(1)
    off, p_off, l_off = _run(0)
    print("lq_replay_count on / off:", p_on, p_off, " lq_replay_last_count on / off:", l_on, l_off)
    assert len(on) == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), k
    assert all(n == 0 for n in l_off)
    assert p_on == p_off                                       # the pairs replay as before, whatever the last evaluation does
    assert l_on[0] > 0                                         # the replay of the last evaluation did run
    # the workloads reach what they are there for (as in test_gpu_lq_replay.py)
    v, st, it, ls = on[0:4]
    assert (st == 1).any() and (st == 0).any()
    vb, sb, ib, lb = on[12:16]
    assert (lb > ib).any()
    for q in (1, 2):
        assert np.all(on[4 * q + 1] == 3)
    vo, so, io, lo = on[16:20]
    assert not np.isfinite(vo).all() or (so != 0).any()


def test_every_sample_of_the_headline_batch_replays_its_last_evaluation(monkeypatch):
    """B = 1024, theta ~ N(1, 2) > 0: every solve ends through d < d_tol at mu = 0 on gains the replayed pair committed, so every sample's
    last evaluation replays (no sample may fall back to the full sweep), and lq_replay_count still counts the pairs alone: 2 B."""
    monkeypatch.setenv("RATILQR_BLOCK", "0")
    prob, x0, u = rat.synthetic_lq_problem()
    theta = _draw_theta(1024, 1000)
    B = theta.size
    res = {}
    for last in (1, 0):
        ctx = rat.Context(prob, max_batch=B)
        ctx.debug_set("lq_replay_last", last)
        assert ctx.get_path(B) == "fused" and ctx.debug_get("lq_replay") == 1 and ctx.debug_get("lq_replay_last") == last
        res[last] = ctx.solve_batch(x0, u, theta)
        n_last, n_pair = ctx.debug_get("lq_replay_last_count"), ctx.debug_get("lq_replay_count")
        print(f"lq_replay_last = {last}: lq_replay_last_count = {n_last}, lq_replay_count = {n_pair}, B = {B}")
        assert n_last == (B if last else 0)
        assert n_pair == 2 * B
        ctx.debug_set("lq_replay_last_count", 0)
        assert ctx.debug_get("lq_replay_last_count") == 0 and ctx.debug_get("lq_replay_count") == 2 * B
        ctx.debug_set("lq_replay_count", 0)
        assert ctx.debug_get("lq_replay_count") == 0
    for a, b in zip(res[1], res[0]):
        assert np.array_equal(a, b)


def test_no_last_replay_outside_its_problem_class(monkeypatch):
    monkeypatch.setenv("RATILQR_BLOCK", "0")
    cub, x0, u = rat.synthetic_lq_problem(kappa=0.03)
    ctx = rat.Context(cub, max_batch=8)
    ctx.solve_batch(x0, u, np.linspace(0.0, 4.0, 8))
    assert ctx.debug_get("lq_replay_last") == 1 and ctx.debug_get("lq_replay_last_count") == 0
    pl = rat.PowerLawRiskSensitiveProblem(2, 10, 0.01 * np.eye(2), a=1.3, b=1.5, p=2.5, hconst=1.0)
    ctx = rat.Context(pl, max_batch=3)
    ctx.solve_batch(np.zeros(2), 0.1 * np.ones((10, 2)), np.array([0.0, 0.5, 2.0]))
    assert ctx.debug_get("lq_replay_last_count") == 0
    lq, x0, u = rat.synthetic_lq_problem()                     # inside the class, but without a record there is nothing to replay
    ctx = rat.Context(lq, max_batch=8)
    ctx.debug_set("lq_replay", 0)
    ctx.solve_batch(x0, u, np.linspace(0.5, 4.0, 8))
    assert ctx.debug_get("lq_replay_last") == 1 and ctx.debug_get("lq_replay_last_count") == 0 and ctx.debug_get("lq_replay_count") == 0


def test_fused_and_round_based_paths_still_agree(monkeypatch):
    """The fused solve ends on the replayed evaluation, the round-based path on sweep_body's full one: the same bits."""
    monkeypatch.setenv("RATILQR_BLOCK", "0")
    prob, x0, u = rat.synthetic_lq_problem()
    theta = _draw_theta(1024, 1000)[:64]
    res = {}
    for path in ("fused", "rounds"):
        ctx = rat.Context(prob, max_batch=theta.size)
        ctx.set_path(path)
        assert ctx.get_path(theta.size) == path
        res[path] = ctx.solve_batch(x0, u, theta)
        n_last = ctx.debug_get("lq_replay_last_count")
        print(f"{path}: lq_replay_last_count = {n_last}")
        assert n_last == (theta.size if path == "fused" else 0)
    for a, b in zip(res["fused"], res["rounds"]):              # value, status, iterations, line-search counts
        assert np.array_equal(a, b)


def test_an_iter_max_ending_replays_too(monkeypatch):
    """iter_max = 1 at mu = 0: the only candidate's acceptance ends the solve through iter_max, not d < d_tol; its gains are those the first
    (recording) gain sweep solved, so its evaluation replays -- with the bits of the full one."""
    monkeypatch.setenv("RATILQR_BLOCK", "0")
    prob, x0, u = rat.synthetic_lq_problem()
    theta = np.linspace(0.5, 4.0, 16)
    res = {}
    for last in (1, 0):
        ctx = rat.Context(prob, rat.ileqg.make_opts(iter_max=1), max_batch=theta.size)
        ctx.debug_set("lq_replay_last", last)
        res[last] = ctx.solve_batch(x0, u, theta)
        n_last = ctx.debug_get("lq_replay_last_count")
        print(f"iter_max = 1, lq_replay_last = {last}: lq_replay_last_count = {n_last}, iterations {res[last][2].tolist()}")
        assert np.all(res[last][2] == 1)
        assert (n_last > 0) if last else (n_last == 0)
    for a, b in zip(res[1], res[0]):
        assert np.array_equal(a, b)
