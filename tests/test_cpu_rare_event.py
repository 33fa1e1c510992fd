"""rat_policy_rare_event on the host: tests/rare_event_model.py, the NumPy model of the whole call, against closed forms -- no GPU.

Closed form: an LQ problem with kappa = 0 under an affine policy keeps (x_t, u_t) Gaussian, so a linear event watched at a single step has
g ~ N(mu_g, sigma_g^2) with mu_g, sigma_g from the host mean and covariance recursion, and p = P(g > 0) = Phi(mu_g / sigma_g) exactly."""
import math
import os
import re

import numpy as np
import pytest

import ratilqr.jl_amd as rat
import rare_event_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The seed of the closed-form checks, here and in tests/test_gpu_rare_event.py.  It was fixed before the device ran, as one for which the
# model alone meets both conditions of test_closed_form at all three probabilities (0.2, 0.95 and 0.75 standard errors off; the relative
# error 17 to 7800 times below plain Monte Carlo's).
SEED = 20261019
K_CLOSED, N_ITER_CLOSED, RHO = 1 << 16, 12, 0.1
QUANTILES = {1e-3: 3.090232306167813, 1e-6: 4.753424308822899, 1e-9: 5.997807015007686}   # Phi(-q) = p


def linear_case():
    """(2, 1, 4): a stable LQ problem, kappa = 0, an affine policy about its noise-free trajectory"""
    A, B, N = np.array([[0.9, 0.2], [-0.1, 0.8]]), np.array([[0.0], [0.5]]), 4
    prob = rat.LQRiskSensitiveProblem(A, B, Q=np.eye(2), R=np.eye(1), N=N, W=np.array([[0.05, 0.01], [0.01, 0.02]]), Qf=np.eye(2))
    l, L = 0.1 * np.ones((N, 1)), np.tile(np.array([[-0.3, -0.2]]), (N, 1, 1))
    x = np.zeros((N + 1, 2))
    x[0] = [0.5, -0.2]
    for t in range(N):
        x[t + 1] = A @ x[t] + B @ l[t]
    return prob, x, l, L


def linear_event(p):
    """a half-space on (x, u) at step N - 1 with P(violated) = p exactly; returns (event, the exact p)"""
    prob, x, l, L = linear_case()
    a, t = np.array([1.0, 0.5, 0.25]), prob.N - 1
    mu, sigma = rm.linear_gaussian_event(prob, x, l, L, a, t)
    q = QUANTILES[p]
    return rat.halfspace(a, -mu - q * sigma, steps=t), 0.5 * math.erfc(q / math.sqrt(2.0))


@pytest.fixture(scope="module")
def closed():
    prob, x, l, L = linear_case()
    out = {}
    for p in QUANTILES:
        ev, exact = linear_event(p)
        out[p] = (rm.rare_event(prob, x, l, L, ev, K_CLOSED, seed=SEED, n_iter=N_ITER_CLOSED, rho=RHO), exact)
    return out


@pytest.mark.parametrize("p", sorted(QUANTILES))
def test_closed_form(closed, p):
    r, exact = closed[p]
    plain = math.sqrt((1.0 - exact) / (exact * K_CLOSED))            # plain Monte Carlo's relative error at the same K: derivable
    print(f"p = {exact:.6e}: PROB {r['prob']:.6e} SE {r['prob_se']:.3e} ({abs(r['prob'] - exact) / r['prob_se']:.2f} sigma), "
          f"SE/PROB {r['prob_se'] / r['prob']:.3e} against plain {plain:.3e}, {r['n_iter']} iterations, ESS {r['ess']:.0f}")
    assert abs(exact / p - 1.0) < 1e-9
    assert r["flag"] == rm.OK
    assert abs(r["prob"] - exact) <= 5.0 * r["prob_se"]
    assert r["prob_se"] / r["prob"] < plain


def test_plain_monte_carlo_does_not_resolve_what_the_call_does(closed):
    """the gap: at n_iter = 0 the same K sees no violation of the 1e-9 event"""
    prob, x, l, L = linear_case()
    ev, _ = linear_event(1e-9)
    r = rm.rare_event(prob, x, l, L, ev, K_CLOSED, seed=SEED, n_iter=0)
    assert r["n_viol"] == 0 and r["prob"] == 0.0 and r["flag"] == rm.NOT_REACHED and np.all(r["logw"] == 0.0)
    assert closed[1e-9][0]["n_viol"] > 1000


def test_shift_update_is_the_weighted_elite_mean():
    """One update from s = 0: the model's shift against sum_E w z / sum_E w formed independently -- np.add.reduce over the rollouts laid out
    in the stated order (the lane's rollouts in order, the binary tree over the 256 lanes, the 64 slots in index order).  From s = 0 every
    weight is 1 and z = xi, so the two are the same additions: equal bits."""
    prob, x, l, L = linear_case()
    ev, _ = linear_event(1e-6)
    K = 3 * rm.SLOTS * rm.THREADS + 77                                # more than one rollout per lane, a ragged tail
    r = rm.rare_event(prob, x, l, L, ev, K, seed=SEED, n_iter=1, rho=RHO)
    assert r["n_iter"] == 1 and r["flag"] == rm.NOT_REACHED and r["trace"][0, 0] < 0
    M, logw, dom, xi = rm.one_pass(prob, x, l, L, ev.dense(prob.n, prob.m, prob.N), SEED, 1, K, np.zeros((prob.N, prob.n)))
    assert np.all(logw == 0.0) and not dom.any()
    v = np.sort(M)
    gamma = v[int(np.ceil(K * (1.0 - RHO))) - 1]
    assert gamma == r["trace"][0, 0]
    E = M >= gamma
    assert E.sum() == r["trace"][0, 1] == K - int(np.ceil(K * (1.0 - RHO))) + 1      # (no ties: a continuous margin)
    assert r["trace"][0, 2] == E.sum()                                # unit weights: the effective sample size is the count

    def ordered(t):                                                   # t [K, ...]
        it = -(-K // (rm.SLOTS * rm.THREADS))
        pad = np.zeros((it * rm.SLOTS * rm.THREADS,) + t.shape[1:])
        pad[:K] = t
        acc = np.add.reduce(pad.reshape((it, rm.SLOTS, rm.THREADS) + t.shape[1:]), axis=0)
        h = rm.THREADS // 2
        while h:
            acc = np.add.reduce(np.stack([acc[:, :h], acc[:, h:2 * h]]), axis=0)
            h //= 2
        return np.add.reduce(acc[:, 0], axis=0)
    w = E.astype(np.float64)
    ref = ordered(w[:, None, None] * xi) / ordered(w)
    assert np.array_equal(r["shift"], ref)
    assert np.allclose(r["shift"], xi[E].mean(axis=0), rtol=0, atol=1e-13)
    assert r["trace"][0, 3] == np.sqrt((ref * ref).sum())


def test_abi_export_and_constants():
    import ctypes as C
    from ratilqr.jl_amd import _native as nv
    assert "rat_policy_rare_event" in nv.EXPORTS
    assert hasattr(C.CDLL(nv.SO_PATH), "rat_policy_rare_event")
    hdr = open(os.path.join(ROOT, "include", "ratilqr.h")).read()
    dev = open(os.path.join(ROOT, "ratilqr.jl_amd", "csrc", "rare_event.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define RAT_RE_(\w+)\s+(\d+)", hdr)}
    for i, k in enumerate(nv.RE_SLOTS):
        assert val[k.upper()] == i, k
    assert (val["NSTAT"], val["NTRACE"]) == (nv.RE_NSTAT, nv.RE_NTRACE) == (12, 4)
    assert (val["OK"], val["NOT_REACHED"], val["EMPTY"], val["NONFINITE"]) == (nv.RE_OK, nv.RE_NOT_REACHED, nv.RE_EMPTY, nv.RE_NONFINITE)
    assert (rm.OK, rm.NOT_REACHED, rm.EMPTY, rm.NONFINITE) == (nv.RE_OK, nv.RE_NOT_REACHED, nv.RE_EMPTY, nv.RE_NONFINITE)
    assert int(re.search(r"#define RE_NSTAT (\d+)", dev).group(1)) == val["NSTAT"] and int(re.search(r"#define RE_NTRACE (\d+)", dev).group(1)) == val["NTRACE"]
    for name, mine in (("RE_PASS_STRIDE", rm.PASS_STRIDE), ("RE_CHUNK_STRIDE", rm.CHUNK_STRIDE)):
        assert int(re.search(r"#define " + name + r" (0x[0-9A-Fa-f]+)ull", dev).group(1), 16) == mine
    assert int(re.search(r"#define RE_SLOTS (\d+)", dev).group(1)) == rm.SLOTS
