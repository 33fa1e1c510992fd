"""The host side of rat_policy_worst_case_params (tests/wc_params_model.py): the restatement of the device's sums against np.longdouble on
the shapes of tests/test_gpu_wc_params.py (this is where CPU_DEV_* are measured: every figure is printed), against the closed-form
tilted Gaussian of the tiny source within five standard errors, the centre rule behind leading DomainErrors, exact symmetry, and an
identity hook (mean = p, covariance exactly 0)."""
import re
from pathlib import Path

import numpy as np
import pytest

import user_params_model as pm
import wc_params_model as wp
from wc_trajectory_model import CHUNK, row_weights

ROOT = Path(__file__).resolve().parent.parent
BOUNDS, THETAS = (0.1, np.inf), (0.0, 0.5)
KS = (1, 3, 4, 65, CHUNK + 5)
CLOSED_K, CLOSED_SEED, N_SE = 1 << 16, 11, 5.0


def tiny_sample(P, K, seed=1, nan_first=0, nan_every=0):
    """(q, J) of the tiny source with P parameters on NumPy's normals; nan_first leading rollouts and every nan_every-th are DomainErrors"""
    mu, C, a, b = wp.tiny_tables(P)
    z = np.random.default_rng(seed + P).standard_normal((K, P))
    q = wp.tiny_q(mu, C, z)
    bad = np.zeros(K, bool)
    bad[:nan_first] = True
    if nan_every:
        bad[nan_every - 1::nan_every] = True
    q[bad, 0] = np.nan
    return q, wp.tiny_cost(q, a, b)


def lqc_p():
    """the fourteen nominal parameters with a NaN threshold of ordinary size: the "scale" hook does not read it, and beside 1e300 the
    square of np.longdouble's own rounding of a mean is beyond float64"""
    p = pm.LQC_P.copy()
    p[13] = 50.0
    return p


def lqc_sample(K):
    """q [K, 14] of the LQ + cubic source's "scale" hook and a cost: the 12 x 4 case's own rollouts at its K = 128, beyond that a
    smooth function of q and a disturbance (the restatement reads q, J and y alone)"""
    c = pm.case("lq12")
    r = np.random.default_rng(5)
    p = lqc_p()
    if K <= c.K:
        return c.q("scale", p=p)[:K], c.model("scale", True, p=p)[0][:K]
    q = pm.np_params("scale", p, r.standard_normal((K, 2)), r.random((K, 1)), **c.idx)
    return q, 3.0 + 4.0 * q[:, 10] + 9.0 * q[:, 11] ** 2 + 2.0 * q[:, 0] + 0.3 * r.standard_normal(K)


def run(q, J, cross=True):
    y, dead, wc = row_weights(J, BOUNDS, THETAS)
    c_q, c_J = wp.centre(q, J)
    return wp.moments(q, J, c_q, c_J, y, dead, cross=cross), wp.direct(q, J, y, dead), (c_q, c_J), (y, dead, wc)


CASES = [("tiny", P, K) for P in (1, 16, 17, 32) for K in KS] + [("lqc14", 14, K) for K in (128, CHUNK + 5)]


@pytest.mark.parametrize("kind,P,K", CASES)
def test_model_against_longdouble(kind, P, K):
    q, J = tiny_sample(P, K, nan_every=(0 if K < 4 else 7)) if kind == "tiny" else lqc_sample(K)
    got, ref, (c_q, c_J), (y, dead, wc) = run(q, J)
    dm, dc, dj = wp.deviation(got[:3], ref, c_q, c_J, ref[3])
    print(f"{kind} P={P} K={K}: mean {dm:.2e} cov_q {dc:.2e} cov_qJ {dj:.2e}")
    assert dm <= wp.CPU_DEV_MEAN and dc <= wp.CPU_DEV_COV and dj <= wp.CPU_DEV_QJ, (dm, dc, dj)
    assert np.array_equal(got[1], got[1].swapaxes(-1, -2), equal_nan=True)                # exactly symmetric
    ess = np.concatenate([wc["bounds"]["ess"], wc["thetas"]["ess"]])
    assert np.allclose(got[3][~dead], ess[~dead], rtol=1e-9)
    plain = wp.moments(q, J, c_q, c_J, y, dead, cross=False)
    assert plain[2] is None and np.array_equal(plain[0], got[0], equal_nan=True) and np.array_equal(plain[1], got[1], equal_nan=True)
    if K == 1:                                                        # one rollout is its own centre
        assert np.array_equal(got[0], np.repeat(q[:1], 4, axis=0)) and not got[1].any() and not got[2].any()


def test_the_centre_skips_leading_domain_errors():
    q, J = tiny_sample(17, 300, nan_first=5)
    assert np.isnan(J[:5]).all() and not np.isnan(J[5])
    c_q, c_J = wp.centre(q, J)
    assert np.array_equal(c_q[:17], q[5]) and not c_q[17:].any() and c_J == J[5]
    got, ref, _, _ = run(q, J)
    dm, dc, dj = wp.deviation(got[:3], ref, c_q, c_J, ref[3])
    assert np.isfinite(got[0]).all() and dm <= wp.CPU_DEV_MEAN and dc <= wp.CPU_DEV_COV and dj <= wp.CPU_DEV_QJ
    # no rollout has a cost: the centres are 0, every row is dead
    Jn = np.full(300, np.nan)
    c_q, c_J = wp.centre(q, Jn)
    assert not c_q.any() and c_J == 0.0
    y, dead, _ = row_weights(Jn, BOUNDS, THETAS)
    mean, cov, qJ, _ = wp.moments(q, Jn, c_q, c_J, y, dead)
    assert dead.all() and np.isnan(mean).all() and np.isnan(cov).all() and np.isnan(qJ).all()
    # a centre that is not finite is 0 in that entry alone; one beyond the first 2^16 rollouts is not looked for
    q2 = q.copy()
    q2[5, 3] = np.inf
    c2, _ = wp.centre(q2, J)
    assert c2[3] == 0.0 and np.array_equal(np.delete(c2[:17], 3), np.delete(q[5], 3))
    late = np.full(CHUNK + 3, np.nan)
    late[CHUNK + 1] = 2.0
    assert not wp.centre(np.ones((CHUNK + 3, 2)), late)[0].any()


def test_an_identity_hook_gives_the_nominal_parameters_exactly():
    p = lqc_p()
    K = 257
    q = np.repeat(p[None], K, axis=0)
    J = np.random.default_rng(2).standard_normal(K) ** 2
    got, _, _, _ = run(q, J)
    assert np.array_equal(got[0], np.repeat(p[None], 4, axis=0)) and not got[1].any() and not got[2].any()


def closed_form_check(q, J, rows, out, tables, label):
    """every row with a finite tilt against exp(theta J) N(mu, C C') within N_SE standard errors, the errors from the closed form's
    own moments and the row's effective sample size; returns the worst ratio"""
    mu, C, a, b = tables
    worst = 0.0
    for r in range(rows["theta"].size):
        if rows["flag"][r] != 0:
            continue
        mean, cov, qJ, var_J, feasible = wp.closed_form(mu, C, a, b, rows["theta"][r])
        assert feasible
        se = wp.closed_form_se(cov, qJ, var_J, rows["ess"][r])
        for name, g, ref, s in (("mean", out[0][r], mean, se[0]), ("cov_q", out[1][r], cov, se[1]), ("cov_qJ", out[2][r], qJ, se[2])):
            ratio = float((np.abs(g - ref) / s).max())
            print(f"{label} row {r} theta {rows['theta'][r]:.3g} ess {rows['ess'][r]:.0f}: {name} {ratio:.2f} standard errors")
            worst = max(worst, ratio)
            assert ratio <= N_SE, (label, r, name, ratio)
    return worst


def closed_form_tables():
    return wp.tiny_tables(3, corr=4.0)                                # three correlated parameters


def test_restatement_against_the_closed_form():
    mu, C, a, b = closed_form_tables()
    corr = (C @ C.T) / np.sqrt(np.outer(np.diag(C @ C.T), np.diag(C @ C.T)))
    assert np.abs(corr - np.eye(3)).max() > 0.2
    z, _ = pm.gen_draws(CLOSED_SEED, CLOSED_K, 3, 0)                  # the device generator's parameter normals under that seed
    q = wp.tiny_q(mu, C, z)
    J = wp.tiny_cost(q, a, b)
    bounds, thetas = (0.05,), (0.0, 0.5, 1.0)
    y, dead, wc = row_weights(J, bounds, thetas)
    c_q, c_J = wp.centre(q, J)
    out = wp.moments(q, J, c_q, c_J, y, dead)
    rows = {k: np.concatenate([wc["bounds"][k], wc["thetas"][k]]) for k in ("theta", "flag", "ess")}
    assert (rows["flag"] == 0).all()
    closed_form_check(q, J, rows, out, (mu, C, a, b), "host")
    # the tilt moves the mean along cov_qJ: dE[q]/dtheta = Cov(q, J), here by a central difference of the closed form at theta = 0.5
    h = 1e-4
    d = (wp.closed_form(mu, C, a, b, 0.5 + h)[0] - wp.closed_form(mu, C, a, b, 0.5 - h)[0]) / (2 * h)
    assert np.allclose(d, wp.closed_form(mu, C, a, b, 0.5)[2], rtol=1e-6)


def test_the_entry_point_is_exported_and_mirrored():
    header = (ROOT / "include" / "ratilqr.h").read_text()
    assert re.search(r"rat_rc\s+rat_policy_worst_case_params\s*\(", header)
    import ratilqr.jl_amd as rat
    assert "rat_policy_worst_case_params" in rat.native.EXPORTS and hasattr(rat.Context, "policy_worst_case_params")
    assert "policy_worst_case_params" in (ROOT / "julia" / "RATiLQRAMD.jl").read_text()
    with pytest.raises(Exception):
        rat.GenericContext.policy_worst_case_params(object.__new__(rat.GenericContext))
    share = rat.explained_share(np.array([[[4.0, 0.0], [0.0, 0.0]]]), np.array([[1.0, 0.0]]), np.array([0.5]))
    assert share[0, 0] == 0.5 and np.isnan(share[0, 1])
