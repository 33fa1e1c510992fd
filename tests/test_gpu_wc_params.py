"""rat_policy_worst_case_params on the GPU (csrc/policy_mc.hip: wcp_centre, wcp_moments, wcp_final behind the replay and the SRC_PARAMS
kernel): the rows against policy_worst_case bit for bit; means, covariances and cov_qJ against the NumPy restatement of
tests/wc_params_model.py on the q that sample_params returns and the costs the evaluation returned; the theta = 0 mean against the plain
mean; the same bits again, row by row and without the cost sums; exact symmetry; an identity hook; a hook that fails for some
rollouts; injected parameter streams; the refusals; the closed-form tilted Gaussian at K = 2^16.

Shapes: the tiny source (n = m = 1, N = 2) with P = 1 (one live lane), 16 (a full block), 17 (a second block with one live row, the
mirrored block), 32 (full), and the LQ + cubic source 12 x 4 at N = 5 with its fourteen parameters; K = 1, 3 (fewer than an MFMA's four
rollouts), 4, 65 (a wavefront and one) and 2^16 + 5 (mc_chunk's first boundary: two chunks, the centre from the first alone).  Rows:
a finite kl_bound, kl_bound = +Inf (saturated), theta = 0 and theta > 0.

Tolerance against the restatement: MARGIN x CPU_DEV_* of tests/wc_params_model.py -- the restatement's own distance from np.longdouble,
measured on the host, times a margin for the fixed but different order in which an MFMA adds its four products and for products the
compiler fuses into the sum behind them.  The closed form: five standard errors, from the closed form's own moments and the row's
effective sample size."""
import numpy as np
import pytest

import ratilqr.jl_amd as rat
import user_params_model as pm
import wc_params_model as wp
from test_cpu_wc_params import BOUNDS, CLOSED_K, CLOSED_SEED, KS, THETAS, closed_form_check, closed_form_tables, lqc_p
from wc_trajectory_model import CHUNK, weights_from_rows

pytestmark = pytest.mark.gpu
X0, L_OPEN = np.array([0.3]), np.zeros((2, 1))
_CTX = {}


def tiny_context(P, hook="gauss", nan_above=None, tables=None):
    """one handle per tiny source: (ctx, tables); sampling is on with P parameter normals"""
    key = (P, hook, nan_above, tables is not None)
    if key not in _CTX:
        mu, C, a, b = wp.tiny_tables(P) if tables is None else tables
        ctx = rat.Context(rat.DeviceSourceProblem(wp.tiny_source(P, C, a, b, hook, nan_above), 1, 1, 2, np.eye(1), params=mu))
        _CTX[key] = (ctx, (mu, C, a, b))
    ctx, tables = _CTX[key]
    ctx.set_params(tables[0])
    ctx.set_param_sampling(rat.ParamSampling(P, 0))
    return ctx, tables


def tiny_evaluate(ctx, K, seed):
    return ctx.policy_evaluate_noise(X0, L_OPEN, None, noise=rat.UserNoise(1, 0, seed=seed), K=K, want_costs=True)


def both(o):
    return {k: np.concatenate([o["bounds"][k], o["thetas"][k]]) for k in o["bounds"]}


def same_bits(a, b, label, keys=None):
    for part in ("bounds", "thetas"):
        for k in (a[part] if keys is None else keys):
            assert np.array_equal(a[part][k], b[part][k], equal_nan=True), (label, part, k)


def check(ctx, q, costs, label, bounds=BOUNDS, thetas=THETAS):
    """the call on the last evaluation against policy_worst_case's rows (bit for bit), the restatement on (q, costs), the plain mean at
    theta = 0, itself again, and cost=False; returns (out, (mean, cov, cov_qJ) over all rows)"""
    out = ctx.policy_worst_case_params(kl_bounds=bounds, thetas=thetas)
    wc = ctx.policy_worst_case(kl_bounds=bounds, thetas=thetas)
    for part in ("bounds", "thetas"):
        for k in wc[part]:
            assert np.array_equal(out[part][k], wc[part][k], equal_nan=True), (label, part, k)
    o = both(out)
    K, P = q.shape
    R = len(bounds) + len(thetas)
    got = (o["mean_q"], o["cov_q"], o["cov_qJ"])
    assert got[0].shape == (R, P) and got[1].shape == (R, P, P) and got[2].shape == (R, P) and o["explained_share"].shape == (R, P)
    y, dead = weights_from_rows(costs, o["theta"], o["flag"])
    c_q, c_J = wp.centre(q, costs)
    ref = wp.moments(q, costs, c_q, c_J, y, dead)
    ok = ~np.isnan(costs)
    with np.errstate(all="ignore"):
        mean_J = np.array([np.nan if dead[r] else (y[r][ok] * costs[ok]).sum() / y[r][ok].sum() for r in range(R)])
    dm, dc, dj = wp.deviation(got, ref, c_q, c_J, mean_J)
    print(f"{label}: against the restatement mean {dm:.2e} cov_q {dc:.2e} cov_qJ {dj:.2e}")
    assert dm <= wp.MARGIN * wp.CPU_DEV_MEAN and dc <= wp.MARGIN * wp.CPU_DEV_COV and dj <= wp.MARGIN * wp.CPU_DEV_QJ, (label, dm, dc, dj)
    assert np.array_equal(got[1], got[1].swapaxes(-1, -2), equal_nan=True)                 # exactly symmetric
    for r in range(R):                                               # the nominal row: the plain mean over the rollouts with a cost
        if o["theta"][r] == 0.0 and o["flag"][r] == 0:
            plain = q[ok].mean(axis=0)
            assert np.abs(got[0][r] - plain).max() <= 1e-13 * max(np.abs(plain).max(), 1.0), (label, r)
    same_bits(out, ctx.policy_worst_case_params(kl_bounds=bounds, thetas=thetas), (label, "again"))
    plain = ctx.policy_worst_case_params(kl_bounds=bounds, thetas=thetas, cost=False)
    assert "cov_qJ" not in plain["bounds"] and "explained_share" not in plain["thetas"]
    same_bits(plain, out, (label, "cost=False"), keys=plain["bounds"].keys())
    return out, got


# ---- 1-5, 9. the shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("P", [1, 16, 17, 32])
def test_tiny_source_against_the_restatement(P, K):
    ctx, (mu, C, a, b) = tiny_context(P)
    r = tiny_evaluate(ctx, K, seed=7)
    q = ctx.sample_params(K, seed=7)
    assert r["n_ok"] == K and np.allclose(r["costs"], wp.tiny_cost(q, a, b), rtol=1e-13, atol=1e-14)
    out, got = check(ctx, q, r["costs"], f"tiny P={P} K={K}")
    flags = both(out)["flag"]
    assert flags[1] == 1 and flags[2] == 0 and flags[3] == 0          # kl = +Inf saturates; theta = 0 and theta > 0 do not
    if K > 4:
        sat = int(np.argmax(r["costs"]))
        # the saturated row is the rollout that attains Jmax: c_q + (q - c_q) to two roundings, and exactly no covariance
        assert np.abs(got[0][1] - q[sat]).max() <= 4 * np.finfo(float).eps * np.abs(q).max() and not got[1][1].any()
        share = both(out)["explained_share"][2]
        assert np.all((share >= 0.0) & (share <= 1.0 + 1e-12))


@pytest.mark.parametrize("K", [4, 65, CHUNK + 5])
def test_the_twelve_by_four_source(K):
    c = pm.case("lq12")
    N, p = 5, lqc_p()
    if "lqc" not in _CTX:
        _CTX["lqc"] = rat.Context(c.problem("scale", p=p, N=N))
    ctx = _CTX["lqc"]
    ctx.set_params(p)
    ctx.set_param_sampling(rat.ParamSampling(pm.PARAM_NORMALS, pm.PARAM_UNIFORMS))
    r0 = np.random.default_rng(3)
    x_nom, l, L = 0.5 * r0.standard_normal((N + 1, c.n)), 0.8 * r0.standard_normal((N, c.m)), 0.1 * r0.standard_normal((N, c.m, c.n))
    r = ctx.policy_evaluate_noise(x_nom, l, L, noise=c.user_noise(seed=21), K=K, want_costs=True)
    q = ctx.sample_params(K, seed=21)
    assert r["n_ok"] == K
    out, got = check(ctx, q, r["costs"], f"lqc14 K={K}")
    moved = sorted((c.idx["pi0"], c.idx["pi1"], c.idx["pi2"]))
    still = [i for i in range(14) if i not in moved]
    assert np.array_equal(got[0][:, still], np.repeat(p[None, still], 4, axis=0))          # a parameter the hook leaves alone: exactly nominal,
    assert not got[1][:, still].any() and not got[1][:, :, still].any() and not got[2][:, still].any()      # exactly no variance
    assert np.all(got[1][2][moved, moved] > 0.0)


def test_row_by_row():
    ctx, _ = tiny_context(17)
    tiny_evaluate(ctx, 301, seed=4)
    bounds = tuple(0.01 * (i + 1) ** 2 for i in range(15)) + (np.inf,)
    a = ctx.policy_worst_case_params(kl_bounds=bounds, thetas=(0.0, 0.4))
    same_bits(a, ctx.policy_worst_case_params(kl_bounds=bounds, thetas=(0.0, 0.4)), "again")
    assert a["bounds"]["flag"][-1] == 1 and np.all(a["bounds"]["flag"][:-1] == 0)
    for i, d in enumerate(bounds):                                   # a row alone and among others: the same bits
        one = ctx.policy_worst_case_params(kl_bounds=(d,))["bounds"]
        for k in one:
            assert np.array_equal(one[k][0], a["bounds"][k][i], equal_nan=True), (i, k)
    one = ctx.policy_worst_case_params(thetas=(0.4,))["thetas"]
    for k in one:
        assert np.array_equal(one[k][0], a["thetas"][k][1], equal_nan=True), k


# ---- 6. an identity hook ----------------------------------------------------------------------------------------------------------------------
def test_an_identity_hook_gives_the_nominal_parameters_exactly():
    ctx, (mu, _, _, _) = tiny_context(17, hook="identity")
    r = tiny_evaluate(ctx, 300, seed=2)
    assert r["n_ok"] == 300
    o = both(ctx.policy_worst_case_params(kl_bounds=(0.1,), thetas=(0.0, 0.5)))
    assert np.array_equal(o["mean_q"], np.repeat(mu[None], 3, axis=0)) and not o["cov_q"].any() and not o["cov_qJ"].any()
    assert np.isnan(o["explained_share"]).all()                       # nothing varies


# ---- 7. a hook that fails ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [300, CHUNK + 5])
def test_rollouts_without_parameters_carry_no_weight(K):
    ctx, (mu, C, a, b) = tiny_context(17, nan_above=1.0)
    r = tiny_evaluate(ctx, K, seed=13)
    q = ctx.sample_params(K, seed=13)
    bad = np.isnan(q[:, 0])
    assert 0.05 * K < bad.sum() < 0.3 * K and np.array_equal(np.isnan(r["costs"]), bad) and r["n_domain"] == bad.sum()
    out, got = check(ctx, q, r["costs"], f"nan hook K={K}")
    assert all(np.isfinite(g).all() for g in got)
    # the centre rule behind leading DomainErrors: a seed whose first rollouts fail
    first = np.flatnonzero(~bad)[0]
    assert np.array_equal(wp.centre(q, r["costs"])[0][:17], q[first])


def test_the_centre_skips_leading_domain_errors():
    ctx, _ = tiny_context(17, nan_above=1.0)
    for seed in range(40):                                           # (sample_params alone: no rollouts) a seed whose first rollout fails
        if np.isnan(ctx.sample_params(4, seed=seed)[0, 0]):
            break
    else:
        pytest.fail("no seed under 40 fails the first rollout")
    r = tiny_evaluate(ctx, 67, seed=seed)
    q = ctx.sample_params(67, seed=seed)
    assert np.isnan(r["costs"][0])
    check(ctx, q, r["costs"], f"leading DomainError seed={seed}")


# ---- 8. injected parameter streams ------------------------------------------------------------------------------------------------------------
def test_injected_parameter_streams_are_served():
    P, K = 17, CHUNK + 5
    ctx, (mu, C, a, b) = tiny_context(P)
    z = np.random.default_rng(8).standard_normal((K, P))
    ctx.set_param_sampling(rat.ParamSampling(P, 0, zpn=z))
    r = tiny_evaluate(ctx, K, seed=5)
    q = ctx.sample_params(K)
    assert np.array_equal(q, wp.tiny_q(mu, C, z))                    # the hook's bits on the injected normals
    check(ctx, q, r["costs"], "injected parameter draws")
    r2 = tiny_evaluate(ctx, 100, seed=5)                             # a shorter call reads the same rows
    assert np.array_equal(r2["costs"], r["costs"][:100])
    check(ctx, q[:100], r2["costs"], "injected parameter draws, K = 100")


# ---- 10. the refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    ctx, _ = tiny_context(3)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*no evaluation"):                    # nothing to replay yet
        ctx.policy_worst_case_params(thetas=(0.0,))
    tiny_evaluate(ctx, 20, seed=1)
    for kw in (dict(), dict(kl_bounds=(-0.1,)), dict(kl_bounds=(np.nan,)), dict(thetas=(np.inf,)), dict(thetas=(-1.0,)),
               dict(kl_bounds=np.ones(17)), dict(thetas=np.ones(17))):                       # rat_policy_worst_case's argument refusals
        with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*rat_policy_worst_case_params"):
            ctx.policy_worst_case_params(**kw)
    assert ctx.policy_worst_case_params(thetas=(0.0,))["thetas"]["ess"][0] == 20             # ... leave the handle usable
    ctx.policy_worst_case(kl_bounds=(0.1,), costs=np.arange(20.0))                           # uploaded costs are no evaluation's
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*rat_policy_worst_case_params.*no evaluation"):
        ctx.policy_worst_case_params(thetas=(0.0,))
    # sampling off on the handle
    ctx.set_param_sampling(None)
    tiny_evaluate(ctx, 20, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*rat_policy_worst_case_params.*rat_policy_params_sampling"):
        ctx.policy_worst_case_params(thetas=(0.0,))
    # ... and switched on behind an evaluation that ran with it off: the replay guard
    ctx.set_param_sampling(rat.ParamSampling(3, 0))
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*rat_policy_worst_case_params.*changed since the evaluation"):
        ctx.policy_worst_case_params(thetas=(0.0,))
    # under N(0, W); on injected noise draws
    ctx.policy_evaluate(X0, L_OPEN, K=16, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rat_policy_worst_case_params.*rat_user_noise"):
        ctx.policy_worst_case_params(thetas=(0.0,))
    ctx.policy_evaluate_noise(X0, L_OPEN, None, noise=rat.UserNoise(1, 0, zn=np.zeros((4, 2, 1))))
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rat_policy_worst_case_params.*injected"):
        ctx.policy_worst_case_params(thetas=(0.0,))
    # changed parameters behind the evaluation
    tiny_evaluate(ctx, 20, seed=1)
    good = ctx.policy_worst_case_params(thetas=(0.0,))
    ctx.set_params(wp.tiny_tables(3)[0] + 0.5)
    with pytest.raises(rat.RatError, match="RAT_ERR_ARG.*changed since the evaluation"):
        ctx.policy_worst_case_params(thetas=(0.0,))
    # a correct call afterwards succeeds
    ctx.set_params(wp.tiny_tables(3)[0])
    tiny_evaluate(ctx, 20, seed=1)
    same_bits(good, ctx.policy_worst_case_params(thetas=(0.0,)), "after the refusals")
    # not a source model; general sizes
    fam = rat.Context(rat.LQRiskSensitiveProblem(np.eye(2), np.eye(2), Q=np.eye(2), R=np.eye(2), N=3, W=np.eye(2), Qf=np.eye(2)))
    fam.policy_evaluate(np.zeros(2), np.zeros((3, 2)), K=8, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rat_policy_worst_case_params.*not a source model"):
        fam.policy_worst_case_params(thetas=(0.0,))
    assert fam.policy_worst_case_trajectory(thetas=(0.0,))["thetas"]["flag"][0] == 0
    wide_prob, wx0, wu = rat.synthetic_lq_problem(n=16, m=4, N=5, seed=3, w=1e-2)
    wide = rat.Context(wide_prob)
    wide.policy_evaluate(wx0, wu, K=8, seed=1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*rat_policy_worst_case_params"):
        wide.policy_worst_case_params(thetas=(0.0,))


# ---- 11. the closed form ----------------------------------------------------------------------------------------------------------------------
def test_closed_form_on_the_device():
    tables = closed_form_tables()
    ctx, (mu, C, a, b) = tiny_context(3, tables=tables)
    r = tiny_evaluate(ctx, CLOSED_K, seed=CLOSED_SEED)
    assert r["n_ok"] == CLOSED_K
    out = ctx.policy_worst_case_params(kl_bounds=(0.05,), thetas=(0.0, 0.5, 1.0))
    o = both(out)
    assert (o["flag"] == 0).all()
    q = ctx.sample_params(CLOSED_K, seed=CLOSED_SEED)
    closed_form_check(q, r["costs"], o, (o["mean_q"], o["cov_q"], o["cov_qJ"]), (mu, C, a, b), "device")
    # the nominal row's explained shares against the closed form's squared correlations
    mean, cov, qJ, var_J, _ = wp.closed_form(mu, C, a, b, 0.0)
    assert np.allclose(o["explained_share"][1], qJ ** 2 / (np.diag(cov) * var_J), atol=0.02)
