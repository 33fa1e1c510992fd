"""NumPy model of rat_policy_worst_case_params' moment kernels (csrc/policy_mc.hip: wcp_centre, wcp_moments, wcp_final) -- test aid shared by
tests/test_cpu_wc_params.py, tests/test_gpu_wc_params.py and tools/policy_wc_params_bench.py.

`moments` restates the device's schedule, which is wct_moments' with one step (tests/wc_trajectory_model.py): the rollouts in chunks of
2^16; inside a chunk groups of four rollouts, group g belonging to wavefront g mod 32, each wavefront adding its groups in order -- per
row one product sum_k (y Dq_i)(Dq_j) over the four rollouts of a group, as the MFMAs form it (two tiles of sixteen parameters: the
blocks (0,0), (0,1), (1,1); every entry of a block is its own sum, so the model forms the 32 x 32 matrix and reads its upper triangle)
-- the wavefronts of a slot and the four rollout lanes added in index order into the slot's partial, chunk after chunk, the eight slots
in index order, then  mean = c_q + S1 / S0,  cov_q = S2 / S0 - m m'  (the upper triangle serving both halves) and
cov_qJ = SJq / S0 - m (SJ / S0), with yj = y DJ, SJ = sum yj, SJq = sum yj Dq.  Dq = q - c_q, DJ = J - c_J.  A rollout whose cost is NaN
is selected out (D = 0, y = 0) whatever its q holds.

`centre`: the q and the cost of the first rollout among the first min(K, 2^16) whose cost is not NaN; 0 where not finite, or where there
is no such rollout.

`direct` is an independent answer: np.longdouble, the weighted means first and the covariances about them, no centre, no grouping.

`deviation` measures a result against a reference per row, each output relative to its own scale: the mean against the larger of its
largest entry and the largest standard deviation; cov_q against its largest entry plus the largest squared offset of the mean from the
centre, and cov_qJ against its largest entry plus the largest |mean - c_q| |mean_J - c_J| -- the covariances are differences of terms
of that size (S2 / S0 and m m'), and where a parameter does not vary, or one rollout carries all the weight, the difference is zero and
the terms are all there is.

CPU_DEV_*: the largest deviation of `moments` (float64, the device's order) from `direct` (np.longdouble) over the shapes of
tests/test_cpu_wc_params.py, measured on the host (that test prints every figure and holds them to these constants).  The device is
held to MARGIN times these figures against `moments`: its order of summation is the model's except inside an MFMA, whose four products
it adds in a fixed order of its own, and where the compiler fuses a product into the sum behind it.

The tiny source (`tiny_source`): n = 1, m = 1, f = x + u, c = 0, h = sum a_i q_i + 1/2 sum b_i q_i^2, rat_user_noise writes 0, and
rat_user_params sets q = p + C z: the nominal p is the mean, C a lower-triangular table in the source text, z the parameter normals.
The tilted law exp(theta J) N(p, C C') is Gaussian with precision (C C')^-1 - theta diag(b) (`closed_form`)."""
import numpy as np

import user_noise_model as um
from wc_trajectory_model import CHUNK, NW, SLOTS, WAVES

MAXP = 32
MARGIN = 8.0
# measured by tests/test_cpu_wc_params.py::test_model_against_longdouble (the case that produced each figure beside it)
CPU_DEV_MEAN = 4.3e-16       # the 12 x 4 source's fourteen parameters, K = 65541 (measured 4.26e-16)
CPU_DEV_COV = 5.4e-16        # the tiny source, P = 17, K = 65 (measured 5.39e-16)
CPU_DEV_QJ = 2.8e-16         # the tiny source, P = 16, K = 65541 (measured 2.73e-16)


def centre(q, costs):
    """(c_q [32], c_J) of the device"""
    q = np.asarray(q, float)
    K, P = q.shape
    J = np.asarray(costs, float).ravel()
    c, cJ = np.zeros(MAXP), 0.0
    live = np.flatnonzero(~np.isnan(J[:min(K, CHUNK)]))
    if live.size:
        c[:P] = q[live[0]]
        cJ = J[live[0]]
    return np.where(np.isfinite(c), c, 0.0), (cJ if np.isfinite(cJ) else 0.0)


def moments(q, costs, c_q, c_J, y, dead, cross=True):
    """mean_q [R, P], cov_q [R, P, P], cov_qJ [R, P] (None without cross) and the kernel's own ESS [R], in the device's order"""
    q = np.asarray(q, float)
    K, P = q.shape
    J = np.asarray(costs, float).ravel()
    ok = ~np.isnan(J)
    with np.errstate(all="ignore"):
        qt = np.zeros((K, MAXP))
        qt[:, :P] = q
        D = np.where(ok[:, None], qt - c_q[None], 0.0)
        DJ = np.where(ok, J - c_J, 0.0)
    D[:, P:] = 0.0
    y = np.where(ok[None, :], y, 0.0)
    R = y.shape[0]
    pS2, pS1, pSq = np.zeros((R, SLOTS, MAXP, MAXP)), np.zeros((R, SLOTS, MAXP)), np.zeros((R, SLOTS, MAXP))
    pS = np.zeros((R, SLOTS, 4))                                       # S0, sum y^2, SJ, SJ2
    for k0 in range(0, K, CHUNK):
        kc = min(CHUNK, K - k0)
        G = -(-kc // 4)
        It = -(-G // NW)
        Dp, DJp, yp = np.zeros((It * NW * 4, MAXP)), np.zeros(It * NW * 4), np.zeros((R, It * NW * 4))
        Dp[:kc], DJp[:kc], yp[:, :kc] = D[k0:k0 + kc], DJ[k0:k0 + kc], y[:, k0:k0 + kc]
        Dp, DJp, yp = Dp.reshape(It, NW, 4, MAXP), DJp.reshape(It, NW, 4), yp.reshape(R, It, NW, 4)      # group it * NW + W: wavefront W
        acc = np.zeros((R, NW, MAXP, MAXP))
        s1, sq = np.zeros((R, NW, 4, MAXP)), np.zeros((R, NW, 4, MAXP))
        sc = np.zeros((R, NW, 4, 4))
        for it in range(It):
            yi = yp[:, it]                                            # [R, NW, 4]
            yd = yi[..., None] * Dp[None, it]                         # [R, NW, 4, 32]
            for kk in range(4):
                acc += yd[:, :, kk, :, None] * Dp[None, it, :, kk, None, :]
            s1 += yd
            sc[..., 0] += yi
            sc[..., 1] += yi * yi
            if cross:
                yj = yi * DJp[None, it]
                sc[..., 2] += yj
                sc[..., 3] += yj * DJp[None, it]
                sq += yj[..., None] * Dp[None, it]
        acc, s1, sq, sc = (v.reshape((R, SLOTS, WAVES) + v.shape[2:]) for v in (acc, s1, sq, sc))
        v2, v1, vq, vs = np.zeros((R, SLOTS, MAXP, MAXP)), np.zeros((R, SLOTS, MAXP)), np.zeros((R, SLOTS, MAXP)), np.zeros((R, SLOTS, 4))
        for wv in range(WAVES):
            v2 += acc[:, :, wv]
            for kk in range(4):
                v1 += s1[:, :, wv, kk]
                vq += sq[:, :, wv, kk]
                vs += sc[:, :, wv, kk]
        pS2 += v2
        pS1 += v1
        pSq += vq
        pS += vs
    S2, S1, Sq, S = (np.zeros_like(p[:, 0]) for p in (pS2, pS1, pSq, pS))
    for s in range(SLOTS):
        S2 += pS2[:, s]
        S1 += pS1[:, s]
        Sq += pSq[:, s]
        S += pS[:, s]
    with np.errstate(all="ignore"):
        S0 = S[:, 0]
        m = S1 / S0[:, None]
        S2u = np.triu(S2) + np.triu(S2, 1).swapaxes(-1, -2)
        cov = S2u / S0[:, None, None] - m[:, :, None] * m[:, None, :]
        qJ = Sq / S0[:, None] - m * (S[:, 2] / S0)[:, None]
        mean = c_q[None] + m
        ess = S0 * S0 / S[:, 1]
    mean, cov, qJ = mean[:, :P].copy(), cov[:, :P, :P].copy(), qJ[:, :P].copy()
    mean[dead], cov[dead], qJ[dead] = np.nan, np.nan, np.nan
    return mean, cov, (qJ if cross else None), ess


def direct(q, costs, y, dead):
    """(mean_q, cov_q, cov_qJ, mean_J [R], var_J [R]) in np.longdouble, straight from the definition with p = y / sum y"""
    q = np.asarray(q, float)
    K, P = q.shape
    J = np.asarray(costs, float).ravel()
    ok = ~np.isnan(J)
    ql, Jl = q[ok].astype(np.longdouble), J[ok].astype(np.longdouble)
    R = y.shape[0]
    mean, cov, qJ, mJ, vJ = np.full((R, P), np.nan), np.full((R, P, P), np.nan), np.full((R, P), np.nan), np.full(R, np.nan), np.full(R, np.nan)
    for r in range(R):
        if dead[r]:
            continue
        p = y[r][ok].astype(np.longdouble)
        p = p / p.sum()
        mu, muJ = (p[:, None] * ql).sum(axis=0), (p * Jl).sum()
        qc, Jc = ql - mu, Jl - muJ
        mean[r], cov[r] = mu.astype(np.float64), np.dot((qc * p[:, None]).T, qc).astype(np.float64)
        qJ[r], mJ[r], vJ[r] = (p[:, None] * qc * Jc[:, None]).sum(axis=0).astype(np.float64), float(muJ), float((p * Jc * Jc).sum())
    return mean, cov, qJ, mJ, vJ


def deviation(got, ref, c_q, c_J, mean_J):
    """(worst mean_q, cov_q, cov_qJ deviation) over the rows, each relative to its scale (the module's docstring); got / ref: (mean_q,
    cov_q, cov_qJ or None); mean_J [R]: the reference's mean cost.  NaN must meet NaN."""
    tiny = np.finfo(float).tiny
    (mean, cov, qJ), (mean_r, cov_r, qJ_r) = got, ref[:3]
    assert np.array_equal(np.isnan(mean), np.isnan(mean_r)) and np.array_equal(np.isnan(cov), np.isnan(cov_r))
    P = mean.shape[1]
    dm = dc = dj = 0.0
    for r in range(mean.shape[0]):
        if np.isnan(mean_r[r]).any():
            continue
        off = np.abs(mean_r[r] - c_q[:P]).max()
        dm = max(dm, float(np.abs(mean[r] - mean_r[r]).max() / max(np.abs(mean_r[r]).max(), np.sqrt(np.abs(cov_r[r]).max()), tiny)))
        dc = max(dc, float(np.abs(cov[r] - cov_r[r]).max() / max(np.abs(cov_r[r]).max() + off * off, tiny)))
        if qJ is not None:
            assert np.array_equal(np.isnan(qJ[r]), np.isnan(qJ_r[r]))
            dj = max(dj, float(np.abs(qJ[r] - qJ_r[r]).max() / max(np.abs(qJ_r[r]).max() + off * abs(mean_J[r] - c_J), tiny)))
    return dm, dc, dj


# ---- the tiny source ------------------------------------------------------------------------------------------------------------------------
def tiny_tables(P, seed=3, corr=0.5, b_scale=0.3):
    """(mu [P], C [P, P] lower triangular, a [P], b [P]) of the tiny source with P parameters"""
    r = np.random.default_rng(seed + 100 * P)
    mu = 1.0 + 0.5 * r.standard_normal(P)
    C = np.tril(corr * 0.2 * r.standard_normal((P, P)), -1) / max(np.sqrt(P), 1.0) + np.diag(0.2 + 0.1 * r.random(P))
    a = r.standard_normal(P) / np.sqrt(P)
    b = b_scale * r.standard_normal(P) / np.sqrt(P)
    return mu, C, a, b


def _table(name, v):
    return f"    const double {name}[{v.size}] = {{" + ", ".join(repr(float(x)) for x in v.ravel()) + "};\n"


def tiny_source(P, C, a, b, hook="gauss", nan_above=None):
    """the HIP text: hook "gauss" q = p + C z (row by row, the products added in index order); "identity" leaves q alone; nan_above:
    a rollout whose first parameter normal is beyond it gets q[0] = NaN (a DomainError of the hook)"""
    src = r"""
template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p) { xn[0] = x[0] + u[0]; }
template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p) { return 0.0 * x[0]; }
template <class T> __device__ T rat_user_h(const T *x, const double *p) {
#pragma clang fp contract(off)
""" + _table("TA", a) + _table("TB", b) + f"""    T s = 0.0;
    for (int i = 0; i < {P}; ++i) s += TA[i] * p[i];
    T s2 = 0.0;
    for (int i = 0; i < {P}; ++i) s2 += TB[i] * (p[i] * p[i]);
    return s + 0.5 * s2;
}}
""" + um.NOISE_HEAD + "    w[0] = 0.0 * rng.normal();\n}\n" + r"""
#define RAT_USER_PARAMS
template <class R> __device__ void rat_user_params(R &rng, const double *p, double *q) {
#pragma clang fp contract(off)
"""
    if hook == "gauss":
        src += _table("TC", C) + f"""    double z[{P}];
    for (int i = 0; i < {P}; ++i) z[i] = rng.normal();
    for (int i = 0; i < {P}; ++i) {{
        double s = 0.0;
        for (int j = 0; j <= i; ++j) s += TC[i * {P} + j] * z[j];
        q[i] = p[i] + s;
    }}
"""
        if nan_above is not None:
            src += f"    if (z[0] > {float(nan_above)!r}) q[0] = sqrt({float(nan_above)!r} - z[0]);\n"
    return src + "}\n"


def tiny_q(mu, C, z, nan_above=None):
    """q [K, P] of the "gauss" hook on the parameter normals z [K, P]: the device's bits"""
    K, P = z.shape
    q = np.zeros((K, P))
    for i in range(P):
        s = np.zeros(K)
        for j in range(i + 1):
            s = s + C[i, j] * z[:, j]
        q[:, i] = mu[i] + s
    if nan_above is not None:
        q[z[:, 0] > nan_above, 0] = np.nan
    return q


def tiny_cost(q, a, b):
    """J [K] of the tiny source: h(q), the sums in index order; NaN where q holds one"""
    s, s2 = np.zeros(q.shape[0]), np.zeros(q.shape[0])
    for i in range(q.shape[1]):
        s = s + a[i] * q[:, i]
    for i in range(q.shape[1]):
        s2 = s2 + b[i] * (q[:, i] * q[:, i])
    return s + 0.5 * s2


def closed_form(mu, C, a, b, theta):
    """(mean [P], cov [P, P], cov_qJ [P], var_J, feasible) of exp(theta J) N(mu, C C'), J = a'q + 1/2 q' diag(b) q: the Gaussian with
    precision Sigma^-1 - theta diag(b) and mean cov (Sigma^-1 mu + theta a); Cov(q, J) = cov (a + b mean) and
    Var J = g' cov g + 1/2 tr((B cov)^2), g = a + b mean.  feasible: theta b_i lambda_max(Sigma) < 1 for every i"""
    Sig = C @ C.T
    Si = np.linalg.inv(Sig)
    cov = np.linalg.inv(Si - theta * np.diag(b))
    cov = 0.5 * (cov + cov.T)
    mean = cov @ (Si @ mu + theta * a)
    g = a + b * mean
    BC = np.diag(b) @ cov
    return mean, cov, cov @ g, float(g @ cov @ g + 0.5 * np.trace(BC @ BC)), bool(theta * np.abs(b).max() * np.linalg.eigvalsh(Sig).max() < 1.0)


def closed_form_se(cov, cov_qJ, var_J, ess):
    """standard errors (mean [P], cov [P, P], cov_qJ [P]) of the sample moments of `ess` independent draws of a Gaussian with these
    moments: cov / ess; (cov_ii cov_jj + cov_ij^2) / ess; (cov_ii var_J + cov_qJ_i^2) / ess (J taken as jointly Gaussian with q: its
    quadratic part is small beside the linear one in the cases of the tests)"""
    d = np.diag(cov)
    return np.sqrt(d / ess), np.sqrt((d[:, None] * d[None, :] + cov * cov) / ess), np.sqrt((d * var_J + cov_qJ * cov_qJ) / ess)
