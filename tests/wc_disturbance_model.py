"""NumPy model of rat_policy_worst_case_disturbance's moment kernels (csrc/policy_mc.hip: wcd_centre, wcd_moments, wcd_final) -- test aid.

`moments` restates the device's schedule, which is wct_moments' (tests/wc_trajectory_model.py): the rollouts in chunks of 2^16; inside a
chunk groups of four rollouts, group g belonging to wavefront g mod 32, each wavefront adding its groups in order -- per step and row one
product sum_k (y Dw_i)(Dw_j) and one sum_k (y Dw_i)(Dz_j) over the four rollouts of a group, as the two MFMAs form them -- the wavefronts
of a slot and the four rollout lanes added in index order into the slot's partial, chunk after chunk, the eight slots added in index
order, then  mean_w = c_w + S1w / S0,  cov_w = S2ww / S0 - m_w m_w'  (the upper triangle of S2ww serving both halves) and
cov_wz = S2wz / S0 - m_w m_z'.  Dw = w_t - c_w[t], Dz = (x_t, u_t) - c_t.  A rollout whose cost is NaN is selected out (D = 0, y = 0)
whatever its w and trajectory hold.

The centre c_w, restated (`centre_w`): the w_t of the first rollout among the first min(K, 2^16) whose cost is not NaN; 0 where that value
is not finite, and everywhere if there is no such rollout.  It is the same for every row and known before the first chunk's sums.

`direct` is an independent answer: np.longdouble, the weighted means first and the covariances about them, no centre, no grouping.

`closed_form` is the tilted law itself for an LQ problem with kappa = 0 under an affine policy, from first principles: with the stacked
noise w = (w_0 .. w_{N-1}) ~ N(0, Sigma) the closed-loop trajectory is affine in w, z_t = zd_t + Mz_t w, the cost one quadratic form
J = c0 + b'w + 1/2 w'H w, and  exp(theta J) N(0, Sigma)  is, completing the square, the Gaussian with
Cov* = (Sigma^-1 - theta H)^-1 and E* w = theta Cov* b; Cov*(w_t, z_t) is the t-th block row of Cov* Mz_t'."""
import numpy as np

from wc_trajectory_model import CHUNK, NW, SLOTS, WAVES, tile


def centre_w(w, costs):
    """c_w [N, 16] of the device"""
    w = np.asarray(w, float)
    K, N, n = w.shape
    J = np.asarray(costs, float).ravel()
    c = np.zeros((N, 16))
    live = np.flatnonzero(~np.isnan(J[:min(K, CHUNK)]))
    if live.size:
        c[:, :n] = w[live[0]]
    return np.where(np.isfinite(c), c, 0.0)


def moments(w, x, u, costs, c_w, c_z, y, dead, cross=True):
    """mean_w [R, N, n], cov_w [R, N, n, n], cov_wz [R, N, n, n+m] (None without cross) and the kernel's own ESS [R], in the device's order"""
    w, x, u = np.asarray(w, float), np.asarray(x, float), np.asarray(u, float)
    K, N, n = w.shape
    m = u.shape[2]
    J = np.asarray(costs, float).ravel()
    ok = ~np.isnan(J)
    with np.errstate(all="ignore"):
        wt = np.zeros((K, N, 16))
        wt[:, :, :n] = w
        Dw = np.where(ok[:, None, None], wt - c_w[None], 0.0)
        Dz = np.where(ok[:, None, None], tile(x, u)[:, :N] - c_z[None, :N], 0.0)
    Dw[:, :, n:] = 0.0
    Dz[:, :, n:12] = 0.0
    Dz[:, :, 12 + m:] = 0.0
    if not cross:
        Dz[:] = 0.0
    y = np.where(ok[None, :], y, 0.0)
    R = y.shape[0]
    pWW, pWZ = np.zeros((R, SLOTS, N, 16, 16)), np.zeros((R, SLOTS, N, 16, 16))
    pS1w, pS1z = np.zeros((R, SLOTS, N, 16)), np.zeros((R, SLOTS, N, 16))
    pS0, pY2 = np.zeros((R, SLOTS)), np.zeros((R, SLOTS))
    for k0 in range(0, K, CHUNK):
        kc = min(CHUNK, K - k0)
        G = -(-kc // 4)
        It = -(-G // NW)
        Dwp, Dzp = np.zeros((It * NW * 4, N, 16)), np.zeros((It * NW * 4, N, 16))
        Dwp[:kc], Dzp[:kc] = Dw[k0:k0 + kc], Dz[k0:k0 + kc]
        yp = np.zeros((R, It * NW * 4))
        yp[:, :kc] = y[:, k0:k0 + kc]
        Dwp, Dzp = Dwp.reshape(It, NW, 4, N, 16), Dzp.reshape(It, NW, 4, N, 16)      # group it * NW + W belongs to wavefront W
        yp = yp.reshape(R, It, NW, 4)
        aww, awz = np.zeros((R, NW, N, 16, 16)), np.zeros((R, NW, N, 16, 16))
        s1w, s1z = np.zeros((R, NW, 4, N, 16)), np.zeros((R, NW, 4, N, 16))
        s0, sy2 = np.zeros((R, NW, 4)), np.zeros((R, NW, 4))
        for it in range(It):
            yd = yp[:, it, :, :, None, None] * Dwp[None, it]          # [R, NW, 4, N, 16]
            for kk in range(4):
                aww += yd[:, :, kk, :, :, None] * Dwp[None, it, :, kk, :, None, :]
                if cross:
                    awz += yd[:, :, kk, :, :, None] * Dzp[None, it, :, kk, :, None, :]
            s1w += yd
            if cross:
                s1z += yp[:, it, :, :, None, None] * Dzp[None, it]
            s0 += yp[:, it]
            sy2 += yp[:, it] * yp[:, it]
        aww, awz = aww.reshape(R, SLOTS, WAVES, N, 16, 16), awz.reshape(R, SLOTS, WAVES, N, 16, 16)
        s1w, s1z = s1w.reshape(R, SLOTS, WAVES, 4, N, 16), s1z.reshape(R, SLOTS, WAVES, 4, N, 16)
        s0, sy2 = s0.reshape(R, SLOTS, WAVES, 4), sy2.reshape(R, SLOTS, WAVES, 4)
        vww, vwz = np.zeros((R, SLOTS, N, 16, 16)), np.zeros((R, SLOTS, N, 16, 16))
        v1w, v1z = np.zeros((R, SLOTS, N, 16)), np.zeros((R, SLOTS, N, 16))
        v0, vy = np.zeros((R, SLOTS)), np.zeros((R, SLOTS))
        for wv in range(WAVES):
            vww += aww[:, :, wv]
            vwz += awz[:, :, wv]
            for kk in range(4):
                v1w += s1w[:, :, wv, kk]
                v1z += s1z[:, :, wv, kk]
                v0 += s0[:, :, wv, kk]
                vy += sy2[:, :, wv, kk]
        pWW += vww
        pWZ += vwz
        pS1w += v1w
        pS1z += v1z
        pS0 += v0
        pY2 += vy
    SWW, SWZ, S1w, S1z, S0, Y2 = (np.zeros_like(p[:, 0]) for p in (pWW, pWZ, pS1w, pS1z, pS0, pY2))
    for s in range(SLOTS):
        SWW += pWW[:, s]
        SWZ += pWZ[:, s]
        S1w += pS1w[:, s]
        S1z += pS1z[:, s]
        S0 += pS0[:, s]
        Y2 += pY2[:, s]
    idx = list(range(n)) + list(range(12, 12 + m))
    with np.errstate(all="ignore"):
        mw, mz = S1w / S0[:, None, None], S1z / S0[:, None, None]
        S2u = np.triu(SWW) + np.triu(SWW, 1).swapaxes(-1, -2)
        cov_w = S2u / S0[:, None, None, None] - mw[..., :, None] * mw[..., None, :]
        cov_wz = SWZ / S0[:, None, None, None] - mw[..., :, None] * mz[..., None, :]
        mean_w = c_w[None] + mw
        ess = S0 * S0 / Y2
    mean_w, cov_w, cov_wz = mean_w[:, :, :n], cov_w[:, :, :n, :n], cov_wz[:, :, :n][:, :, :, idx]
    mean_w[dead], cov_w[dead], cov_wz[dead] = np.nan, np.nan, np.nan
    return mean_w, cov_w, (cov_wz if cross else None), ess


def dense_z(x, u):
    """(K, N+1, n), (K, N, m) -> (K, N, n+m): (x_t, u_t) at the steps that have a disturbance"""
    x, u = np.asarray(x, float), np.asarray(u, float)
    return np.concatenate([x[:, :u.shape[1]], u], axis=2)


def direct(w, x, u, costs, y, dead, want_se=False):
    """the same in np.longdouble, straight from the definition: means sum p v, covariances sum p (a - mean_a)(b - mean_b)', p = y / sum y.
    want_se: also the delta-method standard error of every entry as a self-normalised estimate, sqrt(sum p_k^2 (phi_k - phi_hat)^2) with
    phi_k = w_k for a mean and (a_k - mean_a)(b_k - mean_b) for a covariance entry, from the same rollouts"""
    w = np.asarray(w, float)
    K, N, n = w.shape
    ok = ~np.isnan(np.asarray(costs, float).ravel())
    wl, zl = w[ok].astype(np.longdouble), dense_z(x, u)[ok].astype(np.longdouble)
    R, d = y.shape[0], zl.shape[2]
    mean, cov, cwz = np.full((R, N, n), np.nan), np.full((R, N, n, n), np.nan), np.full((R, N, n, d), np.nan)
    se = tuple(np.full_like(a, np.nan) for a in (mean, cov, cwz))
    for r in range(R):
        if dead[r]:
            continue
        p = y[r][ok].astype(np.longdouble)
        p = p / p.sum()
        for t in range(N):
            mu, mz = (p[:, None] * wl[:, t]).sum(axis=0), (p[:, None] * zl[:, t]).sum(axis=0)
            wc, zc = wl[:, t] - mu, zl[:, t] - mz
            cw, cz = np.dot((wc * p[:, None]).T, wc), np.dot((wc * p[:, None]).T, zc)
            mean[r, t], cov[r, t], cwz[r, t] = mu.astype(np.float64), cw.astype(np.float64), cz.astype(np.float64)
            if want_se:
                p2 = p * p
                se[0][r, t] = np.sqrt((p2[:, None] * wc * wc).sum(axis=0)).astype(np.float64)
                se[1][r, t] = np.sqrt((p2[:, None, None] * (wc[:, :, None] * wc[:, None, :] - cw[None]) ** 2).sum(axis=0)).astype(np.float64)
                se[2][r, t] = np.sqrt((p2[:, None, None] * (wc[:, :, None] * zc[:, None, :] - cz[None]) ** 2).sum(axis=0)).astype(np.float64)
    return (mean, cov, cwz) + ((se,) if want_se else ())


def deviation(got, ref, c_w, zs=None, K=1):
    """(worst mean_w, cov_w, cov_wz deviation) over rows and steps, each relative to its step's scale, as wc_trajectory_model.deviation
    takes it: the mean against the larger of its largest entry and the step's largest standard deviation of w; cov_w against its largest
    entry -- where that is exactly zero, or below what `direct` itself can resolve ((8 + K) eps_longdouble |w|)^2, against the largest
    squared offset of the mean from the centre; cov_wz against sd(w) sd(z), the largest standard deviation of w times z_off [R, N]: the
    largest of sd(z) and |mean_z - c_z| at the step (where all of (x_t, u_t) is one point -- x_0, an open-loop u_t -- that offset from
    the centre is the size of the terms cov_wz is the difference of), after what `direct` cannot resolve of a z that does not vary --
    there its z - mean_z and its sum p (w - mean_w) are both its own rounding, ((8 + K) eps_longdouble)^2 |z| |w| their product -- is
    taken off.  zs = (z_off, z_abs) [R, N] each: `z_offset` of the reference moments of (x_t, u_t).
    got / ref: (mean_w, cov_w, cov_wz or None).  NaN must meet NaN."""
    eps_ld = float(np.finfo(np.longdouble).eps)
    tiny = np.finfo(float).tiny
    (mean, cov, cwz), (mean_r, cov_r, cwz_r) = got, ref
    assert np.array_equal(np.isnan(mean), np.isnan(mean_r)) and np.array_equal(np.isnan(cov), np.isnan(cov_r))
    dm = dc = dz = 0.0
    for r in range(mean.shape[0]):
        if np.isnan(mean_r[r]).any():
            continue
        for t in range(mean.shape[1]):
            own = ((8.0 + K) * eps_ld * np.abs(mean_r[r, t]).max()) ** 2
            sc = np.abs(cov_r[r, t]).max()
            off2 = ((mean_r[r, t] - c_w[t]) ** 2).max()
            if sc <= own:
                sc = max(off2, tiny)
            sd_w = np.sqrt(max(np.abs(cov_r[r, t]).max(), off2))
            sm = max(np.abs(mean_r[r, t]).max(), np.sqrt(np.abs(cov_r[r, t]).max()), tiny)
            dc = max(dc, float(max(np.abs(cov[r, t] - cov_r[r, t]).max() - own, 0.0) / sc))
            dm = max(dm, float(np.abs(mean[r, t] - mean_r[r, t]).max() / sm))
            if cwz is not None and zs is not None:
                assert np.array_equal(np.isnan(cwz[r, t]), np.isnan(cwz_r[r, t]))
                own_z = ((8.0 + K) * eps_ld) ** 2 * zs[1][r, t] * max(sd_w, np.abs(mean_r[r, t]).max())
                dz = max(dz, float(max(np.abs(cwz[r, t] - cwz_r[r, t]).max() - own_z, 0.0) / max(sd_w * zs[0][r, t], tiny)))
    return dm, dc, dz


def z_offset(mean_z, cov_z, c_z_dense):
    """(z_off, z_abs) [R, N] of `deviation` from reference moments of (x_t, u_t): mean_z [R, N, d], cov_z [R, N, d, d], the centre [N, d]"""
    sd = np.sqrt(np.abs(np.diagonal(cov_z, axis1=-2, axis2=-1)).max(axis=-1))
    return np.maximum(sd, np.abs(mean_z - c_z_dense[None]).max(axis=-1)), np.abs(mean_z).max(axis=-1)


def closed_form(prob, x0, l, L, xbar, theta):
    """(mean_w [N, n], cov_w [N, n, n], cov_wz [N, n, n+m], feasible, lam_max) of exp(theta J) q for u_k = l_k + L_k (x_k - xbar_k) from x_0
    on an LQRiskSensitiveProblem with kappa = 0 (L None: open loop); lam_max is the largest eigenvalue of C'HC, Sigma = C C': the tilt
    exists for theta lam_max < 1"""
    n, m, N = prob.n, prob.m, prob.N
    assert prob.kappa == 0.0
    A, B = np.asarray(prob.A, float), np.asarray(prob.B, float)
    l = np.asarray(l, float)
    L = np.zeros((N, m, n)) if L is None else np.asarray(L, float)
    xbar = np.zeros((N + 1, n)) if xbar is None else np.asarray(xbar, float)
    tv = lambda tab, k: tab[k] if prob.cost_tv else tab
    off = l - np.einsum("kij,kj->ki", L, xbar[:N])                    # u_k = off_k + L_k x_k
    xd, Mx = np.zeros((N + 1, n)), np.zeros((N + 1, n, N * n))        # x_k = xd_k + Mx_k w
    xd[0] = x0
    for k in range(N):
        Acl = A + B @ L[k]
        xd[k + 1] = Acl @ xd[k] + B @ off[k]
        Mx[k + 1] = Acl @ Mx[k]
        Mx[k + 1][:, k * n:(k + 1) * n] += np.eye(n)
    ud = off + np.einsum("kij,kj->ki", L, xd[:N])
    Mu = np.einsum("kij,kjc->kic", L, Mx[:N])
    b, H = np.zeros(N * n), np.zeros((N * n, N * n))
    for k in range(N):                                               # the gradient and the Hessian of J in w, term by term
        Q, R, P, qv, rv = (np.asarray(tv(t, k), float) for t in (prob.Q, prob.R, prob.P, prob.qv, prob.rv))
        X, U = Mx[k], Mu[k]
        b += X.T @ (Q @ xd[k] + qv + P.T @ ud[k]) + U.T @ (R @ ud[k] + rv + P @ xd[k])
        H += X.T @ Q @ X + U.T @ R @ U + U.T @ P @ X + X.T @ P.T @ U
    b += Mx[N].T @ (prob.Qf @ xd[N] + prob.qvf)
    H += Mx[N].T @ prob.Qf @ Mx[N]
    H = 0.5 * (H + H.T)
    Sig = np.zeros((N * n, N * n))
    for k in range(N):
        Sig[k * n:(k + 1) * n, k * n:(k + 1) * n] = prob.W(k)
    C = np.linalg.cholesky(Sig)
    G = C.T @ H @ C
    lam = float(np.linalg.eigvalsh(0.5 * (G + G.T)).max())
    Kin = np.eye(N * n) - theta * G                                   # Sigma^-1 - theta H = C^-T (I - theta C'HC) C^-1
    feasible = theta * lam < 1.0
    cov = C @ np.linalg.solve(0.5 * (Kin + Kin.T), C.T)
    cov = 0.5 * (cov + cov.T)
    mean = theta * cov @ b
    mean_w, cov_w, cov_wz = np.zeros((N, n)), np.zeros((N, n, n)), np.zeros((N, n, n + m))
    for t in range(N):
        sl = slice(t * n, (t + 1) * n)
        mean_w[t], cov_w[t] = mean[sl], cov[sl, sl]
        cov_wz[t] = cov[sl] @ np.concatenate([Mx[t], Mu[t]], axis=0).T
    return mean_w, cov_w, cov_wz, feasible, lam
