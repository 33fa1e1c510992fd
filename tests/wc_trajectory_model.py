"""NumPy model of rat_policy_worst_case_trajectory's moment kernels (csrc/policy_mc.hip: wct_weights, wct_moments, wct_final) -- test aid.

`moments` restates the device's schedule: the rollouts in chunks of 2^16; inside a chunk groups of four rollouts, group g belonging to
wavefront g mod 32 (slot g mod 32 // 4, wavefront g mod 4 of the slot), each wavefront adding its groups in order -- one product
sum_k (y D_i)(D_j) over the four rollouts of a group per step and row, as the MFMA forms it -- the wavefronts of a slot and the four rollout
lanes added in index order into the slot's partial, chunk after chunk, the eight slots added in index order, then
mean = c + S1 / S0 and cov = S2 / S0 - (S1 / S0)(S1 / S0)' with the upper triangle of S2 serving both halves.  D = z - c about the centre
c the caller gives; a rollout whose cost is NaN is selected out (D = 0, y = 0) whatever its trajectory holds.

`direct` is an independent answer: np.longdouble, the weighted mean first and the covariance about it, no centre, no grouping."""
import numpy as np

from worst_case_model import EMPTY, NONFINITE, SATURATED, worst_case

CHUNK, SLOTS, WAVES = 1 << 16, 8, 4
NW = SLOTS * WAVES


def tile(x, u):
    """(K, N+1, n), (K, N, m) -> (K, N+1, 16): the 12 + 4 tile, zero padded; u at step N is 0"""
    K, T, n = x.shape
    z = np.zeros((K, T, 16))
    z[:, :, :n] = x
    z[:, :T - 1, 12:12 + u.shape[2]] = u
    return z


def centre(x_c, l):
    """the centre of the device: (x_c[t], l[t]) in the tile, 0 where not finite"""
    c = tile(np.asarray(x_c, float)[None], np.asarray(l, float)[None])[0]
    return np.where(np.isfinite(c), c, 0.0)


def weights_from_rows(costs, theta, flag):
    """y [R, K] and dead [R] from the rows' theta and flag: exp(theta (J - Jmax)), 1 at theta = 0, the maxima alone on a saturated row,
    nothing on an empty or non-finite sample; 0 at a NaN cost"""
    J = np.asarray(costs, dtype=np.float64).ravel()
    th, fl = np.asarray(theta, float).ravel(), np.asarray(flag).ravel()
    ok = ~np.isnan(J)
    Jmax = J[ok].max() if ok.any() else np.nan
    y = np.zeros((th.size, J.size))
    with np.errstate(all="ignore"):
        for r in range(th.size):
            if fl[r] in (EMPTY, NONFINITE):
                continue
            if fl[r] == SATURATED:
                y[r] = np.where(ok & (J == Jmax), 1.0, 0.0)
            elif th[r] == 0.0:
                y[r] = np.where(ok, 1.0, 0.0)
            else:
                y[r] = np.where(ok, np.exp(th[r] * (np.where(ok, J, Jmax) - Jmax)), 0.0)
    return y, np.array([f in (EMPTY, NONFINITE) for f in fl], dtype=bool)


def row_weights(costs, kl_bounds=(), thetas=()):
    """(y [R, K], dead [R], rows): the weight of every rollout per row -- bounds, then thetas -- from the rows of worst_case_model"""
    wc = worst_case(np.asarray(costs, dtype=np.float64).ravel(), kl_bounds, thetas)
    y, dead = weights_from_rows(costs, np.concatenate([wc["bounds"]["theta"], wc["thetas"]["theta"]]),
                                np.concatenate([wc["bounds"]["flag"], wc["thetas"]["flag"]]))
    return y, dead, wc


def moments(x, u, costs, c, y, dead):
    """mean [R, N+1, n+m] and cov [R, N+1, n+m, n+m] in the device's order"""
    x, u = np.asarray(x, float), np.asarray(u, float)
    K, T, n = x.shape
    m = u.shape[2]
    J = np.asarray(costs, float).ravel()
    ok = ~np.isnan(J)
    with np.errstate(all="ignore"):
        D = np.where(ok[:, None, None], tile(x, u) - c[None], 0.0)
    D[:, :, n:12] = 0.0
    D[:, :, 12 + m:] = 0.0
    D[:, T - 1, 12:] = 0.0
    y = np.where(ok[None, :], y, 0.0)
    R = y.shape[0]
    pS2, pS1 = np.zeros((R, SLOTS, T, 16, 16)), np.zeros((R, SLOTS, T, 16))
    pS0, pY2 = np.zeros((R, SLOTS)), np.zeros((R, SLOTS))
    for k0 in range(0, K, CHUNK):
        kc = min(CHUNK, K - k0)
        G = -(-kc // 4)
        It = -(-G // NW)
        Dp = np.zeros((It * NW * 4, T, 16))
        Dp[:kc] = D[k0:k0 + kc]
        yp = np.zeros((R, It * NW * 4))
        yp[:, :kc] = y[:, k0:k0 + kc]
        Dp = Dp.reshape(It, NW, 4, T, 16)                   # group it * NW + W belongs to wavefront W
        yp = yp.reshape(R, It, NW, 4)
        acc = np.zeros((R, NW, T, 16, 16))
        s1 = np.zeros((R, NW, 4, T, 16))
        s0, sy2 = np.zeros((R, NW, 4)), np.zeros((R, NW, 4))
        for it in range(It):
            yd = yp[:, it, :, :, None, None] * Dp[None, it]  # [R, NW, 4, T, 16]
            for kk in range(4):
                acc += yd[:, :, kk, :, :, None] * Dp[None, it, :, kk, :, None, :]
            s1 += yd
            s0 += yp[:, it]
            sy2 += yp[:, it] * yp[:, it]
        acc = acc.reshape(R, SLOTS, WAVES, T, 16, 16)
        s1 = s1.reshape(R, SLOTS, WAVES, 4, T, 16)
        s0, sy2 = s0.reshape(R, SLOTS, WAVES, 4), sy2.reshape(R, SLOTS, WAVES, 4)
        v2, v1 = np.zeros((R, SLOTS, T, 16, 16)), np.zeros((R, SLOTS, T, 16))
        v0, vy = np.zeros((R, SLOTS)), np.zeros((R, SLOTS))
        for w in range(WAVES):
            v2 += acc[:, :, w]
            for kk in range(4):
                v1 += s1[:, :, w, kk]
                v0 += s0[:, :, w, kk]
                vy += sy2[:, :, w, kk]
        pS2 += v2
        pS1 += v1
        pS0 += v0
        pY2 += vy
    S2, S1, S0, Y2 = (np.zeros_like(p[:, 0]) for p in (pS2, pS1, pS0, pY2))
    for s in range(SLOTS):
        S2 += pS2[:, s]
        S1 += pS1[:, s]
        S0 += pS0[:, s]
        Y2 += pY2[:, s]
    idx = list(range(n)) + list(range(12, 12 + m))
    with np.errstate(all="ignore"):
        mu = S1 / S0[:, None, None]
        S2u = np.triu(S2) + np.triu(S2, 1).swapaxes(-1, -2)
        cov = S2u / S0[:, None, None, None] - mu[..., :, None] * mu[..., None, :]
        mean = c[None] + mu
    mean, cov = mean[:, :, idx], cov[:, :, idx][:, :, :, idx]
    mean[dead], cov[dead] = np.nan, np.nan
    with np.errstate(all="ignore"):
        ess = S0 * S0 / Y2
    return mean, cov, ess


def direct(x, u, costs, y, dead):
    """the same in np.longdouble, straight from the definition: mean = sum w z, cov = sum w (z - mean)(z - mean)', w = y / sum y"""
    x, u = np.asarray(x, float), np.asarray(u, float)
    K, T, n = x.shape
    m = u.shape[2]
    ok = ~np.isnan(np.asarray(costs, float).ravel())
    idx = list(range(n)) + list(range(12, 12 + m))
    z = tile(x, u)[ok][:, :, idx].astype(np.longdouble)
    R, d = y.shape[0], n + m
    mean, cov = np.full((R, T, d), np.nan), np.full((R, T, d, d), np.nan)
    for r in range(R):
        if dead[r]:
            continue
        w = y[r][ok].astype(np.longdouble)
        w = w / w.sum()
        for t in range(T):
            mu = (w[:, None] * z[:, t]).sum(axis=0)
            zc = z[:, t] - mu
            mean[r, t] = mu.astype(np.float64)
            cov[r, t] = np.dot((zc * w[:, None]).T, zc).astype(np.float64)
    return mean, cov


def split(mean, cov, n, m):
    """the parts Context.policy_worst_case_trajectory returns"""
    return dict(mean_x=mean[:, :, :n], cov_x=cov[:, :, :n, :n], mean_u=mean[:, :-1, n:], cov_u=cov[:, :-1, n:, n:], cov_xu=cov[:, :-1, :n, n:])


def deviation(mean, cov, mean_ref, cov_ref, c_dense, K=1):
    """(worst mean deviation, worst covariance deviation) over rows and steps, each relative to its step's scale: the covariance against the
    largest covariance entry of the step -- where that is exactly zero (one rollout carries all the weight) against the largest squared
    offset of the mean from the centre, the size of the two terms whose difference the covariance is -- and the mean against the larger of
    its largest entry and the step's largest standard deviation.  What the reference itself cannot resolve is taken off first: `direct`
    forms z - mean in np.longdouble, so where every rollout is at the same point (x_0, or an open-loop u_t) its covariance is not 0 but
    the square of its rounding of z - mean, of order (eps_longdouble |z|)^2 times at most K^2 for the K terms of its mean; ((8 + K) eps_longdouble |z|)^2 is allowed, below 1e-28 |z|^2
    at K = 2^18.  NaN must meet NaN."""
    assert np.array_equal(np.isnan(mean), np.isnan(mean_ref)) and np.array_equal(np.isnan(cov), np.isnan(cov_ref))
    eps_ld = float(np.finfo(np.longdouble).eps)
    dm = dc = 0.0
    for r in range(mean.shape[0]):
        if np.isnan(mean_ref[r]).any():
            continue
        for t in range(mean.shape[1]):
            own = ((8.0 + K) * eps_ld * np.abs(mean_ref[r, t]).max()) ** 2
            sc = np.abs(cov_ref[r, t]).max()
            if sc <= own:
                sc = max(((mean_ref[r, t] - c_dense[t]) ** 2).max(), np.finfo(float).tiny)
            sm = max(np.abs(mean_ref[r, t]).max(), np.sqrt(np.abs(cov_ref[r, t]).max()), np.finfo(float).tiny)
            dc = max(dc, float(max(np.abs(cov[r, t] - cov_ref[r, t]).max() - own, 0.0) / sc))
            dm = max(dm, float(np.abs(mean[r, t] - mean_ref[r, t]).max() / sm))
    return dm, dc
