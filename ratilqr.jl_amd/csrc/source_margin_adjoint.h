// source_margin_adjoint.h -- the adjoint sweep of rat_policy_margin_gradient (include/ratilqr.h): dM_ik / du_t of every replayed rollout k
// of a source model for every event i of the call, M_ik = max over the window of g_i(t, z_t), g_i(t, z) = z' Q_i z + a_i' z + b_i of
// z = (x_t, u_t), with the recorded disturbances held fixed and the loop closed downstream.  Compiled by hiprtc behind the user's source;
// RAT_N and RAT_M come from the command line, and so does RAT_N_MARGIN, the events of the call (1 .. 4).  A module of its own (kind
// SRC_MARGIN_ADJOINT), compiled by the first margin-gradient call.
//
//   t*       = the first step of the window that attains M_ik: NOT recomputed here.  ev_eval's sibling (launch_ev_argmax, policy_mc.hip)
//              forms g on the matrix cores and records the step with the margin; a plain-FMA g here could order two near-equal steps the
//              other way.  t* = -1: the margin is NaN (every g of the window is), the sweep is all zeros and the rollout has no weight.
//   at t*      g_z = (Q_i + Q_i') z + a_i,  z = (x_t*, u_t*), u_N = 0;   gu_t* = its u part (t* < N);   lambda_t* = its x part + L_t*' gu_t*
//   t > t*     gu_t = 0, exactly
//   t < t*     g_t = f_z(x_t, u_t)' lambda_{t+1};   gu_t = its u part;   lambda_t = its x part + L_t' gu_t   (open loop: the x part alone)
//
// The team of source_adjoint_lanes.h, with one lambda per event.  The events are swept JOINTLY: per step one column of f_z per lane, dotted
// with each event's lambda (j = 0 .. n - 1 in order, fused multiply-adds from 0), and one close per event.  An event whose t* lies below
// the step contributes exact zeros by SELECTION, not through 0 * f_z (which is NaN where f_z is not finite) and not by a branch around
// the exchanges.  What a team may skip is the evaluation of f at the steps t >= max_i t*, where no event of the rollout reads it: that
// holds no exchange.
// g_z at t* costs sixteen exchanges of z within the team and sixteen fused multiply-adds against the lane's row of Q_i + Q_i', which the
// workgroup forms once in LDS from the tile the events call uploads (entry (k, i) at k * 16 + i: Q_i's row i, column k); no AD, no MFMA.
//
// A rollout without a cost (NaN: DomainError) is passed over: nothing is loaded, computed or stored for it, and the moment kernel
// selects it out.  A rollout with a cost whose sensitivities for event i hold a NaN or an Inf anywhere (g_z at t*, any component of any
// g_t below) is flagged in bad[i] and counted in n_bad[i]; its gu is stored as it came out and is selected out downstream, never
// multiplied.  An event's sweep reads nothing of another event's but the shared f_z: its bits do not depend on the other events.
#pragma once

#ifndef RAT_USER_NOISE
#error "the source does not define RAT_USER_NOISE: rat_policy_margin_gradient replays rat_policy_evaluate_noise, which needs '#define RAT_USER_NOISE' and rat_user_noise(k, x, u, rng, w, p)"
#endif
#ifdef RAT_USER_POLICY
#error "the source defines RAT_USER_POLICY: rat_user_policy is not templated, so the control law is not differentiable by rat_ad.h (rat_policy_margin_gradient serves the affine law alone)"
#endif
#if RAT_N_MARGIN < 1 || RAT_N_MARGIN > SRC_MARGIN_MAX
#error "RAT_N_MARGIN must be in 1 .. 4"
#endif
#include "source_adjoint_lanes.h"

extern "C" __global__ __launch_bounds__(64) void rat_src_margin_adjoint(SrcMarginArgs a) {
    constexpr int E = RAT_N_MARGIN;
    __shared__ double s_S[E * 256];                                   // Q_e + Q_e' in the tile: entry (i, k) at e * 256 + k * 16 + i
    __shared__ double s_a[E * 16];
#ifdef RAT_USER_F_JACOBIAN
    __shared__ double s_col[4][ADJ_COLUMNS];
#else
    double (*const s_col)[ADJ_COLUMNS] = nullptr;
#endif
    const AdjTeam T(a);
    const int N = a.N, i = T.i;
    if (a.quad) {
        for (int e = T.lane; e < E * 256; e += 64) {
            const int ev = e >> 8, k = (e >> 4) & 15, r = e & 15;
            s_S[e] = a.Qt[ev * 256 + k * 16 + r] + a.Qt[ev * 256 + r * 16 + k];
        }
    }
    for (int e = T.lane; e < E * 16; e += 64) s_a[e] = a.at[e];
    __syncthreads();
    int ts[E], tmax = -1;
    double sd[E], lam[E][RAT_N];
    bool bad[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {                                     // g_z at t*, component i, and lambda_N
        ts[e] = T.ok ? a.tstar[(long)e * a.ldt + T.q] : -1;
        if (ts[e] < 0 || ts[e] > N) ts[e] = -1;                       // (nothing outside 0 .. N is ever an index)
        tmax = ts[e] > tmax ? ts[e] : tmax;
        double z = 0.0;
        if (T.act && ts[e] >= 0) {
            if (T.isx) z = T.xq[(long)ts[e] * RAT_N + i];
            else if (ts[e] < N) z = T.uq[(long)ts[e] * RAT_M + (i - 12)];
        }
        double g = s_a[e * 16 + i];
        if (a.quad) {
#pragma unroll
            for (int k = 0; k < 16; ++k) g = __builtin_fma(s_S[e * 256 + k * 16 + i], adj_from(z, T.team + k), g);
        }
        const bool seeded = T.act && ts[e] >= 0 && (T.isx || ts[e] < N);   // (u_N = 0 is no variable: t* = N has no u part)
        sd[e] = seeded ? g : 0.0;
        bad[e] = seeded && !adj_finite(g);
        const double l0 = (ts[e] == N && T.isx) ? sd[e] : 0.0;
#pragma unroll
        for (int j = 0; j < RAT_N; ++j) lam[e][j] = adj_from(l0, T.team + j);
    }
    for (int t = N - 1; t >= 0; --t) {
        const bool need = t < tmax;                                   // (uniform over the team: some event of the rollout reads f_z here)
        adj_jacobian(T, t, a.p, need, s_col[T.kk]);
        double col[RAT_N];                                            // column zi of [f_x | f_u]
#pragma unroll
        for (int j = 0; j < RAT_N; ++j) col[j] = 0.0;
        if (T.act && need) {
            rat_dual xd[RAT_N], ud[RAT_M];
            adj_seed(T, t, xd, ud);
            adj_column(T, xd, ud, a.p, s_col[T.kk], col);
        }
        adj_columns_read();
#pragma unroll
        for (int e = 0; e < E; ++e) {
            double dot = 0.0;
#pragma unroll
            for (int j = 0; j < RAT_N; ++j) dot = __builtin_fma(col[j], lam[e][j], dot);
            const double g = !T.act ? 0.0 : (t < ts[e]) ? dot : (t == ts[e]) ? sd[e] : 0.0;   // selected: above t* exact zeros
            bad[e] = bad[e] || !adj_finite(g);
            (void)adj_close(T, t, g, a.L, lam[e]);
            if (T.ok && !T.isx) a.gu[((T.q * E + e) * N + t) * 4 + (i - 12)] = g;   // (zero in a padding lane)
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) adj_flag(T, bad[e], a.bad, (long)e * a.ldb + T.q, a.n_bad + e);
}
