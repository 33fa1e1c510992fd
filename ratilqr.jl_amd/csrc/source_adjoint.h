// source_adjoint.h -- the adjoint sweep of rat_policy_gradient / rat_policy_tail_gradient (include/ratilqr.h): dJ_k / du_t of every
// replayed rollout of a source model, with the recorded disturbances held fixed and the loop closed downstream.  Compiled by hiprtc
// behind the user's source; RAT_N and RAT_M come from the command line.  A module of its own (kind SRC_ADJOINT), compiled by the first
// gradient call.
//
//   lambda_N = h_x(x_N)
//   g_t      = c_z(t, x_t, u_t) + f_z(x_t, u_t)' lambda_{t+1},   z = (x, u),   t = N - 1 .. 0
//   gu_t     = the u part of g_t
//   lambda_t = (x part of g_t) + L_t' gu_t        (open loop, L == NULL: the x part alone)
//
// The team, its exchanges and the Jacobian hook are source_adjoint_lanes.h's.  What is this kernel's own: component i of g_t is c's
// partial from one rat_dual evaluation of rat_user_c, and behind it the lane's column of f_z dotted with lambda (j = 0 .. n - 1 in order,
// fused multiply-adds); c and h stay by AD under the hook.
//
// A rollout without a cost (NaN: DomainError) is passed over: nothing is loaded, computed or stored for it, and the moment kernel
// selects it out.  A rollout with a cost whose sensitivities hold a NaN or an Inf anywhere (h_x, any component of any g_t) is flagged in
// bad and counted; its gu is stored as it came out and is selected out downstream, never multiplied.
#pragma once

#ifndef RAT_USER_NOISE
#error "the source does not define RAT_USER_NOISE: rat_policy_gradient replays rat_policy_evaluate_noise, which needs '#define RAT_USER_NOISE' and rat_user_noise(k, x, u, rng, w, p)"
#endif
#ifdef RAT_USER_POLICY
#error "the source defines RAT_USER_POLICY: rat_user_policy is not templated, so the control law is not differentiable by rat_ad.h (rat_policy_gradient serves the affine law alone)"
#endif
#include "source_adjoint_lanes.h"

extern "C" __global__ __launch_bounds__(64) void rat_src_adjoint(SrcAdjointArgs a) {
#ifdef RAT_USER_F_JACOBIAN
    __shared__ double s_col[4][ADJ_COLUMNS];
#else
    double (*const s_col)[ADJ_COLUMNS] = nullptr;
#endif
    const AdjTeam T(a);
    const int N = a.N;
    double lam[RAT_N];
    bool bad = false;
    adj_terminal(T, N, a.p, lam, bad);
    for (int t = N - 1; t >= 0; --t) {
        adj_jacobian(T, t, a.p, true, s_col[T.kk]);
        double g = 0.0;
        if (T.act) {
            rat_dual xd[RAT_N], ud[RAT_M];
            double col[RAT_N];
            adj_seed(T, t, xd, ud);
            g = rat_user_c<rat_dual>(t, xd, ud, a.p).d;               // c_z, component zi
            adj_column(T, xd, ud, a.p, s_col[T.kk], col);
#pragma unroll
            for (int j = 0; j < RAT_N; ++j) g = __builtin_fma(col[j], lam[j], g);
            bad = bad || !adj_finite(g);
        }
        adj_columns_read();
        (void)adj_close(T, t, g, a.L, lam);
        if (T.ok && !T.isx) a.gu[(T.q * N + t) * 4 + (T.i - 12)] = g; // (zero in a padding lane)
    }
    adj_flag(T, bad, a.bad, T.q, a.n_bad);
}
