// source_adjoint_params.h -- the adjoint sweep of rat_policy_param_gradient / rat_policy_tail_param_gradient (include/ratilqr.h):
// dJ_k / dp and dJ_k / dx_0 of every replayed rollout of a source model, with the recorded disturbances and the control law held fixed.
// Compiled by hiprtc behind the user's source, which defines RAT_USER_PARAMS_AD: its rat_user_f, rat_user_c and rat_user_h are templated
// on a second type P for the parameters.  RAT_N, RAT_M and RAT_N_PARAMS (0 .. 32: the problem's parameter count) come from the command
// line.  A module of its own (kind SRC_ADJOINT_P), compiled by the first call; it is the only module that instantiates T = P = rat_dual.
//
//   lambda_N = h_x(x_N),                                        gp  = h_p(x_N)
//   g_t      = c_z(t, x_t, u_t) + f_z(x_t, u_t)' lambda_{t+1},  gp += c_p(t, x_t, u_t) + f_p(x_t, u_t)' lambda_{t+1},   t = N - 1 .. 0
//   lambda_t = (x part of g_t) + L_t' gu_t                      (open loop, L == NULL: the x part alone)
//   dJ_k / dp = gp,   dJ_k / dx_0 = lambda_0
//
// The lambda recursion is rat_src_adjoint's (source_adjoint.h) on the team of source_adjoint_lanes.h; gu is not stored.  The parameter
// pass rides on it: lane i evaluates c and f once more at (x_t, u_t) as duals of zero tangent with p as rat_dual[RAT_N_PARAMS] seeded in
// direction i (and, with more than sixteen parameters, again in direction 16 + i); c's partial and, behind it, the lane's column of f_p
// dotted with lambda_{t+1} (j = 0 .. n - 1 in order, fused multiply-adds) is the step's term, added to the lane's gp.  No cross-lane
// traffic; a lane with no parameter evaluates nothing and holds an exact zero.  With RAT_USER_F_JACOBIAN the hook serves f_x, f_u; f_p
// always comes from AD of rat_user_f.
//
// With parameter sampling on (RAT_USER_PARAMS_ON) every lane forms the rollout's own q again from the replayed seed and the global
// rollout index, as rat_src_user_events does, and everything above is evaluated at q: the derivative is with respect to a common
// additive shift of the drawn parameters.  rat_user_params itself is not differentiated.
//
// A rollout without a cost (NaN: DomainError) is passed over by predicate.  A rollout with a cost but a NaN or Inf in h_x, any g_t, h_p or
// any parameter term is flagged in bad and counted; what it stores is selected out downstream, never multiplied.
#pragma once

#ifndef RAT_USER_NOISE
#error "the source does not define RAT_USER_NOISE: rat_policy_param_gradient replays rat_policy_evaluate_noise, which needs '#define RAT_USER_NOISE' and rat_user_noise(k, x, u, rng, w, p)"
#endif
#ifdef RAT_USER_POLICY
#error "the source defines RAT_USER_POLICY: rat_user_policy is not templated, so the control law is not differentiable by rat_ad.h (rat_policy_param_gradient serves the affine law alone)"
#endif
#ifndef RAT_USER_PARAMS_AD
#error "the source does not define RAT_USER_PARAMS_AD: rat_policy_param_gradient differentiates with respect to p, which needs '#define RAT_USER_PARAMS_AD' and rat_user_f, rat_user_c, rat_user_h templated on the parameters' type (template <class T, class P> ... const P *p)"
#endif
#if !defined(RAT_N_PARAMS) || RAT_N_PARAMS < 0 || RAT_N_PARAMS > 32
#error "rat_policy_param_gradient is compiled for 0 .. 32 parameters (RAT_N_PARAMS)"
#endif
#include "source_adjoint_lanes.h"
#include "source_params.h"

#define ADJP_TILES ((RAT_N_PARAMS + 15) / 16)                         /* parameter tiles of sixteen directions: 0, 1 or 2 */

#if RAT_N_PARAMS > 0
// p with direction `dir` seeded
__device__ __forceinline__ void adjp_seed(const double *p, int dir, rat_dual (&pd)[RAT_N_PARAMS]) {
#pragma unroll
    for (int j = 0; j < RAT_N_PARAMS; ++j) pd[j] = rat_dual(p[j], j == dir ? 1.0 : 0.0);
}
#endif

extern "C" __global__ __launch_bounds__(64) void rat_src_adjoint_p(SrcAdjointPArgs a) {
#ifdef RAT_USER_F_JACOBIAN
    __shared__ double s_col[4][ADJ_COLUMNS];
#else
    double (*const s_col)[ADJ_COLUMNS] = nullptr;
#endif
    const AdjTeam T(a);
    const int N = a.N, i = T.i;
    const bool ok = T.ok;
    const double *__restrict__ xq = T.xq, *__restrict__ uq = T.uq;
    // the rollout's parameters: the problem's, or with sampling on its own q (an overdraw or a NaN there was the rollout kernel's to
    // report: the stored cost is NaN)
    src_rollout_params own;
    int pover = 0;
    if (ok) (void)own.draw(T.q + a.j0, a.seed, a.zpn, a.zpu, a.p, pover);
    const double *p = own.of(a.p);
    double lam[RAT_N], gp[2] = {0.0, 0.0}, l0 = 0.0;
    bool bad = false;
#if RAT_N_PARAMS > 0
#pragma unroll
    for (int b = 0; b < ADJP_TILES; ++b) {                            // gp = h_p(x_N), direction 16 b + i (ahead of lambda_N: fewer live registers)
        if (ok && 16 * b + i < RAT_N_PARAMS) {
            rat_dual xd[RAT_N], pd[RAT_N_PARAMS];
#pragma unroll
            for (int j = 0; j < RAT_N; ++j) xd[j] = rat_dual(xq[(long)N * RAT_N + j], 0.0);
            adjp_seed(p, 16 * b + i, pd);
            gp[b] = rat_user_h<rat_dual>(xd, pd).d;
            bad = bad || !adj_finite(gp[b]);
        }
    }
#endif
    adj_terminal(T, N, p, lam, bad);
    for (int t = N - 1; t >= 0; --t) {
        adj_jacobian(T, t, p, true, s_col[T.kk]);
#if RAT_N_PARAMS > 0
#pragma unroll
        for (int b = 0; b < ADJP_TILES; ++b) {                        // the parameter pass: c_p + f_p' lambda_{t+1}, direction 16 b + i
            if (ok && 16 * b + i < RAT_N_PARAMS) {
                rat_dual xd[RAT_N], ud[RAT_M], xn[RAT_N], pd[RAT_N_PARAMS];
#pragma unroll
                for (int j = 0; j < RAT_N; ++j) xd[j] = rat_dual(xq[(long)t * RAT_N + j], 0.0);
#pragma unroll
                for (int j = 0; j < RAT_M; ++j) ud[j] = rat_dual(uq[(long)t * RAT_M + j], 0.0);
                adjp_seed(p, 16 * b + i, pd);
                double s = rat_user_c<rat_dual>(t, xd, ud, pd).d;
                rat_user_f<rat_dual>(xd, ud, xn, pd);
#pragma unroll
                for (int j = 0; j < RAT_N; ++j) s = __builtin_fma(xn[j].d, lam[j], s);
                bad = bad || !adj_finite(s);
                gp[b] += s;
            }
        }
#endif
        double g = 0.0;
        if (T.act) {
            rat_dual xd[RAT_N], ud[RAT_M];
            double col[RAT_N];
            adj_seed(T, t, xd, ud);
            g = rat_user_c<rat_dual>(t, xd, ud, p).d;                 // c_z, component zi
            adj_column(T, xd, ud, p, s_col[T.kk], col);
#pragma unroll
            for (int j = 0; j < RAT_N; ++j) g = __builtin_fma(col[j], lam[j], g);
            bad = bad || !adj_finite(g);
        }
        adj_columns_read();
        l0 = adj_close(T, t, g, a.L, lam);                            // (after step 0: lambda_0, component i; zero in a padding lane)
    }
    if (ok) {
        a.gp[T.q * 32 + i] = gp[0];
        a.gp[T.q * 32 + 16 + i] = gp[1];
        if (T.isx) a.lam0[T.q * 12 + i] = l0;
    }
    adj_flag(T, bad, a.bad, T.q, a.n_bad);
}
