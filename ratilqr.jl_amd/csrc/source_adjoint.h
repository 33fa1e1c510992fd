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
// A team of sixteen lanes per rollout, four rollouts per wavefront -- the moment kernels' own layout (policy_mc.hip): lane
// (i = lane & 15, kk = lane >> 4) is direction i of the padded 12 + 4 tile for rollout 4 blockIdx.x + kk.  Lane i seeds direction i of z in
// one rat_dual evaluation of rat_user_c and one of rat_user_f; its own column of f_z dotted with lambda (j = 0 .. n - 1 in order, fused
// multiply-adds behind c's partial) is component i of g_t, with no cross-lane traffic.  lambda is replicated in the registers of the
// team.  What crosses lanes per step is gu (four values from lanes 12 .. 15, for L_t' gu) and the new lambda (n values), by ds_bpermute
// within the team.  Dead lanes (i >= n in 0 .. 11, i - 12 >= m) compute nothing and contribute exact zeros.  With RAT_USER_F_JACOBIAN the
// columns of f_z come from rat_user_f_jacobian as in rat_src_linearize: lane 0 of the team calls it and the columns go through LDS; c and
// h stay by AD.
//
// A rollout without a cost (NaN: DomainError) is passed over: nothing is loaded, computed or stored for it, and the moment kernel
// selects it out.  A rollout with a cost whose sensitivities hold a NaN or an Inf anywhere (h_x, any component of any g_t) is flagged in
// bad and counted; its gu is stored as it came out and is selected out downstream, never multiplied.
// Every lane of the wavefront runs every step (the exchanges and, with the Jacobian hook, the barriers are wavefront-wide): there is no
// early return.
#pragma once
#include "rat_ad.h"
#include "source_step.h"
#include "source_adjoint_lanes.h"

#ifndef RAT_USER_NOISE
#error "the source does not define RAT_USER_NOISE: rat_policy_gradient replays rat_policy_evaluate_noise, which needs '#define RAT_USER_NOISE' and rat_user_noise(k, x, u, rng, w, p)"
#endif
#ifdef RAT_USER_POLICY
#error "the source defines RAT_USER_POLICY: rat_user_policy is not templated, so the control law is not differentiable by rat_ad.h (rat_policy_gradient serves the affine law alone)"
#endif


extern "C" __global__ __launch_bounds__(64) void rat_src_adjoint(SrcAdjointArgs a) {
#ifdef RAT_USER_F_JACOBIAN
    __shared__ double s_col[4][(RAT_N + RAT_M) * RAT_N];              // per team: column z of [f_x | f_u] at z * RAT_N
#endif
    const int lane = threadIdx.x, i = lane & 15, kk = lane >> 4, team = lane & 48;
    const long q = (long)blockIdx.x * 4 + kk;
    const int N = a.N;
    const bool ok = q < a.kc && !src_nan(a.cost[q < a.kc ? q : 0]);
    const bool isx = i < 12;
    const bool act = ok && (isx ? (i < RAT_N) : (i - 12 < RAT_M));    // (a dead lane, the K tail, a rollout without a cost: exact zeros)
    const int zi = isx ? i : RAT_N + (i - 12);                        // the lane's direction in z = (x, u)
    const double *__restrict__ xq = a.xs + q * (long)(N + 1) * RAT_N;
    const double *__restrict__ uq = a.us + q * (long)N * RAT_M;
    double lam[RAT_N];
    bool bad = false;
    {                                                                 // lambda_N = h_x(x_N)
        double g = 0.0;
        if (act && isx) {
            rat_dual xd[RAT_N];
#pragma unroll
            for (int j = 0; j < RAT_N; ++j) xd[j] = rat_dual(xq[(long)N * RAT_N + j], j == zi ? 1.0 : 0.0);
            g = rat_user_h<rat_dual>(xd, a.p).d;
            bad = bad || !adj_finite(g);
        }
#pragma unroll
        for (int j = 0; j < RAT_N; ++j) lam[j] = adj_from(g, team + j);
    }
    for (int t = N - 1; t >= 0; --t) {
#ifdef RAT_USER_F_JACOBIAN
        if (ok && i == 0) {                                           // f_returns_jacobian (ileqg.jl:302-311): A, B column-major
            double x[RAT_N], u[RAT_M], xn[RAT_N], A[RAT_N * RAT_N], B[RAT_N * RAT_M];
#pragma unroll
            for (int j = 0; j < RAT_N; ++j) x[j] = xq[(long)t * RAT_N + j];
#pragma unroll
            for (int j = 0; j < RAT_M; ++j) u[j] = uq[(long)t * RAT_M + j];
            rat_user_f_jacobian(x, u, xn, A, B, a.p);
            for (int e = 0; e < RAT_N * RAT_N; ++e) s_col[kk][e] = A[e];
            for (int e = 0; e < RAT_N * RAT_M; ++e) s_col[kk][RAT_N * RAT_N + e] = B[e];
        }
        __syncthreads();
#endif
        double g = 0.0;
        if (act) {
            rat_dual xd[RAT_N], ud[RAT_M];
#pragma unroll
            for (int j = 0; j < RAT_N; ++j) xd[j] = rat_dual(xq[(long)t * RAT_N + j], j == zi ? 1.0 : 0.0);
#pragma unroll
            for (int j = 0; j < RAT_M; ++j) ud[j] = rat_dual(uq[(long)t * RAT_M + j], RAT_N + j == zi ? 1.0 : 0.0);
            g = rat_user_c<rat_dual>(t, xd, ud, a.p).d;               // c_z, component zi
#ifdef RAT_USER_F_JACOBIAN
#pragma unroll
            for (int j = 0; j < RAT_N; ++j) g = __builtin_fma(s_col[kk][zi * RAT_N + j], lam[j], g);
#else
            rat_dual xn[RAT_N];
            rat_user_f<rat_dual>(xd, ud, xn, a.p);                    // column zi of [f_x | f_u]
#pragma unroll
            for (int j = 0; j < RAT_N; ++j) g = __builtin_fma(xn[j].d, lam[j], g);
#endif
            bad = bad || !adj_finite(g);
        }
#ifdef RAT_USER_F_JACOBIAN
        __syncthreads();                                              // (the columns are read: the next step may write)
#endif
        double gu[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) gu[j] = adj_from(g, team + 12 + j);
        double ln = 0.0;
        if (act && isx) {                                             // lambda_t, component i
            ln = g;
            if (a.L) {
#pragma unroll
                for (int j = 0; j < RAT_M; ++j) ln = __builtin_fma(a.L[(long)t * LSTR + j * 12 + i], gu[j], ln);
            }
        }
#pragma unroll
        for (int j = 0; j < RAT_N; ++j) lam[j] = adj_from(ln, team + j);
        if (ok && !isx) a.gu[(q * N + t) * 4 + (i - 12)] = g;         // (zero in a padding lane)
    }
    int b = bad ? 1 : 0;
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) b |= __builtin_amdgcn_ds_bpermute((lane ^ s) << 2, b);
    if (ok && i == 0) {
        a.bad[q] = b;
        if (b) (void)__hip_atomic_fetch_add(a.n_bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
