// source_adjoint_lanes.h -- the team of the adjoint sweeps (source_adjoint.h, source_adjoint_params.h, source_margin_adjoint.h): what
// the three kernels do in the same way, once.
//
// A team of sixteen lanes per rollout, four rollouts per wavefront -- the moment kernels' own layout (policy_mc.hip): lane
// (i = lane & 15, kk = lane >> 4) is direction i of the padded 12 + 4 tile for rollout 4 blockIdx.x + kk.  Lane i seeds direction zi of
// z = (x, u) in one rat_dual evaluation; its own column of f_z dotted with lambda is component i of g_t, with no cross-lane traffic.
// lambda is replicated in the registers of the team.  What crosses lanes per step is gu (four values from lanes 12 .. 15, for L_t' gu)
// and the new lambda (n values), by ds_bpermute within the team.  Dead lanes (i >= n in 0 .. 11, i - 12 >= m), the K tail and a rollout
// without a cost (NaN: DomainError) compute nothing and contribute exact zeros.  With RAT_USER_F_JACOBIAN the columns of f_z come from
// rat_user_f_jacobian as in rat_src_linearize: lane 0 of the team calls it and the columns go through LDS between two barriers.
//
// The exchanges and the barriers are wavefront-wide: every lane of the wavefront calls adj_terminal, adj_jacobian, adj_columns_read,
// adj_close and adj_flag at every step, unconditionally, and nothing here returns early.  A value that does not count is SELECTED out,
// never multiplied by zero (0 * Inf is NaN).
#pragma once
#include "rat_ad.h"
#include "source_step.h"

// the value lane `src` of the wavefront holds (no <hip/hip_runtime.h> under hiprtc): both halves through ds_bpermute
__device__ __forceinline__ double adj_from(double v, int src) {
    int w[2];
    __builtin_memcpy(w, &v, 8);
    w[0] = __builtin_amdgcn_ds_bpermute(src << 2, w[0]);
    w[1] = __builtin_amdgcn_ds_bpermute(src << 2, w[1]);
    double r;
    __builtin_memcpy(&r, w, 8);
    return r;
}
__device__ __forceinline__ bool adj_finite(double v) { return __builtin_fabs(v) < __builtin_inf(); }

// a lane's place in its team and its rollout's staged trajectory (the head of the kernels' argument blocks, source_args.h)
struct AdjTeam {
    int lane, i, kk, team;
    long q;                                                           // the rollout, in the chunk
    bool ok, isx, act;
    int zi;                                                           // the lane's direction in z = (x, u)
    const double *__restrict__ xq, *__restrict__ uq;
    __device__ __forceinline__ AdjTeam(const SrcAdjointHead &a)
        : lane(threadIdx.x), i(lane & 15), kk(lane >> 4), team(lane & 48), q((long)blockIdx.x * 4 + kk),
          ok(q < a.kc && !src_nan(a.cost[q < a.kc ? q : 0])), isx(i < 12),
          act(ok && (isx ? (i < RAT_N) : (i - 12 < RAT_M))),          // (a dead lane, the K tail, a rollout without a cost: exact zeros)
          zi(isx ? i : RAT_N + (i - 12)), xq(a.xs + q * (long)(a.N + 1) * RAT_N), uq(a.us + q * (long)a.N * RAT_M) {}
};

#define ADJ_COLUMNS ((RAT_N + RAT_M) * RAT_N)                         /* doubles per team in the kernels' s_col: column z of [f_x | f_u] at z * RAT_N */

// The Jacobian stage (cols: the team's block of s_col, or null without the hook): f_returns_jacobian (ileqg.jl:302-311), A, B
// column-major, at step t where the team `need`s it; the barrier is for every lane
__device__ __forceinline__ void adj_jacobian(const AdjTeam &T, int t, const double *p, bool need, double *cols) {
#ifdef RAT_USER_F_JACOBIAN
    if (T.ok && need && T.i == 0) {
        double x[RAT_N], u[RAT_M], xn[RAT_N], A[RAT_N * RAT_N], B[RAT_N * RAT_M];
#pragma unroll
        for (int j = 0; j < RAT_N; ++j) x[j] = T.xq[(long)t * RAT_N + j];
#pragma unroll
        for (int j = 0; j < RAT_M; ++j) u[j] = T.uq[(long)t * RAT_M + j];
        rat_user_f_jacobian(x, u, xn, A, B, p);
        for (int e = 0; e < RAT_N * RAT_N; ++e) cols[e] = A[e];
        for (int e = 0; e < RAT_N * RAT_M; ++e) cols[RAT_N * RAT_N + e] = B[e];
    }
    __syncthreads();
#endif
}
// behind the step's adj_column: the columns are read, the next step may write
__device__ __forceinline__ void adj_columns_read() {
#ifdef RAT_USER_F_JACOBIAN
    __syncthreads();
#endif
}

// x_t (t = N: x_N) and u_t as duals seeded in the lane's direction
__device__ __forceinline__ void adj_seed_x(const AdjTeam &T, int t, rat_dual (&xd)[RAT_N]) {
#pragma unroll
    for (int j = 0; j < RAT_N; ++j) xd[j] = rat_dual(T.xq[(long)t * RAT_N + j], j == T.zi ? 1.0 : 0.0);
}
__device__ __forceinline__ void adj_seed(const AdjTeam &T, int t, rat_dual (&xd)[RAT_N], rat_dual (&ud)[RAT_M]) {
    adj_seed_x(T, t, xd);
#pragma unroll
    for (int j = 0; j < RAT_M; ++j) ud[j] = rat_dual(T.uq[(long)t * RAT_M + j], RAT_N + j == T.zi ? 1.0 : 0.0);
}
// column zi of [f_x | f_u] at the seeded (xd, ud): from the team's block of s_col, or one rat_dual evaluation of rat_user_f.  What it is
// dotted with, and from which start value, is the kernel's own: the start is part of the bits
__device__ __forceinline__ void adj_column(const AdjTeam &T, const rat_dual (&xd)[RAT_N], const rat_dual (&ud)[RAT_M], const double *p,
                                           const double *cols, double (&col)[RAT_N]) {
#ifdef RAT_USER_F_JACOBIAN
#pragma unroll
    for (int j = 0; j < RAT_N; ++j) col[j] = cols[T.zi * RAT_N + j];
#else
    rat_dual xn[RAT_N];
    rat_user_f<rat_dual>(xd, ud, xn, p);
#pragma unroll
    for (int j = 0; j < RAT_N; ++j) col[j] = xn[j].d;
#endif
}

// lambda_N = h_x(x_N), replicated in the team
__device__ __forceinline__ void adj_terminal(const AdjTeam &T, int N, const double *p, double (&lam)[RAT_N], bool &bad) {
    double g = 0.0;
    if (T.act && T.isx) {
        rat_dual xd[RAT_N];
        adj_seed_x(T, N, xd);
        g = rat_user_h<rat_dual>(xd, p).d;
        bad = bad || !adj_finite(g);
    }
#pragma unroll
    for (int j = 0; j < RAT_N; ++j) lam[j] = adj_from(g, T.team + j);
}

// The close of step t: gu_t is the u part of the team's g (lanes 12 .. 15), lambda_t = (x part of g) + L_t' gu_t (L null, open loop: the
// x part alone), replicated into lam.  Returns the lane's own component of lambda_t (zero in a padding lane)
__device__ __forceinline__ double adj_close(const AdjTeam &T, int t, double g, const double *L, double (&lam)[RAT_N]) {
    double gu[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gu[j] = adj_from(g, T.team + 12 + j);
    double ln = 0.0;
    if (T.act && T.isx) {
        ln = g;
        if (L) {
#pragma unroll
            for (int j = 0; j < RAT_M; ++j) ln = __builtin_fma(L[(long)t * LSTR + j * 12 + T.i], gu[j], ln);
        }
    }
#pragma unroll
    for (int j = 0; j < RAT_N; ++j) lam[j] = adj_from(ln, T.team + j);
    return ln;
}

// The flag: bad OR-ed over the team, stored at flags[at] by lane 0 and counted (an integer atomic: a count has no order)
__device__ __forceinline__ void adj_flag(const AdjTeam &T, bool bad, int *flags, long at, int *count) {
    int b = bad ? 1 : 0;
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) b |= __builtin_amdgcn_ds_bpermute((T.lane ^ s) << 2, b);
    if (T.ok && T.i == 0) {
        flags[at] = b;
        if (b) (void)__hip_atomic_fetch_add(count, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
