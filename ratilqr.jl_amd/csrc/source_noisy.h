// source_noisy.h -- the Monte-Carlo rollout kernel of source models (rat_policy_evaluate, include/ratilqr.h).  Compiled by hiprtc behind the
// user's source (rat_user_f / rat_user_c / rat_user_h; RAT_N, RAT_M from the command line) as a module of its own, on the first
// rat_policy_evaluate of a source problem: a handle that never evaluates a policy never pays for it (as a third kernel of the model
// module it lengthened that module's compile by 7-16 %, around and over the tenth allowed: DESIGN.md section 7, profiles/policy_mc.md).
#pragma once
#include "rat_normal.h"
#include "rat_philox.h"
#include "source_step.h"
#include "source_policy.h"

// ---- noisy rollout: one lane per Monte-Carlo rollout, the state in registers ------------------------------------------------------------
// noisy_rollout_kernel (kernels.hip) restated for a model the library does not know at build time: x_{t+1} = f(x_t, u_t) + chol_lower(W(t)) z_t
// open loop or under u_t = l_t + L_t (x_t - xbar_t), and the realised cost c(0, x_0, u_0) + ... + c(N-1, ..) + h(x_N) of every rollout.
// The noise is the family kernel's: injected z at (k N + t) n + j, or Philox4x32-10 with counter (k lo, k hi, t >> 1, j) and key (seed lo,
// seed hi), both outputs of one Box-Muller transform for steps 2 i and 2 i + 1 -- a seed names the same noise for a family problem and for
// the same problem written as source.  The products with the Cholesky factor run over its lower triangle in the family kernel's order
// (the zeros it adds beyond the diagonal change nothing).  A DomainError rollout writes NaN.
extern "C" __global__ __launch_bounds__(64) void rat_src_noisy_rollout(SrcNoisyArgs a) {
    const int lane = threadIdx.x;
    const long k = (long)blockIdx.x * a.tpw + lane;
    if (lane >= a.tpw || k >= a.K) return;
    const int N = a.N;
    double x[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) x[q] = (q < RAT_N) ? a.xnom[q] : 0.0;
    double znext[RAT_N];
#pragma unroll
    for (int q = 0; q < RAT_N; ++q) znext[q] = 0.0;
    double cost = 0.0;
    int dom = 0;
#ifdef RAT_USER_POLICY
    double up[4] = {0.0, 0.0, 0.0, 0.0};                              // the control applied at step t - 1
#endif
    for (int t = 0; t < N; ++t) {
        double u[4];
        if (a.L) {
            double dx[12];
#pragma unroll
            for (int q = 0; q < 12; ++q) dx[q] = x[q] - a.xnom[(long)t * XSTR + q];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double Ldx = src_gain_row(a.L + (long)t * LSTR + j * 12, dx);
                u[j] = a.l[(long)t * USTR + j] + Ldx;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) u[j] = a.l[(long)t * USTR + j];
        }
#ifdef RAT_USER_POLICY
        if (rat_src_policy(t, x, u, up, a.p)) dom = 1;                // the user's controller: u is the applied control from here on
#endif
        bool inok = true;
#pragma unroll
        for (int q = 0; q < RAT_N; ++q) inok = inok && !src_nan(x[q]);
#pragma unroll
        for (int q = 0; q < RAT_M; ++q) inok = inok && !src_nan(u[q]);
        const double ct = rat_user_c<double>(t, x, u, a.p);           // integrate_cost: c(t, x_t, u_t) in order   (ileqg.jl:118-121)
        cost += ct;
        double xn[RAT_N];
        rat_user_f<double>(x, u, xn, a.p);
        bool outnan = src_nan(ct);
#pragma unroll
        for (int q = 0; q < RAT_N; ++q) outnan = outnan || src_nan(xn[q]);
        if (inok && outnan) dom = 1;                                  // the reference's DomainError
        double z[RAT_N];
        if (a.z) {
#pragma unroll
            for (int q = 0; q < RAT_N; ++q) z[q] = a.z[(k * N + t) * (long)RAT_N + q];
        } else if ((t & 1) == 0) {
#pragma unroll
            for (int q = 0; q < RAT_N; ++q) {
                unsigned r[4];
                philox4x32_10((unsigned)k, (unsigned)(k >> 32), (unsigned)(t >> 1), (unsigned)q, (unsigned)a.seed, (unsigned)(a.seed >> 32), r);
                ratn_box_muller(u01(r[0], r[1]), u01(r[2], r[3]), &z[q], &znext[q]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < RAT_N; ++q) z[q] = znext[q];
        }
        const double *__restrict__ Wc = a.Wchol + (a.W_tv ? (long)t * 192 : 0);
#pragma unroll
        for (int i = 0; i < RAT_N; ++i) {
            double w = 0.0;                                           // w_t = chol_lower(W(t)) z_t
#pragma unroll
            for (int q = 0; q <= i; ++q) w = __builtin_fma(Wc[i * 16 + q], z[q], w);
            x[i] = xn[i] + w;
        }
    }
    bool inok = true;
#pragma unroll
    for (int q = 0; q < RAT_N; ++q) inok = inok && !src_nan(x[q]);
    const double hc = rat_user_h<double>(x, a.p);                     // ... then h(x_N)   (ileqg.jl:122)
    if (inok && src_nan(hc)) dom = 1;
    cost += hc;
    a.cost[k] = dom ? __builtin_nan("") : cost;
}
