// source_step.h -- what the rollout kernels of source models share (source_kernels.h, source_pets.h, source_noisy.h, source_user_noise.h,
// source_rare.h, source_events.h; DESIGN.md section 7, "the step of a source-model rollout"): the size guards, the NaN predicate and the
// affine law.  The choice between a rollout's own parameters and the problem's is src_rollout_params at the end of source_params.h, which
// builds on this header.  Compiled by hiprtc behind the user's source; RAT_N, RAT_M come from the command line; like every header of
// EMBED_H (Makefile: source_embed.inc) it is embedded in the library at build time, nothing is read from disk at run time.  Every function is
// force-inlined and takes its arrays by reference (x: 12 entries, RAT_N live; u: 4 entries, RAT_M live).  A piece is used by a kernel only
// where the kernel's registers, spills and scratch stay what they were with the text written out: profiles/source_step.md lists which
// kernel uses what.
#pragma once
#include "source_args.h"

#if !defined(RAT_N) || !defined(RAT_M)
#error "RAT_N and RAT_M must be defined"
#endif
#if RAT_N > SRC_MAX_N || RAT_M > SRC_MAX_M
#error "source models are compiled for n <= 12, m <= 4"
#endif

__device__ __forceinline__ bool src_nan(double v) { return v != v; }

// one row of L_t (x_t - xbar_t) (ileqg.jl:82, :104): three accumulators over the thirds of the row, rollout_kernel's order (kernels.hip)
__device__ __forceinline__ double src_gain_row(const double *Lr, const double (&dx)[12]) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        a0 = __builtin_fma(Lr[q], dx[q], a0);
        a1 = __builtin_fma(Lr[4 + q], dx[4 + q], a1);
        a2 = __builtin_fma(Lr[8 + q], dx[8 + q], a2);
    }
    return (a0 + a1) + a2;
}

// u_t = l_t + L_t (x_t - xbar_t), or l_t where L is null (open loop); xnom [N+1][12], l [N][4], L [N][4][12]
__device__ __forceinline__ void src_affine(int t, const double (&x)[12], const double *xnom, const double *l, const double *L, double (&u)[4]) {
    if (L) {
        double dx[12];
#pragma unroll
        for (int q = 0; q < 12; ++q) dx[q] = x[q] - xnom[(long)t * XSTR + q];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double Ldx = src_gain_row(L + (long)t * LSTR + i * 12, dx);
            u[i] = l[(long)t * USTR + i] + Ldx;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] = l[(long)t * USTR + i];
    }
}
