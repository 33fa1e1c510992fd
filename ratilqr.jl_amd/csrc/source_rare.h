// source_rare.h -- the rollout kernel of rat_policy_rare_event_noise (include/ratilqr.h): a source model under its rat_user_noise, the
// normals drawn from a shifted proposal, and the margin of one safety event in place of the trajectory and the cost.  Compiled by hiprtc
// behind rat_rng.h -- with RAT_RNG_SHIFT, which this module alone defines (source_model.cpp puts it in front of rat_rng.h) -- and the
// user's source, which defines RAT_USER_NOISE and rat_user_noise; RAT_N, RAT_M, RAT_PETS_NORMALS, RAT_PETS_UNIFORMS come from the command
// line.  A module of its own, compiled by the first call that needs it.
//
// Rollout part: one lane per rollout, the step of rat_src_user_noisy_rollout (source_user_noise.h) operation for operation -- the
// feedback sums in its order (src_affine of source_step.h here, the same sums written out there), c, the sampler, f, its DomainError
// rule (c and h are evaluated for that rule alone: no cost is formed).  The step is a second text, not a shared function (a shared one
// moves the registers of both kernels: profiles/source_step.md), so "operation for operation" is kept by hand and watched by
// tests/test_gpu_rare_event_noise.py.  The generator is keyed as there: the global rollout index in the Philox counter, the pass's seed
// as the key.  rng.normal() returns shift[t][i] + xi and adds -s z + s^2 / 2 to the lane's logw (rat_rng.h); the step's shift row is one
// address for the wavefront, so its loads are scalar or broadcast.
// Margin part: g(t, z) = z' Q z + a' z + b of z = (x_t, u_t) as ev_eval (policy_mc.hip) and re_g (rare_event.hip) form it, so that under
// a zero shift the margins are rat_policy_events' bit for bit.  Every lane puts its (x_t, u_t) in the 12 + 4 tile order into row `lane`
// of a wavefront-private LDS block (64 rows, stride 17: the sixteen columns of a group fall in different banks); the wavefront then
// walks the four groups of sixteen rollouts: in group c lane (col = lane & 15, kq = lane >> 4) loads Z[kq + 4 r][16 c + col], r = 0 .. 3,
// and forms g -- the a' z products, the four v_mfma_f64_16x16x4 of Q Z, the c . z products, the butterfly over the four kq lanes -- and
// the lane with kq == c, which is lane 16 c + col, the owner of that rollout, keeps the value.  No lane leaves early: lanes without a
// rollout (the K tail, lane >= tpw) skip the rollout part, hold zeros, take part in every group and store nothing.
// With RAT_RARE_USER_EVENT (rat_policy_rare_event_user; RAT_N_EVENT comes with it) the rollout part is the same text and the margin part is
// one rat_user_event call per step on the lane's own (x_t, u_t), u_N = 0, as rat_src_user_events (source_events.h) makes it: g arrives as
// NaN, entry a.event is the step's g, every step 0 .. N is watched.  No LDS, no MFMA, no butterfly: no lane works with another.
// With RAT_PARAM_SHIFT (rat_policy_rare_event_params; either variant, parameter sampling on) the shift table has a row N: entry i shifts
// the i-th rng.normal() of rat_user_params (source_params.h), whose likelihood ratio is where the lane's logw starts.
#pragma once
#include "rat_rng.h"
#include "source_step.h"
#include "source_policy.h"
#include "source_params.h"

#ifndef RAT_RNG_SHIFT
#error "source_rare.h is compiled with RAT_RNG_SHIFT in front of rat_rng.h"
#endif
#ifndef RAT_USER_NOISE
#error "the source does not define RAT_USER_NOISE: rat_policy_rare_event_noise needs '#define RAT_USER_NOISE' and rat_user_noise(k, x, u, rng, w, p)"
#endif
#if RAT_PETS_NORMALS < 1 || RAT_PETS_NORMALS > 12
#error "rat_policy_rare_event_noise shifts 1 .. 12 normals per step"
#endif
#ifdef RAT_RARE_USER_EVENT
#ifndef RAT_USER_EVENT
#error "the source does not define RAT_USER_EVENT: rat_policy_rare_event_user needs '#define RAT_USER_EVENT' and rat_user_event(k, x, u, g, p)"
#endif
#if !defined(RAT_N_EVENT) || RAT_N_EVENT < 1 || RAT_N_EVENT > 16
#error "rat_user_event is compiled for 1 .. 16 events (RAT_N_EVENT)"
#endif
#endif

#ifndef RAT_RARE_USER_EVENT
#define SRCRE_LD 17
#define SRCRE_SYNC() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront")

typedef double srcre_d4 __attribute__((ext_vector_type(4)));

// __shfl_xor(v, mask) over the 64 lanes (no <hip/hip_runtime.h> under hiprtc): both halves through ds_bpermute
__device__ __forceinline__ double srcre_xor(double v, int lane, int mask) {
    int w[2];
    __builtin_memcpy(w, &v, 8);
    const int src = (lane ^ mask) << 2;
    w[0] = __builtin_amdgcn_ds_bpermute(src, w[0]);
    w[1] = __builtin_amdgcn_ds_bpermute(src, w[1]);
    double r;
    __builtin_memcpy(&r, w, 8);
    return r;
}

// g(z) of the lane's column, re_g of rare_event.hip: every lane of the column returns the same bits
template <bool QUAD>
__device__ __forceinline__ double srcre_g(const double (&zv)[4], const double *s_a, const double *s_q, int lane, int kq, int col, double b) {
    const double *ae = s_a + kq;
    double p = ae[0] * zv[0] + ae[4] * zv[1] + ae[8] * zv[2] + ae[12] * zv[3];
    if (QUAD) {
        const double *qe = s_q + kq * 16 + col;
        srcre_d4 c = (srcre_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) c = __builtin_amdgcn_mfma_f64_16x16x4f64(qe[kb * 64], zv[kb], c, 0, 0, 0);
        p += c[0] * zv[0] + c[1] * zv[1] + c[2] * zv[2] + c[3] * zv[3];
    }
    p += srcre_xor(p, lane, 16);
    p += srcre_xor(p, lane, 32);
    return p + b;
}
#endif

extern "C" __global__ __launch_bounds__(64) void rat_src_rare_rollout(SrcRareArgs a) {
    const int lane = threadIdx.x;
    const long j = (long)blockIdx.x * a.tpw + lane;
    const bool live = lane < a.tpw && j < a.K;
    const int N = a.N;
#ifndef RAT_RARE_USER_EVENT
    __shared__ double s_q[256], s_a[16], s_z[64 * SRCRE_LD];
    const int col = lane & 15, kq = lane >> 4;
    if (a.quad) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s_q[lane + 64 * q] = a.Qt[lane + 64 * q];
    }
    if (lane < 16) s_a[lane] = a.at[lane];
    __syncthreads();
#endif
    rat_rng rng;
    rng.gen = true;
    rng.zn = nullptr; rng.zu = nullptr;
    rng.g0 = (unsigned)j; rng.g1 = (unsigned)(j >> 32); rng.t = 0;
    rng.k0 = (unsigned)a.seed; rng.k1 = (unsigned)(a.seed >> 32);
    rng.in = 0; rng.iu = 0; rng.over = 0; rng.spare_n = 0.0; rng.spare_u = 0.0;
    rng.shift = a.shift; rng.logw = 0.0;
    double x[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) x[q] = (live && q < RAT_N) ? a.xnom[q] : 0.0;
    const double nan = __builtin_nan("");
    double M = nan;
    int dom = 0;
    // this rollout's parameters, where sampling is on, from N(0, 1) / U[0, 1): not shifted, nothing added to logw -- or under
    // RAT_PARAM_SHIFT (rat_policy_rare_event_params) the normals from the proposal shifted by row N of the shift table, and the lane's
    // logw starts from the parameter part (a lane without a rollout calls none of the user's functions and holds nothing here)
    src_rollout_params own;
#ifdef RAT_PARAM_SHIFT
    if (live && own.draw(j, a.seed, a.zpn, a.zpu, a.p, rng.over, a.shift + N * 12, rng.logw)) dom = 1;
#else
    if (live && own.draw(j, a.seed, a.zpn, a.zpu, a.p, rng.over)) dom = 1;
#endif
    const double *p = own.of(a.p);
#ifdef RAT_USER_POLICY
    double up[4] = {0.0, 0.0, 0.0, 0.0};                              // the control applied at step t - 1
#endif
#ifndef RAT_RARE_USER_EVENT
    double *row = s_z + lane * SRCRE_LD;
#endif
    for (int t = 0;; ++t) {
        double u[4] = {0.0, 0.0, 0.0, 0.0};
        if (live && t < N) {
            src_affine(t, x, a.xnom, a.l, a.L, u);                    // (rat_src_user_noisy_rollout's sums, in its order)
#ifdef RAT_USER_POLICY
            if (rat_src_policy(t, x, u, up, p)) dom = 1;              // the user's controller: the margin, c, the sampler and f see the applied control
#endif
        }
#ifdef RAT_RARE_USER_EVENT
        if (live) {
            double g[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) g[e] = nan;
            rat_user_event(t, x, u, g, p);                            // (x has 12 entries, RAT_N of them live; u is 0 at t == N)
            double gv = nan;
#pragma unroll
            for (int e = 0; e < RAT_N_EVENT; ++e) gv = (e == a.event) ? g[e] : gv;
            if (gv > M || src_nan(M)) M = gv;                         // (a NaN g never replaces a number)
        }
#else
        if (t >= a.t_lo && t <= a.t_hi) {                             // (uniform over the grid)
#pragma unroll
            for (int q = 0; q < 12; ++q) row[q] = (q < RAT_N) ? x[q] : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) row[12 + q] = (q < RAT_M) ? u[q] : 0.0;   // (u is 0 at t == N and on a lane without a rollout)
            SRCRE_SYNC();
            double gv = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double *zc = s_z + (16 * c + col) * SRCRE_LD + kq;
                const double zv[4] = {zc[0], zc[4], zc[8], zc[12]};
                const double gc = a.quad ? srcre_g<true>(zv, s_a, s_q, lane, kq, col, a.b) : srcre_g<false>(zv, s_a, s_q, lane, kq, col, a.b);
                if (kq == c) gv = gc;                                 // lane 16 c + col owns rollout 16 c + col of the wavefront
            }
            SRCRE_SYNC();
            if (gv > M || src_nan(M)) M = gv;                         // (a NaN g never replaces a number)
        }
#endif
        if (t == N) break;
        if (live) {
            bool inok = true;
#pragma unroll
            for (int q = 0; q < RAT_N; ++q) inok = inok && !src_nan(x[q]);
#pragma unroll
            for (int q = 0; q < RAT_M; ++q) inok = inok && !src_nan(u[q]);
            const double ct = rat_user_c<double>(t, x, u, p);         // (for the DomainError rule alone)
            rng.t = (unsigned)t; rng.in = 0; rng.iu = 0;
            rng.shift = a.shift + t * 12;
            double w[RAT_N];
#pragma unroll
            for (int q = 0; q < RAT_N; ++q) w[q] = 0.0;
            rat_user_noise(t, x, u, rng, w, p);
            double xn[RAT_N];
            rat_user_f<double>(x, u, xn, p);
            bool outnan = src_nan(ct);
#pragma unroll
            for (int q = 0; q < RAT_N; ++q) outnan = outnan || src_nan(xn[q]) || src_nan(w[q]);
            if (inok && outnan) dom = 1;                              // the reference's DomainError, and a NaN disturbance
#pragma unroll
            for (int q = 0; q < RAT_N; ++q) x[q] = xn[q] + w[q];      // x_{t+1} = f(x_t, u_t) + w_t
        }
    }
    if (!live) return;                                                // (behind the last group: nothing follows that needs the lane)
    bool inok = true;
#pragma unroll
    for (int q = 0; q < RAT_N; ++q) inok = inok && !src_nan(x[q]);
    const double hc = rat_user_h<double>(x, p);
    if (inok && src_nan(hc)) dom = 1;
    a.margin[j] = dom ? nan : M;
    a.logw[j] = rng.logw;
    a.dom[j] = dom;
    if (rng.over) *a.overdraw = rng.over;
}
