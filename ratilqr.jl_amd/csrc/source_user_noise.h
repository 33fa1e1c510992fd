// source_user_noise.h -- the Monte-Carlo rollout kernel of source models under user-written process noise (rat_policy_evaluate_noise,
// include/ratilqr.h "Source models").  Compiled by hiprtc behind rat_rng.h and the user's source, which defines RAT_USER_NOISE and
// rat_user_noise next to rat_user_f / rat_user_c / rat_user_h; RAT_N, RAT_M, RAT_PETS_NORMALS, RAT_PETS_UNIFORMS come from the command
// line.  A module of its own, compiled by the first call that needs it, as source_noisy.h is: a handle that never evaluates under user
// noise never pays for it.
#pragma once
#include "rat_rng.h"
#include "source_step.h"
#include "source_policy.h"
#include "source_params.h"

#ifndef RAT_USER_NOISE
#error "the source does not define RAT_USER_NOISE: rat_policy_evaluate_noise needs '#define RAT_USER_NOISE' and rat_user_noise(k, x, u, rng, w, p)"
#endif

// ---- noisy rollout under the user's sampler: one lane per Monte-Carlo rollout, the state in registers ----------------------------------
// rat_src_noisy_rollout (source_noisy.h) with w_t = rat_user_noise(t, x_t, u_t, rng) in place of chol_lower(W(t)) z_t: the same feedback
// law u_t = l_t + L_t (x_t - xbar_t), the same cost order c(0) .. c(N-1) then h, the same DomainError rule -- and a NaN in w whose
// inputs x_t, u_t had none is a DomainError too.  The draws are rat_rng's (rat_rng.h), keyed as source_pets.h keys them: injected slots
// (j N + t) normals + i / (j N + t) uniforms + i with j counted from the launch's first rollout (the host stages a chunk at a time), or
// Philox4x32-10 with the GLOBAL rollout index j + j0 in the counter and the caller's seed as the key -- no per-chunk seeds, so the result
// does not depend on how K is cut into launches.  Every per-lane array is indexed by unrolled loop counters only, so nothing is forced into scratch;
// what spills is a matter of size (the pendulum of the tests: none; the 12 x 4 LQ source with 12 normals and a uniform: all 512 registers
// and 636 B per lane, 628 B under the clamp + rate hook, profiles/policy_user_policy.md -- every rng draw is a Philox block inlined at its
// call site).  The sampler runs before f: with f first the 12 x 4 source spilled 1940 B per lane.  The affine law is
// written out here, not src_affine (source_step.h): with the helper one row of the resource table moves (profiles/source_step.md).
// x_out / u_out (either may be null): dense [n x (N+1)] / [m x N] per rollout, rollout slowest -- rat_rollout_noisy's layout -- written
// straight from the lane; a DomainError rollout writes what it computed and a NaN cost.
// w_out (null but for rat_policy_worst_case_disturbance's replay): dense [n x N] per rollout, the w the sampler wrote, before it is added.
extern "C" __global__ __launch_bounds__(64) void rat_src_user_noisy_rollout(SrcUserNoisyArgs a) {
    const int lane = threadIdx.x;
    const long j = (long)blockIdx.x * a.tpw + lane;
    if (lane >= a.tpw || j >= a.K) return;
    const int N = a.N;
    const long g = j + a.j0;
    rat_rng rng;
    rng.gen = (a.zn == nullptr && a.zu == nullptr);
    rng.zn = nullptr; rng.zu = nullptr;
    rng.g0 = (unsigned)g; rng.g1 = (unsigned)(g >> 32); rng.t = 0;
    rng.k0 = (unsigned)a.seed; rng.k1 = (unsigned)(a.seed >> 32);
    rng.in = 0; rng.iu = 0; rng.over = 0; rng.spare_n = 0.0; rng.spare_u = 0.0;
    double x[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) x[q] = (q < RAT_N) ? a.xnom[q] : 0.0;
    double *__restrict__ xo = a.x_out ? a.x_out + j * (long)(N + 1) * RAT_N : nullptr;
    double *__restrict__ uo = a.u_out ? a.u_out + j * (long)N * RAT_M : nullptr;
    double cost = 0.0;
    int dom = 0;
    src_rollout_params own;
    if (own.draw(g, a.seed, a.zpn, a.zpu, a.p, rng.over)) dom = 1;
    const double *p = own.of(a.p);
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
            for (int i = 0; i < 4; ++i) {
                const double *Lr = a.L + (long)t * LSTR + i * 12;
                double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {                         // L_t (x_t - xbar_t)   (ileqg.jl:104), rat_src_noisy_rollout's order
                    a0 = __builtin_fma(Lr[q], dx[q], a0);
                    a1 = __builtin_fma(Lr[4 + q], dx[4 + q], a1);
                    a2 = __builtin_fma(Lr[8 + q], dx[8 + q], a2);
                }
                u[i] = a.l[(long)t * USTR + i] + ((a0 + a1) + a2);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) u[i] = a.l[(long)t * USTR + i];
        }
#ifdef RAT_USER_POLICY
        if (rat_src_policy(t, x, u, up, p)) dom = 1;                  // the user's controller: u_out, c, the sampler and f see the applied control
#endif
        if (xo) {
#pragma unroll
            for (int q = 0; q < RAT_N; ++q) xo[(long)t * RAT_N + q] = x[q];
        }
        if (uo) {
#pragma unroll
            for (int q = 0; q < RAT_M; ++q) uo[(long)t * RAT_M + q] = u[q];
        }
        bool inok = true;
#pragma unroll
        for (int q = 0; q < RAT_N; ++q) inok = inok && !src_nan(x[q]);
#pragma unroll
        for (int q = 0; q < RAT_M; ++q) inok = inok && !src_nan(u[q]);
        const double ct = rat_user_c<double>(t, x, u, p);             // integrate_cost: c(t, x_t, u_t) in order   (ileqg.jl:118-121)
        cost += ct;
        rng.t = (unsigned)t; rng.in = 0; rng.iu = 0;
        if (!rng.gen) {
            if (RAT_PETS_NORMALS > 0) rng.zn = a.zn + (j * N + t) * (long)RAT_PETS_NORMALS;
            if (RAT_PETS_UNIFORMS > 0) rng.zu = a.zu + (j * N + t) * (long)RAT_PETS_UNIFORMS;
        }
        double w[RAT_N];
#pragma unroll
        for (int q = 0; q < RAT_N; ++q) w[q] = 0.0;
        rat_user_noise(t, x, u, rng, w, p);
        if (a.w_out) {
#pragma unroll
            for (int q = 0; q < RAT_N; ++q) a.w_out[(j * N + t) * (long)RAT_N + q] = w[q];
        }
        double xn[RAT_N];
        rat_user_f<double>(x, u, xn, p);
        bool outnan = src_nan(ct);
#pragma unroll
        for (int q = 0; q < RAT_N; ++q) outnan = outnan || src_nan(xn[q]) || src_nan(w[q]);
        if (inok && outnan) dom = 1;                                  // the reference's DomainError, and a NaN disturbance
#pragma unroll
        for (int q = 0; q < RAT_N; ++q) x[q] = xn[q] + w[q];          // x_{t+1} = f(x_t, u_t) + w_t
    }
    if (xo) {
#pragma unroll
        for (int q = 0; q < RAT_N; ++q) xo[(long)N * RAT_N + q] = x[q];
    }
    bool inok = true;
#pragma unroll
    for (int q = 0; q < RAT_N; ++q) inok = inok && !src_nan(x[q]);
    const double hc = rat_user_h<double>(x, p);                       // ... then h(x_N)   (ileqg.jl:122)
    if (inok && src_nan(hc)) dom = 1;
    cost += hc;
    a.cost[j] = dom ? __builtin_nan("") : cost;
    if (rng.over) *a.overdraw = rng.over;
}
