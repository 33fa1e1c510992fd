// source_sobol.h -- the rollout kernel of rat_policy_sobol (include/ratilqr.h "Which uncertainty drives the cost"): the pick-freeze
// rollouts of the first-order and total Sobol indices of a source model's Monte-Carlo cost.  Compiled by hiprtc behind rat_rng.h and the
// user's source with -DRAT_RNG_PICK=1 (source_model.cpp: SRC_SOBOL), which gives rat_rng and rat_param_rng a second key and the masks
// that choose, draw by draw, between the stream of seed_a and the stream of seed_b (rat_rng.h, source_params.h).  A module of its own,
// compiled by the first call that needs it: every other kind's module is what it was.
#pragma once
#ifndef RAT_RNG_PICK
#error "source_sobol.h is compiled with RAT_RNG_PICK"
#endif
#include "rat_rng.h"
#include "source_step.h"
#include "source_policy.h"
#include "source_params.h"

#ifndef RAT_USER_NOISE
#error "the source does not define RAT_USER_NOISE: rat_policy_sobol needs '#define RAT_USER_NOISE' and rat_user_noise(k, x, u, rng, w, p)"
#endif

// ---- one lane per (base sample, variant) ------------------------------------------------------------------------------------------------
// rat_src_user_noisy_rollout's step (source_user_noise.h) under the generator: the same affine law written out, the same cost order
// c(0) .. c(N-1) then h, the same DomainError rule (a NaN parameter, a NaN disturbance), the same policy hook, the parameters drawn in
// front of step 0.  The variant is blockIdx.y -- 0: A, every draw from the stream of seed_a; 1: B, every draw from the stream of seed_b;
// 2 + i: group i's draws from B, the rest from A -- so it is the same in all lanes of a wavefront: the four masks and both keys are
// scalars, and which key a draw takes is a scalar select on a constant draw index, not a branch that splits the wavefront.  The base
// sample's global index j + j0 is the Philox counter under either key, so row 0 is bit for bit the cost of rat_policy_evaluate_noise
// under seed_a, row 1 that under seed_b, and no row depends on how K is cut into launches.
extern "C" __global__ __launch_bounds__(64) void rat_src_sobol_rollout(SrcSobolArgs a) {
    const int lane = threadIdx.x;
    const long j = (long)blockIdx.x * a.tpw + lane;
    if (lane >= a.tpw || j >= a.K) return;
    const int N = a.N;
    const int v = blockIdx.y;
    const long g = j + a.j0;
    rat_rng rng;
    rng.gen = true;
    rng.zn = nullptr; rng.zu = nullptr;
    rng.g0 = (unsigned)g; rng.g1 = (unsigned)(g >> 32); rng.t = 0;
    rng.k0 = (unsigned)a.seed_a; rng.k1 = (unsigned)(a.seed_a >> 32);
    rng.kb0 = (unsigned)a.seed_b; rng.kb1 = (unsigned)(a.seed_b >> 32);
    rng.pick_n = a.pick[v][2]; rng.pick_u = a.pick[v][3];
    rng.in = 0; rng.iu = 0; rng.over = 0; rng.spare_n = 0.0; rng.spare_u = 0.0;
    double x[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) x[q] = (q < RAT_N) ? a.xnom[q] : 0.0;
    double cost = 0.0;
    int dom = 0;
    src_rollout_params own;
    if (own.draw(g, a.seed_a, nullptr, nullptr, a.p, rng.over, a.seed_b, a.pick[v][0], a.pick[v][1])) dom = 1;
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
                for (int q = 0; q < 4; ++q) {                         // L_t (x_t - xbar_t), rat_src_user_noisy_rollout's order
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
        if (rat_src_policy(t, x, u, up, p)) dom = 1;                  // the user's controller: c, the sampler and f see the applied control
#endif
        bool inok = true;
#pragma unroll
        for (int q = 0; q < RAT_N; ++q) inok = inok && !src_nan(x[q]);
#pragma unroll
        for (int q = 0; q < RAT_M; ++q) inok = inok && !src_nan(u[q]);
        const double ct = rat_user_c<double>(t, x, u, p);             // integrate_cost: c(t, x_t, u_t) in order
        cost += ct;
        rng.t = (unsigned)t; rng.in = 0; rng.iu = 0;
        double w[RAT_N];
#pragma unroll
        for (int q = 0; q < RAT_N; ++q) w[q] = 0.0;
        rat_user_noise(t, x, u, rng, w, p);
        double xn[RAT_N];
        rat_user_f<double>(x, u, xn, p);
        bool outnan = src_nan(ct);
#pragma unroll
        for (int q = 0; q < RAT_N; ++q) outnan = outnan || src_nan(xn[q]) || src_nan(w[q]);
        if (inok && outnan) dom = 1;                                  // the reference's DomainError, and a NaN disturbance
#pragma unroll
        for (int q = 0; q < RAT_N; ++q) x[q] = xn[q] + w[q];          // x_{t+1} = f(x_t, u_t) + w_t
    }
    bool inok = true;
#pragma unroll
    for (int q = 0; q < RAT_N; ++q) inok = inok && !src_nan(x[q]);
    const double hc = rat_user_h<double>(x, p);                       // ... then h(x_N)
    if (inok && src_nan(hc)) dom = 1;
    cost += hc;
    a.y[(long)v * a.ldy + j] = dom ? __builtin_nan("") : cost;
    if (rng.over) *a.overdraw = rng.over;
}
