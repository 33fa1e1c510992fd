// source_pets.h -- the rollout kernel of generative source models (PETS, include/ratilqr.h "Generative source models").  Compiled by hiprtc
// behind rat_rng.h and the user's source, which defines rat_user_f_stochastic / rat_user_c / rat_user_h; RAT_N, RAT_M, RAT_PETS_NORMALS,
// RAT_PETS_UNIFORMS come from the command line.
//
// rat_src_pets_rollout restates compute_cost_worker (pets.jl:76-98) for a model the library does not know at build time: one lane per
// trajectory, the state in registers, the K trajectories of a control sample on consecutive lanes (they share its control loads); each
// step adds c(t, x_t, u_t) and then draws x_{t+1} = f_stochastic(x_t, u_t, rng, use_true_model); h(x_N) last.  The per-sample mean is the
// family's pets_mean_kernel (kernels.hip), launched after this kernel.
#pragma once
#include "rat_rng.h"
#include "source_step.h"

extern "C" __global__ __launch_bounds__(64) void rat_src_pets_rollout(SrcPetsArgs a) {
    const int lane = threadIdx.x;
    const long j = (long)blockIdx.x * a.tpw + lane;
    if (lane >= a.tpw || j >= a.S * a.K) return;
    const long ii = j / a.K;
    const int N = a.N;
    const long g = j + a.traj0;
    rat_rng rng;
    rng.gen = (a.zn == nullptr && a.zu == nullptr);
    rng.zn = nullptr; rng.zu = nullptr;
    rng.g0 = (unsigned)g; rng.g1 = (unsigned)(g >> 32); rng.t = 0;
    rng.k0 = (unsigned)a.seed; rng.k1 = (unsigned)(a.seed >> 32);
    rng.over = 0; rng.spare_n = 0.0; rng.spare_u = 0.0;
    double x[RAT_N];
#pragma unroll
    for (int q = 0; q < RAT_N; ++q) x[q] = a.x0[q];
    const double *__restrict__ uc = a.controls + ii * N * USTR;
    double cost = 0.0;
    for (int t = 0; t < N; ++t) {
        double u[RAT_M];
#pragma unroll
        for (int q = 0; q < RAT_M; ++q) u[q] = uc[(long)t * USTR + q];
        cost += rat_user_c<double>(t, x, u, a.p);                     // c(t - 1, x_t, u_t) of pets.jl:90 (time index from 0)
        rng.t = (unsigned)t; rng.in = 0; rng.iu = 0;
        if (!rng.gen) {
            if (RAT_PETS_NORMALS > 0) rng.zn = a.zn + (j * N + t) * (long)RAT_PETS_NORMALS;
            if (RAT_PETS_UNIFORMS > 0) rng.zu = a.zu + (j * N + t) * (long)RAT_PETS_UNIFORMS;
        }
        double xn[RAT_N];
        rat_user_f_stochastic(x, u, rng, a.use_true, xn, a.p);        // pets.jl:91
#pragma unroll
        for (int q = 0; q < RAT_N; ++q) x[q] = xn[q];
    }
    cost += rat_user_h<double>(x, a.p);                               // pets.jl:94
    a.traj_cost[j] = cost;
    if (rng.over) *a.overdraw = rng.over;
}
