// source_events.h -- the evaluation kernel of rat_policy_events_user (include/ratilqr.h): the user's rat_user_event on the replayed
// trajectories of a source model, in place of ev_eval's quadratic g (policy_mc.hip).  Compiled by hiprtc behind the user's source, which
// defines RAT_USER_EVENT and rat_user_event; RAT_N, RAT_M and RAT_N_EVENT come from the command line.  A module of its own, compiled by the
// first call that names an n_event.
//
// One lane per rollout of the chunk, walking t = 0 .. N: the lane loads its own row x_t (RAT_N doubles of xs [kc][N+1][ldx]) and u_t (RAT_M
// doubles of us [kc][N][ldu]; zeros at t == N), sets g[0 .. 16) to NaN and calls rat_user_event once for all events.  An entry the function
// leaves alone stays NaN and is passed over exactly as ev_eval passes over a NaN g: it never replaces a number in M, is not "> 0", sets no
// bit.  M, tau and the step's bits stay in registers; the outputs are ev_eval's -- margin and tau [RAT_N_EVENT + 1][ldy] with "any" (the
// largest margin, the earliest step) in the last row, mask [N+1][ldy] -- so ev_sums and ev_final run behind this kernel unchanged.  A
// rollout whose stored cost is NaN is selected out (NaN, -1, 0): its trajectory is not read and the function is not called for it.
// Global access: a lane's row is 8 RAT_N contiguous bytes (96 at n = 12), the lanes of a wavefront lie (N + 1) rows apart, so a step's
// load touches one or two 128-byte lines per lane and none is shared between lanes; the next step reads on in the same lines, so every
// byte that comes from memory is used once, by the lane that fetched it.  The stores (margin, tau, mask) are coalesced over the lanes.
#pragma once
#include "source_step.h"
#include "source_params.h"

#ifndef RAT_USER_EVENT
#error "the source does not define RAT_USER_EVENT: rat_policy_events_user needs '#define RAT_USER_EVENT' and rat_user_event(k, x, u, g, p)"
#endif
#if !defined(RAT_N_EVENT) || RAT_N_EVENT < 1 || RAT_N_EVENT > 16
#error "rat_user_event is compiled for 1 .. 16 events (RAT_N_EVENT)"
#endif

extern "C" __global__ __launch_bounds__(64) void rat_src_user_events(SrcEventArgs a) {
    const long q = (long)blockIdx.x * 64 + threadIdx.x;
    if (q >= a.kc) return;                                            // (the K tail: no lane works with another)
    const int N = a.N;
    const double nan = __builtin_nan("");
    const bool ok = !src_nan(a.cost[q]);                              // selected, not multiplied: the trajectory may hold NaN
    const double *xq = a.xs + q * (N + 1) * a.ldx, *uq = a.us + q * N * a.ldu;
    double M[RAT_N_EVENT];
    int tau[RAT_N_EVENT];
    // the rollout's parameters, where sampling is on, formed again from its global index and the replayed evaluation's seed (or the stored
    // injected draws): a handful of Philox blocks, no stored copy.  An overdraw or a NaN here was the rollout kernel's to report (the stored
    // cost is NaN)
    src_rollout_params own;
    int pover = 0;
    if (ok) (void)own.draw(q + a.j0, a.seed, a.zpn, a.zpu, a.p, pover);
    const double *p = own.of(a.p);
#pragma unroll
    for (int e = 0; e < RAT_N_EVENT; ++e) { M[e] = nan; tau[e] = -1; }
    for (int t = 0; t <= N; ++t) {
        unsigned bits = 0u;
        if (ok) {
            double x[RAT_N], u[RAT_M], g[16];
#pragma unroll
            for (int i = 0; i < RAT_N; ++i) x[i] = xq[(long)t * a.ldx + i];
#pragma unroll
            for (int i = 0; i < RAT_M; ++i) u[i] = (t < N) ? uq[(long)t * a.ldu + i] : 0.0;
#pragma unroll
            for (int e = 0; e < 16; ++e) g[e] = nan;
            rat_user_event(t, x, u, g, p);
#pragma unroll
            for (int e = 0; e < RAT_N_EVENT; ++e) {
                const double gv = g[e];
                if (gv > M[e] || src_nan(M[e])) M[e] = gv;            // (a NaN g never replaces a number)
                if (gv > 0.0) {
                    bits |= 1u << e;
                    if (tau[e] < 0) tau[e] = t;
                }
            }
            if (bits) bits |= 1u << RAT_N_EVENT;
        }
        if (a.mask) a.mask[(long)t * a.ldy + q] = bits;
    }
    double Ma = nan;
    int ta = -1;
#pragma unroll
    for (int e = 0; e < RAT_N_EVENT; ++e) {
        a.margin[(long)e * a.ldy + q] = ok ? M[e] : nan;
        a.tau[(long)e * a.ldy + q] = ok ? tau[e] : -1;
        if (M[e] > Ma || src_nan(Ma)) Ma = M[e];
        if (tau[e] >= 0 && (ta < 0 || tau[e] < ta)) ta = tau[e];
    }
    a.margin[(long)RAT_N_EVENT * a.ldy + q] = ok ? Ma : nan;
    a.tau[(long)RAT_N_EVENT * a.ldy + q] = ok ? ta : -1;
}
