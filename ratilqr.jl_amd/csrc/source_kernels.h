// source_kernels.h -- the two model kernels of the runtime-compiled family (RAT_MODEL_SOURCE).  Compiled by hiprtc behind the user's
// source, which defines rat_user_f / rat_user_c / rat_user_h (include/ratilqr.h, "Source models"); RAT_N, RAT_M come from the command
// line.
//
// The kernels restate rollout_kernel and linearize_kernel (kernels.hip) for a model the library does not know at build time: same slots,
// same candidate step sizes eps lambda^k (repeated multiplication), same d = maximum(norm(l_t - u_t)) with NaN propagation, same domain
// signalling (status = RAT_ST_DOMAIN and value Inf for nominal trajectories, flag_c = 2 for candidates), same record layout (layout.h).
// Everything downstream -- sweeps, line-search selection, gather -- reads only those records, so it runs unchanged.
#pragma once
#include "rat_ad.h"
#include "source_step.h"

#define SRC_NZ (RAT_N + RAT_M)
__device__ inline int src_pad(int i) { return i < RAT_N ? i : 12 + (i - RAT_N); }   // z index -> row / column of the padded 16-wide tile

// ---- rollout: one lane per trajectory, the state in registers ----------------------------------------------------------------------
// (a one-step software prefetch of l, dl, xbar and L was measured: no change in solves/s at 2.5x the VGPRs; profiles/source_model.md)
extern "C" __global__ __launch_bounds__(64) void rat_src_rollout(SrcRollArgs a) {
    const int lane = threadIdx.x;
    const StateDev &st = a.st;
    const int N = st.N;
    const int ncand = (a.mode == 0) ? st.B : st.B * st.E;
    const int c = blockIdx.x * a.tpw + lane;
    if (lane >= a.tpw || c >= ncand) return;
    int b = 0, k = 0;
    if (a.mode == 0) { b = c; if (st.status[b] != ST_RUNNING) return; }
    else { b = c / st.E; k = c - b * st.E; if (st.ls_active[b] == 0) return; }
    const int nom = st.slot_nom[b];
    const int slot_n = b * (st.E + 1) + nom;
    const int slot_o = (a.mode == 0) ? slot_n : cand_slot(b, k, nom, st.E);
    const double *__restrict__ xbar = st.xs + (long)slot_n * st.x_stride;
    const double *__restrict__ lnom = (a.mode == 0) ? a.u0 : st.us + (long)slot_n * st.u_stride;
    double *__restrict__ xo = st.xs + (long)slot_o * st.x_stride;
    double *__restrict__ uo = st.us + (long)slot_o * st.u_stride;
    const int lsel = st.lsel[b];
    const double *__restrict__ Lb = st.L + (long)lsel * st.l_half + (long)b * N * LSTR;
    const double *__restrict__ dlb = st.dl + (long)lsel * st.dl_half + (long)b * N * USTR;
    double eps = 0.0;
    if (a.mode == 1) {
        eps = st.ls_eps[b];
        for (int q = 0; q < k; ++q) eps *= a.op.lambda;             // eps_k = eps * lambda^k by repeated multiplication (ileqg.jl:530, :557)
    }
    double x[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) x[q] = (q < RAT_N) ? ((a.mode == 0) ? a.x0[q] : xbar[q]) : 0.0;
#pragma unroll
    for (int q = 0; q < 12; ++q) xo[q] = x[q];
    double dmax = -__builtin_inf();
    bool dnan = false;
    int dom = 0;
    for (int t = 0; t < N; ++t) {
        double u[4];
        if (a.mode == 1) {
            double dx[12];
#pragma unroll
            for (int q = 0; q < 12; ++q) dx[q] = x[q] - xbar[(long)t * XSTR + q];
            double dq[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double Ldx = src_gain_row(Lb + (long)t * LSTR + j * 12, dx);
                const double c_l = lnom[(long)t * USTR + j];
                const double lnew = c_l + eps * dlb[(long)t * USTR + j];   // l + eps dl   (:509)
                u[j] = lnew + Ldx;
                const double du = c_l - u[j];
                dq[j] = du * du;
            }
            const double dn = __builtin_sqrt(dq[0] + dq[1] + dq[2] + dq[3]);
            if (dn != dn) dnan = true;                                // maximum() propagates NaN
            else if (dn > dmax) dmax = dn;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) u[j] = lnom[(long)t * USTR + j];
        }
        bool inok = true;
#pragma unroll
        for (int q = 0; q < RAT_N; ++q) inok = inok && !src_nan(x[q]);
#pragma unroll
        for (int q = 0; q < RAT_M; ++q) inok = inok && !src_nan(u[q]);
        double xn[RAT_N];
        rat_user_f<double>(x, u, xn, a.p);
        bool outnan = false;
#pragma unroll
        for (int q = 0; q < RAT_N; ++q) { outnan = outnan || src_nan(xn[q]); x[q] = xn[q]; }
        if (inok && outnan) dom = 1;                                  // the reference's DomainError
#pragma unroll
        for (int q = 0; q < 12; ++q) xo[(long)(t + 1) * XSTR + q] = x[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) uo[(long)t * USTR + j] = u[j];
    }
    if (a.mode == 1) {
        st.d_c[c] = dnan ? __builtin_nan("") : dmax;
        st.flag_c[c] = dom ? 2 : 0;
    } else if (dom) {
        st.status[b] = 4;                                             // RAT_ST_DOMAIN
        st.value[b] = __builtin_inf();
    }
}

// ---- linearise: one wavefront per (trajectory, t) -------------------------------------------------------------------------------------
// Lanes over the n + m dual directions give the columns of [A | B] (or rat_user_f_jacobian on lane 0); lanes over the (i <= j) pairs of
// z = (x, u) give the hyper-dual entries of c: the Hessian (mirrored from the upper triangle, Symmetric(...) in ileqg.jl:270-271), the
// gradient (diagonal pairs) and the value.  At t = N the pairs run over x only and the function is h.
#define SRC_SH (192 + 256 + 16 + 2)
extern "C" __global__ __launch_bounds__(64 * SRC_LIN_WAVES) void rat_src_linearize(SrcLinArgs a) {
    __shared__ double sh[SRC_LIN_WAVES][SRC_SH];
    __shared__ int shdom[SRC_LIN_WAVES];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, j = l & 15;
    const StateDev &st = a.st;
    const int N = st.N;
    const int nchunk = (N + SRC_LIN_WAVES) / SRC_LIN_WAVES;
    const int c = blockIdx.x / nchunk;
    const int t = (blockIdx.x - c * nchunk) * SRC_LIN_WAVES + w;
    bool act = t <= N;
    int b = c, slot = 0;
    if (a.mode == 0) {
        act = act && st.status[b] == ST_RUNNING;
        slot = b * (st.E + 1) + st.slot_nom[b];
    } else {
        b = c / st.E;
        act = act && st.ls_active[b] != 0;
        slot = cand_slot(b, c - b * st.E, st.slot_nom[b], st.E);
    }
    double *zs = sh[w], *cs = zs + 192, *gq = cs + 256, *cv = gq + 16;
    for (int e = l; e < SRC_SH; e += 64) zs[e] = 0.0;
    if (l < 4 - RAT_M) cs[(12 + RAT_M + l) * 16 + 12 + RAT_M + l] = 1.0;       // unit diagonal in the padded rows of R
    if (l == 0) shdom[w] = 0;
    __syncthreads();
    double x[12], u[4];
#pragma unroll
    for (int q = 0; q < 12; ++q) x[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) u[q] = 0.0;
    const double *__restrict__ xp = st.xs + (long)slot * st.x_stride + (long)t * XSTR;
    const double *__restrict__ up = st.us + (long)slot * st.u_stride + (long)t * USTR;
    if (act) {
#pragma unroll
        for (int q = 0; q < RAT_N; ++q) x[q] = xp[q];
        if (t < N) {
#pragma unroll
            for (int q = 0; q < RAT_M; ++q) u[q] = up[q];
        }
    }
    bool inok = true;
#pragma unroll
    for (int q = 0; q < RAT_N; ++q) inok = inok && !src_nan(x[q]);
#pragma unroll
    for (int q = 0; q < RAT_M; ++q) inok = inok && !src_nan(u[q]);
    int dom = 0;
    if (act && t < N) {
#ifdef RAT_USER_F_JACOBIAN
        if (l == 0) {                                                 // f_returns_jacobian (ileqg.jl:302-311)
            double xn[RAT_N], A[RAT_N * RAT_N], B[RAT_N * RAT_M];
            rat_user_f_jacobian(x, u, xn, A, B, a.p);
            for (int i = 0; i < RAT_N; ++i) {
                if (src_nan(xn[i]) && inok) dom = 1;
                for (int q = 0; q < RAT_N; ++q) zs[i * 16 + q] = A[i + RAT_N * q];
                for (int g = 0; g < RAT_M; ++g) zs[i * 16 + 12 + g] = B[i + RAT_N * g];
            }
        }
#else
        if (l < SRC_NZ) {                                             // column l of [f_x | f_u]
            rat_dual xd[RAT_N], ud[RAT_M], xn[RAT_N];
#pragma unroll
            for (int q = 0; q < RAT_N; ++q) xd[q] = rat_dual(x[q], q == l ? 1.0 : 0.0);
#pragma unroll
            for (int q = 0; q < RAT_M; ++q) ud[q] = rat_dual(u[q], RAT_N + q == l ? 1.0 : 0.0);
            rat_user_f<rat_dual>(xd, ud, xn, a.p);
            const int col = src_pad(l);
#pragma unroll
            for (int i = 0; i < RAT_N; ++i) {
                if (src_nan(xn[i].v) && inok) dom = 1;
                zs[i * 16 + col] = xn[i].d;
            }
        }
#endif
        const int npair = SRC_NZ * (SRC_NZ + 1) / 2;
        for (int p = l; p < npair; p += 64) {                         // pair (i, j), i <= j, of z = (x, u), row by row
            int i = 0, rem = p;
            while (rem >= SRC_NZ - i) { rem -= SRC_NZ - i; ++i; }
            const int jj = i + rem;
            rat_hdual xh[RAT_N], uh[RAT_M];
#pragma unroll
            for (int q = 0; q < RAT_N; ++q) xh[q] = rat_hdual(x[q], q == i ? 1.0 : 0.0, q == jj ? 1.0 : 0.0, 0.0);
#pragma unroll
            for (int q = 0; q < RAT_M; ++q) uh[q] = rat_hdual(u[q], RAT_N + q == i ? 1.0 : 0.0, RAT_N + q == jj ? 1.0 : 0.0, 0.0);
            const rat_hdual r = rat_user_c<rat_hdual>(t, xh, uh, a.p);
            const int pi = src_pad(i), pj = src_pad(jj);
            cs[pi * 16 + pj] = r.e12;
            cs[pj * 16 + pi] = r.e12;
            if (i == jj) gq[pi] = r.e1;
            if (p == 0) cv[0] = r.v;
            if (src_nan(r.v) && inok) dom = 1;
        }
    } else if (act) {                                                 // terminal: h, h_x, h_xx   (ileqg.jl:314-316)
        const int npair = RAT_N * (RAT_N + 1) / 2;
        for (int p = l; p < npair; p += 64) {
            int i = 0, rem = p;
            while (rem >= RAT_N - i) { rem -= RAT_N - i; ++i; }
            const int jj = i + rem;
            rat_hdual xh[RAT_N];
#pragma unroll
            for (int q = 0; q < RAT_N; ++q) xh[q] = rat_hdual(x[q], q == i ? 1.0 : 0.0, q == jj ? 1.0 : 0.0, 0.0);
            const rat_hdual r = rat_user_h<rat_hdual>(xh, a.p);
            cs[i * 12 + jj] = r.e12;
            cs[jj * 12 + i] = r.e12;
            if (i == jj) gq[i] = r.e1;
            if (p == 0) cv[0] = r.v;
            if (src_nan(r.v) && inok) dom = 1;
        }
    }
    if (dom) shdom[w] = 1;
    __syncthreads();
    if (!act) return;
    double *__restrict__ tp = st.tiles + tile_slot(st, b, slot) * st.tile_stride + (long)t * TSTRIDE;
    if (t < N) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int e = 64 * r + l;
            tp[TS_REG(r, l)] = zs[e];
            tp[TS_REG(3 + r, l)] = (j < 12) ? cs[e] : 0.0;          // columns 12..15 of rows 0..11 are dead slots: zeros
        }
        tp[TS_REG(6, l)] = cs[192 + l];                              // [c_ux | c_uu]
        if (l < 16) tp[TS_QR + l] = gq[l];                           // [c_x | c_u]
        if (l == 0) { tp[TS_q] = cv[0]; tp[TS_PAD] = 0.0; }         // c
    } else {
        for (int e = l; e < 144; e += 64) tp[TT_Q + e] = cs[e];
        if (l < 12) tp[TT_QV + l] = gq[l];
        if (l == 0) tp[TT_q] = cv[0];
    }
    if (l == 0 && shdom[w]) {
        if (a.mode == 0) { st.status[b] = 4; st.value[b] = __builtin_inf(); }
        else st.flag_c[c] = 2;
    }
}
