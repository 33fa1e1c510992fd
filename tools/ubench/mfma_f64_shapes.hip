// v_mfma_f64_4x4x4_4b_f64 against v_mfma_f64_16x16x4_f64 for (matrix) x (vector) products on gfx950: (1) operand / accumulator layout of
// the 4x4x4 form from one-hot inputs, (2) bit equality of a K-slice chain in both forms on the same operand registers, (3) issue cost,
// dependent-chain latency and whether the 4x4x4 form blocks vector issue -- bare chains, the closed-loop rollout step in three forms, and
// row 12 of T = (column 12 of V)' Y of the replayed sweeps (sweep_dual.h: replay_body) in the forms it has and could have.
// hipcc --offload-arch=gfx950 -O3 mfma_f64_shapes.hip -o mfma_f64_shapes        (results: profiles/vec_mfma4.md)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include "../../ratilqr.jl_amd/csrc/device_utils.h"      // MFMA, MFMA4, mm3, mm3_4, mm4_4, bform3_from_blocks: the helpers as the kernels use them

typedef unsigned long long u64;
#define CK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d: %s\n", hipGetErrorName(e_), __LINE__, #x); exit(2); } } while (0)
#define LAUNCHED() do { CK(hipGetLastError()); CK(hipDeviceSynchronize()); } while (0)

// ------------------------------------------------------------------------------------------------ (1) layout
__global__ void layout_kernel(double *out) {             // block = (la, lb): A one-hot (2.0) on lane la, B one-hot (3.0) on lane lb
    const int l = threadIdx.x, la = blockIdx.x >> 6, lb = blockIdx.x & 63;
    out[blockIdx.x * 64 + l] = MFMA4(l == la ? 2.0 : 0.0, l == lb ? 3.0 : 0.0, 0.0);
}
__global__ void acc_kernel(double *out) { out[threadIdx.x] = MFMA4(0.0, 0.0, 1.0 + threadIdx.x); }
__global__ void bform_kernel(double *out) {              // lane (g, j) carries 100 (j >> 2) + 10 g + (j & 3): which lane lands where
    const int l = threadIdx.x, j = l & 15, g = l >> 4;
    double r[3];
    bform3_from_blocks(100.0 * (j >> 2) + 10.0 * g + (j & 3), r);
    for (int s = 0; s < 3; ++s) out[s * 64 + l] = r[s];
}

// ------------------------------------------------------------------------------------------------ (2) bit equality
__host__ __device__ inline u64 mix(u64 x) { x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31); }
__host__ __device__ inline double bits2d(u64 b) { double d; memcpy(&d, &b, 8); return d; }
__host__ __device__ inline u64 d2bits(double d) { u64 b; memcpy(&b, &d, 8); return b; }
__host__ __device__ inline double rnd40(u64 h) {         // random sign and mantissa, exponent uniform over 40 binades around 1
    return bits2d((h & 0x800FFFFFFFFFFFFFull) | ((u64)(1023 - 20 + (int)((h >> 52) % 41)) << 52));
}
__host__ __device__ inline double special(u64 h) {
    switch ((h >> 8) & 7) {
    case 0: return 0.0;
    case 1: return -0.0;
    case 2: return bits2d(h & 0x000FFFFFFFFFFFFFull);                         // denormal
    case 3: return bits2d((h & 0x000FFFFFFFFFFFFFull) | 0x8000000000000000ull);
    case 4: return ((h >> 11) & 15) ? bits2d(0x0010000000000000ull | (h & 0x800FFFFFFFFFFFFFull)) : INFINITY;     // (mostly: smallest normals)
    case 5: return ((h >> 11) & 15) ? bits2d(0x7FE0000000000000ull | (h & 0x800FFFFFFFFFFFFFull)) : -INFINITY;    // (mostly: largest binade)
    case 6: return ((h >> 11) & 15) ? rnd40(mix(h)) * 0x1p-1000 : bits2d(0x7FF8000000000000ull | (h & 0xFFFFull)); // (mostly: products underflow)
    default: return rnd40(mix(h)) * 0x1p-520;                                 // products land among the denormals
    }
}
// operand sets: mode 0 random over 40 binades; 1 heavy cancellation (k = 1, 3 of a slice cancel k = 0, 2 up to a few ulps, odd slices the
// even ones); 2 specials mixed in; 3 the n = 3, m = 2 tile (rows >= n and K entries beyond n, m are zero)
__host__ __device__ inline void gen(int mode, u64 set, int l, double (&a)[4], double (&b)[4], double &c) {
    const int j = l & 15, g = l >> 4;
    for (int s = 0; s < 4; ++s) {
        const u64 ha = mix(set * 1315423911ull + (u64)(l * 16 + s * 2)), hb = mix(set * 2654435761ull + (u64)(l * 16 + s * 2 + 1) + (1ull << 40));
        a[s] = rnd40(ha); b[s] = rnd40(hb);
        if (mode == 1) {
            const int gb = g & ~1, lbse = gb * 16 + j, sb = s & ~1;
            const u64 pa = mix(set * 1315423911ull + (u64)(lbse * 16 + sb * 2)), pb = mix(set * 2654435761ull + (u64)(lbse * 16 + sb * 2 + 1) + (1ull << 40));
            a[s] = rnd40(pa); b[s] = rnd40(pb);
            if ((g & 1) != (s & 1)) a[s] = -a[s] * (1.0 + (double)(ha & 7) * 0x1p-52 * (double)((ha >> 3) & 1 ? 1 : 1024));
        }
        if (mode == 2) {
            if ((ha & 7) == 0) a[s] = special(ha);
            if ((hb & 7) == 0) b[s] = special(hb);
        }
        if (mode == 3) {
            const bool klive = (s == 0 && g < 3) || (s == 3 && g < 2);
            if (!(klive && j < 3)) a[s] = 0.0;
            if (!klive) b[s] = 0.0;
        }
    }
    const u64 hc = mix(set * 40503ull + (u64)l + (2ull << 40));
    c = rnd40(hc);
    if (mode == 1) c *= 0x1p-30;
    if (mode == 2 && (hc & 7) == 0) c = special(hc);
    if (mode == 3 && (hc & 1)) c = 0.0;
}
// res[0] words compared, [1] words that differ, [2] of those: both NaN, [3] non-finite results, [4] first differing (set << 8 | lane) + 1
template <int S>
__global__ void biteq_kernel(int mode, int sets, u64 *res, double *dump, int ndump) {
    const int l = threadIdx.x, j = l & 15;
    u64 ncmp = 0, ndiff = 0, nnan = 0, nnf = 0;
    for (int it = 0; it < sets; ++it) {
        const u64 set = (u64)blockIdx.x * sets + it;
        double a[4], b[4], c;
        gen(mode, set, l, a, b, c);
        const int q = j >> 2;
        d4 c16 = {0.0, 0.0, 0.0, 0.0};                   // the same start value on the element both forms compute: register j >> 2 of this lane
        c16[0] = q == 0 ? c : 0.0; c16[1] = q == 1 ? c : 0.0; c16[2] = q == 2 ? c : 0.0; c16[3] = q == 3 ? c : 0.0;
        double r4 = c;
#pragma unroll
        for (int s = 0; s < S; ++s) { c16 = MFMA(a[s], b[s], c16); r4 = MFMA4(a[s], b[s], r4); }
        const double r16 = q == 0 ? c16[0] : q == 1 ? c16[1] : q == 2 ? c16[2] : c16[3];
        const u64 w4 = d2bits(r4), w16 = d2bits(r16);
        ++ncmp;
        if (w4 != w16) { ++ndiff; if (r4 != r4 && r16 != r16) ++nnan; atomicCAS(&res[4], 0ull, ((set << 8) | (u64)l) + 1); }
        if (!(fabs(r4) <= 1.79e308)) ++nnf;
        if (set < (u64)ndump) { dump[(set * 64 + l) * 2] = r4; dump[(set * 64 + l) * 2 + 1] = r16; }
    }
    atomicAdd(&res[0], ncmp); atomicAdd(&res[1], ndiff); atomicAdd(&res[2], nnan); atomicAdd(&res[3], nnf);
}

// ------------------------------------------------------------------------------------------------ row 12 of T in the replays
// mm3(v, y) is v'y; the replays read only row 12 of it (register 3 on the lanes g == 0): sum_k v[k][12] y[k][j].  In the 4x4x4 form the A
// operand needs column 12 of v on the lanes j & 3 == 0 of every bank (row 0 of each block): bank 3 of each 16-lane row copied to the other
// banks, bank_bcast<3>, 6 v_mov_dpp per register.  Row 0 of each block then lands on the lanes g == 0, where T's row 12 is read today.
__device__ __forceinline__ double trow4(const d4 &v, const d4 &y) {
    const double a[3] = {bank_bcast<3>(v[0]), bank_bcast<3>(v[1]), bank_bcast<3>(v[2])}, b[3] = {y[0], y[1], y[2]};
    return mm3_4(a, b, 0.0);
}
// both recursions from ONE chain: recursion B's column 12 rides in column 13 of recursion A's operand (quad permutation [0, 0, 2, 3] and a
// select on the lanes j == 13), so block row 1 is recursion B's T row; it lands on the lanes g == 1 and crosses to g == 0 by v_permlane16_swap
__device__ __forceinline__ void trow4_pair(const d4 &va, const d4 &vb, const d4 &y, bool j13, bool odd, double &ta, double &tb) {
    double a[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const double q = __hiloint2double(__builtin_amdgcn_mov_dpp(__double2hiint(vb[s]), 0xE0, 0xF, 0xF, false),
                                          __builtin_amdgcn_mov_dpp(__double2loint(vb[s]), 0xE0, 0xF, 0xF, false));
        a[s] = bank_bcast<3>(j13 ? q : va[s]);
    }
    const double b[3] = {y[0], y[1], y[2]};
    ta = mm3_4(a, b, 0.0);
    tb = row_partner<0>(ta, odd);
}
// res[0] words compared (lanes g == 0), [1] single chain differs from mm3(v, y)[3], [2] / [3] the pair's A / B row differs
__global__ void trow_kernel(int mode, int sets, u64 *res) {
    const int l = threadIdx.x, j = l & 15, g = l >> 4;
    u64 ncmp = 0, d1 = 0, d2 = 0, d3 = 0;
    for (int it = 0; it < sets; ++it) {
        const u64 set = (u64)blockIdx.x * sets + it;
        double a[4], b[4], c;
        gen(mode, set, l, a, b, c);
        const d4 va = {a[0], a[1], a[2], 0.0}, y = {b[0], b[1], b[2], 0.0};
        gen(mode, set + (1ull << 32), l, a, b, c);
        const d4 vb = {a[0], a[1], a[2], 0.0};
        const d4 ra = mm3(va, y, (d4){0, 0, 0, 0}), rb = mm3(vb, y, (d4){0, 0, 0, 0});
        const double t1 = trow4(va, y);
        double ta, tb;
        trow4_pair(va, vb, y, j == 13, (g & 1) != 0, ta, tb);
        if (g == 0) { ++ncmp; d1 += d2bits(t1) != d2bits(ra[3]); d2 += d2bits(ta) != d2bits(ra[3]); d3 += d2bits(tb) != d2bits(rb[3]); }
    }
    atomicAdd(&res[0], ncmp); atomicAdd(&res[1], d1); atomicAdd(&res[2], d2); atomicAdd(&res[3], d3);
}

// ------------------------------------------------------------------------------------------------ (3) timing
#define NVF 4      // v_fma_f64 per 4x4x4 MFMA in the mixed loop: 4 x 4 cycles = 16 cycles = one 4x4x4 MFMA if it takes 4 passes
enum { T_IND16, T_IND4, T_FMA, T_IND4_FMA, T_CH16, T_CH4, T_CH4_DPP, T_STEP16, T_STEP4_DPP, T_STEP4_REP, T_ROW16, T_ROW16_TWO, T_ROW16_STACK, T_ROW4, T_ROW4_TWO, T_ROW4_PAIR, T_COUNT };
template <int MODE>
__global__ void time_kernel(double *out, u64 *cyc, int iters, double kap) {
    const int l = threadIdx.x & 63, j = l & 15, g = l >> 4;
    const d4 zero4 = {0.0, 0.0, 0.0, 0.0};
    // operands shaped like the rollout's: zA = [A|B] slices (rows >= 12 zero), La = L slices (rows repeat every four), small entries
    double zA[4], La[3], zR[3][4], xb[3], cx[3], v[NVF];
    for (int s = 0; s < 4; ++s) zA[s] = (j < 12) ? 1e-2 * ((j * 7 + 4 * s + g) % 11 - 5) + ((j == 4 * s + g) ? 0.9 : 0.0) : 0.0;
    for (int s = 0; s < 3; ++s) La[s] = -1e-2 * (((j & 3) * 5 + 4 * s + g) % 7);
    for (int r = 0; r < 3; ++r) for (int s = 0; s < 4; ++s) {     // row-replicated A operand of rows 4 r .. 4 r + 3
        const int jj = 4 * r + (j & 3);
        zR[r][s] = 1e-2 * ((jj * 7 + 4 * s + g) % 11 - 5) + ((jj == 4 * s + g) ? 0.9 : 0.0);
    }
    for (int s = 0; s < 3; ++s) { xb[s] = 0.1 * (4 * s + g + 1); cx[s] = 0.05 * (4 * s + g); }
    for (int i = 0; i < NVF; ++i) v[i] = l * 1e-9 + i;
    const double lnom = 0.01 * g;
    double x1 = 0.1 * (4 * (j >> 2) + g + 1);                      // the vector one double per lane (4x4x4 output layout)
    d4 a0 = zero4, a1 = zero4, a2 = zero4, a3 = zero4;
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    const double a = l * 1e-3, b = 1.0 + l * 1e-4;
    // row 12 of T: v (both recursions) loop-carried through the row it produces, Y fixed
    d4 va = {0.01 * (l % 7), 0.02 * (l % 5), 0.03 * (l % 3), 0.0}, vb = {0.02 * (l % 3), 0.01 * (l % 5), 0.03 * (l % 7), 0.0};
    const d4 yy = {0.1 * (g + 1), 0.05 * (j % 4), -0.02 * (j % 3), 0.0};
    const bool j13 = j == 13, odd = (g & 1) != 0;
    const u64 t0 = __builtin_readcyclecounter();
    for (int it = 0; it < iters; ++it) {
        if (MODE >= T_ROW16 && MODE <= T_ROW4_PAIR) {
            double ta = 0.0, tb = 0.0;
            if (MODE == T_ROW16) ta = mm3(va, yy, zero4)[3];
            if (MODE == T_ROW16_TWO) { ta = mm3(va, yy, zero4)[3]; tb = mm3(vb, yy, zero4)[3]; }
            if (MODE == T_ROW16_STACK) {                            // replay_body<true, STACK>
                d4 vs;
#pragma unroll
                for (int r = 0; r < 3; ++r) vs[r] = row_ror8_merge<0x2>(va[r], vb[r]);
                vs[3] = 0.0;
                const d4 tm = mm3(vs, yy, zero4);
                ta = tm[3]; tb = tm[1];
            }
            if (MODE == T_ROW4) ta = trow4(va, yy);
            if (MODE == T_ROW4_TWO) { ta = trow4(va, yy); tb = trow4(vb, yy); }
            if (MODE == T_ROW4_PAIR) trow4_pair(va, vb, yy, j13, odd, ta, tb);
#pragma unroll
            for (int r = 0; r < 3; ++r) { va[r] = fma(va[r], 0.5, ta); vb[r] = fma(vb[r], 0.5, tb); }
        }
        if (MODE == T_IND16) { a0 = MFMA(a, b, a0); a1 = MFMA(a, b, a1); a2 = MFMA(a, b, a2); a3 = MFMA(a, b, a3); }
        if (MODE == T_IND4 || MODE == T_IND4_FMA || MODE == T_FMA) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (MODE != T_FMA) { if (q == 0) s0 = MFMA4(a, b, s0); if (q == 1) s1 = MFMA4(a, b, s1); if (q == 2) s2 = MFMA4(a, b, s2); if (q == 3) s3 = MFMA4(a, b, s3); }
                if (MODE != T_IND4) {
#pragma unroll
                    for (int i = 0; i < NVF; ++i) v[i] = fma(v[i], 1.0000001, 1e-9);
                }
            }
        }
        if (MODE == T_CH16) { const d4 xb4 = {xb[0], xb[1], xb[2], 0.0}; const d4 za = {zA[0], zA[1], zA[2], 0.0}; const d4 d = mm3(za, xb4, zero4); xb[0] = d[0]; xb[1] = d[1]; xb[2] = d[2]; }
        if (MODE == T_CH4) { const double za[3] = {zA[0], zA[1], zA[2]}; const double d = mm3_4(za, xb, 0.0); xb[0] = d; xb[1] = d; xb[2] = d; }
        if (MODE == T_CH4_DPP) { const double za[3] = {zA[0], zA[1], zA[2]}; const double d = mm3_4(za, xb, 0.0); bform3_from_blocks(d, xb); }
        if (MODE == T_STEP16) {                                     // the closed-loop step of rollin_body, recursion only
            d4 xa = MFMA(zA[0], xb[0], zero4); xa = MFMA(zA[1], xb[1], xa); xa = MFMA(zA[2], xb[2], xa);
            d4 fb = MFMA(La[0], xb[0] - cx[0], zero4); fb = MFMA(La[1], xb[1] - cx[1], fb); fb = MFMA(La[2], xb[2] - cx[2], fb);
            const double u = lnom + fb[0];
            xa = MFMA(zA[3], u, xa);
#pragma unroll
            for (int r = 0; r < 3; ++r) xb[r] = xa[r] + kap * (xb[r] * xb[r] * xb[r]);
        }
        if (MODE == T_STEP4_DPP) {                                  // 4x4x4 chains, x_{t+1} to B-form through DPP; u needs no move (L's rows repeat)
            const double za[3] = {zA[0], zA[1], zA[2]}, dx[3] = {xb[0] - cx[0], xb[1] - cx[1], xb[2] - cx[2]};
            double xa = mm3_4(za, xb, 0.0);
            const double fb = mm3_4(La, dx, 0.0);
            const double u = lnom + fb;
            xa = MFMA4(zA[3], u, xa);
            x1 = xa + kap * (x1 * x1 * x1);
            bform3_from_blocks(x1, xb);
        }
        if (MODE == T_STEP4_REP) {                                  // 4x4x4 chains, one per B-form register with a row-replicated A operand: no moves
            const double dx[3] = {xb[0] - cx[0], xb[1] - cx[1], xb[2] - cx[2]};
            double xr[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) { const double za[3] = {zR[r][0], zR[r][1], zR[r][2]}; xr[r] = mm3_4(za, xb, 0.0); }
            const double fb = mm3_4(La, dx, 0.0);
            const double u = lnom + fb;
#pragma unroll
            for (int r = 0; r < 3; ++r) xb[r] = MFMA4(zR[r][3], u, xr[r]) + kap * (xb[r] * xb[r] * xb[r]);
        }
    }
    double s = s0 + s1 + s2 + s3;
    for (int i = 0; i < NVF; ++i) s += v[i];
    asm volatile("" :: "v"(a0[0]), "v"(a1[0]), "v"(a2[0]), "v"(a3[0]), "v"(s), "v"(x1), "v"(xb[0]), "v"(xb[1]), "v"(xb[2]), "v"(va[0]), "v"(va[1]), "v"(va[2]), "v"(vb[0]), "v"(vb[1]), "v"(vb[2]));
    const u64 t1 = __builtin_readcyclecounter();
    out[MODE * 256 + threadIdx.x] = a0[0] + a1[1] + a2[2] + a3[3] + s + xb[0] + xb[1] + xb[2] + va[0] + vb[0];
    if (l == 0) cyc[threadIdx.x >> 6] = t1 - t0;
}

template <int MODE> static void run_time(const char *name, double *out, u64 *cyc, int per_iter) {
    const int iters = 2000;
    u64 h[4];
    double xo[256];
    for (int waves = 1; waves <= 4; waves *= 4) {                  // one wave on one SIMD; four waves, one per SIMD
        for (int rep = 0; rep < 2; ++rep) { hipLaunchKernelGGL(time_kernel<MODE>, dim3(1), dim3(64 * waves), 0, 0, out, cyc, iters, 1e-3); LAUNCHED(); }
        CK(hipMemcpy(h, cyc, sizeof h, hipMemcpyDeviceToHost));
        CK(hipMemcpy(xo, out + MODE * 256, sizeof xo, hipMemcpyDeviceToHost));
        printf("  %-58s %d wave(s): cycles per iteration", name, waves);
        for (int w = 0; w < waves; ++w) printf(" %.1f", (double)h[w] / iters);
        if (per_iter > 1) printf("  (%.1f per MFMA)", (double)h[0] / iters / per_iter);
        printf("   [lane 0: %.6g]\n", xo[0]);
    }
}

int main() {
    double *out; u64 *res;
    CK(hipMalloc(&out, 8 * 4096 * 64)); CK(hipMalloc(&res, 8 * 64));
    int bad = 0;
    // ---- (1) layout ------------------------------------------------------------------------------------------------------
    {
        std::vector<double> h(4096 * 64);
        hipLaunchKernelGGL(layout_kernel, dim3(4096), dim3(64), 0, 0, out); LAUNCHED();
        CK(hipMemcpy(h.data(), out, 8 * h.size(), hipMemcpyDeviceToHost));
        // hypothesis: D lane (i, 4 q + c) = sum_k A lane (k, 4 q + i) x B lane (k, 4 q + c)
        int wrong = 0;
        for (int la = 0; la < 64; ++la) for (int lb = 0; lb < 64; ++lb) for (int lo = 0; lo < 64; ++lo) {
            const int i = lo >> 4, q = (lo & 15) >> 2, c = lo & 3;
            const bool hit = (la >> 4) == (lb >> 4) && (la & 15) == 4 * q + i && (lb & 15) == 4 * q + c;
            const double want = hit ? 6.0 : 0.0, got = h[(la * 64 + lb) * 64 + lo];
            if (got != want) { if (wrong < 8) printf("  layout: A lane %d, B lane %d -> D lane %d = %g, expected %g\n", la, lb, lo, got, want); ++wrong; }
        }
        printf("(1) layout of v_mfma_f64_4x4x4_4b_f64, 64 x 64 one-hot pairs: D lane (g, j) = sum_k A lane (k, 4 (j >> 2) + g) * B lane (k, j): %s (%d of 262144 entries off)\n",
               wrong ? "NO" : "yes", wrong);
        bad |= wrong != 0;
        hipLaunchKernelGGL(acc_kernel, dim3(1), dim3(64), 0, 0, out); LAUNCHED();
        CK(hipMemcpy(h.data(), out, 8 * 64, hipMemcpyDeviceToHost));
        int accw = 0; for (int l = 0; l < 64; ++l) accw += h[l] != 1.0 + l;
        printf("    accumulator: C of lane l arrives in D of lane l: %s\n", accw ? "NO" : "yes");
        bad |= accw != 0;
        hipLaunchKernelGGL(bform_kernel, dim3(1), dim3(64), 0, 0, out); LAUNCHED();
        CK(hipMemcpy(h.data(), out, 8 * 192, hipMemcpyDeviceToHost));
        int bw = 0;
        for (int s = 0; s < 3; ++s) for (int l = 0; l < 64; ++l) {                 // bank s of the row, column kept modulo 4
            const double want = 100.0 * s + 10.0 * (l >> 4) + (l & 3);
            if (h[s * 64 + l] != want) { if (bw < 8) printf("  bform: register %d lane %d = %g, expected %g\n", s, l, h[s * 64 + l], want); ++bw; }
        }
        printf("    bform3_from_blocks: register s of lane (g, j) = bank s of row g, column j & 3: %s\n", bw ? "NO" : "yes");
        bad |= bw != 0;
    }
    // ---- (2) bit equality ------------------------------------------------------------------------------------------------
    {
        const int ndump = 256, blocks = 1024;
        double *dump; CK(hipMalloc(&dump, 8 * ndump * 128));
        std::vector<double> hd(ndump * 128);
        const char *mn[4] = {"random, 40 binades", "heavy cancellation", "+-0, denormals, inf, NaN mixed in", "n = 3, m = 2 tile, zeros elsewhere"};
        const int sets[4] = {1000, 250, 250, 250};
        printf("(2) 4x4x4 chain against 16x16x4 chain, same operand registers and start value, every lane's element compared word for word\n");
        printf("    | operand sets | slices | sets | words compared | words differing | of those both NaN | non-finite results | host fma chain in K order equal (first %d sets) |\n    |---|---|---|---|---|---|---|---|\n", ndump);
        for (int mode = 0; mode < 4; ++mode) for (int S = 3; S <= 4; ++S) {
            u64 r[8];
            CK(hipMemset(res, 0, 64));
            if (S == 3) hipLaunchKernelGGL(biteq_kernel<3>, dim3(blocks), dim3(64), 0, 0, mode, sets[mode], res, dump, ndump);
            else hipLaunchKernelGGL(biteq_kernel<4>, dim3(blocks), dim3(64), 0, 0, mode, sets[mode], res, dump, ndump);
            LAUNCHED();
            CK(hipMemcpy(r, res, 64, hipMemcpyDeviceToHost));
            CK(hipMemcpy(hd.data(), dump, 8 * hd.size(), hipMemcpyDeviceToHost));
            // the first ndump sets, recomputed on the host
            int heq = 0, hn = 0;
            const int nd = ndump;
            for (int set = 0; set < nd; ++set) {
                double A[64][4], B[64][4], C[64];
                for (int l = 0; l < 64; ++l) gen(mode, set, l, A[l], B[l], C[l]);
                for (int lo = 0; lo < 64; ++lo) {
                    const int i = lo >> 4, q = (lo & 15) >> 2;
                    double acc = C[lo];
                    for (int s = 0; s < S; ++s) for (int k = 0; k < 4; ++k) acc = fma(A[k * 16 + 4 * q + i][s], B[k * 16 + (lo & 15)][s], acc);
                    const double dv = hd[(set * 64 + lo) * 2];
                    heq += (d2bits(acc) == d2bits(dv)) || (acc != acc && dv != dv); ++hn;
                }
            }
            printf("    | %s | %d | %d | %llu | %llu | %llu | %llu | %d of %d |\n", mn[mode], S, blocks * sets[mode], r[0], r[1], r[2], r[3], heq, hn);
            if (r[1]) printf("      first differing word: set %llu lane %llu\n", (r[4] - 1) >> 8, (r[4] - 1) & 255);
            bad |= r[1] != 0 || r[0] != (u64)blocks * sets[mode] * 64;       // (nothing compared is a failure, not a pass)
        }
        printf("    row 12 of T on the lanes g == 0: one 4x4x4 chain per recursion, and one chain for both, against mm3(v, y)[3] of each recursion\n");
        printf("    | operand sets | words compared | single chain differs | pair: recursion A differs | pair: recursion B differs |\n    |---|---|---|---|---|\n");
        for (int mode = 0; mode < 3; ++mode) {
            u64 r[8];
            CK(hipMemset(res, 0, 64));
            hipLaunchKernelGGL(trow_kernel, dim3(256), dim3(64), 0, 0, mode, 250, res);
            LAUNCHED();
            CK(hipMemcpy(r, res, 64, hipMemcpyDeviceToHost));
            printf("    | %s | %llu | %llu | %llu | %llu |\n", mn[mode], r[0], r[1], r[2], r[3]);
            bad |= (r[1] | r[2] | r[3]) != 0 || r[0] != 256ull * 250 * 16;
        }
    }
    // ---- (3) timing ------------------------------------------------------------------------------------------------------
    {
        u64 *cyc; CK(hipMalloc(&cyc, 64));
        printf("(3) cycles per loop iteration (s_memtime), 2000 iterations\n");
        run_time<T_IND16>("4 independent 16x16x4", out, cyc, 4);
        run_time<T_IND4>("4 independent 4x4x4", out, cyc, 4);
        run_time<T_FMA>("16 independent v_fma_f64", out, cyc, 1);
        run_time<T_IND4_FMA>("4 x (4x4x4 + 4 v_fma_f64) interleaved", out, cyc, 1);
        run_time<T_CH16>("chain of 3 16x16x4, D feeds the next B", out, cyc, 1);
        run_time<T_CH4>("chain of 3 4x4x4, D feeds the next B (no moves)", out, cyc, 1);
        run_time<T_CH4_DPP>("chain of 3 4x4x4 + bform3_from_blocks", out, cyc, 1);
        run_time<T_STEP16>("closed-loop step, 7 x 16x16x4", out, cyc, 1);
        run_time<T_STEP4_DPP>("closed-loop step, 7 x 4x4x4 + bform3_from_blocks", out, cyc, 1);
        run_time<T_STEP4_REP>("closed-loop step, 15 x 4x4x4, row-replicated A, no moves", out, cyc, 1);
        run_time<T_ROW16>("T row 12, one recursion: mm3 16x16x4", out, cyc, 1);
        run_time<T_ROW4>("T row 12, one recursion: bank_bcast<3> + 3 x 4x4x4", out, cyc, 1);
        run_time<T_ROW16_TWO>("T row 12, two recursions: two mm3 16x16x4", out, cyc, 1);
        run_time<T_ROW16_STACK>("T row 12, two recursions: stacked mm3 16x16x4 (today)", out, cyc, 1);
        run_time<T_ROW4_TWO>("T row 12, two recursions: two 4x4x4 chains", out, cyc, 1);
        run_time<T_ROW4_PAIR>("T row 12, two recursions: one 4x4x4 chain + row swap", out, cyc, 1);
    }
    printf("%s\n", bad ? "GATE: layout or bit equality FAILED" : "layout and bit equality hold");
    return bad;
}
