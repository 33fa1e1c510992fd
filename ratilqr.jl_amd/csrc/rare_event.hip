// rare_event.hip -- the kernels of rat_policy_rare_event (rare_event.h has the chain, the keying and the scratch layout).
//
// re_rollout is noisy_rollout_kernel (kernels.hip) and ev_eval (policy_mc.hip) in one pass, without the trajectory in between: the same
// operations in the same order on every state, control and g, so that with a zero shift the margins are rat_policy_events' bit for bit.
// Layout: a wavefront takes sixteen rollouts as the columns of Z [16 components][16 rollouts]; lane (col = lane & 15, kq = lane >> 4)
// owns Z[kq + 4 r][col], r = 0 .. 3 -- state components kq, kq + 4, kq + 8 and control component kq -- which is ev_eval's B operand of
// Q Z.  A step exchanges x, u and the noise of a rollout between its four lanes through a wavefront-private LDS row per rollout (odd
// strides: the sixteen columns fall in different banks, the four kq lanes of a column read one address); each lane then runs the
// row of [A | B] (LDS, staged once per workgroup), of L_t and of chol(W(t)) (global, L1-resident) of each of its components, draws its
// three normals of a step pair with one Philox block and one Box-Muller transform each, and adds its part of logw.  The shift is read
// from LDS ([N][12], staged once per workgroup: four addresses per wavefront and step, a broadcast each).  The cost is not formed: the
// call does not use it.
#include "rare_event.h"

#include <cstring>

#include "device_utils.h"
#include "mc_tree.h"
#include "rat_normal.h"
#include "rat_philox.h"
#include "rat_pow.h"

namespace {

typedef double re_d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool re_nan(double v) { return v != v; }

// (the reductions are mc_tree.h's block_tree and block_tree_n: the trees of policy_mc.hip, one definition)

// kernels.hip's powchk: Julia's DomainError for a negative base with a fractional exponent
__device__ __forceinline__ double re_powchk(double bse, double e, int &dom) {
    const double r = rat_pow(bse, e);
    if (r != r && bse == bse) dom = 1;
    return r;
}

// the Philox key and counter of rollout i (rare_event.h, "Keying")
__device__ __forceinline__ void re_key(const ReArgs &a, long i, unsigned long long &cseed, long &k) {
    const long ci = i / a.chunk;
    k = i - ci * a.chunk;
    cseed = a.seed + RE_CHUNK_STRIDE * (unsigned long long)ci;
}

// g(z) of the lane's column, as ev_eval forms it: every lane of the column returns the same bits
template <bool QUAD>
__device__ __forceinline__ double re_g(const double (&zv)[4], const double *s_a, const double *s_q, int kq, int col, double b) {
    const double *ae = s_a + kq;
    double p = ae[0] * zv[0] + ae[4] * zv[1] + ae[8] * zv[2] + ae[12] * zv[3];
    if (QUAD) {
        const double *qe = s_q + kq * 16 + col;
        re_d4 c = (re_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) c = __builtin_amdgcn_mfma_f64_16x16x4f64(qe[kb * 64], zv[kb], c, 0, 0, 0);
        p += c[0] * zv[0] + c[1] * zv[1] + c[2] * zv[2] + c[3] * zv[3];
    }
    p += __shfl_xor(p, 16);
    p += __shfl_xor(p, 32);
    return p + b;
}

#define RE_XU_LD 17
#define RE_Z_LD 13

template <bool QUAD, bool LQ>
__global__ __launch_bounds__(MC_THREADS, 2) void re_rollout(ReArgs a) {
    extern __shared__ double s_shift[];                               // [N][12]
    __shared__ double s_q[QUAD ? 256 : 1], s_a[16], s_zt[LQ ? 192 : 1];   // s_zt: [A | B], 12 x 16 row-major
    __shared__ double s_xu[4][16 * RE_XU_LD], s_dx[4][16 * RE_Z_LD], s_z[4][16 * RE_Z_LD];
    const ProblemDev &pb = a.pb;
    const int tid = threadIdx.x, N = pb.N, n = pb.n, m = pb.m;
    if (QUAD) s_q[tid] = a.Qt[tid];
    if (tid < 16) s_a[tid] = a.at[tid];
    if (LQ && tid < 192) s_zt[tid] = pb.Zt[tid];
    for (int i = tid; i < N * 12; i += MC_THREADS) s_shift[i] = a.shift[i];
    __syncthreads();
    const int w = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    double *xu = s_xu[w] + col * RE_XU_LD, *dxs = s_dx[w] + col * RE_Z_LD, *zs = s_z[w] + col * RE_Z_LD;
    const double nan = __builtin_nan("");
    const long G = (a.K + 15) >> 4;
    for (long g = (long)blockIdx.x * 4 + w; g < G; g += (long)gridDim.x * 4) {           // (uniform over the wavefront)
        const long i = 16 * g + col;
        const bool live = i < a.K;                                    // (the K tail: the lane runs rollout K - 1 again and stores nothing)
        unsigned long long cseed;
        long k;
        re_key(a, live ? i : a.K - 1, cseed, k);
        double x[3], znext[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 3; ++r) x[r] = a.xnom[kq + 4 * r];
        double lw = 0.0, M = nan;
        int dom = 0;
        for (int t = 0; t <= N; ++t) {
            double zv[4] = {x[0], x[1], x[2], 0.0};
            double u = 0.0;
            if (t < N) {
                u = a.l[(long)t * USTR + kq];
                if (a.L) {                                            // L_t (x_t - xbar_t)
#pragma unroll
                    for (int r = 0; r < 3; ++r) dxs[kq + 4 * r] = x[r] - a.xnom[(long)t * XSTR + kq + 4 * r];
                    WAVE_SYNC();
                    double acc = 0.0;
#pragma unroll
                    for (int q = 0; q < 12; ++q) acc = fma(a.L[(long)t * LSTR + kq * 12 + q], dxs[q], acc);
                    u += acc;
                }
                zv[3] = (kq < m) ? u : 0.0;
            }
            if (t >= a.t_lo && t <= a.t_hi) {                         // (uniform over the grid)
                const double gv = re_g<QUAD>(zv, s_a, s_q, kq, col, a.b);
                if (gv > M || re_nan(M)) M = gv;                      // (a NaN g never replaces a number)
            }
            if (t == N) break;
            const int kw = pb.W_tv ? t : 0;
            double z[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int c = kq + 4 * r;
                if (c < n) {
                    if ((t & 1) == 0) {                               // both outputs of one Box-Muller transform: steps t and t + 1
                        unsigned rr[4];
                        philox4x32_10((unsigned)k, (unsigned)(k >> 32), (unsigned)(t >> 1), (unsigned)c, (unsigned)cseed, (unsigned)(cseed >> 32), rr);
                        ratn_box_muller(u01(rr[0], rr[1]), u01(rr[2], rr[3]), &z[r], &znext[r]);
                    } else z[r] = znext[r];
                    const double sv = s_shift[t * 12 + c];            // z = s + xi; logw += -s z + s^2 / 2
                    z[r] = z[r] + sv;
                    lw += fma(-sv, z[r], 0.5 * sv * sv);
                } else z[r] = 0.0;
                xu[c] = x[r];
                zs[c] = z[r];
            }
            xu[12 + kq] = u;
            WAVE_SYNC();
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int c = kq + 4 * r;
                double xn = 0.0;
                if (LQ) {
                    double dyn = 0.0;
#pragma unroll
                    for (int q = 0; q < 16; ++q) dyn = fma(s_zt[c * 16 + q], xu[q], dyn);
                    if (pb.kappa != 0.0) dyn += pb.kappa * (x[r] * x[r] * x[r]);
                    xn = dyn;
                } else if (c < n) {
#pragma unroll 1
                    for (int j = 0; j < 4; ++j) {                     // x^a + u^b; the cost's x^p and u^pu can raise the DomainError too
                        const double v = re_powchk((j & 1) ? u : x[r], j == 0 ? pb.pl_a : j == 1 ? pb.pl_b : j == 2 ? pb.pl_p : pb.pl_pu, dom);
                        if (j < 2) xn = (j == 0) ? v : xn + v;
                    }
                }
                double wv = 0.0;                                      // w_t = chol_lower(W(t)) z_t
#pragma unroll
                for (int q = 0; q < 12; ++q) wv = fma(a.Wchol[(long)kw * 192 + c * 16 + q], zs[q], wv);
                x[r] = (c < n) ? xn + wv : 0.0;
            }
            WAVE_SYNC();
        }
        lw += __shfl_xor(lw, 16);
        lw += __shfl_xor(lw, 32);
        dom |= __shfl_xor(dom, 16);
        dom |= __shfl_xor(dom, 32);
        if (kq == 0 && live) {
            a.margin[i] = dom ? nan : M;
            a.logw[i] = lw;
            a.dom[i] = dom;
        }
    }
}

// gamma and the iteration's code from the select's row
__global__ void re_level(ReArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double *row = a.scratch + RE_O_TR + TR_O_ROWS;
    const double val = row[1], flag = row[7];
    int code;
    if (flag == 2.0) code = 2;
    else if (flag == 3.0 || re_nan(val)) code = 3;
    else code = (val >= 0.0) ? 1 : 0;
    const double gamma = (code == 1) ? 0.0 : (code == 0) ? val : __builtin_nan("");
    a.scratch[RE_O_LVL] = gamma;
    reinterpret_cast<int *>(a.scratch + RE_O_CTL)[0] = code;
    double *tr = a.scratch + RE_O_TRACE + a.iter * RE_NTRACE;
    tr[0] = gamma; tr[1] = __builtin_nan(""); tr[2] = __builtin_nan(""); tr[3] = __builtin_nan("");
}

__global__ __launch_bounds__(MC_THREADS) void re_pass_a(ReArgs a) {
    __shared__ double sh[MC_THREADS];
    const long T = (long)MC_BLOCKS * MC_THREADS;
    double cnt = 0.0, ndom = 0.0, mx = -__builtin_inf(), mn = __builtin_inf();
    for (long i = (long)blockIdx.x * MC_THREADS + threadIdx.x; i < a.K; i += T) {
        if (a.dom[i]) { ndom += 1.0; continue; }
        const double lw = a.logw[i];
        cnt += 1.0;
        mx = (lw > mx || re_nan(lw)) ? lw : mx;                       // (a NaN logw reaches the flag)
        mn = (lw < mn || re_nan(lw)) ? lw : mn;
    }
    cnt = block_tree<0>(cnt, sh);
    ndom = block_tree<0>(ndom, sh);
    const double bad = block_tree<0>((mx == mx && mn == mn) ? 0.0 : 1.0, sh);   // (the trees' comparisons would drop a NaN)
    mx = block_tree<2>(mx, sh);
    mn = block_tree<1>(mn, sh);
    if (bad != 0.0) { mx = __builtin_nan(""); mn = __builtin_nan(""); }
    if (threadIdx.x == 0) {
        double *p = a.scratch + RE_O_PA;
        p[0 * MC_BLOCKS + blockIdx.x] = cnt; p[1 * MC_BLOCKS + blockIdx.x] = ndom;
        p[2 * MC_BLOCKS + blockIdx.x] = mx; p[3 * MC_BLOCKS + blockIdx.x] = mn;
    }
}

struct ReHead { double n_ok, n_dom, lmax, lmin; };

// second level of pass A's tree: lane i holds the partial of workgroup i (a NaN partial makes the extreme NaN)
__device__ __forceinline__ ReHead re_head(const double *scr, double *sh) {
    const int tid = threadIdx.x;
    const double *p = scr + RE_O_PA;
    ReHead r;
    r.n_ok = block_tree<0>(p[0 * MC_BLOCKS + tid], sh);
    r.n_dom = block_tree<0>(p[1 * MC_BLOCKS + tid], sh);
    const double mx = p[2 * MC_BLOCKS + tid], mn = p[3 * MC_BLOCKS + tid];
    const double bad = block_tree<0>((mx == mx && mn == mn) ? 0.0 : 1.0, sh);
    r.lmax = block_tree<2>(mx, sh);
    r.lmin = block_tree<1>(mn, sh);
    if (bad != 0.0) { r.lmax = __builtin_nan(""); r.lmin = __builtin_nan(""); }
    return r;
}

__global__ __launch_bounds__(MC_THREADS) void re_pass_b(ReArgs a) {
    __shared__ double sh[3 * MC_THREADS];
    const ReHead hd = re_head(a.scratch, sh);
    const long T = (long)MC_BLOCKS * MC_THREADS;
    double v[3] = {0.0, 0.0, 0.0};
    for (long i = (long)blockIdx.x * MC_THREADS + threadIdx.x; i < a.K; i += T) {
        if (!(a.margin[i] > 0.0)) continue;                           // (a DomainError rollout's margin is NaN)
        const double wt = exp(a.logw[i] - hd.lmax);
        v[0] += wt;
        v[1] += wt * wt;
        v[2] += 1.0;
    }
    block_tree_n<3>(v, sh);
    if (threadIdx.x == 0) {
        double *p = a.scratch + RE_O_PB;
        p[0 * MC_BLOCKS + blockIdx.x] = v[0]; p[1 * MC_BLOCKS + blockIdx.x] = v[1]; p[2 * MC_BLOCKS + blockIdx.x] = v[2];
    }
}

__global__ __launch_bounds__(MC_THREADS) void re_final(ReArgs a) {
    __shared__ double sh[3 * MC_THREADS];
    const int tid = threadIdx.x;
    const ReHead hd = re_head(a.scratch, sh);
    const double *p = a.scratch + RE_O_PB;
    double v[3] = {p[0 * MC_BLOCKS + tid], p[1 * MC_BLOCKS + tid], p[2 * MC_BLOCKS + tid]};
    block_tree_n<3>(v, sh);
    if (tid != 0) return;
    const double nan = __builtin_nan(""), n = hd.n_ok, S1 = v[0], S2 = v[1], nv = v[2];
    const int bad = reinterpret_cast<const int *>(a.scratch + RE_O_CTL)[1];
    const int code = reinterpret_cast<const int *>(a.scratch + RE_O_CTL)[0];
    double *o = a.scratch + RE_O_STATS;
    const double e = exp(hd.lmax);                                    // the weights were formed about max logw
    const double prob = e * S1 / n;
    double s2 = S2 - S1 * S1 / n;
    if (s2 < 0.0) s2 = 0.0;
    const double se = (n >= 2.0) ? e * sqrt(s2 / (n - 1.0) / n) : nan;
    double flag = a.reached ? 0.0 : 1.0;
    if (!(n > 0.0)) flag = 2.0;
    else if (bad || code == 3 || !(fabs(hd.lmax) < __builtin_inf()) || !(fabs(hd.lmin) < __builtin_inf()) || !(prob < __builtin_inf())) flag = 3.0;
    const bool dead = flag >= 2.0;
    o[0] = dead ? nan : prob;
    o[1] = dead ? nan : se;
    o[2] = dead ? nan : (nv > 0.0 ? S1 * S1 / S2 : 0.0);
    o[3] = nv; o[4] = n; o[5] = hd.n_dom;
    o[6] = (n > 0.0) ? hd.lmax : nan; o[7] = (n > 0.0) ? hd.lmin : nan;
    o[8] = flag;
    o[9] = (double)a.n_run;
    o[10] = (a.n_run > 0) ? a.scratch[RE_O_LVL] : nan;
    o[11] = 0.0;
}

// One workgroup per (slot, step pair): lane tid of slot s takes the rollouts s * 256 + tid, + RE_SLOTS * 256, ... in order, draws the
// pair's normals of every elite rollout again (re_rollout's Philox blocks) and adds w xi per step and component; the lanes combine in
// the fixed tree into the slot's partial.  The workgroups of step pair 0 also sum w, w^2 and the elite count.
__global__ __launch_bounds__(MC_THREADS) void re_elite(ReArgs a) {
    __shared__ double sh[8 * MC_THREADS];
    const int slot = blockIdx.x, tp = blockIdx.y, tid = threadIdx.x, N = a.pb.N, n = a.pb.n;
    const double lmax = re_head(a.scratch, sh).lmax, gamma = a.scratch[RE_O_LVL];
    double a0[12], a1[12], sw[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 12; ++c) { a0[c] = 0.0; a1[c] = 0.0; }
    const long T = (long)RE_SLOTS * MC_THREADS;
    for (long i = (long)slot * MC_THREADS + tid; i < a.K; i += T) {
        if (!(a.margin[i] >= gamma)) continue;                        // (NaN margins -- DomainError rollouts among them -- are no elite)
        const double wt = exp(a.logw[i] - lmax);
        sw[0] += wt; sw[1] += wt * wt; sw[2] += 1.0;
        unsigned long long cseed;
        long k;
        re_key(a, i, cseed, k);
#pragma unroll
        for (int c = 0; c < 12; ++c) {
            if (c < n) {                                              // (uniform over the grid)
                unsigned rr[4];
                double z0, z1;
                philox4x32_10((unsigned)k, (unsigned)(k >> 32), (unsigned)tp, (unsigned)c, (unsigned)cseed, (unsigned)(cseed >> 32), rr);
                ratn_box_muller(u01(rr[0], rr[1]), u01(rr[2], rr[3]), &z0, &z1);
                a0[c] += wt * z0;
                a1[c] += wt * z1;
            }
        }
    }
    const bool odd = 2 * tp + 1 < N;                                  // (an odd horizon leaves half of the last pair unused)
#pragma unroll
    for (int c0 = 0; c0 < 12; c0 += 4) {
        double v[8] = {a0[c0], a0[c0 + 1], a0[c0 + 2], a0[c0 + 3], a1[c0], a1[c0 + 1], a1[c0 + 2], a1[c0 + 3]};
        block_tree_n<8>(v, sh);
        if (tid == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a.part[((size_t)(2 * tp) * 12 + c0 + q) * RE_SLOTS + slot] = v[q];
                if (odd) a.part[((size_t)(2 * tp + 1) * 12 + c0 + q) * RE_SLOTS + slot] = v[4 + q];
            }
        }
    }
    if (tp == 0) {
        block_tree_n<3>(sw, sh);
        if (tid == 0)
            for (int q = 0; q < 3; ++q) a.part[((size_t)N * 12 + q) * RE_SLOTS + slot] = sw[q];
    }
}

// re_elite for rat_rng's stream (rat_policy_rare_event_noise; a.pb.n is P, the normals a step declares): one workgroup per (slot, step),
// the same lanes, trips, tree and slot order.  An elite rollout replays the ceil(P / 2) Philox blocks of step t -- counter (g lo, g hi,
// t, q) with g the global rollout index, key seed_p, one Box-Muller transform each: normals 2 q and 2 q + 1 (rat_rng.h) -- whether or not
// the rollout drew them: a component it did not draw adds sampling noise to the update and no bias to the estimate.  The workgroups of
// step 0 also sum w, w^2 and the elite count.
// rat_policy_rare_event_params (a.pn > 0): row N of the grid replays the a.pn parameter normals -- the blocks with the step word
// 0xFFFFFFFF of source_params.h -- into the partials behind the three sums, and a.fix takes the rows that stay still out of the grid: with
// bit 0 the grid is row N alone, with bit 1 it ends at row N - 1.  The first row of the grid, whichever it is, sums w, w^2 and the count.
__global__ __launch_bounds__(MC_THREADS) void re_elite_rng(ReArgs a) {
    __shared__ double sh[4 * MC_THREADS];
    const int slot = blockIdx.x, tid = threadIdx.x, N = a.pb.N;
    const int t = (int)blockIdx.y + ((a.pn > 0 && (a.fix & 1)) ? N : 0);
    const bool prow = t == N;                                         // (uniform over the workgroup)
    const int P = prow ? a.pn : a.pb.n;
    const unsigned tw = prow ? 0xFFFFFFFFu : (unsigned)t;
    const size_t e0 = prow ? (size_t)N * 12 + 3 : (size_t)t * 12;
    const double lmax = re_head(a.scratch, sh).lmax, gamma = a.scratch[RE_O_LVL];
    double acc[12], sw[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 12; ++c) acc[c] = 0.0;
    const long T = (long)RE_SLOTS * MC_THREADS;
    for (long i = (long)slot * MC_THREADS + tid; i < a.K; i += T) {
        if (!(a.margin[i] >= gamma)) continue;                        // (NaN margins -- DomainError rollouts among them -- are no elite)
        const double wt = exp(a.logw[i] - lmax);
        sw[0] += wt; sw[1] += wt * wt; sw[2] += 1.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            if (2 * q < P) {                                          // (uniform over the grid)
                unsigned rr[4];
                double z0, z1;
                philox4x32_10((unsigned)i, (unsigned)(i >> 32), tw, (unsigned)q, (unsigned)a.seed, (unsigned)(a.seed >> 32), rr);
                ratn_box_muller(u01(rr[0], rr[1]), u01(rr[2], rr[3]), &z0, &z1);
                acc[2 * q] += wt * z0;
                acc[2 * q + 1] += wt * z1;                            // (the spare output of an odd P: never stored)
            }
        }
    }
#pragma unroll
    for (int c0 = 0; c0 < 12; c0 += 4) {
        if (c0 >= P) break;                                           // (uniform over the grid)
        double v[4] = {acc[c0], acc[c0 + 1], acc[c0 + 2], acc[c0 + 3]};
        block_tree_n<4>(v, sh);
        if (tid == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (c0 + q < P) a.part[(e0 + c0 + q) * RE_SLOTS + slot] = v[q];
        }
    }
    if (blockIdx.y == 0) {
        block_tree_n<3>(sw, sh);
        if (tid == 0)
            for (int q = 0; q < 3; ++q) a.part[((size_t)N * 12 + q) * RE_SLOTS + slot] = sw[q];
    }
}

__device__ __forceinline__ double re_slot_sum(const double *part, size_t e) {
    double v = 0.0;
    for (int s = 0; s < RE_SLOTS; ++s) v += part[e * RE_SLOTS + s];
    return v;
}

// the slots in index order; s += sum_E w xi / sum_E w, all of it or (a sum that is not finite, no weight) none of it; the trace row.
// With a.pn > 0 (rat_policy_rare_event_params) the parameter row, ps += sum_E w xi^p / sum_E w, is the second part of the same update: a
// part that a.fix holds still is neither checked nor moved, an entry that is not finite in either moving part drops both, and |ps| goes
// beside the trace.  The step part's sums keep their lanes and their tree, so a call without a parameter row returns the bits it returned.
__global__ __launch_bounds__(MC_THREADS) void re_update(ReArgs a) {
    __shared__ double sh[MC_THREADS];
    __shared__ double s_ps[12];
    __shared__ int s_bad;
    const int tid = threadIdx.x, N = a.pb.N, n = a.pb.n, ne = N * 12, pn = a.pn;
    const bool mv_s = !(pn > 0 && (a.fix & 1)), mv_p = pn > 0 && !(a.fix & 2);
    if (tid == 0) s_bad = 0;
    __syncthreads();
    const double W = re_slot_sum(a.part, (size_t)ne), W2 = re_slot_sum(a.part, (size_t)ne + 1), cnt = re_slot_sum(a.part, (size_t)ne + 2);
    int bad = !(W > 0.0 && W < __builtin_inf());
    if (mv_s) {
        for (int e = tid; e < ne; e += MC_THREADS) {
            if (e % 12 >= n) continue;
            const double d = re_slot_sum(a.part, (size_t)e) / W;
            if (!(fabs(a.shift[e] + d) < __builtin_inf())) bad = 1;
        }
    }
    if (mv_p && tid < pn) {
        const double d = re_slot_sum(a.part, (size_t)ne + 3 + tid) / W;
        if (!(fabs(a.shift[ne + tid] + d) < __builtin_inf())) bad = 1;
    }
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    bad = s_bad;
    double ss = 0.0;
    for (int e = tid; e < ne; e += MC_THREADS) {
        if (e % 12 >= n) continue;
        double sv = a.shift[e];
        if (!bad && mv_s) { sv += re_slot_sum(a.part, (size_t)e) / W; a.shift[e] = sv; }
        ss += sv * sv;
    }
    ss = block_tree<0>(ss, sh);
    if (tid < pn) {                                                   // (pn <= 12: the row is summed by one lane, in index order)
        double pv = a.shift[ne + tid];
        if (!bad && mv_p) { pv += re_slot_sum(a.part, (size_t)ne + 3 + tid) / W; a.shift[ne + tid] = pv; }
        s_ps[tid] = pv;
    }
    __syncthreads();
    if (tid == 0) {
        double *tr = a.scratch + RE_O_TRACE + a.iter * RE_NTRACE;
        tr[1] = cnt; tr[2] = W * W / W2; tr[3] = sqrt(ss);
        if (pn > 0) {
            double pss = 0.0;
            for (int e = 0; e < pn; ++e) pss += s_ps[e] * s_ps[e];
            a.scratch[RE_O_PTRACE + a.iter] = sqrt(pss);
        }
        if (bad) reinterpret_cast<int *>(a.scratch + RE_O_CTL)[1] = 1;
    }
}

}  // namespace

void launch_re_rollout(const ReArgs &a, bool quad, hipStream_t s) {
    const long nb = (((a.K + 15) >> 4) + 3) >> 2;                     // four groups of sixteen rollouts per workgroup
    const dim3 grid((unsigned)(nb < 2048 ? nb : 2048));
    const size_t lds = (size_t)a.pb.N * 12 * sizeof(double);
    const bool lq = a.pb.model == 1;                                  // (the LQ family; otherwise the power-law one)
    if (quad && lq) hipLaunchKernelGGL((re_rollout<true, true>), grid, dim3(MC_THREADS), lds, s, a);
    else if (quad) hipLaunchKernelGGL((re_rollout<true, false>), grid, dim3(MC_THREADS), lds, s, a);
    else if (lq) hipLaunchKernelGGL((re_rollout<false, true>), grid, dim3(MC_THREADS), lds, s, a);
    else hipLaunchKernelGGL((re_rollout<false, false>), grid, dim3(MC_THREADS), lds, s, a);
}

void launch_re_level(const ReArgs &a, double rho, hipStream_t s) {
    TrArgs t;
    memset(&t, 0, sizeof(t));
    t.cost = a.margin; t.K = a.K; t.n_alpha = 1; t.alpha[0] = 1.0 - rho; t.scratch = a.scratch + RE_O_TR; t.weights = nullptr;
    launch_policy_tr(t, s);
    hipLaunchKernelGGL(re_level, dim3(1), dim3(64), 0, s, a);
}

void launch_re_adapt(const ReArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(re_pass_a, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, a);
    hipLaunchKernelGGL(re_elite, dim3(RE_SLOTS, (unsigned)((a.pb.N + 1) / 2)), dim3(MC_THREADS), 0, s, a);
    hipLaunchKernelGGL(re_update, dim3(1), dim3(MC_THREADS), 0, s, a);
}

void launch_re_adapt_rng(const ReArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(re_pass_a, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, a);
    const int rows = ((a.pn > 0 && (a.fix & 1)) ? 0 : a.pb.N) + ((a.pn > 0 && !(a.fix & 2)) ? 1 : 0);   // (the caller moves at least one part)
    hipLaunchKernelGGL(re_elite_rng, dim3(RE_SLOTS, (unsigned)rows), dim3(MC_THREADS), 0, s, a);
    hipLaunchKernelGGL(re_update, dim3(1), dim3(MC_THREADS), 0, s, a);
}

void launch_re_final(const ReArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(re_pass_a, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, a);
    hipLaunchKernelGGL(re_pass_b, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, a);
    hipLaunchKernelGGL(re_final, dim3(1), dim3(MC_THREADS), 0, s, a);
}
