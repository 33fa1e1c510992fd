// policy_mc.hip -- Monte-Carlo policy evaluation (rat_policy_evaluate): the statistics of K rollout costs, formed on the device.
//
// The K costs stay in HBM (8 B per rollout); two passes read them and three launches form everything the call returns:
//   mc_pass1   count, DomainError count, min, max, sum                    -> part1[MC_P1][MC_BLOCKS]
//   mc_pass2   mean, Jmax from part1; sum (J - mean)^2 and, per theta,
//              sum d, sum d^2 of d = exp(theta (J - Jmax)) - y_ref          -> part2[MC_P2][MC_BLOCKS]
//   mc_final   both sets of partials -> stats[8], risk[16], risk_se[16]
// The summation order is fixed: lane g of the MC_BLOCKS x MC_THREADS grid sums elements g, g + T, g + 2 T, ... in order, the lanes of a
// workgroup combine in a fixed binary tree through LDS, and the MC_BLOCKS partials combine in the same tree (one lane per partial) at the
// head of the next launch -- the launch boundary is the only synchronisation between workgroups.  No floating-point atomics: two calls
// with the same arguments return the same bits.
//
// exp(theta (J - Jmax)) has every exponent <= 0 (no overflow for any theta).  The sums per theta are taken about
// y_ref = exp(theta (mean - Jmax)): mean(y) = y_ref + sum d / n and (n - 1) var(y) = sum d^2 - (sum d)^2 / n are the sums of y and y^2
// restated so that the subtraction does not cancel as theta sd(J) -> 0 (d is centred to first order).
#include "policy_mc.h"
#include <cstring>

#include "mc_tree.h"

namespace {

__device__ __forceinline__ bool mc_nan(double v) { return v != v; }

// (block_tree and block_tree_n, the fixed trees over the MC_THREADS values of a workgroup, are mc_tree.h's)

struct McHead { double n_ok, n_dom, mn, mx, sum; };

// second level of pass 1's tree: lane i holds the partial of workgroup i
__device__ __forceinline__ McHead reduce_part1(const double *part1, double *sh) {
    const int tid = threadIdx.x;
    McHead r;
    r.n_ok = block_tree<0>(part1[0 * MC_BLOCKS + tid], sh);
    r.n_dom = block_tree<0>(part1[1 * MC_BLOCKS + tid], sh);
    r.mn = block_tree<1>(part1[2 * MC_BLOCKS + tid], sh);
    r.mx = block_tree<2>(part1[3 * MC_BLOCKS + tid], sh);
    r.sum = block_tree<0>(part1[4 * MC_BLOCKS + tid], sh);
    return r;
}

__global__ __launch_bounds__(MC_THREADS) void mc_pass1(McArgs a) {
    __shared__ double sh[MC_THREADS];
    const long T = (long)MC_BLOCKS * MC_THREADS;
    double cnt = 0.0, ndom = 0.0, mn = __builtin_inf(), mx = -__builtin_inf(), sum = 0.0;
    for (long k = (long)blockIdx.x * MC_THREADS + threadIdx.x; k < a.K; k += T) {
        double J = a.cost[k];
        if (a.dom && a.dom[k]) { J = __builtin_nan(""); a.cost[k] = J; }   // (each element belongs to one lane)
        if (mc_nan(J)) ndom += 1.0;
        else {
            cnt += 1.0;
            mn = J < mn ? J : mn;
            mx = J > mx ? J : mx;
            sum += J;
        }
    }
    cnt = block_tree<0>(cnt, sh);
    ndom = block_tree<0>(ndom, sh);
    mn = block_tree<1>(mn, sh);
    mx = block_tree<2>(mx, sh);
    sum = block_tree<0>(sum, sh);
    if (threadIdx.x == 0) {
        double *p = a.scratch;
        p[0 * MC_BLOCKS + blockIdx.x] = cnt; p[1 * MC_BLOCKS + blockIdx.x] = ndom; p[2 * MC_BLOCKS + blockIdx.x] = mn;
        p[3 * MC_BLOCKS + blockIdx.x] = mx; p[4 * MC_BLOCKS + blockIdx.x] = sum;
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_pass2(McArgs a) {
    __shared__ double sh[MC_THREADS];
    const McHead hd = reduce_part1(a.scratch, sh);
    const double mean = hd.sum / hd.n_ok, Jmax = hd.mx;
    double yref[MC_MAX_THETA], sd[MC_MAX_THETA], sd2[MC_MAX_THETA];
#pragma unroll
    for (int i = 0; i < MC_MAX_THETA; ++i) {
        yref[i] = (i < a.n_theta) ? exp(a.theta[i] * (mean - Jmax)) : 0.0;
        sd[i] = 0.0; sd2[i] = 0.0;
    }
    double s2 = 0.0;
    const long T = (long)MC_BLOCKS * MC_THREADS;
    for (long k = (long)blockIdx.x * MC_THREADS + threadIdx.x; k < a.K; k += T) {
        const double J = a.cost[k];
        if (mc_nan(J)) continue;
        const double dj = J - mean;
        s2 += dj * dj;
#pragma unroll
        for (int i = 0; i < MC_MAX_THETA; ++i) {
            if (i < a.n_theta) {
                const double d = exp(a.theta[i] * (J - Jmax)) - yref[i];
                sd[i] += d;
                sd2[i] += d * d;
            }
        }
    }
    double *p = a.scratch + MC_P1 * MC_BLOCKS;
    s2 = block_tree<0>(s2, sh);
    if (threadIdx.x == 0) p[blockIdx.x] = s2;
#pragma unroll
    for (int i = 0; i < MC_MAX_THETA; ++i) {
        if (i < a.n_theta) {                                          // (uniform over the workgroup)
            const double v1 = block_tree<0>(sd[i], sh), v2 = block_tree<0>(sd2[i], sh);
            if (threadIdx.x == 0) { p[(1 + 2 * i) * MC_BLOCKS + blockIdx.x] = v1; p[(2 + 2 * i) * MC_BLOCKS + blockIdx.x] = v2; }
        }
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_final(McArgs a) {
    __shared__ double sh[MC_THREADS];
    const int tid = threadIdx.x;
    const McHead hd = reduce_part1(a.scratch, sh);
    const double *p = a.scratch + MC_P1 * MC_BLOCKS;
    double *out = a.scratch + (MC_P1 + MC_P2) * MC_BLOCKS;
    const double nan = __builtin_nan("");
    const double n = hd.n_ok;
    const bool any = n > 0.0;
    const double mean = any ? hd.sum / n : nan, Jmax = any ? hd.mx : nan;
    const double s2 = block_tree<0>(p[tid], sh);
    const double var = (n >= 2.0) ? s2 / (n - 1.0) : nan;
    const double se_mean = sqrt(var / n);
    if (tid == 0) {
        out[0] = n; out[1] = hd.n_dom; out[2] = mean; out[3] = var; out[4] = any ? hd.mn : nan; out[5] = Jmax; out[6] = se_mean; out[7] = 0.0;
    }
    for (int i = 0; i < a.n_theta; ++i) {
        const double v1 = block_tree<0>(p[(1 + 2 * i) * MC_BLOCKS + tid], sh), v2 = block_tree<0>(p[(2 + 2 * i) * MC_BLOCKS + tid], sh);
        if (tid != 0) continue;
        const double th = a.theta[i];
        double risk = mean, se = se_mean;
        if (th != 0.0) {
            const double yref = exp(th * (mean - Jmax));
            const double ybar = yref + v1 / n;
            double vy = (n >= 2.0) ? (v2 - v1 * v1 / n) / (n - 1.0) : nan;
            if (vy < 0.0) vy = 0.0;
            risk = any ? Jmax + log(ybar) / th : nan;
            se = sqrt(vy) / (ybar * th * sqrt(n));                    // delta method: sd(y) / (mean(y) theta sqrt(n))
        }
        out[8 + i] = risk;
        out[8 + MC_MAX_THETA + i] = se;
    }
}


// ---- rat_policy_worst_case: sup { E_p[J] : KL(p || q) <= d } over the K costs ----------------------------------------------------------
// The dual is one-dimensional: with y_k = exp(theta (J_k - Jmax)), Z = mean y, m = sum y J / sum y and KL(theta) = theta (m - Jmax) - log Z
// (non-decreasing from KL(0) = 0 to log(n / n_max)), the bound is Jmax + (log Z + d) / theta at the theta* where KL(theta*) = d.  The search
// for theta* runs on the device in a fixed number of launches ("Worst-case cost within the KL ball"):
//   mc_pass1    as for rat_policy_evaluate                                               -> part1
//   wc_var      sum (J - mean)^2 and n_max = #{J == Jmax}                                -> var
//   wc_search   x WC_PASSES.  Pass p places WC_NPT thetas per bound -- pass 0 on the geometric grid theta_0 4^(j - 7) around the Gaussian
//               answer theta_0 = sqrt(2 d) / sd(J), later passes at lo + (hi - lo) (j + 1) / 17 -- and sums, per theta,
//               A = sum (y - y_ref) and B = sum y (J - c) over the costs.  Its head first reduces the previous pass's partials, forms
//               KL at that pass's thetas and picks the sub-interval that contains d: the bracket lives in the scratch, nothing is read
//               back.  Brackets and partials alternate between two sets, so that a workgroup that is ahead never overwrites what another
//               still reads.
//   wc_final    theta* = the middle of the last bracket; per row (every bound, then every given theta) A, sum (y - y_ref)^2, B,
//               sum y (J - c)^2 and sum y (J - Jmax)^2                                                          -> final partials, row info
//   wc_rows     second level of those sums; writes the rows
//   wc_weights  y_k / sum y of the first row, elementwise
// Every sum runs in mc_pass1's order (lane g sums elements g, g + T, ...; the LDS tree; the second level at the head of the next launch).
// Centring: c = mean and y_ref = exp(theta (mean - Jmax)) while theta (Jmax - mean) <= WC_CENTRE_MAX -- then, with y - y_ref formed as
// y_ref expm1(theta (J - mean)), KL = theta B / sum y - log1p(A / (n y_ref)) holds its digits as theta sd(J) -> 0, where theta (m - Jmax)
// and log Z are each far larger than their difference -- and c = Jmax, y_ref = 0 beyond (y_ref would underflow; KL is of order one there).

struct WcHead { double n, mean, Jmax, s2, nmax, sd, klmax, kind; };

// what every launch after wc_var knows about the sample (kind: WC_ST_SEARCH unless the sample is empty or holds an infinity)
__device__ __forceinline__ WcHead wc_head(const double *scr, double *sh) {
    const McHead hd = reduce_part1(scr + WC_O_P1, sh);
    double v[2] = {scr[WC_O_PV + threadIdx.x], scr[WC_O_PV + MC_BLOCKS + threadIdx.x]};
    block_tree_n<2>(v, sh);
    WcHead r;
    r.n = hd.n_ok; r.mean = hd.sum / hd.n_ok; r.Jmax = hd.mx; r.s2 = v[0]; r.nmax = v[1];
    r.sd = sqrt(r.s2 / r.n);
    r.klmax = log(r.n / r.nmax);
    r.kind = !(hd.n_ok > 0.0) ? WC_ST_EMPTY : !(hd.mn > -__builtin_inf() && hd.mx < __builtin_inf()) ? WC_ST_NONFINITE : WC_ST_SEARCH;
    return r;
}

__device__ __forceinline__ double wc_theta0(const WcHead &h, double d) { return sqrt(2.0 * d) / h.sd; }

__device__ __forceinline__ double wc_bound_state(const WcHead &h, double d) {
    if (h.kind != WC_ST_SEARCH) return h.kind;
    if (d == 0.0) return WC_ST_ZERO;                                  // (decided before the saturation rule: all costs equal, d = 0)
    if (d >= h.klmax) return WC_ST_SAT;
    const double t0 = wc_theta0(h, d);
    return (t0 > 0.0 && t0 < __builtin_inf()) ? WC_ST_SEARCH : WC_ST_SAT;
}

// theta j of search pass `pass` in the bracket [lo, hi]
__device__ __forceinline__ double wc_grid(int pass, int j, double lo, double hi, double theta0) {
    const double t = (pass == 0) ? theta0 * ldexp(1.0, 2 * (j - WC_GEO_BELOW)) : lo + (hi - lo) * ((double)(j + 1) / (double)(WC_NPT + 1));
    return t < WC_THETA_CAP ? t : WC_THETA_CAP;
}

// y_ref of a theta: exp(theta (mean - Jmax)) where the sums are centred about the mean, 0 where they are taken about Jmax
__device__ __forceinline__ double wc_yref(double th, const WcHead &h) {
    return (th * (h.Jmax - h.mean) <= WC_CENTRE_MAX) ? exp(th * (h.mean - h.Jmax)) : 0.0;
}

// one cost's terms at one theta: dd = y - y_ref and yc = y (J - c), from dm = J - mean and dx = J - Jmax.  Centred, y - y_ref is formed as
// y_ref expm1(theta dm), exact to its own last digits: exp(theta dx) - y_ref would carry y's rounding, 1e-16 absolute against a sum of
// order kl_bound per cost
__device__ __forceinline__ void wc_term(double th, double yref, bool centred, double dm, double dx, double &dd, double &yc) {
    if (centred) {
        dd = yref * expm1(th * dm);
        yc = (yref + dd) * dm;
    } else {
        dd = exp(th * dx);
        yc = dd * dx;
    }
}

// log Z - theta (c - Jmax) from A = sum (y - y_ref)
__device__ __forceinline__ double wc_lz(double yref, double A, double n) { return (yref != 0.0) ? log1p(A / (n * yref)) : log(A / n); }
__device__ __forceinline__ double wc_sumy(double yref, double A, double n) { return (yref != 0.0) ? n * yref + A : A; }
__device__ __forceinline__ double wc_kl(double th, double yref, double A, double B, double n) {
    return th * (B / wc_sumy(yref, A, n)) - wc_lz(yref, A, n);
}

// the bracket and state of bound b as search pass `pass` finds them: pass 0 decides the state from the sample alone, a later pass (and
// wc_final, as pass WC_PASSES) reduces the partials of pass - 1 and narrows.  Every lane of every workgroup computes the same values.
__device__ __forceinline__ void wc_bracket(const WcArgs &a, const WcHead &h, int b, int pass, double *sh, double &lo, double &hi, double &st) {
    const double d = a.bound[b];
    if (pass == 0) { lo = 0.0; hi = 0.0; st = wc_bound_state(h, d); return; }
    const double *bi = a.scratch + WC_O_BRK + ((pass & 1) * WC_MAX_BOUND + b) * 4;
    lo = bi[0]; hi = bi[1]; st = bi[2];
    if (st != WC_ST_SEARCH) return;
    const double *ps = a.scratch + WC_O_PS + (size_t)((pass - 1) & 1) * WC_PS_SET + (size_t)b * 2 * WC_NPT * MC_BLOCKS;
    const double theta0 = wc_theta0(h, d);
    double prev = lo, nlo = lo, nhi = hi;
    bool found = false;
    for (int q0 = 0; q0 < WC_NPT; q0 += 4) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = ps[(2 * q0 + q) * MC_BLOCKS + threadIdx.x];
        block_tree_n<8>(v, sh);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const double t = wc_grid(pass - 1, q0 + jj, lo, hi, theta0);
            const double kl = wc_kl(t, wc_yref(t, h), v[2 * jj], v[2 * jj + 1], h.n);
            if (!found) {
                if (kl >= d) { found = true; nlo = prev; nhi = t; }
                prev = t;
            }
        }
    }
    if (!found) {
        if (pass == 1) st = WC_ST_SAT;                                // KL(theta_top) < d
        else nlo = prev;                                              // (hi had KL >= d when it was chosen)
    }
    lo = nlo; hi = nhi;
}

__global__ __launch_bounds__(MC_THREADS) void wc_var(WcArgs a) {
    __shared__ double sh[2 * MC_THREADS];
    const McHead hd = reduce_part1(a.scratch + WC_O_P1, sh);
    const double mean = hd.sum / hd.n_ok, Jmax = hd.mx;
    double v[2] = {0.0, 0.0};
    const long T = (long)MC_BLOCKS * MC_THREADS;
    for (long k = (long)blockIdx.x * MC_THREADS + threadIdx.x; k < a.K; k += T) {
        const double J = a.cost[k];
        if (mc_nan(J)) continue;
        const double dj = J - mean;
        v[0] += dj * dj;
        v[1] += (J == Jmax) ? 1.0 : 0.0;
    }
    block_tree_n<2>(v, sh);
    if (threadIdx.x == 0) { a.scratch[WC_O_PV + blockIdx.x] = v[0]; a.scratch[WC_O_PV + MC_BLOCKS + blockIdx.x] = v[1]; }
}

__global__ __launch_bounds__(MC_THREADS) void wc_search(WcArgs a) {
    __shared__ double sh[8 * MC_THREADS];
    const WcHead h = wc_head(a.scratch, sh);
    const long T = (long)MC_BLOCKS * MC_THREADS;
    for (int b = 0; b < a.n_bound; ++b) {                             // (bounds in turn: 16 thetas x 2 sums is what a lane holds)
        double lo, hi, st;
        wc_bracket(a, h, b, a.pass, sh, lo, hi, st);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            double *bo = a.scratch + WC_O_BRK + (((a.pass + 1) & 1) * WC_MAX_BOUND + b) * 4;
            bo[0] = lo; bo[1] = hi; bo[2] = st; bo[3] = 0.0;
        }
        if (st != WC_ST_SEARCH) continue;                             // (uniform over the grid)
        const double theta0 = wc_theta0(h, a.bound[b]);
        double th[WC_NPT], yr[WC_NPT], A[WC_NPT], B[WC_NPT];
        bool cen[WC_NPT];
#pragma unroll
        for (int j = 0; j < WC_NPT; ++j) {
            th[j] = wc_grid(a.pass, j, lo, hi, theta0);
            yr[j] = wc_yref(th[j], h);
            cen[j] = __builtin_amdgcn_readfirstlane((int)(yr[j] != 0.0)) != 0;   // (the same in every lane: a scalar branch)
            A[j] = 0.0; B[j] = 0.0;
        }
        for (long k = (long)blockIdx.x * MC_THREADS + threadIdx.x; k < a.K; k += T) {
            const double J = a.cost[k];
            if (mc_nan(J)) continue;
            const double dm = J - h.mean, dx = J - h.Jmax;
#pragma unroll
            for (int j = 0; j < WC_NPT; ++j) {
                double dd, yc;
                wc_term(th[j], yr[j], cen[j], dm, dx, dd, yc);
                A[j] += dd;
                B[j] += yc;
            }
        }
        double *ps = a.scratch + WC_O_PS + (size_t)(a.pass & 1) * WC_PS_SET + (size_t)b * 2 * WC_NPT * MC_BLOCKS;
#pragma unroll
        for (int q0 = 0; q0 < WC_NPT; q0 += 4) {
            double v[8];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) { v[2 * jj] = A[q0 + jj]; v[2 * jj + 1] = B[q0 + jj]; }
            block_tree_n<8>(v, sh);
            if (threadIdx.x == 0) {
#pragma unroll
                for (int q = 0; q < 8; ++q) ps[(2 * q0 + q) * MC_BLOCKS + blockIdx.x] = v[q];
            }
        }
    }
}

__global__ __launch_bounds__(MC_THREADS) void wc_final(WcArgs a) {
    __shared__ double sh[8 * MC_THREADS];
    __shared__ double s_th[WC_MAX_ROWS], s_st[WC_MAX_ROWS];
    const WcHead h = wc_head(a.scratch, sh);
    const int nrows = a.n_bound + a.n_theta;
    for (int b = 0; b < a.n_bound; ++b) {
        double lo, hi, st;
        wc_bracket(a, h, b, WC_PASSES, sh, lo, hi, st);
        if (threadIdx.x == 0) { s_th[b] = (st == WC_ST_SEARCH) ? 0.5 * (lo + hi) : 0.0; s_st[b] = st; }
    }
    if (threadIdx.x < a.n_theta) {
        const double t = a.theta[threadIdx.x];
        s_th[a.n_bound + threadIdx.x] = t;
        s_st[a.n_bound + threadIdx.x] = (h.kind != WC_ST_SEARCH) ? h.kind : (t == 0.0 ? WC_ST_ZERO : WC_ST_SEARCH);
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x < nrows) {
        a.scratch[WC_O_INFO + 2 * threadIdx.x] = s_th[threadIdx.x];
        a.scratch[WC_O_INFO + 2 * threadIdx.x + 1] = s_st[threadIdx.x];
    }
    const long T = (long)MC_BLOCKS * MC_THREADS;
    for (int r0 = 0; r0 < nrows; r0 += WC_FROWS) {
        const int ns = (nrows - r0 < WC_FROWS) ? nrows - r0 : WC_FROWS;
        double th[WC_FROWS], yr[WC_FROWS], acc[WC_FROWS][WC_NFIN];
        bool cen[WC_FROWS], live[WC_FROWS];                          // (live: the row needs sums; the others are written from the sample alone)
#pragma unroll
        for (int s = 0; s < WC_FROWS; ++s) {
            live[s] = __builtin_amdgcn_readfirstlane((int)(s < ns && s_st[r0 + s] == WC_ST_SEARCH)) != 0;
            th[s] = live[s] ? s_th[r0 + s] : 0.0;
            yr[s] = wc_yref(th[s], h);
            cen[s] = __builtin_amdgcn_readfirstlane((int)(yr[s] != 0.0)) != 0;
            acc[s][0] = acc[s][1] = acc[s][2] = acc[s][3] = acc[s][4] = 0.0;
        }
        for (long k = (long)blockIdx.x * MC_THREADS + threadIdx.x; k < a.K; k += T) {
            const double J = a.cost[k];
            if (mc_nan(J)) continue;
            const double dm = J - h.mean, dx = J - h.Jmax;
#pragma unroll
            for (int s = 0; s < WC_FROWS; ++s) {
                if (live[s]) {                                        // (uniform)
                    double dd, yc;
                    wc_term(th[s], yr[s], cen[s], dm, dx, dd, yc);
                    acc[s][0] += dd;
                    acc[s][1] += dd * dd;
                    acc[s][2] += yc;
                    acc[s][3] += yc * (cen[s] ? dm : dx);
                    acc[s][4] += (cen[s] ? yr[s] + dd : dd) * dx * dx;
                }
            }
        }
#pragma unroll
        for (int s = 0; s < WC_FROWS; ++s) {
            if (s < ns) {
                double v[WC_NFIN] = {acc[s][0], acc[s][1], acc[s][2], acc[s][3], acc[s][4]};
                block_tree_n<WC_NFIN>(v, sh);
                if (threadIdx.x == 0) {
#pragma unroll
                    for (int q = 0; q < WC_NFIN; ++q) a.scratch[WC_O_PF + ((r0 + s) * WC_NFIN + q) * MC_BLOCKS + blockIdx.x] = v[q];
                }
            }
        }
    }
}

__global__ __launch_bounds__(MC_THREADS) void wc_rows(WcArgs a) {
    __shared__ double sh[WC_NFIN * MC_THREADS];
    const WcHead h = wc_head(a.scratch, sh);
    const int nrows = a.n_bound + a.n_theta;
    const double nan = __builtin_nan(""), n = h.n;
    const double se_mean = (n >= 2.0) ? sqrt(h.s2 / (n - 1.0) / n) : nan;
    for (int r = 0; r < nrows; ++r) {
        double v[WC_NFIN];
#pragma unroll
        for (int q = 0; q < WC_NFIN; ++q) v[q] = a.scratch[WC_O_PF + (r * WC_NFIN + q) * MC_BLOCKS + threadIdx.x];
        block_tree_n<WC_NFIN>(v, sh);
        if (threadIdx.x != 0) continue;
        const double th = a.scratch[WC_O_INFO + 2 * r], st = a.scratch[WC_O_INFO + 2 * r + 1];
        double o[WC_NSTAT], sumy = nan;
        if (st == WC_ST_EMPTY || st == WC_ST_NONFINITE) {
            for (int q = 0; q < 7; ++q) o[q] = nan;
            o[7] = (st == WC_ST_EMPTY) ? 2.0 : 3.0;
        } else if (st == WC_ST_ZERO) {
            o[0] = 0.0; o[1] = 0.0; o[2] = h.mean; o[3] = se_mean; o[4] = h.mean; o[5] = h.s2 / n; o[6] = n; o[7] = 0.0;
            sumy = n;
        } else if (st == WC_ST_SAT) {
            o[0] = __builtin_inf(); o[1] = h.klmax; o[2] = h.Jmax; o[3] = nan; o[4] = h.Jmax; o[5] = 0.0; o[6] = h.nmax; o[7] = 1.0;
        } else {
            const double A = v[0], A2 = v[1], B = v[2], B2 = v[3], B2x = v[4];
            const double yr = wc_yref(th, h), c = (yr != 0.0) ? h.mean : h.Jmax;
            sumy = wc_sumy(yr, A, n);
            const double lz = wc_lz(yr, A, n), mc = B / sumy, kl = th * mc - lz;
            const double d = (r < a.n_bound) ? a.bound[r] : kl;
            // the tilted variance about the nearer of the two centres: E (J - c)^2 - (m - c)^2 cancels where m is far from c
            const double mx = (yr != 0.0) ? mc + (h.mean - h.Jmax) : mc;
            double tvar = (fabs(mc) <= fabs(mx)) ? B2 / sumy - mc * mc : B2x / sumy - mx * mx;
            if (tvar < 0.0) tvar = 0.0;
            double vy = (n >= 2.0) ? (A2 - A * A / n) / (n - 1.0) : nan;
            if (vy < 0.0) vy = 0.0;
            o[0] = th; o[1] = kl; o[2] = c + (lz + d) / th;
            o[3] = sqrt(vy) / ((sumy / n) * th * sqrt(n));            // delta method, as mc_final's risk_se
            o[4] = c + mc; o[5] = tvar;
            o[6] = sumy * sumy / (A2 + 2.0 * yr * A + n * yr * yr);    // sum y^2 = sum (y - y_ref)^2 + 2 y_ref A + n y_ref^2
            o[7] = 0.0;
        }
        for (int q = 0; q < WC_NSTAT; ++q) a.scratch[WC_O_ROWS + r * WC_NSTAT + q] = o[q];
        if (r == 0) {
            double *x = a.scratch + WC_O_AUX;
            x[0] = th; x[1] = sumy; x[2] = h.Jmax; x[3] = st; x[4] = h.nmax; x[5] = n; x[6] = 0.0; x[7] = 0.0;
        }
    }
}

__global__ __launch_bounds__(MC_THREADS) void wc_weights(WcArgs a) {
    const double *x = a.scratch + WC_O_AUX;
    const double th = x[0], sumy = x[1], Jmax = x[2], st = x[3], nmax = x[4];
    const long T = (long)gridDim.x * MC_THREADS;
    for (long k = (long)blockIdx.x * MC_THREADS + threadIdx.x; k < a.K; k += T) {
        const double J = a.cost[k];
        double w;
        if (mc_nan(J)) w = 0.0;
        else if (st == WC_ST_SAT) w = (J == Jmax) ? 1.0 / nmax : 0.0;
        else if (st == WC_ST_SEARCH || st == WC_ST_ZERO) w = exp(th * (J - Jmax)) / sumy;
        else w = __builtin_nan("");
        a.weights[k] = w;
    }
}

// ---- rat_policy_tail_risk: the alpha-quantile v (value at risk) and CVaR = v + sum (J - v)^+ / (n - a) of the K costs ------------------------
// v is the k-th smallest OK cost, k = clamp(ceil(a), 1, n), a = n alpha: a radix select over the costs' keys (tr_key: the bit pattern made
// monotone), TR_BITS bits a pass, every level of the call at once:
//   mc_pass1    as for rat_policy_evaluate: n, min, max                                   -> part1
//   tr_select   x TR_PASSES.  The head of pass p forms every level's state -- the p digits fixed so far and the rank left among the keys
//               that carry them -- from the state and the histogram of pass p - 1: it walks the level's 256 bins to the one where the
//               running count reaches the rank.  The sweep then counts, per distinct prefix, the digit p of the keys that carry it:
//               levels that share a prefix share a histogram (`rep`, the lowest such level), distinct prefixes of one length exclude each
//               other, so a cost makes at most one LDS add a pass.  Histograms are u32 in LDS, flushed with integer atomics into the
//               pass's own zeroed set: integer sums are exact, the order cannot change a bit.  Digits on which the keys of min and max
//               agree are shared by every key: those passes sweep nothing (costs of one policy share sign and exponent; all costs equal
//               need no sweep at all).
//   tr_sums     the head fixes the last digit: the prefix is v's key.  Per level P1 = sum (J - v)^+, P2 = sum ((J - v)^+)^2, c_gt = #{J > v},
//               c_eq = #{J == v} in mc_pass1's order, TR_SROWS levels a sweep                                  -> partials
//   tr_rows     second level of those sums; writes the rows
//   tr_weights  the tail distribution of the first level, elementwise
// A level's state, histogram walk and sums never read another level's: a row's bits do not depend on its company.
typedef unsigned long long tr_u64;

// ascending key order is ascending value order; -0.0 counts as +0.0
__device__ __forceinline__ tr_u64 tr_key(double J) {
    const tr_u64 b = (J == 0.0) ? 0ull : (tr_u64)__double_as_longlong(J);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double tr_value(tr_u64 key) { return __longlong_as_double((long long)((key >> 63) ? (key ^ (1ull << 63)) : ~key)); }

struct TrHead { double n, mx; tr_u64 kmin; int d0; bool live; double flag; };

// what every launch knows about the sample; d0: the first digit on which the keys of min and max differ (TR_PASSES: all costs equal)
__device__ __forceinline__ TrHead tr_head(const double *scr, double *sh) {
    const McHead hd = reduce_part1(scr + TR_O_P1, sh);
    TrHead r;
    r.n = hd.n_ok; r.mx = hd.mx;
    r.flag = !(hd.n_ok > 0.0) ? 2.0 : !(hd.mn > -__builtin_inf() && hd.mx < __builtin_inf()) ? 3.0 : 0.0;
    r.live = r.flag == 0.0;
    r.kmin = tr_key(hd.mn);
    const tr_u64 x = r.kmin ^ tr_key(hd.mx);
    r.d0 = (x == 0) ? TR_PASSES : (__clzll((long long)x) / TR_BITS);
    return r;
}

// a = n alpha as one rounded product: kept out of the subtractions that follow it (n - a, k - a), which the compiler would otherwise fuse
// with it -- __dmul_rn is a plain product to this compiler and is fused like one
__device__ __forceinline__ double tr_prod(double n, double alpha) {
#pragma clang fp contract(off)
    return n * alpha;
}

// k = clamp(ceil(a), 1, n)
__device__ __forceinline__ double tr_rank(double n, double av) {
    double k = ceil(av);
    k = k < 1.0 ? 1.0 : k;
    return k > n ? n : k;
}

__device__ __forceinline__ tr_u64 *tr_gpfx(double *scr) { return (tr_u64 *)(scr + TR_O_STATE); }
__device__ __forceinline__ tr_u64 *tr_grr(double *scr) { return tr_gpfx(scr) + (TR_PASSES + 1) * TR_MAX_ALPHA; }

// the state of every level before digit pass p (p = TR_PASSES: after the last), in LDS; workgroup 0 also stores it for the next launch.
// Lane (l, c) = (tid >> 4, tid & 15) sums bins 16 c .. 16 c + 15 of level l's histogram of pass p - 1; the lane whose chunk holds the rank
// walks its 16 bins.  s_cs is [MC_THREADS].  Every workgroup computes the same values.
__device__ __forceinline__ void tr_state(const TrArgs &a, const TrHead &h, int p, tr_u64 *s_pfx, unsigned *s_rank, int *s_rep, unsigned *s_cs) {
    const int tid = threadIdx.x, l = tid >> 4, c = tid & 15;
    tr_u64 *g_pfx = tr_gpfx(a.scratch), *g_rr = tr_grr(a.scratch);
    __syncthreads();
    if (p == 0) {
        if (tid < a.n_alpha) { s_pfx[tid] = 0; s_rank[tid] = (unsigned)tr_rank(h.n, tr_prod(h.n, a.alpha[tid])); }
    } else {
        const bool on = l < a.n_alpha, walk = (p - 1) >= h.d0;           // (walk is uniform over the grid)
        tr_u64 pfx = 0;
        unsigned rank = 0, cs = 0;
        const unsigned *hist = nullptr;
        if (on) {
            pfx = g_pfx[(p - 1) * TR_MAX_ALPHA + l];
            const tr_u64 rr = g_rr[(p - 1) * TR_MAX_ALPHA + l];
            rank = (unsigned)(rr & 0xffffffffull);
            if (walk) {
                hist = (const unsigned *)(a.scratch + TR_O_HIST) + ((size_t)(p - 1) * TR_MAX_ALPHA + (size_t)(rr >> 32)) * TR_BINS + 16 * c;
                for (int j = 0; j < 16; ++j) cs += hist[j];
            }
        }
        s_cs[tid] = cs;
        if (on && c == 0) {                                           // a pass that swept nothing: the digit every key shares
            s_pfx[l] = (pfx << TR_BITS) | (walk ? 0ull : ((h.kmin >> (64 - TR_BITS * p)) & (tr_u64)(TR_BINS - 1)));
            s_rank[l] = rank;
        }
        __syncthreads();
        if (on && walk) {
            unsigned run = 0;
            for (int j = 0; j < c; ++j) run += s_cs[l * 16 + j];
            if (run < rank && rank <= run + cs) {                     // (one lane of the level: the counts below the prefix reach the rank)
                int dg = 16 * c + 15;
                for (int j = 0; j < 16; ++j) {
                    const unsigned cnt = hist[j];
                    if (run + cnt >= rank) { dg = 16 * c + j; break; }
                    run += cnt;
                }
                s_pfx[l] = (pfx << TR_BITS) | (tr_u64)dg;
                s_rank[l] = rank - run;
            }
        }
    }
    __syncthreads();
    if (tid < a.n_alpha) {
        int rep = tid;
        for (int j = tid - 1; j >= 0; --j) if (s_pfx[j] == s_pfx[tid]) rep = j;
        s_rep[tid] = rep;
        if (blockIdx.x == 0) {
            g_pfx[p * TR_MAX_ALPHA + tid] = s_pfx[tid];
            g_rr[p * TR_MAX_ALPHA + tid] = (tr_u64)s_rank[tid] | ((tr_u64)rep << 32);
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(MC_THREADS) void tr_select(TrArgs a) {
    __shared__ double sh[MC_THREADS];
    __shared__ unsigned s_hist[TR_MAX_ALPHA * TR_BINS], s_cs[MC_THREADS], s_rank[TR_MAX_ALPHA];
    __shared__ tr_u64 s_pfx[TR_MAX_ALPHA];
    __shared__ int s_rep[TR_MAX_ALPHA];
    const TrHead h = tr_head(a.scratch, sh);
    if (!h.live) return;                                              // (uniform over the grid, like every return below)
    tr_state(a, h, a.pass, s_pfx, s_rank, s_rep, s_cs);
    if (a.pass < h.d0) return;                                        // every key carries the same digit here
    const int tid = threadIdx.x;
    for (int i = tid; i < TR_MAX_ALPHA * TR_BINS; i += MC_THREADS) s_hist[i] = 0u;
    tr_u64 pf[TR_MAX_ALPHA];
    bool act[TR_MAX_ALPHA];                                          // the level counts for its prefix (the same in every lane: scalar)
#pragma unroll
    for (int l = 0; l < TR_MAX_ALPHA; ++l) {
        act[l] = __builtin_amdgcn_readfirstlane((int)(l < a.n_alpha && s_rep[l] == l)) != 0;
        const tr_u64 v = act[l] ? s_pfx[l] : 0ull;
        pf[l] = ((tr_u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32)) << 32) |
                (tr_u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v & 0xffffffffull));
    }
    __syncthreads();
    const int sd = 64 - TR_BITS * (a.pass + 1);
    const long T = (long)MC_BLOCKS * MC_THREADS;
    for (long k0 = (long)blockIdx.x * MC_THREADS + tid; k0 < a.K; k0 += 4 * T) {      // four loads in flight; a count has no order
        double J[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const long k = k0 + u * T; J[u] = (k < a.K) ? a.cost[k] : __builtin_nan(""); }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (mc_nan(J[u])) continue;
            const tr_u64 key = tr_key(J[u]);
            const tr_u64 hi = (a.pass == 0) ? 0ull : (key >> (sd + TR_BITS));
            int slot = -1;
#pragma unroll
            for (int l = 0; l < TR_MAX_ALPHA; ++l) if (act[l] && hi == pf[l]) slot = l;
            if (slot >= 0) atomicAdd(&s_hist[slot * TR_BINS + (int)((key >> sd) & (tr_u64)(TR_BINS - 1))], 1u);
        }
    }
    __syncthreads();
    unsigned *g_hist = (unsigned *)(a.scratch + TR_O_HIST) + (size_t)a.pass * TR_MAX_ALPHA * TR_BINS;
    for (int i = tid; i < a.n_alpha * TR_BINS; i += MC_THREADS) {
        const unsigned cnt = s_hist[i];
        if (cnt) atomicAdd(&g_hist[i], cnt);
    }
}

__global__ __launch_bounds__(MC_THREADS) void tr_sums(TrArgs a) {
    __shared__ double sh[TR_NSUM * MC_THREADS];
    __shared__ unsigned s_cs[MC_THREADS], s_rank[TR_MAX_ALPHA];
    __shared__ tr_u64 s_pfx[TR_MAX_ALPHA];
    __shared__ int s_rep[TR_MAX_ALPHA];
    const TrHead h = tr_head(a.scratch, sh);
    if (!h.live) return;
    tr_state(a, h, TR_PASSES, s_pfx, s_rank, s_rep, s_cs);
    const long T = (long)MC_BLOCKS * MC_THREADS;
    for (int r0 = 0; r0 < a.n_alpha; r0 += TR_SROWS) {
        const int ns = (a.n_alpha - r0 < TR_SROWS) ? a.n_alpha - r0 : TR_SROWS;
        double v[TR_SROWS], acc[TR_SROWS][TR_NSUM];
#pragma unroll
        for (int s = 0; s < TR_SROWS; ++s) {
            v[s] = (s < ns) ? tr_value(s_pfx[r0 + s]) : 0.0;
            acc[s][0] = acc[s][1] = acc[s][2] = acc[s][3] = 0.0;
        }
        for (long k = (long)blockIdx.x * MC_THREADS + threadIdx.x; k < a.K; k += T) {
            const double J = a.cost[k];
            if (mc_nan(J)) continue;
#pragma unroll
            for (int s = 0; s < TR_SROWS; ++s) {
                if (s < ns) {                                         // (uniform)
                    const bool gt = J > v[s];
                    const double d = gt ? J - v[s] : 0.0;             // about v: nothing cancels
                    acc[s][0] += d;
                    acc[s][1] += d * d;
                    acc[s][2] += gt ? 1.0 : 0.0;
                    acc[s][3] += (J == v[s]) ? 1.0 : 0.0;
                }
            }
        }
#pragma unroll
        for (int s = 0; s < TR_SROWS; ++s) {
            if (s < ns) {
                double q[TR_NSUM] = {acc[s][0], acc[s][1], acc[s][2], acc[s][3]};
                block_tree_n<TR_NSUM>(q, sh);
                if (threadIdx.x == 0) {
#pragma unroll
                    for (int i = 0; i < TR_NSUM; ++i) a.scratch[TR_O_PS + ((r0 + s) * TR_NSUM + i) * MC_BLOCKS + blockIdx.x] = q[i];
                }
            }
        }
    }
}

__global__ __launch_bounds__(MC_THREADS) void tr_rows(TrArgs a) {
    __shared__ double sh[TR_NSUM * MC_THREADS];
    const TrHead h = tr_head(a.scratch, sh);
    const double nan = __builtin_nan(""), n = h.n;
    for (int r = 0; r < a.n_alpha; ++r) {
        double q[TR_NSUM] = {0.0, 0.0, 0.0, 0.0};
        if (h.live) {
#pragma unroll
            for (int i = 0; i < TR_NSUM; ++i) q[i] = a.scratch[TR_O_PS + (r * TR_NSUM + i) * MC_BLOCKS + threadIdx.x];
        }
        block_tree_n<TR_NSUM>(q, sh);
        if (threadIdx.x != 0) continue;
        double o[TR_NSTAT], w_gt = nan, w_eq = nan, val = nan;
        o[0] = a.alpha[r];
        if (!h.live) {
            for (int i = 1; i < 7; ++i) o[i] = nan;
            o[7] = h.flag;
        } else {
            const double P1 = q[0], P2 = q[1], cgt = q[2], ceq = q[3];
            const double av = tr_prod(n, a.alpha[r]), tail = n - av, k = tr_rank(n, av);
            val = tr_value(tr_gpfx(a.scratch)[TR_PASSES * TR_MAX_ALPHA + r]);
            if (tail < 1.0) {                                         // thinner than one rollout: k = n, v = Jmax, c_eq = n_max
                o[1] = val; o[2] = val; o[3] = nan; o[4] = tail; o[5] = ceq; o[6] = log(n / ceq); o[7] = 1.0;
                w_gt = 0.0; w_eq = 1.0 / ceq;
            } else {
                const double frac = k - av, ra = (n - k - cgt) + frac, wv = ra / ceq;   // ra: the mass, in rollouts, left on the atom at v
                double s2 = P2 - P1 * P1 / n;
                if (s2 < 0.0) s2 = 0.0;
                o[1] = val;
                o[2] = val + P1 / tail;                               // Rockafellar-Uryasev: ties and the fractional atom need no special case
                o[3] = (n >= 2.0) ? sqrt(n * s2 / (n - 1.0)) / tail : nan;
                o[4] = tail;
                o[5] = tail * tail / (cgt + ceq * wv * wv);
                o[6] = (cgt * log(n / tail) + (ra > 0.0 ? ra * log(n * wv / tail) : 0.0)) / tail;
                o[7] = 0.0;
                w_gt = 1.0 / tail; w_eq = wv / tail;
            }
        }
        for (int i = 0; i < TR_NSTAT; ++i) a.scratch[TR_O_ROWS + r * TR_NSTAT + i] = o[i];
        if (r == 0) {
            double *x = a.scratch + TR_O_AUX;
            x[0] = val; x[1] = w_gt; x[2] = w_eq; x[3] = h.flag; x[4] = 0.0; x[5] = 0.0; x[6] = 0.0; x[7] = 0.0;
        }
    }
}

__global__ __launch_bounds__(MC_THREADS) void tr_weights(TrArgs a) {
    const double *x = a.scratch + TR_O_AUX;
    const double v = x[0], w_gt = x[1], w_eq = x[2], flag = x[3];
    const long T = (long)gridDim.x * MC_THREADS;
    for (long k = (long)blockIdx.x * MC_THREADS + threadIdx.x; k < a.K; k += T) {
        const double J = a.cost[k];
        double w;
        if (mc_nan(J)) w = 0.0;
        else if (flag != 0.0) w = __builtin_nan("");
        else w = (J > v) ? w_gt : (J == v) ? w_eq : 0.0;
        a.weights[k] = w;
    }
}

// ---- the moment replays: weighted moments of what the replayed rollouts held, one schedule for three payloads ------------------------------
// rat_policy_worst_case_trajectory / _disturbance / _params and their rat_policy_tail_* siblings.  One MFMA per group of four rollouts,
// row and product: lane (i = lane & 15, kk = lane >> 4) holds component i of a deviation D of rollout 4 g + kk, so A = y D is
// [16 components][4 rollouts], B = D' is [4 rollouts][16 components] and C += A B is the group's sum y D D'.  Sums per lane (S1 = sum y D)
// and per rollout lane kk (S0 = sum y, sum y^2) ride along; the four rollouts of a lane column are summed at the end.  Order: wavefront w of
// slot s takes the groups s * WT_WAVES + w, + WT_SLOTS * WT_WAVES, ... in order; the wavefronts of a workgroup (and the four rollout
// lanes) are summed in index order through LDS into the workgroup's partial, chunk after chunk in stream order; *_final sums the slots in
// index order.  No floating-point atomics (the replay check counts with an integer one: a count does not depend on the order).
//
// moments_body is that schedule, once.  A payload F says what a lane holds and which products a row forms:
//   TILES, VECS, SCALARS   C tiles per row, sums per lane, sums per rollout lane (scalars 0 and 1 are S0 and sum y^2, which moments_body
//                          adds itself); the LDS per wavefront and row is their tiles | vectors | scalars
//   o_tile, o_vec, o_scalar   where each lands in the partial (the WT_O_* / WD_O_* / WP_O_* of policy_mc.h)
//   batch()                the row batch of the workgroup: the grid axis behind the step, or, for the one-step parameters, the step's own
//   part(row, slot)        the partial of (row, the workgroup's step, slot)
//   load(q, ok, J)         the lane's deviations of rollout q (ok: it has a cost, J; otherwise exact zeros: selected, not multiplied --
//                          the data may hold NaN)
//   row(c, v, s, y, has, d)   one row's MFMAs and sums: has false selects the rollout out of both operands
// Everything is resolved at compile time and inlined: the kernels below are the instantiations.
typedef double wt_d4 __attribute__((ext_vector_type(4)));
#define WD_NONE 0x7fffffff

__device__ __forceinline__ wt_d4 wt_mfma(double a, double b, wt_d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// With TAIL (the liveness schedule of the tail calls, policy_mc.h) the wavefront reads its group's liveness word first -- wave-uniform, a
// group is one wavefront's work, so the tests are scalar branches -- skips a group dead in every row of the workgroup before any load,
// issues nothing for a row the group is dead in, and selects a rollout without weight in a row out of both operands of that row's
// products.
template <class F, bool TAIL>
__device__ __forceinline__ void moments_body(const F &f, const WtArgs &t, const unsigned *lv) {
    constexpr int NT = F::TILES, NV = F::VECS, NS = F::SCALARS, O_V = NT * 256, O_S = O_V + NV * 64;
    __shared__ double sh[WT_WAVES][O_S + NS * 4];
    const int slot = blockIdx.x, r0 = F::batch() * WT_ROWS;
    const int nr = (t.nrows - r0 < WT_ROWS) ? t.nrows - r0 : WT_ROWS;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, kk = lane >> 4;
    wt_d4 c[WT_ROWS][NT];
    double v[WT_ROWS][NV], s[WT_ROWS][NS];
#pragma unroll
    for (int r = 0; r < WT_ROWS; ++r) {
#pragma unroll
        for (int b = 0; b < NT; ++b) c[r][b] = (wt_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int b = 0; b < NV; ++b) v[r][b] = 0.0;
#pragma unroll
        for (int b = 0; b < NS; ++b) s[r][b] = 0.0;
    }
    const long kc = t.kc, G = (kc + 3) >> 2;
    for (long g = (long)slot * WT_WAVES + w; g < G; g += (long)WT_SLOTS * WT_WAVES) {      // (uniform over the wavefront)
        unsigned on = 0xffu;
        if (TAIL) {
            on = (unsigned)__builtin_amdgcn_readfirstlane((int)((lv[g] >> r0) & 0xffu));
            if (on == 0u) continue;                                   // dead in every row of the workgroup: nothing is loaded
        }
        const long q = 4 * g + kk;
        const bool live = q < kc;                                     // (the K tail)
        const double J = live ? t.cost[q] : 0.0;
        const bool ok = live && !mc_nan(J);
        const typename F::Dev d = f.load(q, ok, J);
#pragma unroll
        for (int r = 0; r < WT_ROWS; ++r) {
            if (r < nr && (!TAIL || ((on >> r) & 1u))) {              // (uniform over the workgroup; with TAIL over the wavefront)
                const double y = ok ? t.y[(long)(r0 + r) * t.ldy + q] : 0.0;
                f.row(c[r], v[r], s[r], y, !TAIL || y != 0.0, d);
                s[r][0] += y; s[r][1] += y * y;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < WT_ROWS; ++r) {
        if (r < nr) {
            __syncthreads();                                          // (the previous row's sums are read)
#pragma unroll
            for (int b = 0; b < NT; ++b)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) sh[w][b * 256 + (kk + 4 * reg) * 16 + i] = c[r][b][reg];   // C: row (lane >> 4) + 4 reg, column lane & 15
#pragma unroll
            for (int b = 0; b < NV; ++b) sh[w][O_V + b * 64 + lane] = v[r][b];
            if (i == 0) {
#pragma unroll
                for (int b = 0; b < NS; ++b) sh[w][O_S + b * 4 + kk] = s[r][b];
            }
            __syncthreads();
            double *p = f.part(r0 + r, slot);
            const int e = threadIdx.x;
#pragma unroll
            for (int b = 0; b < NT; ++b) {
                double a = 0.0;
                for (int w2 = 0; w2 < WT_WAVES; ++w2) a += sh[w2][b * 256 + e];
                p[F::o_tile(b) + e] += a;
            }
            if (e < NV * 16) {                                        // vector e >> 4, component e & 15
                double a = 0.0;
                for (int w2 = 0; w2 < WT_WAVES; ++w2) for (int k2 = 0; k2 < 4; ++k2) a += sh[w2][O_V + (e >> 4) * 64 + k2 * 16 + (e & 15)];
                p[F::o_vec(e >> 4) + (e & 15)] += a;
            } else if (e < NV * 16 + NS) {
                double a = 0.0;
                for (int w2 = 0; w2 < WT_WAVES; ++w2) for (int k2 = 0; k2 < 4; ++k2) a += sh[w2][O_S + (e - NV * 16) * 4 + k2];
                p[F::o_scalar(e - NV * 16)] += a;
            }
        }
    }
}

// The replay check of rollout q, whose stored cost is J: the replay found the same bits (NaN equals NaN; dom_re: its DomainError flag)
__device__ __forceinline__ bool replay_same(const WtArgs &a, long q, double J) {
    double Jr = a.cost_re[q];
    if (a.dom_re && a.dom_re[q]) Jr = __builtin_nan("");
    return (mc_nan(J) && mc_nan(Jr)) || __double_as_longlong(J) == __double_as_longlong(Jr);
}

// The first rollout of the chunk that has a cost, WD_NONE where none has (the whole workgroup calls it).  c_w, c_q and c_J are that
// rollout's: as good a guess of where a draw lies as any one draw -- within a few standard deviations of the mean wherever the sampler
// puts that -- and known before the first sums, the same for every row.
__device__ __forceinline__ int first_with_cost(const double *cost, long kc) {
    __shared__ int first;
    if (threadIdx.x == 0) first = WD_NONE;
    __syncthreads();
    for (long q = threadIdx.x; q < kc; q += MC_THREADS)
        if (!mc_nan(cost[q])) { atomicMin(&first, (int)q); break; }                      // (an integer minimum: no order in it)
    __syncthreads();
    return first;
}

// S[q] = sum over the slots, in index order, of the partials p [WT_SLOTS][PART] (the whole workgroup calls it; S is ready on return)
template <int PART>
__device__ __forceinline__ void slot_sum(const double *p, double *S) {
    for (int q = threadIdx.x; q < PART; q += MC_THREADS) {
        double v = 0.0;
        for (int s = 0; s < WT_SLOTS; ++s) v += p[s * PART + q];
        S[q] = v;
    }
    __syncthreads();
}

// a row of an empty or non-finite sample: its moments are NaN
__device__ __forceinline__ bool row_dead(const double *wc, int r) {
    const double st = wc[WC_O_INFO + 2 * r + 1];
    return st == WC_ST_EMPTY || st == WC_ST_NONFINITE;
}

// ---- rat_policy_worst_case_trajectory: D = (x_t, u_t) - c_t in the 12 + 4 tile, one product -------------------------------------------------
__global__ __launch_bounds__(MC_THREADS) void wct_centre(const double *x, const double *u, int n, int m, int N, double *c) {
    for (int e = blockIdx.x * MC_THREADS + threadIdx.x; e < (N + 1) * 16; e += gridDim.x * MC_THREADS) {
        const int t = e >> 4, i = e & 15;
        double v = 0.0;
        if (i < 12) { if (i < n) v = x[t * 12 + i]; }
        else if (i - 12 < m && t < N) v = u[t * 4 + (i - 12)];
        if (!(fabs(v) < __builtin_inf())) v = 0.0;                    // (a centre is only a centre: any finite value serves)
        c[e] = v;
    }
}

__global__ __launch_bounds__(MC_THREADS) void wct_weights(WtArgs a) {
    const double Jmax = a.wc[WC_O_AUX + 2];
    const long T = (long)gridDim.x * MC_THREADS;
    int bad = 0;
    for (long q = (long)blockIdx.x * MC_THREADS + threadIdx.x; q < a.kc; q += T) {
        const double J = a.cost[q];
        bad += replay_same(a, q, J) ? 0 : 1;
        for (int r = 0; r < a.nrows; ++r) {
            const double th = a.wc[WC_O_INFO + 2 * r], st = a.wc[WC_O_INFO + 2 * r + 1];
            double y = 0.0;                                           // (a DomainError rollout, an empty or non-finite sample: no weight)
            if (!mc_nan(J)) {
                if (st == WC_ST_SEARCH) y = exp(th * (J - Jmax));
                else if (st == WC_ST_ZERO) y = 1.0;
                else if (st == WC_ST_SAT) y = (J == Jmax) ? 1.0 : 0.0;
            }
            a.y[(long)r * a.ldy + q] = y;
        }
    }
    if (bad) atomicAdd(a.mismatch, bad);
}

// ---- the tail calls' rows: every level's (v, y_eq, state) behind the tail-risk chain, then the weights and the liveness words per chunk ----
// tlt_levels repeats tr_rows' second level of the sums and its arithmetic for the atom -- the same partials in the same tree, so y_eq is
// the w_eq tail of TR_O_AUX bit for bit at level 0 -- for every level, and writes them where the worst-case kernels keep (theta, state).
__global__ __launch_bounds__(MC_THREADS) void tlt_levels(TrArgs a, double *wc) {
    __shared__ double sh[TR_NSUM * MC_THREADS];
    const TrHead h = tr_head(a.scratch, sh);
    const double n = h.n;
    for (int r = 0; r < a.n_alpha; ++r) {
        double q[TR_NSUM] = {0.0, 0.0, 0.0, 0.0};
        if (h.live) {
#pragma unroll
            for (int i = 0; i < TR_NSUM; ++i) q[i] = a.scratch[TR_O_PS + (r * TR_NSUM + i) * MC_BLOCKS + threadIdx.x];
        }
        block_tree_n<TR_NSUM>(q, sh);
        if (threadIdx.x != 0) continue;
        double v = 0.0, ye = 0.0, st = (h.flag == 2.0) ? WC_ST_EMPTY : WC_ST_NONFINITE;
        if (h.live) {
            const double cgt = q[2], ceq = q[3];
            const double av = tr_prod(n, a.alpha[r]), tail = n - av, k = tr_rank(n, av);
            v = tr_value(tr_gpfx(a.scratch)[TR_PASSES * TR_MAX_ALPHA + r]);
            if (tail < 1.0) ye = 1.0;                                 // thinner than one rollout: v = Jmax, the weight on the rollouts that reach it
            else { const double frac = k - av, ra = (n - k - cgt) + frac; ye = ra / ceq; }
            st = WC_ST_SEARCH;
        }
        wc[WC_O_INFO + 2 * r] = v; wc[WC_O_INFO + 2 * r + 1] = st; wc[TL_O_YEQ + r] = ye;
    }
}

// Lane q of a wavefront takes rollout q; the four lanes of a group combine their rows' "y != 0" bits by two exchanges within the group
// (the loop runs over whole groups, so the four are in it together) and the first writes the word.
__global__ __launch_bounds__(MC_THREADS) void tlt_weights(WtArgs a, unsigned *lv) {
    const long T = (long)gridDim.x * MC_THREADS, kc4 = (a.kc + 3) & ~3l;
    int bad = 0;
    for (long q = (long)blockIdx.x * MC_THREADS + threadIdx.x; q < kc4; q += T) {
        const bool in = q < a.kc;                                     // (the K tail: no cost, no weight, no bit)
        const double J = in ? a.cost[q] : __builtin_nan("");
        if (in) bad += replay_same(a, q, J) ? 0 : 1;
        const double S = (a.sample && in) ? a.sample[q] : J;          // (the sample the levels were selected on: the costs, or an event's margins)
        unsigned bits = 0u;
        for (int r = 0; r < a.nrows; ++r) {
            const double v = a.wc[WC_O_INFO + 2 * r], st = a.wc[WC_O_INFO + 2 * r + 1], ye = a.wc[TL_O_YEQ + r];
            double y = 0.0;                                           // (a DomainError rollout, an empty or non-finite sample: no weight)
            if (!mc_nan(S) && st == WC_ST_SEARCH) y = (S > v) ? 1.0 : (S == v) ? ye : 0.0;
            if (in) a.y[(long)r * a.ldy + q] = y;
            bits |= (y != 0.0) ? (1u << r) : 0u;
        }
        bits |= (unsigned)__shfl_xor((int)bits, 1);
        bits |= (unsigned)__shfl_xor((int)bits, 2);
        if ((q & 3) == 0) lv[q >> 2] = bits;
    }
    if (bad) atomicAdd(a.mismatch, bad);
}

struct TrajectoryMoments {
    static constexpr int TILES = 1, VECS = 1, SCALARS = 2;
    static __device__ __forceinline__ constexpr int o_tile(int) { return 0; }
    static __device__ __forceinline__ constexpr int o_vec(int) { return WT_O_S1; }
    static __device__ __forceinline__ constexpr int o_scalar(int s) { return s == 0 ? WT_O_S0 : WT_O_SY2; }
    static __device__ __forceinline__ int batch() { return blockIdx.z; }
    struct Dev { double D; };
    const WtArgs &a;
    const int t, i;
    const bool isx, comp;
    const double c;
    __device__ __forceinline__ TrajectoryMoments(const WtArgs &a_)
        : a(a_), t(blockIdx.y), i(threadIdx.x & 15), isx(i < 12),
          comp(isx ? (i < a_.n) : (i - 12 < a_.m && t < a_.N)),       // (padding lanes, and u at step N, stay zero)
          c(a_.centre[t * 16 + i]) {}
    __device__ __forceinline__ double *part(int row, int slot) const { return a.part + (((size_t)row * (a.N + 1) + t) * WT_SLOTS + slot) * WT_PART; }
    __device__ __forceinline__ Dev load(long q, bool ok, double) const {
        double D = 0.0;
        if (ok && comp) D = (isx ? a.xs[(q * (a.N + 1) + t) * a.ldx + i] : a.us[(q * a.N + t) * a.ldu + (i - 12)]) - c;
        return Dev{D};
    }
    __device__ __forceinline__ void row(wt_d4 (&C)[TILES], double (&v)[VECS], double (&)[SCALARS], double y, bool has, const Dev &d) const {
        const double Dr = has ? d.D : 0.0, yd = has ? y * d.D : 0.0;
        C[0] = wt_mfma(yd, Dr, C[0]);
        v[0] += yd;
    }
};

__global__ __launch_bounds__(WT_WAVES * 64) void wct_moments(WtArgs a) { moments_body<TrajectoryMoments, false>(TrajectoryMoments(a), a, nullptr); }
__global__ __launch_bounds__(WT_WAVES * 64) void tlt_moments(WtArgs a, const unsigned *live) { moments_body<TrajectoryMoments, true>(TrajectoryMoments(a), a, live); }

__global__ __launch_bounds__(MC_THREADS) void wct_final(WtArgs a) {
    __shared__ double S[WT_PART];
    const int t = blockIdx.x, r = blockIdx.y, e = threadIdx.x, N = a.N, d = a.n + a.m;
    slot_sum<WT_PART>(a.part + ((size_t)r * (N + 1) + t) * WT_SLOTS * WT_PART, S);
    const double nan = __builtin_nan("");
    const bool dead = row_dead(a.wc, r);
    const double s0 = S[WT_O_S0];
    const size_t o = (size_t)r * (N + 1) + t;
    if (e < d * d) {                                                  // column-major; the upper triangle of the tile serves both halves
        const int ii = e % d, jj = e / d;
        const int ti = (ii < a.n) ? ii : 12 + ii - a.n, tj = (jj < a.n) ? jj : 12 + jj - a.n;
        const int lo = ti < tj ? ti : tj, hi = ti < tj ? tj : ti;
        const double mi = S[WT_O_S1 + ti] / s0, mj = S[WT_O_S1 + tj] / s0;
        a.cov[o * d * d + e] = dead ? nan : S[lo * 16 + hi] / s0 - mi * mj;
    }
    if (e < d) {
        const int ti = (e < a.n) ? e : 12 + e - a.n;
        a.mean[o * d + e] = dead ? nan : a.centre[t * 16 + ti] + S[WT_O_S1 + ti] / s0;
    }
    if (t == 0 && e == 0) { a.ess[2 * r] = s0; a.ess[2 * r + 1] = S[WT_O_SY2]; }
}

// ---- rat_policy_worst_case_disturbance: Dw = w_t - c_w[t] (lanes i < n; lanes 12 .. 15 stay zero) and Dz = (x_t, u_t) - c_t ------------------
// Per group, step and row one MFMA A = y Dw, B = Dw for sum y Dw Dw', and with CROSS a second one with the same A and B = Dz:
// C[i][j] = sum y Dw_i Dz_j, w's component the row.  S1w and, with CROSS, S1z ride along.  c_w: first_with_cost's rollout.
__global__ __launch_bounds__(MC_THREADS) void wcd_centre(WdArgs a) {
    const int q = first_with_cost(a.t.cost, a.t.kc), N = a.t.N;
    for (int e = threadIdx.x; e < N * 16; e += MC_THREADS) {
        const int t = e >> 4, i = e & 15;
        double v = 0.0;
        if (q != WD_NONE && i < a.t.n) v = a.ws[((long)q * N + t) * a.ldw + i];
        if (!(fabs(v) < __builtin_inf())) v = 0.0;                    // (a centre is only a centre: any finite value serves)
        a.cw[e] = v;
    }
}

template <bool CROSS>
struct DisturbanceMoments {
    static constexpr int TILES = CROSS ? 2 : 1, VECS = CROSS ? 2 : 1, SCALARS = 2;
    static __device__ __forceinline__ constexpr int o_tile(int b) { return b == 0 ? 0 : WD_O_WZ; }
    static __device__ __forceinline__ constexpr int o_vec(int b) { return b == 0 ? WD_O_S1W : WD_O_S1Z; }
    static __device__ __forceinline__ constexpr int o_scalar(int s) { return s == 0 ? WD_O_S0 : WD_O_SY2; }
    static __device__ __forceinline__ int batch() { return blockIdx.z; }
    struct Dev { double Dw, Dz; };
    const WdArgs &a;
    const int t, i;
    const bool isx, compw, compz;
    const double cw, cz;
    __device__ __forceinline__ DisturbanceMoments(const WdArgs &a_)
        : a(a_), t(blockIdx.y), i(threadIdx.x & 15), isx(i < 12),
          compw(i < a_.t.n),                                          // (padding lanes stay zero)
          compz(isx ? (i < a_.t.n) : (i - 12 < a_.t.m)),              // (t < N throughout)
          cw(a_.cw[t * 16 + i]), cz(a_.t.centre[t * 16 + i]) {}
    __device__ __forceinline__ double *part(int row, int slot) const { return a.part + (((size_t)row * a.t.N + t) * WT_SLOTS + slot) * WD_PART; }
    __device__ __forceinline__ Dev load(long q, bool ok, double) const {
        const int N = a.t.N;
        double Dw = 0.0, Dz = 0.0;
        if (ok && compw) Dw = a.ws[(q * N + t) * a.ldw + i] - cw;
        if (CROSS && ok && compz) Dz = (isx ? a.t.xs[(q * (N + 1) + t) * a.t.ldx + i] : a.t.us[(q * N + t) * a.t.ldu + (i - 12)]) - cz;
        return Dev{Dw, Dz};
    }
    __device__ __forceinline__ void row(wt_d4 (&C)[TILES], double (&v)[VECS], double (&)[SCALARS], double y, bool has, const Dev &d) const {
        const double Dwr = has ? d.Dw : 0.0, yd = has ? y * d.Dw : 0.0;
        C[0] = wt_mfma(yd, Dwr, C[0]);
        if constexpr (CROSS) {
            const double Dzr = has ? d.Dz : 0.0;
            C[1] = wt_mfma(yd, Dzr, C[1]);
            v[1] += has ? y * d.Dz : 0.0;
        }
        v[0] += yd;
    }
};

template <bool CROSS>
__global__ __launch_bounds__(WT_WAVES * 64) void wcd_moments(WdArgs a) { moments_body<DisturbanceMoments<CROSS>, false>(DisturbanceMoments<CROSS>(a), a.t, nullptr); }
template <bool CROSS>
__global__ __launch_bounds__(WT_WAVES * 64) void tld_moments(WdArgs a, const unsigned *live) { moments_body<DisturbanceMoments<CROSS>, true>(DisturbanceMoments<CROSS>(a), a.t, live); }

__global__ __launch_bounds__(MC_THREADS) void wcd_final(WdArgs a) {
    __shared__ double S[WD_PART];
    const int t = blockIdx.x, r = blockIdx.y, e = threadIdx.x, N = a.t.N, n = a.t.n, d = a.t.n + a.t.m;
    slot_sum<WD_PART>(a.part + ((size_t)r * N + t) * WT_SLOTS * WD_PART, S);
    const double nan = __builtin_nan("");
    const bool dead = row_dead(a.t.wc, r);
    const double s0 = S[WD_O_S0];
    const size_t o = (size_t)r * N + t;
    if (e < n * n) {                                                  // column-major; the upper triangle of the tile serves both halves
        const int ii = e % n, jj = e / n;
        const int lo = ii < jj ? ii : jj, hi = ii < jj ? jj : ii;
        const double mi = S[WD_O_S1W + ii] / s0, mj = S[WD_O_S1W + jj] / s0;
        a.cov_w[o * n * n + e] = dead ? nan : S[lo * 16 + hi] / s0 - mi * mj;
    }
    if (a.cov_wz && e < n * d) {                                      // column-major [n][n+m]: w's component the row
        const int ii = e % n, jj = e / n;
        const int tj = (jj < n) ? jj : 12 + jj - n;
        const double mi = S[WD_O_S1W + ii] / s0, mj = S[WD_O_S1Z + tj] / s0;
        a.cov_wz[o * n * d + e] = dead ? nan : S[WD_O_WZ + ii * 16 + tj] / s0 - mi * mj;
    }
    if (e < n) a.mean_w[o * n + e] = dead ? nan : a.cw[t * 16 + e] + S[WD_O_S1W + e] / s0;
    if (t == 0 && e == 0) { a.ess[2 * r] = s0; a.ess[2 * r + 1] = S[WD_O_SY2]; }
}

// ---- rat_policy_gradient / rat_policy_tail_gradient: G = gu_t in lanes 12 .. 15, Dx = x_t - x_nom_t in lanes 0 .. 11, one product ----------
// Per group, step and row one MFMA A = y G, B = Dx: C[12 + j][i] = sum y gu_j Dx_i = dJ / dL_t(j, i) before the division.  A lane holds
// one of the two operands and an exact zero for the other, so the rest of the tile is zeros.  sum y G, sum y^2 G and sum y^2 G^2 ride
// along in the lanes, sum y and sum y^2 over the rollouts with finite sensitivities in the rollout lanes.  A rollout flagged in bad is
// selected out at the load -- of G, of Dx and of the two scalar sums -- so a NaN or Inf of its adjoint reaches nothing.
struct GradientMoments {
    static constexpr int TILES = 1, VECS = 3, SCALARS = 4;
    static __device__ __forceinline__ constexpr int o_tile(int) { return 0; }
    static __device__ __forceinline__ constexpr int o_vec(int b) { return b == 0 ? PG_O_V1 : b == 1 ? PG_O_V2 : PG_O_V3; }
    static __device__ __forceinline__ constexpr int o_scalar(int s) { return s == 0 ? PG_O_S0 : s == 1 ? PG_O_SY2 : s == 2 ? PG_O_SF : PG_O_SF2; }
    static __device__ __forceinline__ int batch() { return blockIdx.z; }
    struct Dev { double G, Dx; bool fin; };
    const PgArgs &a;
    const int t, i;
    const bool compg, compx;
    const double c;
    __device__ __forceinline__ GradientMoments(const PgArgs &a_)
        : a(a_), t(blockIdx.y), i(threadIdx.x & 15),
          compg(i >= 12 && i - 12 < a_.t.m),                          // (padding lanes stay zero; t < N throughout)
          compx(a_.xnom != nullptr && i < a_.t.n),
          c(compx ? a_.xnom[t * 12 + i] : 0.0) {}
    __device__ __forceinline__ double *part(int row, int slot) const { return a.part + (((size_t)row * a.t.N + t) * WT_SLOTS + slot) * PG_PART; }
    __device__ __forceinline__ Dev load(long q, bool ok, double) const {
        const int N = a.t.N;
        const bool fin = ok && a.bad[q] == 0;
        double G = 0.0, Dx = 0.0;
        if (fin && compg) G = a.gu[q * a.ldg + t * 4 + (i - 12)];
        if (fin && compx) Dx = a.t.xs[(q * (N + 1) + t) * a.t.ldx + i] - c;
        return Dev{G, Dx, fin};
    }
    __device__ __forceinline__ void row(wt_d4 (&C)[TILES], double (&v)[VECS], double (&s)[SCALARS], double y, bool has, const Dev &d) const {
        const double Dxr = has ? d.Dx : 0.0, yg = has ? y * d.G : 0.0, yf = d.fin ? y : 0.0;
        C[0] = wt_mfma(yg, Dxr, C[0]);
        v[0] += yg;
        v[1] += y * yg;
        v[2] += yg * yg;
        s[2] += yf;
        s[3] += yf * yf;
    }
};

__global__ __launch_bounds__(WT_WAVES * 64) void pg_moments(PgArgs a) { moments_body<GradientMoments, false>(GradientMoments(a), a.t, nullptr); }
__global__ __launch_bounds__(WT_WAVES * 64) void tlg_moments(PgArgs a, const unsigned *live) { moments_body<GradientMoments, true>(GradientMoments(a), a.t, live); }

// grad_l = sum y gu / sum y and grad_L = sum y gu Dx' / sum y over the rollouts with finite sensitivities; the self-normalised standard
// error sqrt(sum p^2 (gu - mean)^2), p = y / sum y, from the uncentred sums, clamped at 0.  A dead row (an empty or non-finite sample) is
// NaN, as in wct_final; a row none of whose rollouts has finite sensitivities is 0 / 0.
__global__ __launch_bounds__(MC_THREADS) void pg_final(PgArgs a) {
    __shared__ double S[PG_PART];
    const int t = blockIdx.x, r = blockIdx.y, e = threadIdx.x, N = a.t.N, n = a.t.n, m = a.t.m;
    slot_sum<PG_PART>(a.part + ((size_t)r * N + t) * WT_SLOTS * PG_PART, S);
    const double nan = __builtin_nan("");
    const bool dead = row_dead(a.t.wc, r);
    const double sf = S[PG_O_SF], sf2 = S[PG_O_SF2];
    const size_t o = (size_t)r * N + t;
    if (e < m * n) {                                                  // column-major m x n: entry (j, i) at j + m i
        const int j = e % m, ii = e / m;
        a.grad_L[o * m * n + e] = !a.xnom ? 0.0 : dead ? nan : S[(12 + j) * 16 + ii] / sf;   // (open loop: zeros)
    }
    if (e < m) {
        const double mean = S[PG_O_V1 + 12 + e] / sf;
        const double var = ((S[PG_O_V3 + 12 + e] - 2.0 * mean * S[PG_O_V2 + 12 + e]) + mean * mean * sf2) / (sf * sf);
        a.grad_l[o * m + e] = dead ? nan : mean;
        a.grad_l_se[o * m + e] = dead ? nan : (var > 0.0 ? sqrt(var) : (var != var ? nan : 0.0));
    }
    if (t == 0 && e == 0) { a.ess[2 * r] = S[PG_O_S0]; a.ess[2 * r + 1] = S[PG_O_SY2]; }
}

// ---- rat_policy_param_gradient / rat_policy_tail_param_gradient: per lane gp_i, gp_{16 + i} (TWO) and lam0_i, no product -------------------
// A payload without a C tile: what is asked for is first and second moments of each component alone, which ride in the lanes as
// GradientMoments' vectors do.  Component c of a lane puts sum y v, sum y^2 v, sum y^2 v^2 in vectors 3 c .. 3 c + 2; c = 0: gp_i,
// c = 1: lam0_i, c = 2 (TWO): gp_{16 + i}.  A rollout flagged in bad is selected out at the load -- of all three and of the two scalar
// sums -- so a NaN or Inf of its adjoint reaches nothing.
template <bool TWO>
struct ParamGradientMoments {
    static constexpr int NC = TWO ? 3 : 2;
    static constexpr int TILES = 0, VECS = 3 * NC, SCALARS = 4;
    static __device__ __forceinline__ constexpr int o_tile(int) { return 0; }
    static __device__ __forceinline__ constexpr int o_vec(int b) { return b * 16; }
    static __device__ __forceinline__ constexpr int o_scalar(int s) { return PPG_O_S0 + s; }   // S0, sum y^2, and the two over finite rollouts
    static __device__ __forceinline__ int batch() { return blockIdx.y; }
    struct Dev { double V[NC]; bool fin; };
    const PpgArgs &a;
    const int i;
    const bool comp0, compx, comp1;
    __device__ __forceinline__ ParamGradientMoments(const PpgArgs &a_)
        : a(a_), i(threadIdx.x & 15), comp0(i < a_.P), compx(i < a_.t.n && i < 12), comp1(TWO && 16 + i < a_.P) {}   // (padding lanes stay zero)
    __device__ __forceinline__ double *part(int row, int slot) const { return a.part + ((size_t)row * WT_SLOTS + slot) * PPG_PART; }
    __device__ __forceinline__ Dev load(long q, bool ok, double) const {
        Dev d;
        d.fin = ok && a.bad[q] == 0;
        d.V[0] = (d.fin && comp0) ? a.gp[q * 32 + i] : 0.0;
        d.V[1] = (d.fin && compx) ? a.lam0[q * 12 + i] : 0.0;
        if constexpr (TWO) d.V[2] = (d.fin && comp1) ? a.gp[q * 32 + 16 + i] : 0.0;
        return d;
    }
    template <class Tiles>
    __device__ __forceinline__ void row(Tiles &, double (&v)[VECS], double (&s)[SCALARS], double y, bool has, const Dev &d) const {
        const double yf = d.fin ? y : 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const double yv = has ? y * d.V[c] : 0.0;
            v[3 * c] += yv;
            v[3 * c + 1] += y * yv;
            v[3 * c + 2] += yv * yv;
        }
        s[2] += yf;
        s[3] += yf * yf;
    }
};

template <bool TWO>
__global__ __launch_bounds__(WT_WAVES * 64) void ppg_moments(PpgArgs a) { moments_body<ParamGradientMoments<TWO>, false>(ParamGradientMoments<TWO>(a), a.t, nullptr); }
template <bool TWO>
__global__ __launch_bounds__(WT_WAVES * 64) void tlpg_moments(PpgArgs a, const unsigned *live) { moments_body<ParamGradientMoments<TWO>, true>(ParamGradientMoments<TWO>(a), a.t, live); }

// grad_p = sum y gp / sum y and grad_x0 = sum y lam0 / sum y over the rollouts with finite sensitivities, each with its self-normalised
// standard error exactly as pg_final forms grad_l's: uncentred sums, clamped at 0, NaN for a dead row
__global__ __launch_bounds__(MC_THREADS) void ppg_final(PpgArgs a) {
    __shared__ double S[PPG_PART];
    const int r = blockIdx.x, e = threadIdx.x, n = a.t.n, P = a.P;
    slot_sum<PPG_PART>(a.part + (size_t)r * WT_SLOTS * PPG_PART, S);
    const double nan = __builtin_nan("");
    const bool dead = row_dead(a.t.wc, r);
    const double sf = S[PPG_O_SF], sf2 = S[PPG_O_SF2];
    if (e < P + n) {
        const bool isp = e < P;
        const int c = isp ? (e < 16 ? 0 : 2) : 1, i = isp ? (e & 15) : e - P;
        const double s1 = S[(3 * c) * 16 + i], s2 = S[(3 * c + 1) * 16 + i], s3 = S[(3 * c + 2) * 16 + i];
        const double mean = s1 / sf;
        const double var = ((s3 - 2.0 * mean * s2) + mean * mean * sf2) / (sf * sf);
        const double se = var > 0.0 ? sqrt(var) : (var != var ? nan : 0.0);
        double *g = isp ? a.grad_p + (size_t)r * P + e : a.grad_x0 + (size_t)r * n + i;
        double *gs = isp ? a.grad_p_se + (size_t)r * P + e : a.grad_x0_se + (size_t)r * n + i;
        *g = dead ? nan : mean;
        *gs = dead ? nan : se;
    }
    if (e == 0) { a.ess[2 * r] = S[PPG_O_S0]; a.ess[2 * r + 1] = S[PPG_O_SY2]; }
}

// ---- rat_policy_worst_case_params: one step, Dq = q - c_q in up to two tiles of sixteen parameters per lane ----------------------------------
// Lane (i, kk) holds Dq_i (tile 0) and Dq_{16 + i} (tile 1, TWO) of rollout 4 g + kk.  Per group and row A0 = y Dq(tile 0), B0 = Dq(tile 0)
// give block (0,0) of sum y Dq Dq'; with TWO, A0 and B1 give block (0,1) and A1, B1 block (1,1); block (1,0) is (0,1)' and is never
// formed.  S1 per tile and, with CROSS, sum y DJ Dq per tile ride along in the lanes, sum y DJ and sum y DJ^2 in the rollout lanes.
// Padding lanes (parameter index >= P) and padding rollouts enter as exact zeros.  The centres: first_with_cost's rollout, for q and for J.
__global__ __launch_bounds__(MC_THREADS) void wcp_centre(WpArgs a) {
    const int q = first_with_cost(a.t.cost, a.t.kc);
    for (int e = threadIdx.x; e < WP_NCENTRE; e += MC_THREADS) {
        double v = 0.0;
        if (q != WD_NONE && e < a.P) v = a.qs[(long)q * a.P + e];
        if (q != WD_NONE && e == WP_MAXP) v = a.t.cost[q];
        if (!(fabs(v) < __builtin_inf())) v = 0.0;                    // (a centre is only a centre: any finite value serves)
        a.centre[e] = v;
    }
}

template <bool TWO, bool CROSS>
struct ParamMoments {
    static constexpr int NQ = TWO ? 2 : 1;                            // parameter tiles: vectors 0 .. NQ - 1 are S1, NQ .. 2 NQ - 1 (CROSS) are SJq
    static constexpr int TILES = TWO ? 3 : 1, VECS = CROSS ? 2 * NQ : NQ, SCALARS = CROSS ? 4 : 2;
    static __device__ __forceinline__ constexpr int o_tile(int b) { return b * 256; }
    static __device__ __forceinline__ constexpr int o_vec(int b) { return b < NQ ? WP_O_S1 + b * 16 : WP_O_SJQ + (b - NQ) * 16; }
    static __device__ __forceinline__ constexpr int o_scalar(int s) { return WP_O_S0 + s; }   // S0, sum y^2, SJ, SJ2
    static __device__ __forceinline__ int batch() { return blockIdx.y; }
    struct Dev { double D0, D1, DJ; };
    const WpArgs &a;
    const int i;
    const bool comp0, comp1;
    const double c0, c1, cJ;
    __device__ __forceinline__ ParamMoments(const WpArgs &a_)
        : a(a_), i(threadIdx.x & 15), comp0(i < a_.P), comp1(TWO && 16 + i < a_.P),          // (padding lanes stay zero)
          c0(a_.centre[i]), c1(a_.centre[16 + i]), cJ(a_.centre[WP_MAXP]) {}
    __device__ __forceinline__ double *part(int row, int slot) const { return a.part + ((size_t)row * WT_SLOTS + slot) * WP_PART; }
    __device__ __forceinline__ Dev load(long q, bool ok, double J) const {
        double D0 = 0.0, D1 = 0.0;
        if (ok && comp0) D0 = a.qs[q * a.P + i] - c0;
        if (TWO && ok && comp1) D1 = a.qs[q * a.P + 16 + i] - c1;
        return Dev{D0, D1, (CROSS && ok) ? J - cJ : 0.0};
    }
    __device__ __forceinline__ void row(wt_d4 (&C)[TILES], double (&v)[VECS], double (&s)[SCALARS], double y, bool has, const Dev &d) const {
        const double D0r = has ? d.D0 : 0.0, yd0 = has ? y * d.D0 : 0.0;
        C[0] = wt_mfma(yd0, D0r, C[0]);
        v[0] += yd0;
        const double D1r = (TWO && has) ? d.D1 : 0.0;
        if constexpr (TWO) {
            const double yd1 = has ? y * d.D1 : 0.0;
            C[1] = wt_mfma(yd0, D1r, C[1]);
            C[2] = wt_mfma(yd1, D1r, C[2]);
            v[1] += yd1;
        }
        if constexpr (CROSS) {
            const double yj = y * d.DJ;
            s[2] += yj; s[3] += yj * d.DJ; v[NQ] += yj * D0r;
            if constexpr (TWO) v[NQ + 1] += yj * D1r;
        }
    }
};

template <bool TWO, bool CROSS>
__global__ __launch_bounds__(WT_WAVES * 64) void wcp_moments(WpArgs a) { moments_body<ParamMoments<TWO, CROSS>, false>(ParamMoments<TWO, CROSS>(a), a.t, nullptr); }
template <bool TWO, bool CROSS>
__global__ __launch_bounds__(WT_WAVES * 64) void tlp_moments(WpArgs a, const unsigned *live) { moments_body<ParamMoments<TWO, CROSS>, true>(ParamMoments<TWO, CROSS>(a), a.t, live); }

__global__ __launch_bounds__(MC_THREADS) void wcp_final(WpArgs a) {
#pragma clang fp contract(off)                                        // S2 / S0 - m m' with m m' rounded: where one rollout carries all the weight the two are the same product, and the covariance is exactly 0
    __shared__ double S[WP_PART];
    const int r = blockIdx.x, e0 = threadIdx.x, P = a.P;
    slot_sum<WP_PART>(a.part + (size_t)r * WT_SLOTS * WP_PART, S);
    const double nan = __builtin_nan("");
    const bool dead = row_dead(a.t.wc, r);
    const double s0 = S[WP_O_S0];
    for (int e = e0; e < P * P; e += MC_THREADS) {                    // column-major; the upper triangle serves both halves, block (0,1) block (1,0)
        const int ii = e % P, jj = e / P;
        const int lo = ii < jj ? ii : jj, hi = ii < jj ? jj : ii;
        const int blk = (lo >> 4) + (hi >> 4);                        // (0,0) -> 0, (0,1) -> 1, (1,1) -> 2
        const double mi = S[WP_O_S1 + ii] / s0, mj = S[WP_O_S1 + jj] / s0;
        a.cov_q[(size_t)r * P * P + e] = dead ? nan : S[blk * 256 + (lo & 15) * 16 + (hi & 15)] / s0 - mi * mj;
    }
    if (e0 < P) {
        const double mi = S[WP_O_S1 + e0] / s0;
        a.mean_q[(size_t)r * P + e0] = dead ? nan : a.centre[e0] + mi;
        if (a.cov_qJ) a.cov_qJ[(size_t)r * P + e0] = dead ? nan : S[WP_O_SJQ + e0] / s0 - mi * (S[WP_O_SJ] / s0);
    }
    if (e0 == 0) {
        const double mj = S[WP_O_SJ] / s0;
        a.ess[4 * r] = s0; a.ess[4 * r + 1] = S[WP_O_SY2];
        a.ess[4 * r + 2] = a.centre[WP_MAXP] + mj; a.ess[4 * r + 3] = S[WP_O_SJ2] / s0 - mj * mj;
    }
}

// ---- rat_policy_events: violation probabilities of quadratic events on the replayed trajectories ----------------------------------------
// ev_eval: a wavefront takes sixteen rollouts as the columns of Z [16 components][16 rollouts] and walks the steps; lane (col = lane & 15,
// kq = lane >> 4) holds Z[kq + 4 r][col], r = 0 .. 3 -- x components kq, kq + 4, kq + 8 and u component kq -- which is at once the B operand
// of k-block r of Q Z (four 16 x 16 x 4 MFMAs, Q's operands from LDS) and the lane's rows of the product: z' Q z is the lane's four
// products, summed over the four kq lanes of the column by a butterfly (every lane of a column ends with the same bits).  g of a
// (rollout, step, event) is formed from that column alone: its bits depend on no other rollout, event or row.  The running margin, the
// first violating step and the step's indicator bits stay in registers.
// ev_sums: lane tid of slot s takes the rollouts s * 256 + tid, + EV_SLOTS * 256, ... in order; the lanes combine in the fixed LDS tree
// into the slot's partial, chunk after chunk in stream order; ev_final sums the slots in index order.  A workgroup (slot, y, row batch)
// sums either one step's indicators of every event, or one event's per-rollout terms.  No floating-point atomics, and the counts are
// sums of ones in double: exact, so no atomics there either.
// ARGMAX (launch_ev_argmax, rat_policy_margin_gradient): the same text, and the step at which the running margin was last replaced.
template <bool QUAD, bool ARGMAX = false>
__global__ __launch_bounds__(MC_THREADS) void ev_eval(EvArgs a) {
    __shared__ double s_q[QUAD ? EV_MAX * 256 : 1];
    __shared__ double s_a[EV_MAX * 16], s_b[EV_MAX];
    __shared__ int s_lo[EV_MAX], s_hi[EV_MAX];
    const int tid = threadIdx.x, ne = a.n_event, N = a.N;
    if (QUAD) for (int i = tid; i < ne * 256; i += MC_THREADS) s_q[i] = a.Qt[i];
    for (int i = tid; i < ne * 16; i += MC_THREADS) s_a[i] = a.at[i];
    if (tid < ne) { s_b[tid] = a.b[tid]; s_lo[tid] = a.win[2 * tid]; s_hi[tid] = a.win[2 * tid + 1]; }
    __syncthreads();
    const int w = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const double nan = __builtin_nan("");
    const long G = (a.kc + 15) >> 4;
    for (long g = (long)blockIdx.x * 4 + w; g < G; g += (long)gridDim.x * 4) {           // (uniform over the wavefront)
        const long q = 16 * g + col;
        const bool live = q < a.kc;                                   // (the K tail)
        const bool ok = live && !mc_nan(a.cost[live ? q : 0]);        // selected, not multiplied: the trajectory may hold NaN
        const double *xq = a.xs + q * (N + 1) * a.ldx, *uq = a.us + q * N * a.ldu;
        double M[EV_MAX];
        int tau[EV_MAX], ts[ARGMAX ? EV_MAX : 1];
#pragma unroll
        for (int e = 0; e < EV_MAX; ++e) { M[e] = nan; tau[e] = -1; if (ARGMAX) ts[e] = -1; }
        for (int t = 0; t <= N; ++t) {
            double zv[4];
#pragma unroll
            for (int r = 0; r < 3; ++r) zv[r] = (ok && kq + 4 * r < a.n) ? xq[t * a.ldx + kq + 4 * r] : 0.0;
            zv[3] = (ok && kq < a.m && t < N) ? uq[t * a.ldu + kq] : 0.0;
            unsigned bits = 0u;
#pragma unroll
            for (int e = 0; e < EV_MAX; ++e) {
                if (e < ne) {                                         // (uniform over the grid)
                    const double *ae = s_a + e * 16 + kq;
                    double p = ae[0] * zv[0] + ae[4] * zv[1] + ae[8] * zv[2] + ae[12] * zv[3];
                    if (QUAD) {
                        const double *qe = s_q + e * 256 + kq * 16 + col;
                        wt_d4 c = (wt_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
                        for (int kb = 0; kb < 4; ++kb) c = __builtin_amdgcn_mfma_f64_16x16x4f64(qe[kb * 64], zv[kb], c, 0, 0, 0);
                        p += c[0] * zv[0] + c[1] * zv[1] + c[2] * zv[2] + c[3] * zv[3];
                    }
                    p += __shfl_xor(p, 16);
                    p += __shfl_xor(p, 32);
                    const double gv = p + s_b[e];
                    if (t >= s_lo[e] && t <= s_hi[e]) {
                        if (gv > M[e] || mc_nan(M[e])) {              // (a NaN g never replaces a number)
                            M[e] = gv;
                            if (ARGMAX && !mc_nan(gv)) ts[e] = t;
                        }
                        if (gv > 0.0) {
                            bits |= 1u << e;
                            if (tau[e] < 0) tau[e] = t;
                        }
                    }
                }
            }
            if (bits) bits |= 1u << ne;
            if (a.mask && kq == 0 && live) a.mask[(long)t * a.ldy + q] = ok ? bits : 0u;
        }
        if (ARGMAX) {
            if (kq == 0 && live) {
#pragma unroll
                for (int e = 0; e < EV_MAX; ++e) {
                    if (e < ne) {
                        a.margin[(long)e * a.ldy + q] = ok ? M[e] : nan;
                        a.tstar[(long)e * a.ldy + q] = ok ? ts[e] : -1;
                    }
                }
            }
            continue;
        }
        if (kq == 0 && live) {
            double Ma = nan;
            int ta = -1;
#pragma unroll
            for (int e = 0; e < EV_MAX; ++e) {
                if (e < ne) {
                    a.margin[(long)e * a.ldy + q] = ok ? M[e] : nan;
                    a.tau[(long)e * a.ldy + q] = ok ? tau[e] : -1;
                    if (M[e] > Ma || mc_nan(Ma)) Ma = M[e];
                    if (tau[e] >= 0 && (ta < 0 || tau[e] < ta)) ta = tau[e];
                }
            }
            a.margin[(long)ne * a.ldy + q] = ok ? Ma : nan;
            a.tau[(long)ne * a.ldy + q] = ok ? ta : -1;
        }
    }
}

// ev_sums_body: the sums of one chunk, once for the KL rows (ev_sums) and the tail rows (tle_sums).  TAIL reads the liveness word of the
// rollout's group of four first (tlt_weights wrote it: bit r says some y of level r in the group is not zero), a load of one word per four
// lanes.  What it passes over would have added 0 (y == 0, or no indicator bit), which changes no bit of a sum that started at +0 and holds
// no negative term; y != 0 means the rollout has a cost, so the steps' workgroups do not read the costs at all.  Everything else -- the lane
// that takes a rollout, the order it takes them in, the trees, the partials -- is written once: alpha = 0 is the theta = 0 row and the
// switch tail_dense gives the same bits because there is no second copy to keep in step.
template <bool TAIL>
__device__ __forceinline__ void ev_sums_body(const EvArgs &a) {
    __shared__ double sh[(EV_MAX + 1) * MC_THREADS];
    const int slot = blockIdx.x, by = blockIdx.y, r0 = blockIdx.z * EV_ROWS, tid = threadIdx.x;
    const int nr = (a.nrows - r0 < EV_ROWS) ? a.nrows - r0 : EV_ROWS;
    const int nsteps = a.mask ? a.N + 1 : 0, ny = nsteps + a.n_event + 1;
    double *p = a.part + (((size_t)blockIdx.z * ny + by) * EV_SLOTS + slot) * EV_PART;
    const long T = (long)EV_SLOTS * MC_THREADS;
    const unsigned rows = (1u << nr) - 1u;                            // the rows of this workgroup, as bits of a word shifted by r0 (uniform over the workgroup)
    if (by < nsteps) {                                                // one step: sum y [g_e(t) > 0] per row and event
        double acc[EV_ROWS][EV_MAX + 1];
#pragma unroll
        for (int r = 0; r < EV_ROWS; ++r)
#pragma unroll
            for (int e = 0; e <= EV_MAX; ++e) acc[r][e] = 0.0;
        for (long q = (long)slot * MC_THREADS + tid; q < a.kc; q += T) {
            unsigned on = rows, bits;
            bool ok = true;
            if (TAIL) {
                on = (a.live[q >> 2] >> r0) & rows;
                if (on == 0u) continue;                               // no weight in any row of the workgroup: nothing is loaded
                bits = a.mask[(long)by * a.ldy + q];
                if (bits == 0u) continue;                             // no event at this step: no weight is loaded
            } else {
                ok = !mc_nan(a.cost[q]);
                bits = ok ? a.mask[(long)by * a.ldy + q] : 0u;
            }
#pragma unroll
            for (int r = 0; r < EV_ROWS; ++r) {
                if ((on >> r) & 1u) {
                    const double y = ok ? a.y[(long)(r0 + r) * a.ldy + q] : 0.0;
#pragma unroll
                    for (int e = 0; e <= EV_MAX; ++e) acc[r][e] += ((bits >> e) & 1u) ? y : 0.0;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < EV_ROWS; ++r) {
            if (r < nr) {                                             // (uniform over the workgroup)
                block_tree_n<EV_MAX + 1>(acc[r], sh);
                if (tid == 0) {
#pragma unroll
                    for (int e = 0; e <= EV_MAX; ++e) p[r * (EV_MAX + 1) + e] = a.first ? acc[r][e] : p[r * (EV_MAX + 1) + e] + acc[r][e];
                }
            }
        }
        return;
    }
    const int e = by - nsteps;                                        // one event: the per-rollout terms per row, the counts, the largest margin
    double s[EV_ROWS][EV_NSUM], cnt[2] = {0.0, 0.0}, mx = -__builtin_inf();
#pragma unroll
    for (int r = 0; r < EV_ROWS; ++r)
#pragma unroll
        for (int i = 0; i < EV_NSUM; ++i) s[r][i] = 0.0;
    for (long q = (long)slot * MC_THREADS + tid; q < a.kc; q += T) {
        const bool ok = !mc_nan(a.cost[q]);                           // the counts and the largest margin are unweighted: every rollout is read
        const double Mv = a.margin[(long)e * a.ldy + q];
        const int tv = a.tau[(long)e * a.ldy + q];
        const bool A = ok && tv >= 0;
        cnt[0] += A ? 1.0 : 0.0;
        cnt[1] += ok ? 1.0 : 0.0;
        if (ok && Mv > mx) mx = Mv;
        unsigned on = rows;
        if (TAIL) {
            on = (a.live[q >> 2] >> r0) & rows;
            if (on == 0u) continue;
        }
#pragma unroll
        for (int r = 0; r < EV_ROWS; ++r) {
            if ((on >> r) & 1u) {
                const double y = (TAIL || ok) ? a.y[(long)(r0 + r) * a.ldy + q] : 0.0, y2 = y * y;
                s[r][0] += y;
                s[r][1] += A ? y : 0.0;
                s[r][2] += A ? y2 : 0.0;
                s[r][3] += A ? 0.0 : y2;
                if (TAIL) s[r][4] += (y != 0.0) ? y * Mv : 0.0;       // (selected, not multiplied: a rollout without weight may hold a NaN margin)
                else s[r][4] += ok ? y * Mv : 0.0;
                s[r][5] += A ? y * (double)tv : 0.0;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < EV_ROWS; ++r) {
        if (r < nr) {
            block_tree_n<EV_NSUM>(s[r], sh);
            if (tid == 0) {
#pragma unroll
                for (int i = 0; i < EV_NSUM; ++i) p[r * EV_NSUM + i] = a.first ? s[r][i] : p[r * EV_NSUM + i] + s[r][i];
            }
        }
    }
    block_tree_n<2>(cnt, sh);
    mx = block_tree<2>(mx, sh);
    if (tid == 0) {
        p[EV_O_NVIOL] = a.first ? cnt[0] : p[EV_O_NVIOL] + cnt[0];
        p[EV_O_NOK] = a.first ? cnt[1] : p[EV_O_NOK] + cnt[1];
        p[EV_O_MMAX] = (a.first || mx > p[EV_O_MMAX]) ? mx : p[EV_O_MMAX];
    }
}

__global__ __launch_bounds__(MC_THREADS) void ev_sums(EvArgs a) { ev_sums_body<false>(a); }
// (rat_policy_tail_events: the event sums under tail rows, where one rollout in a hundred carries weight)
__global__ __launch_bounds__(MC_THREADS) void tle_sums(EvArgs a) { ev_sums_body<true>(a); }

// ev_final_body: the slots of one (event, row) summed in index order, then the statistics.  A KL row (ev_final) takes its state from the
// row's word of a.wc and leaves N_OK in slot 6 for the host's rat_kl_event_bound; a tail row (tle_final) takes RAT_TR_FLAG of its level,
// and its PROB_ROBUST is the CVaR adversary aimed at the event -- the largest probability of the event under any p with
// dp/dq <= N_OK / TAIL_N -- formed here from the counts and the row.
template <bool TAIL>
__device__ __forceinline__ void ev_final_body(const EvArgs &a) {
    __shared__ double S[EV_NSUM + 3];
    const int e = blockIdx.x, r = blockIdx.y, z = r / EV_ROWS, rr = r % EV_ROWS, tid = threadIdx.x;
    const int nsteps = a.mask ? a.N + 1 : 0, ne1 = a.n_event + 1, ny = nsteps + ne1;
    const double *pe = a.part + ((size_t)z * ny + nsteps + e) * EV_SLOTS * EV_PART;
    if (tid < EV_NSUM + 3) {
        const int i = (tid < EV_NSUM) ? rr * EV_NSUM + tid : EV_O_NVIOL + (tid - EV_NSUM);
        double v = pe[i];
        for (int sl = 1; sl < EV_SLOTS; ++sl) {
            const double x = pe[sl * EV_PART + i];
            v = (i == EV_O_MMAX) ? (x > v ? x : v) : v + x;
        }
        S[tid] = v;
    }
    __syncthreads();
    const double nan = __builtin_nan("");
    double flag;
    bool dead;
    if (TAIL) {
        flag = a.tr[r * TR_NSTAT + 7];
        dead = (flag == 2.0 || flag == 3.0);                          // RAT_TR_EMPTY, RAT_TR_NONFINITE
    } else {
        const double st = a.wc[WC_O_INFO + 2 * r + 1];
        dead = (st == WC_ST_EMPTY || st == WC_ST_NONFINITE);
        flag = (st == WC_ST_SAT) ? 1.0 : (st == WC_ST_EMPTY) ? 2.0 : (st == WC_ST_NONFINITE) ? 3.0 : 0.0;
    }
    const double sy = S[0];
    if (tid == 0) {
        double *o = a.event_out + ((size_t)r * ne1 + e) * EV_NSTAT;
        const double pr = S[1] / sy, se2 = (1.0 - pr) * (1.0 - pr) * S[2] + pr * pr * S[3];
        const double nv = S[EV_NSUM], nok = S[EV_NSUM + 1];
        o[0] = dead ? nan : pr;
        o[1] = dead ? nan : sqrt(se2) / sy;
        o[2] = dead ? nan : S[4] / sy;
        o[3] = dead ? nan : S[EV_NSUM + 2];
        o[4] = dead ? nan : S[5] / S[1];                              // (NaN when no weighted rollout violates: 0 / 0)
        o[5] = dead ? nan : nv;
        if (TAIL) {
            const double tail = a.tr[r * TR_NSTAT + 4];
            double rob = (nv / nok) / (tail / nok);
            rob = rob < 1.0 ? rob : 1.0;
            if (rob < pr) rob = pr;                                   // (every violator in the tail: the two are one number, and rounding must not part them)
            o[6] = dead ? nan : rob;
        } else {
            o[6] = dead ? nan : nok;                                  // N_OK: the host forms PROB_ROBUST from it
        }
        o[7] = flag;
    }
    for (int t = tid; t < nsteps; t += MC_THREADS) {
        const double *ps = a.part + ((size_t)z * ny + t) * EV_SLOTS * EV_PART + rr * (EV_MAX + 1) + e;
        double v = 0.0;
        for (int sl = 0; sl < EV_SLOTS; ++sl) v += ps[sl * EV_PART];
        a.step_out[((size_t)r * ne1 + e) * nsteps + t] = dead ? nan : v / sy;
    }
}

__global__ __launch_bounds__(MC_THREADS) void ev_final(EvArgs a) { ev_final_body<false>(a); }
__global__ __launch_bounds__(MC_THREADS) void tle_final(EvArgs a) { ev_final_body<true>(a); }

// ---- rat_policy_sobol: first-order and total Sobol indices from the pick-freeze costs Y [d + 2][K] ------------------------------------------
// Rows A, B, then the d groups' AB_i (rat_src_sobol_rollout, source_sobol.h).  Three launches, every sum in mc_pass1's order (lane g of the
// MC_BLOCKS x MC_THREADS grid sums base samples g, g + T, ... in order, the LDS tree, the second level at the head of the next launch):
//   sb_pass1   ok[k] = no row of base sample k is NaN; N_OK and sum (y_A + y_B) over the OK samples                   -> part1 [2][B]
//   sb_pass2   mu from part1; per group (blockIdx.y), with a' = y_A - mu, b' = y_B - mu, D = y_i - y_A, s = (a'^2 + b'^2) / 2,
//              ns = b' D, nt = D D:  sum s, s^2, ns, ns^2, ns s, nt, nt^2, nt s                                      -> part2 [d][8][B]
//   sb_final   V = sum s / N_OK; S = sum ns / sum s, T = sum nt / (2 sum s); the standard errors from the ratio linearisation:
//              the residuals e = ns - S s (or nt / 2 - T s) have mean zero by construction, so var(e) = sum e^2 / (N_OK - 1) with
//              sum e^2 = sum ns^2 - 2 S sum ns s + S^2 sum s^2 expanded, and SE = sqrt(var(e) / N_OK) / V.
// Centring about the pooled mean matters: the uncentred numerator mean(y_B (y_i - y_A)) carries mu (y_i - y_A), whose mean is zero but
// whose spread is mu^2 T -- it would dominate the standard error wherever |mu| is large against sd(J).  D is formed from the costs
// themselves, not from the centred values: a group with empty masks has y_i == y_A bit for bit and gets S = T = 0 exactly.
__global__ __launch_bounds__(MC_THREADS) void sb_pass1(SbArgs a) {
    __shared__ double sh[MC_THREADS];
    const long T = (long)MC_BLOCKS * MC_THREADS;
    double cnt = 0.0, sum = 0.0;
    for (long k = (long)blockIdx.x * MC_THREADS + threadIdx.x; k < a.K; k += T) {
        bool ok = true;
        for (int v = 0; v < a.d + 2; ++v) ok = ok && !mc_nan(a.y[(long)v * a.ldy + k]);
        a.ok[k] = ok ? 1 : 0;                                         // (each base sample belongs to one lane)
        if (ok) { cnt += 1.0; sum += a.y[k] + a.y[a.ldy + k]; }
    }
    cnt = block_tree<0>(cnt, sh);
    sum = block_tree<0>(sum, sh);
    if (threadIdx.x == 0) { a.scratch[SB_O_P1 + blockIdx.x] = cnt; a.scratch[SB_O_P1 + MC_BLOCKS + blockIdx.x] = sum; }
}

__global__ __launch_bounds__(MC_THREADS) void sb_pass2(SbArgs a) {
    __shared__ double sh[SB_NSUM * MC_THREADS];
    const double n_ok = block_tree<0>(a.scratch[SB_O_P1 + threadIdx.x], sh);
    const double mu = block_tree<0>(a.scratch[SB_O_P1 + MC_BLOCKS + threadIdx.x], sh) / (2.0 * n_ok);
    const int i = blockIdx.y;
    const double *ya = a.y, *yb = a.y + a.ldy, *yi = a.y + (long)(2 + i) * a.ldy;
    double v[SB_NSUM];
#pragma unroll
    for (int q = 0; q < SB_NSUM; ++q) v[q] = 0.0;
    const long T = (long)MC_BLOCKS * MC_THREADS;
    for (long k = (long)blockIdx.x * MC_THREADS + threadIdx.x; k < a.K; k += T) {
        if (!a.ok[k]) continue;
        const double A = ya[k], ap = A - mu, bp = yb[k] - mu, D = yi[k] - A;
        const double s = 0.5 * (ap * ap + bp * bp), ns = bp * D, nt = D * D;
        v[0] += s; v[1] += s * s;
        v[2] += ns; v[3] += ns * ns; v[4] += ns * s;
        v[5] += nt; v[6] += nt * nt; v[7] += nt * s;
    }
    block_tree_n<SB_NSUM>(v, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < SB_NSUM; ++q) a.scratch[SB_O_P2 + ((size_t)i * SB_NSUM + q) * MC_BLOCKS + blockIdx.x] = v[q];
    }
}

__global__ __launch_bounds__(MC_THREADS) void sb_final(SbArgs a) {
    __shared__ double sh[SB_NSUM * MC_THREADS];
    const int tid = threadIdx.x;
    const double nan = __builtin_nan("");
    const double n = block_tree<0>(a.scratch[SB_O_P1 + tid], sh);
    const double sum = block_tree<0>(a.scratch[SB_O_P1 + MC_BLOCKS + tid], sh);
    double *out = a.scratch + SB_O_OUT, *rows = a.scratch + SB_O_ROWS;
    bool good = false;
    for (int i = 0; i < a.d; ++i) {
        double v[SB_NSUM];
#pragma unroll
        for (int q = 0; q < SB_NSUM; ++q) v[q] = a.scratch[SB_O_P2 + ((size_t)i * SB_NSUM + q) * MC_BLOCKS + tid];
        block_tree_n<SB_NSUM>(v, sh);
        const double V = v[0] / n;
        good = n >= 2.0 && V > 0.0 && V < __builtin_inf();
        if (tid != 0) continue;
        if (i == 0) {                                                 // (sum s and sum s^2 are the same bits in every group's partials)
            double vs = (v[1] - v[0] * v[0] / n) / (n - 1.0);
            if (vs < 0.0) vs = 0.0;
            out[0] = n; out[1] = n > 0.0 ? sum / (2.0 * n) : nan; out[2] = n > 0.0 ? V : nan; out[3] = n >= 2.0 ? sqrt(vs / n) : nan;
            out[4] = good ? 0.0 : (double)SB_FLAG_DEGENERATE; out[5] = (double)a.K - n; out[6] = 0.0; out[7] = 0.0;
        }
        const double S = v[2] / v[0], Tt = v[5] / (2.0 * v[0]);
        double es = v[3] - 2.0 * S * v[4] + S * S * v[1], et = 0.25 * v[6] - Tt * v[7] + Tt * Tt * v[1];
        if (es < 0.0) es = 0.0;
        if (et < 0.0) et = 0.0;
        rows[i * 4 + 0] = good ? S : nan;
        rows[i * 4 + 1] = good ? sqrt(es / (n - 1.0) / n) / V : nan;
        rows[i * 4 + 2] = good ? Tt : nan;
        rows[i * 4 + 3] = good ? sqrt(et / (n - 1.0) / n) / V : nan;
    }
}

}  // namespace

void launch_policy_sobol(const SbArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(sb_pass1, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, a);
    hipLaunchKernelGGL(sb_pass2, dim3(MC_BLOCKS, (unsigned)a.d), dim3(MC_THREADS), 0, s, a);
    hipLaunchKernelGGL(sb_final, dim3(1), dim3(MC_THREADS), 0, s, a);
}

void launch_wct_centre(const double *x, const double *u, int n, int m, int N, double *centre, hipStream_t s) {
    hipLaunchKernelGGL(wct_centre, dim3((unsigned)(((N + 1) * 16 + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, s, x, u, n, m, N, centre);
}

void launch_wct_weights(const WtArgs &a, hipStream_t s) {
    if (a.kc <= 0 || a.nrows <= 0) return;
    const long nb = (a.kc + MC_THREADS - 1) / MC_THREADS;
    hipLaunchKernelGGL(wct_weights, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(MC_THREADS), 0, s, a);
}

// a chunk's sums behind its weights: the dense kernel, or (live: the chunk's liveness words) its tail sibling
template <class A>
static void launch_moments(void (*dense)(A), void (*tail)(A, const unsigned *), dim3 grid, const A &a, const unsigned *live, hipStream_t s) {
    if (live) hipLaunchKernelGGL(tail, grid, dim3(WT_WAVES * 64), 0, s, a, live);
    else hipLaunchKernelGGL(dense, grid, dim3(WT_WAVES * 64), 0, s, a);
}

void launch_wct_chunk(const WtArgs &a, const unsigned *live, hipStream_t s) {
    if (a.kc <= 0 || a.nrows <= 0) return;
    launch_moments(wct_moments, tlt_moments, dim3(WT_SLOTS, (unsigned)(a.N + 1), (unsigned)((a.nrows + WT_ROWS - 1) / WT_ROWS)), a, live, s);
}

void launch_wct_final(const WtArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(wct_final, dim3((unsigned)(a.N + 1), (unsigned)a.nrows), dim3(MC_THREADS), 0, s, a);
}

void launch_wcd_centre(const WdArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(wcd_centre, dim3(1), dim3(MC_THREADS), 0, s, a);
}

void launch_wcd_chunk(const WdArgs &a, const unsigned *live, hipStream_t s) {
    if (a.t.kc <= 0) return;
    const dim3 grid(WT_SLOTS, (unsigned)a.t.N, (unsigned)((a.t.nrows + WT_ROWS - 1) / WT_ROWS));
    if (a.cross) launch_moments(wcd_moments<true>, tld_moments<true>, grid, a, live, s);
    else launch_moments(wcd_moments<false>, tld_moments<false>, grid, a, live, s);
}

void launch_wcd_final(const WdArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(wcd_final, dim3((unsigned)a.t.N, (unsigned)a.t.nrows), dim3(MC_THREADS), 0, s, a);
}

void launch_pg_chunk(const PgArgs &a, const unsigned *live, hipStream_t s) {
    if (a.t.kc <= 0 || a.t.nrows <= 0 || a.t.N <= 0) return;
    launch_moments(pg_moments, tlg_moments, dim3(WT_SLOTS, (unsigned)a.t.N, (unsigned)((a.t.nrows + WT_ROWS - 1) / WT_ROWS)), a, live, s);
}

void launch_pg_final(const PgArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(pg_final, dim3((unsigned)a.t.N, (unsigned)a.t.nrows), dim3(MC_THREADS), 0, s, a);
}

void launch_ppg_chunk(const PpgArgs &a, const unsigned *live, hipStream_t s) {
    if (a.t.kc <= 0 || a.t.nrows <= 0) return;
    const dim3 grid(WT_SLOTS, (unsigned)((a.t.nrows + WT_ROWS - 1) / WT_ROWS));
    if (a.P > 16) launch_moments(ppg_moments<true>, tlpg_moments<true>, grid, a, live, s);
    else launch_moments(ppg_moments<false>, tlpg_moments<false>, grid, a, live, s);
}

void launch_ppg_final(const PpgArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(ppg_final, dim3((unsigned)a.t.nrows), dim3(MC_THREADS), 0, s, a);
}

void launch_wcp_centre(const WpArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(wcp_centre, dim3(1), dim3(MC_THREADS), 0, s, a);
}

void launch_wcp_chunk(const WpArgs &a, const unsigned *live, hipStream_t s) {
    if (a.t.kc <= 0) return;
    const dim3 grid(WT_SLOTS, (unsigned)((a.t.nrows + WT_ROWS - 1) / WT_ROWS));
    if (a.P > 16) {
        if (a.cross) launch_moments(wcp_moments<true, true>, tlp_moments<true, true>, grid, a, live, s);
        else launch_moments(wcp_moments<true, false>, tlp_moments<true, false>, grid, a, live, s);
    } else {
        if (a.cross) launch_moments(wcp_moments<false, true>, tlp_moments<false, true>, grid, a, live, s);
        else launch_moments(wcp_moments<false, false>, tlp_moments<false, false>, grid, a, live, s);
    }
}

void launch_wcp_final(const WpArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(wcp_final, dim3((unsigned)a.t.nrows), dim3(MC_THREADS), 0, s, a);
}

void launch_tlt_levels(const TrArgs &a, double *wc, hipStream_t s) {
    hipLaunchKernelGGL(tlt_levels, dim3(1), dim3(MC_THREADS), 0, s, a, wc);
}

void launch_tlt_weights(const WtArgs &a, unsigned *live, hipStream_t s) {
    if (a.kc <= 0 || a.nrows <= 0) return;
    const long nb = (a.kc + MC_THREADS - 1) / MC_THREADS;
    hipLaunchKernelGGL(tlt_weights, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(MC_THREADS), 0, s, a, live);
}

void launch_ev_chunk(const EvArgs &a, hipStream_t s) {
    if (a.kc <= 0 || a.nrows <= 0 || a.n_event <= 0) return;
    const long nb = (((a.kc + 15) >> 4) + 3) >> 2;                    // four groups of sixteen rollouts per workgroup
    const dim3 ge((unsigned)(nb < 1024 ? nb : 1024));
    if (a.quad) hipLaunchKernelGGL(ev_eval<true>, ge, dim3(MC_THREADS), 0, s, a);
    else hipLaunchKernelGGL(ev_eval<false>, ge, dim3(MC_THREADS), 0, s, a);
    launch_ev_sums(a, s);
}

void launch_ev_argmax(const EvArgs &a, hipStream_t s) {
    if (a.kc <= 0 || a.n_event <= 0) return;
    const long nb = (((a.kc + 15) >> 4) + 3) >> 2;
    const dim3 ge((unsigned)(nb < 1024 ? nb : 1024));
    if (a.quad) hipLaunchKernelGGL((ev_eval<true, true>), ge, dim3(MC_THREADS), 0, s, a);
    else hipLaunchKernelGGL((ev_eval<false, true>), ge, dim3(MC_THREADS), 0, s, a);
}

void launch_ev_sums(const EvArgs &a, hipStream_t s) {
    if (a.kc <= 0 || a.nrows <= 0 || a.n_event <= 0) return;
    const int ny = (a.mask ? a.N + 1 : 0) + a.n_event + 1;
    const dim3 grid(EV_SLOTS, (unsigned)ny, (unsigned)((a.nrows + EV_ROWS - 1) / EV_ROWS));
    if (a.live) hipLaunchKernelGGL(tle_sums, grid, dim3(MC_THREADS), 0, s, a);
    else hipLaunchKernelGGL(ev_sums, grid, dim3(MC_THREADS), 0, s, a);
}

void launch_ev_final(const EvArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)(a.n_event + 1), (unsigned)a.nrows);
    if (a.tr) hipLaunchKernelGGL(tle_final, grid, dim3(MC_THREADS), 0, s, a);
    else hipLaunchKernelGGL(ev_final, grid, dim3(MC_THREADS), 0, s, a);
}

void launch_policy_mc(const McArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(mc_pass1, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, a);
    hipLaunchKernelGGL(mc_pass2, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, a);
    hipLaunchKernelGGL(mc_final, dim3(1), dim3(MC_THREADS), 0, s, a);
}

void launch_policy_tr(const TrArgs &a0, hipStream_t s) {
    TrArgs a = a0;
    McArgs m;
    memset(&m, 0, sizeof(m));
    m.cost = a.cost; m.K = a.K; m.scratch = a.scratch + TR_O_P1;
    hipLaunchKernelGGL(mc_pass1, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, m);
    (void)hipMemsetAsync(a.scratch + TR_O_HIST, 0, (size_t)TR_HIST_DOUBLES * sizeof(double), s);
    for (a.pass = 0; a.pass < TR_PASSES; ++a.pass) hipLaunchKernelGGL(tr_select, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, a);
    hipLaunchKernelGGL(tr_sums, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, a);
    hipLaunchKernelGGL(tr_rows, dim3(1), dim3(MC_THREADS), 0, s, a);
    if (a.weights) {
        const long nb = (a.K + MC_THREADS - 1) / MC_THREADS;
        hipLaunchKernelGGL(tr_weights, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(MC_THREADS), 0, s, a);
    }
}

void launch_policy_wc(const WcArgs &a0, hipStream_t s) {
    WcArgs a = a0;
    McArgs m;
    memset(&m, 0, sizeof(m));
    m.cost = a.cost; m.K = a.K; m.scratch = a.scratch + WC_O_P1;
    hipLaunchKernelGGL(mc_pass1, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, m);
    hipLaunchKernelGGL(wc_var, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, a);
    if (a.n_bound > 0)
        for (a.pass = 0; a.pass < WC_PASSES; ++a.pass) hipLaunchKernelGGL(wc_search, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, a);
    hipLaunchKernelGGL(wc_final, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, a);
    hipLaunchKernelGGL(wc_rows, dim3(1), dim3(MC_THREADS), 0, s, a);
    if (a.weights) {
        const long nb = (a.K + MC_THREADS - 1) / MC_THREADS;
        hipLaunchKernelGGL(wc_weights, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(MC_THREADS), 0, s, a);
    }
}
