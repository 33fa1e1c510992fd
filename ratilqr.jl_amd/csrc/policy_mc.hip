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

namespace {

__device__ __forceinline__ bool mc_nan(double v) { return v != v; }

// the fixed tree over the MC_THREADS values of a workgroup: OP 0 sum, 1 min, 2 max.  Every lane returns the result.
template <int OP>
__device__ __forceinline__ double block_tree(double v, double *sh) {
    const int tid = threadIdx.x;
    __syncthreads();                                                  // (sh may still be read from the previous tree)
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = MC_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const double a = sh[tid], b = sh[tid + s];
            sh[tid] = (OP == 0) ? a + b : (OP == 1) ? (b < a ? b : a) : (b > a ? b : a);
        }
        __syncthreads();
    }
    return sh[0];
}

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

}  // namespace

void launch_policy_mc(const McArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(mc_pass1, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, a);
    hipLaunchKernelGGL(mc_pass2, dim3(MC_BLOCKS), dim3(MC_THREADS), 0, s, a);
    hipLaunchKernelGGL(mc_final, dim3(1), dim3(MC_THREADS), 0, s, a);
}
