// mc_tree.h -- the fixed reduction trees of the policy-assessment kernels (policy_mc.hip, rare_event.hip): one definition, so that every
// kernel that says "the same order" adds in the same order.  Device code only; MC_THREADS lanes per workgroup (policy_mc.h).
#pragma once
#include <hip/hip_runtime.h>

#include "policy_mc.h"

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

// block_tree<0> for NQ sums at once (the same additions in the same order, NQ per barrier): sh is [NQ][MC_THREADS]
template <int NQ>
__device__ __forceinline__ void block_tree_n(double (&v)[NQ], double *sh) {
    const int tid = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; ++q) sh[q * MC_THREADS + tid] = v[q];
    __syncthreads();
    for (int s = MC_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) sh[q * MC_THREADS + tid] = sh[q * MC_THREADS + tid] + sh[q * MC_THREADS + tid + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) v[q] = sh[q * MC_THREADS];
}
