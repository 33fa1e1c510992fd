// policy_mc.h -- the statistics of rat_policy_evaluate (include/ratilqr.h), formed on the device from the K rollout costs (policy_mc.hip).
#pragma once
#include <hip/hip_runtime.h>

#define MC_BLOCKS 256         /* workgroups of the two passes: fixed, so that the summation order depends on K alone */
#define MC_THREADS 256        /* lanes per workgroup (== MC_BLOCKS: one lane per partial in the second level of the tree) */
#define MC_MAX_THETA 16
#define MC_P1 5               /* partials of pass 1: count, domain count, min, max, sum */
#define MC_P2 (1 + 2 * MC_MAX_THETA)   /* partials of pass 2: sum (J - mean)^2, then per theta sum d, sum d^2 */
#define MC_OUT (8 + 2 * MC_MAX_THETA)  /* results: stats[8] | risk[16] | risk_se[16] */
#define MC_SCRATCH ((MC_P1 + MC_P2) * MC_BLOCKS + MC_OUT)   /* doubles: part1 | part2 | out */

struct McArgs {
    double *cost;             // [K] rollout costs; pass 1 writes NaN where dom says DomainError
    const int *dom;           // [K] DomainError flags of the family kernels, or null (the cost is NaN already)
    long K;
    int n_theta;
    double theta[MC_MAX_THETA];
    double *scratch;          // [MC_SCRATCH]
};
// enqueues pass 1, pass 2 and the final reduction on s; the results are a.scratch + (MC_P1 + MC_P2) * MC_BLOCKS
void launch_policy_mc(const McArgs &a, hipStream_t s);
