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

// ---- rat_policy_worst_case: sup { E_p[J] : KL(p || q) <= d } on the K costs, by the one-dimensional dual (policy_mc.hip) -----------------
#define WC_NPT 16             /* theta points a search pass evaluates per bound */
#define WC_MAX_BOUND 16
#define WC_MAX_ROWS 32        /* bound rows, then theta rows */
#define WC_NSTAT 8            /* RAT_WC_NSTAT of the header */
#define WC_GEO_BELOW 7        /* pass 0: theta_0 4^(j - 7), j = 0 .. 15; the top point theta_0 4^8 is theta_top */
#define WC_LINEAR_PASSES 11   /* passes 1 .. 11: 17-section of the bracket; 3 / 17^11 = 8.8e-14 relative */
#define WC_PASSES (1 + WC_LINEAR_PASSES)
#define WC_CENTRE_MAX 32.0    /* sums are centred about the mean while theta (Jmax - mean) <= this, about Jmax beyond */
#define WC_THETA_CAP 1e300    /* grid points are capped here: theta (J - Jmax) stays 0, not NaN, at J == Jmax */
#define WC_FROWS 8            /* rows the final sums form per sweep over the costs */
// states of a bound's search (doubles in the scratch, like everything there)
#define WC_ST_SEARCH 0.0
#define WC_ST_ZERO 1.0        /* d == 0 (or a theta row's theta == 0): the plain mean */
#define WC_ST_SAT 2.0
#define WC_ST_EMPTY 3.0
#define WC_ST_NONFINITE 4.0
// scratch, in doubles: part1 [5][B] | var [2][B] | bracket [2][16][4] | search partials [2][16][32][B] | final partials [32][5][B] |
// row info [32][2] | rows [32][8] | aux [8]        (B = MC_BLOCKS; the brackets and the search partials alternate between passes)
#define WC_O_P1 0
#define WC_O_PV (MC_P1 * MC_BLOCKS)
#define WC_O_BRK (WC_O_PV + 2 * MC_BLOCKS)
#define WC_O_PS (WC_O_BRK + 2 * WC_MAX_BOUND * 4)
#define WC_PS_SET (WC_MAX_BOUND * 2 * WC_NPT * MC_BLOCKS)
#define WC_O_PF (WC_O_PS + 2 * WC_PS_SET)
#define WC_NFIN 5              /* sums per row of the final pass */
#define WC_O_INFO (WC_O_PF + WC_MAX_ROWS * WC_NFIN * MC_BLOCKS)
#define WC_O_ROWS (WC_O_INFO + WC_MAX_ROWS * 2)
#define WC_O_AUX (WC_O_ROWS + WC_MAX_ROWS * WC_NSTAT)
#define WC_SCRATCH (WC_O_AUX + 8)

struct WcArgs {
    double *cost;             // [K] costs, NaN for a DomainError rollout
    long K;
    int n_bound, n_theta;
    int pass;                 // search pass of this launch (wc_search)
    double bound[WC_MAX_BOUND];
    double theta[MC_MAX_THETA];
    double *scratch;          // [WC_SCRATCH]
    double *weights;          // [K] or null
};
// enqueues pass 1 (mc_pass1), the variance pass, WC_PASSES search passes, the final sums, the rows and (a.weights) the weights on s;
// the rows are a.scratch + WC_O_ROWS
void launch_policy_wc(const WcArgs &a, hipStream_t s);
