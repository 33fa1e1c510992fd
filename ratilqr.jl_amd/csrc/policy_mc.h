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

// ---- rat_policy_tail_risk: the alpha-quantile (value at risk) and the conditional value at risk of the K costs (policy_mc.hip) ------------
// A radix select for every level at once, 8 bits a pass: the key of a cost is its bit pattern made monotone (0 canonicalised; a negative
// cost ~bits, any other bits | 1 << 63), a level's state is the digits fixed so far and the rank that is left within them.
#define TR_MAX_ALPHA 16
#define TR_NSTAT 8            /* RAT_TR_NSTAT of the header */
#define TR_BITS 8             /* digit width: [16][256] u32 of LDS per workgroup, 256 bins a level for the head of the next launch to walk */
#define TR_BINS (1 << TR_BITS)
#define TR_PASSES (64 / TR_BITS)
#define TR_NSUM 4             /* sums per level of tr_sums: P1, P2, c_gt, c_eq */
#define TR_SROWS 8            /* levels tr_sums forms per sweep over the costs */
// scratch, in doubles: part1 [5][B] | sums' partials [16][4][B] | rows [16][8] | aux [8] | state [9][16] x (prefix u64, rank u32 | rep u32) |
// histograms [8][16][256] u32 (zeroed at the head of the chain; one set per pass, so no launch clears what another still reads)
#define TR_O_P1 0
#define TR_O_PS (MC_P1 * MC_BLOCKS)
#define TR_O_ROWS (TR_O_PS + TR_MAX_ALPHA * TR_NSUM * MC_BLOCKS)
#define TR_O_AUX (TR_O_ROWS + TR_MAX_ALPHA * TR_NSTAT)
#define TR_O_STATE (TR_O_AUX + 8)
#define TR_O_HIST (TR_O_STATE + (TR_PASSES + 1) * TR_MAX_ALPHA * 2)
#define TR_HIST_DOUBLES (TR_PASSES * TR_MAX_ALPHA * TR_BINS / 2)
#define TR_SCRATCH (TR_O_HIST + TR_HIST_DOUBLES)

struct TrArgs {
    double *cost;             // [K] costs, NaN for a DomainError rollout
    long K;
    int n_alpha;
    int pass;                 // digit pass of this launch (tr_select)
    double alpha[TR_MAX_ALPHA];
    double *scratch;          // [TR_SCRATCH]
    double *weights;          // [K] or null
};
// enqueues pass 1 (mc_pass1), the clearing of the histograms, TR_PASSES select passes, the sums, the rows and (a.weights) the weights on s;
// the rows are a.scratch + TR_O_ROWS
void launch_policy_tr(const TrArgs &a, hipStream_t s);

// ---- rat_policy_worst_case_trajectory: the mean and covariance of (x_t, u_t) under q and under p* ~ exp(theta* J) q (policy_mc.hip) --------
// Per step t and row r, about a centre c_t known before any rollout runs: S0 = sum y, S1 = sum y D, S2 = sum y D D' and sum y^2 over the
// rollouts, D = (x_t, u_t) - c_t in the 12 + 4 tile, y the row's weight of the rollout.  The trajectories are replayed a chunk at a time
// into staging buffers; behind each chunk wct_weights forms the weights (and counts replayed costs that differ from the stored ones) and
// wct_moments adds the chunk's sums into the partial of its workgroup; wct_final sums the partials in index order.
#define WT_SLOTS 8            /* workgroups per (step, row batch): fixed, so that the summation order depends on K alone */
#define WT_WAVES 4            /* wavefronts per workgroup; wavefront w of slot s takes the groups of four rollouts s * 4 + w, + 32, ... */
#define WT_ROWS 8             /* rows a workgroup accumulates (grid.z = row batches) */
#define WT_PART 288           /* doubles per partial: S2 [16][16] | S1 [16] | S0 | sum y^2 | padding */
#define WT_O_S1 256
#define WT_O_S0 272
#define WT_O_SY2 273
#define WT_MAX_ROWSTEPS 3640  /* rows x (N + 1) at most: the partials [rows][N+1][WT_SLOTS][WT_PART] stay below 64 MiB (30 MB: 32 rows, N = 50) */

struct WtArgs {
    const double *xs, *us;    // staged trajectories of the chunk: [kc][N+1][ldx], [kc][N][ldu]
    int ldx, ldu;
    int n, m, N;
    long kc;                  // rollouts of the chunk
    const double *cost;       // [kc] the stored costs of the chunk's rollouts (NaN: DomainError, selected out)
    const double *cost_re;    // [kc] the costs the replay formed
    const int *dom_re;        // [kc] the replay's DomainError flags, or null (its cost is NaN already)
    int nrows;
    const double *wc;         // launch_policy_wc's scratch: row info at WC_O_INFO, Jmax at WC_O_AUX + 2
    double *y;                // [nrows][ldy] weights of the chunk
    long ldy;
    const double *centre;     // [N+1][16]
    double *part;             // [nrows][N+1][WT_SLOTS][WT_PART]
    int *mismatch;            // replayed costs whose bits differ from the stored ones (NaN equals NaN)
    // wct_final only
    double *mean;             // [nrows][N+1][n+m]
    double *cov;              // [nrows][N+1][(n+m)^2] column-major
    double *ess;              // [nrows][2]: S0 and sum y^2 of step 0
    // tlt_weights only
    const double *sample;     // [kc] what the levels were selected on where that is not the costs (rat_policy_margin_gradient: an event's
                              // margins; NaN carries no weight), or null: cost.  The replay check is on cost either way
};
// c[t] = (x[t][0..n), u[t][0..m)) in the 12 + 4 tile, zero padded, zero where the source is not finite; x [N+1][12], u [N][4]
void launch_wct_centre(const double *x, const double *u, int n, int m, int N, double *centre, hipStream_t s);
// one chunk: the weights of its rollouts per row and the replay check (wct_weights; rat_policy_events forms its weights with it too) ...
void launch_wct_weights(const WtArgs &a, hipStream_t s);
// ... then, behind it, the chunk's sums into the partials.  live: the chunk's liveness words (launch_tlt_weights wrote them: the tail
// calls' schedule, below), or null for the dense schedule; launch_wcd_chunk and launch_wcp_chunk take it likewise
void launch_wct_chunk(const WtArgs &a, const unsigned *live, hipStream_t s);
void launch_wct_final(const WtArgs &a, hipStream_t s);

// ---- rat_policy_worst_case_disturbance: the mean and covariance of the disturbance w_t, and its covariance with (x_t, u_t) (policy_mc.hip) ----
// The trajectory call's replay with the rollouts keeping w_t as well (staged [kc][N][ldw]).  Per step t < N and row, about the centres
// c_w[t] and c_t: S0, S1w = sum y Dw, S1z = sum y Dz, S2ww = sum y Dw Dw', S2wz = sum y Dw Dz' and sum y^2, Dw = w_t - c_w[t] in lanes
// 0 .. 11 of the tile, Dz = (x_t, u_t) - c_t as wct_moments has it.  wcd_moments keeps wct_moments' schedule (WT_SLOTS, WT_WAVES, WT_ROWS)
// and issues one MFMA per product; wcd_final sums the slots in index order.  c_w[t] is the w_t of the first rollout of the first chunk
// whose stored cost is not NaN (0 where that is not finite, or where the chunk has none): wcd_centre, behind the first chunk's rollouts.
#define WD_PART 552           /* doubles per partial: S2ww [16][16] | S2wz [16][16] | S1w [16] | S1z [16] | S0 | sum y^2 | padding */
#define WD_O_WZ 256
#define WD_O_S1W 512
#define WD_O_S1Z 528
#define WD_O_S0 544
#define WD_O_SY2 545
#define WD_MAX_ROWSTEPS 1899  /* rows x N at most: the partials [rows][N][WT_SLOTS][WD_PART] stay below 64 MiB (56.5 MB: 32 rows, N = 50) */

struct WdArgs {
    WtArgs t;                 // the replay's fields as wct_weights fills them, and centre = c_t [N+1][16]; part, mean, cov, ess are not read
    const double *ws;         // [kc][N][ldw] the staged disturbances of the chunk
    int ldw;
    int cross;                // S2wz and S1z are wanted
    double *cw;               // [N][16] c_w, zero padded
    double *part;             // [nrows][N][WT_SLOTS][WD_PART]
    // wcd_final only
    double *mean_w;           // [nrows][N][n]
    double *cov_w;            // [nrows][N][n^2] column-major
    double *cov_wz;           // [nrows][N][n (n+m)] column-major, or null
    double *ess;              // [nrows][2]: S0 and sum y^2 of step 0
};
// c_w from the first chunk (a.t.kc, a.t.cost, a.ws): behind that chunk's rollouts, before its sums
void launch_wcd_centre(const WdArgs &a, hipStream_t s);
// one chunk, behind launch_wct_weights: the chunk's sums into the partials
void launch_wcd_chunk(const WdArgs &a, const unsigned *live, hipStream_t s);
void launch_wcd_final(const WdArgs &a, hipStream_t s);

// ---- rat_policy_worst_case_params: the mean and covariance of the rollouts' drawn parameters q, and their covariance with the cost ---------
// The trajectory call's replay; behind each chunk the SRC_PARAMS kernel forms the chunk's q again (staged [kc][P], P = n_params <= 32) and
// wcp_moments adds, per row and about the centres c_q and c_J: S0, sum y^2, S1 = sum y Dq, S2 = sum y Dq Dq' and, with the cost sums,
// sum y DJ, sum y DJ^2 and sum y DJ Dq; Dq = q - c_q in two tiles of sixteen lanes, DJ = J - c_J.  wcp_moments keeps wct_moments' schedule
// (WT_SLOTS, WT_WAVES, WT_ROWS) with one step: one MFMA per group and row for P <= 16, three -- the blocks (0,0), (0,1), (1,1) of S2 --
// above; wcp_final sums the slots in index order and mirrors block (1,0).  c_q and c_J are the q and the cost of the first rollout of the
// first chunk whose stored cost is not NaN (0 where that is not finite, or where the chunk has none): wcp_centre, behind the first
// chunk's q, as wcd_centre.  The partials [rows <= 32][WT_SLOTS][WP_PART] are 1.7 MB at most: no cap on the rows beyond WC_MAX_ROWS.
#define WP_MAXP 32            /* parameters at most (source_params.h) */
#define WP_PART 840           /* doubles per partial: S2 blocks (0,0) | (0,1) | (1,1), [16][16] each | S1 [32] | SJq [32] | S0 | sum y^2 | SJ | SJ2 | padding */
#define WP_O_S1 768
#define WP_O_SJQ 800
#define WP_O_S0 832
#define WP_O_SY2 833
#define WP_O_SJ 834
#define WP_O_SJ2 835
#define WP_NCENTRE 40         /* doubles of the centre: c_q [32] | c_J | padding */

struct WpArgs {
    WtArgs t;                 // the replay's fields as wct_weights fills them (kc, cost, y, ldy, nrows, wc); the trajectory fields are not read
    const double *qs;         // [kc][P] the staged parameters of the chunk
    int P;
    int cross;                // the cost sums are wanted
    double *centre;           // [WP_NCENTRE]
    double *part;             // [nrows][WT_SLOTS][WP_PART]
    // wcp_final only
    double *mean_q;           // [nrows][P]
    double *cov_q;            // [nrows][P^2] column-major
    double *cov_qJ;           // [nrows][P], or null
    double *ess;              // [nrows][4]: S0, sum y^2, and with the cost sums the mean and variance of J the moment kernel finds
};
// the centres from the first chunk (a.t.kc, a.t.cost, a.qs): behind that chunk's q, before its sums
void launch_wcp_centre(const WpArgs &a, hipStream_t s);
// one chunk, behind launch_wct_weights and the chunk's q: the chunk's sums into the partials
void launch_wcp_chunk(const WpArgs &a, const unsigned *live, hipStream_t s);
void launch_wcp_final(const WpArgs &a, hipStream_t s);

// ---- rat_policy_tail_trajectory / _disturbance / _params: the same moments under the CVaR adversary, one row per level (policy_mc.hip) ------
// The rows are rat_policy_tail_risk's (launch_policy_tr on the stored costs); the weights are tr_weights' rule up to the common factor
// 1 / tail, which the moment kernels divide out through S0: y = 1 above the level's quantile v, y_eq on it, 0 below and for a DomainError
// rollout.  tlt_levels, behind the tail-risk chain, writes every level's (v, y_eq, state) where the worst-case kernels keep a row's
// (theta, state) -- a scratch of launch_policy_wc's size, WtArgs::wc -- so that wct_final / wcd_final / wcp_final serve unchanged; a level
// thinner than one rollout is v = Jmax, y_eq = 1.  tlt_weights is wct_weights' counterpart and also writes, per group of four rollouts,
// one word whose bit r says "some y of level r in this group is not zero".  tlt_moments / tld_moments / tlp_moments are wct_moments /
// wcd_moments / wcp_moments with that word read first (one body, moments_body, serves all six; TAIL is a template argument): a
// wavefront issues nothing for a row its group is dead in, loads nothing for a group dead in every row of the workgroup, and selects a
// rollout without weight in a row out of that row's operands.  Adding 0 D to a sum changes no bit where D is finite, so on finite data
// the two schedules agree bit for bit; a rollout without weight that holds Inf or NaN is left out, where the dense schedule forms 0 Inf.
#define TL_O_YEQ WC_O_ROWS    /* y_eq of level r at wc[TL_O_YEQ + r]; v and the state at wc[WC_O_INFO + 2 r], + 1 (WC_ST_SEARCH: live) */
// behind launch_policy_tr(a, s): the levels of a (its scratch) into wc [WC_SCRATCH]
void launch_tlt_levels(const TrArgs &a, double *wc, hipStream_t s);
// one chunk: the weights of its rollouts per level, the replay check and the liveness words live [(kc + 3) / 4] (a.wc: tlt_levels' output)
void launch_tlt_weights(const WtArgs &a, unsigned *live, hipStream_t s);
// ... then, behind it, the chunk's sums into the partials: launch_wct_chunk / launch_wcd_chunk / launch_wcp_chunk with live

// ---- rat_policy_gradient / rat_policy_tail_gradient: the gradient of a row's functional with respect to the policy (policy_mc.hip) ---------
// The trajectory call's replay; behind each chunk rat_src_adjoint (source_adjoint.h, kind SRC_ADJOINT) writes gu_t = dJ_k / du_t of every
// rollout (staged [kc][N][4]) and its flag bad [kc] (a cost, but a NaN or Inf in the sensitivities), and pg_moments adds, per step t < N and
// row: one tile sum y G Dx' -- G = gu_t in lanes 12 .. 15, Dx = x_t - x_nom_t in lanes 0 .. 11 (zeros open loop), so rows 12 .. 15,
// columns 0 .. 11 of the tile are dJ / dL_t -- the per-lane sums sum y G, sum y^2 G, sum y^2 G^2, and per rollout lane sum y and sum y^2
// over the rollouts whose sensitivities are finite.  A flagged rollout is selected out of all of these (both operands of the product
// included), never multiplied; the skeleton's own S0 and sum y^2 still count it.  pg_moments keeps wct_moments' schedule (WT_SLOTS,
// WT_WAVES, WT_ROWS; dense, or the tail calls' liveness schedule); pg_final sums the slots in index order.
#define PG_PART 312           /* doubles per partial: sum y G Dx' [16][16] | sum y G [16] | sum y^2 G [16] | sum y^2 G^2 [16] | S0 | sum y^2 | the two over finite rollouts | padding */
#define PG_O_V1 256
#define PG_O_V2 272
#define PG_O_V3 288
#define PG_O_S0 304
#define PG_O_SY2 305
#define PG_O_SF 306
#define PG_O_SF2 307
#define PG_MAX_ROWSTEPS 3360  /* rows x N at most: the partials [rows][N][WT_SLOTS][PG_PART] stay below 64 MiB (31.9 MB: 32 rows, N = 50) */

struct PgArgs {
    WtArgs t;                 // the replay's fields as wct_weights fills them (xs, ldx, kc, cost, y, ldy, nrows, wc, n, m, N); centre, part, mean, cov, ess are not read
    const double *gu;         // the staged adjoints of the chunk: gu_t of rollout q at gu + q ldg + 4 t
    long ldg;                 // doubles between rollouts: 4 N ([kc][N][4]), or more where the adjoint kernel interleaves several sweeps
    const int *bad;           // [kc] the chunk's non-finite flags
    const double *xnom;       // [N+1][12] the pack's nominal states, or null (open loop: no dJ / dL)
    double *part;             // [nrows][N][WT_SLOTS][PG_PART]
    // pg_final only
    double *grad_l;           // [nrows][N][m]
    double *grad_L;           // [nrows][N][m n] column-major m x n per step (zeros open loop)
    double *grad_l_se;        // [nrows][N][m]
    double *ess;              // [nrows][2]: S0 and sum y^2 of step 0
};
// one chunk, behind launch_wct_weights / launch_tlt_weights and the chunk's adjoints: the chunk's sums into the partials
void launch_pg_chunk(const PgArgs &a, const unsigned *live, hipStream_t s);
void launch_pg_final(const PgArgs &a, hipStream_t s);

// ---- rat_policy_param_gradient / rat_policy_tail_param_gradient: the gradient of a row's functional with respect to the model's parameters
// and the initial state (policy_mc.hip) ---------------------------------------------------------------------------------------------------
// The trajectory call's replay; behind each chunk rat_src_adjoint_p (source_adjoint_params.h, kind SRC_ADJOINT_P) writes per rollout
// gp = dJ_k / dp ([kc][32], zero padded), lam0 = dJ_k / dx_0 ([kc][12], zero padded) and its flag bad [kc], and ppg_moments adds, per row,
// the per-lane sums sum y v, sum y^2 v, sum y^2 v^2 of the three components a lane holds -- gp_i, gp_{16 + i} (TWO: more than sixteen
// parameters) and lam0_i -- and per rollout lane sum y and sum y^2 over the rollouts whose sensitivities are finite.  A flagged rollout
// is selected out at the load; the skeleton's own S0 and sum y^2 still count it.  A payload of moments_body without a C tile (no product
// of two deviations is asked for): wcp_moments' one-step schedule (WT_SLOTS, WT_WAVES, WT_ROWS; dense, or the tail calls' liveness
// schedule); ppg_final sums the slots in index order.
#define PPG_PART 152          /* doubles per partial: 9 vectors [16] (component c, sum k at (3 c + k) * 16) | S0 | sum y^2 | the two over finite rollouts | padding */
#define PPG_O_S0 144
#define PPG_O_SY2 145
#define PPG_O_SF 146
#define PPG_O_SF2 147

struct PpgArgs {
    WtArgs t;                 // the replay's fields as wct_weights fills them (kc, cost, y, ldy, nrows, wc, n); the rest is not read
    const double *gp;         // [kc][32] the staged parameter sensitivities of the chunk
    const double *lam0;       // [kc][12] the staged initial-state sensitivities
    const int *bad;           // [kc] the chunk's non-finite flags
    int P;                    // parameters, 0 .. 32
    double *part;             // [nrows][WT_SLOTS][PPG_PART]
    // ppg_final only
    double *grad_p, *grad_p_se;     // [nrows][P]
    double *grad_x0, *grad_x0_se;   // [nrows][n]
    double *ess;              // [nrows][2]: S0 and sum y^2
};
// one chunk, behind launch_wct_weights / launch_tlt_weights and the chunk's adjoints: the chunk's sums into the partials
void launch_ppg_chunk(const PpgArgs &a, const unsigned *live, hipStream_t s);
void launch_ppg_final(const PpgArgs &a, hipStream_t s);

// ---- rat_policy_events: how often a policy violates quadratic constraints, under q and under every row's tilt (policy_mc.hip) ---------------
// An event is g(t, z) = z' Q z + a' z + b of z = (x_t, u_t) in the 12 + 4 tile, watched over the steps t_lo .. t_hi.  Behind each replayed
// chunk (after wct_weights) ev_eval forms, per rollout and event, the margin M = max g over the window, the first step tau with g > 0 and
// the per-step indicators -- sixteen rollouts as the columns of Q Z, four 16 x 16 x 4 MFMAs per event and step -- and ev_sums adds the
// weighted indicator sums into the partial of its workgroup; ev_final sums the partials in index order.  Event n_event is "any": the
// union of the given ones.
#define EV_MAX 16             /* events a call gives; EV_MAX + 1 with "any" */
#define EV_NSTAT 8            /* RAT_EV_NSTAT of the header */
#define EV_SLOTS 8            /* workgroups per step / per event and row batch: fixed, so that the summation order depends on K alone */
#define EV_ROWS 4             /* rows a workgroup accumulates (grid.z = row batches) */
#define EV_NSUM 6             /* sums per row of an event's block: y | y A | y^2 A | y^2 (1 - A) | y M | y A tau */
#define EV_PART 72            /* doubles per partial: a step's [EV_ROWS][EV_MAX + 1] indicator sums, or an event's [EV_ROWS][EV_NSUM] | N_VIOL | N_OK | max M */
#define EV_O_NVIOL (EV_ROWS * EV_NSUM)
#define EV_O_NOK (EV_O_NVIOL + 1)
#define EV_O_MMAX (EV_O_NVIOL + 2)
#define EV_MAX_PART_BYTES (64l << 20)   /* the partials [row batches][steps + events][EV_SLOTS][EV_PART] stay below this, as WT_MAX_ROWSTEPS keeps the moments' */

struct EvArgs {
    const double *xs, *us;    // staged trajectories of the chunk: [kc][N+1][ldx], [kc][N][ldu]
    int ldx, ldu;
    int n, m, N;
    long kc;                  // rollouts of the chunk
    const double *cost;       // [kc] the stored costs of the chunk's rollouts (NaN: DomainError, selected out)
    int n_event;
    int quad;                 // 0: every event is linear (Q == NULL): no matrix product
    const double *Qt;         // [n_event][16][16] in the tile, entry (k, i) at k * 16 + i: Q_i's row i, column k (quad only)
    const double *at;         // [n_event][16] in the tile
    const double *b;          // [n_event]
    const int *win;           // [n_event][2]: t_lo, t_hi
    double *margin;           // [n_event + 1][ldy] M of the chunk's rollouts, NaN for a DomainError rollout
    int *tau;                 // [n_event + 1][ldy] first violating step, -1: none
    unsigned *mask;           // [N+1][ldy] bit i: event i is in its window and g_i > 0 at that step; or null (no per-step sums)
    long ldy;
    int nrows;
    const double *y;          // [nrows][ldy] weights of the chunk (wct_weights)
    int first;                // this is the call's first chunk: the partials are set, not added to
    double *part;             // [row batches][nsteps + n_event + 1][EV_SLOTS][EV_PART], nsteps = mask ? N + 1 : 0
    // ev_final only
    const double *wc;         // launch_policy_wc's scratch: the rows' states at WC_O_INFO
    double *event_out;        // [nrows][n_event + 1][EV_NSTAT]; slot 6 holds N_OK (the host forms PROB_ROBUST from it)
    double *step_out;         // [nrows][n_event + 1][N+1] (with mask)
    // rat_policy_tail_events only (null otherwise)
    const unsigned *live;     // the chunk's liveness words (launch_tlt_weights): launch_ev_sums enqueues tle_sums in place of ev_sums
    const double *tr;         // launch_policy_tr's rows [nrows][TR_NSTAT]: launch_ev_final enqueues tle_final in place of ev_final
    // launch_ev_argmax only (null otherwise)
    int *tstar;               // [n_event][ldy] the first step of the window that attains the margin, -1 where the margin is NaN
};
// one chunk, behind launch_wct_weights: the events of the staged trajectories, then the chunk's sums into the partials
void launch_ev_chunk(const EvArgs &a, hipStream_t s);
// the second half of launch_ev_chunk alone (ev_sums), behind another kernel that wrote margin, tau and mask as ev_eval writes them
// (rat_policy_events_user: rat_src_user_events of source_events.h); xs, us, Qt, at, b, win are not read
void launch_ev_sums(const EvArgs &a, hipStream_t s);
void launch_ev_final(const EvArgs &a, hipStream_t s);
// ev_eval's sibling for rat_policy_margin_gradient: the same kernel text, so the same g and the same margins bit for bit, which also keeps
// the step at which the running margin was last replaced -- only a strictly greater g replaces it, so that is the FIRST step attaining the
// maximum -- and writes margin [n_event][ldy] and tstar alone (no "any" row, no tau, no mask, no sums behind it); cost, xs, us, Qt, at, b,
// win as launch_ev_chunk reads them
void launch_ev_argmax(const EvArgs &a, hipStream_t s);

// ---- rat_policy_tail_events / _user: the same event sums under the CVaR adversary, one row per level (policy_mc.hip) ----------------------------
// The rows, the weights y (1 above the level's quantile, y_eq on it, 0 below and for a DomainError rollout; ev_final's ratios divide the
// common factor 1 / tail out) and the liveness words are the tail calls' above: launch_policy_tr, launch_tlt_levels, launch_tlt_weights.
// With EvArgs::live set launch_ev_sums enqueues tle_sums: ev_sums' lanes, rollouts, trees and partials (EV_PART, EV_SLOTS) with the
// group's word read first.  A step's workgroup loads nothing for a group without weight in any of its rows, or for a rollout whose
// indicator bits are all clear at that step; an event's workgroup reads cost, margin and tau of every rollout (N_VIOL, N_OK and the
// largest margin are unweighted) and the weights of the rows the group is live in; a rollout without weight in a row is selected out of
// that row's y M.  Adding 0 to a sum changes no bit, so the partials are ev_sums' on the same weights bit for bit, but for a rollout
// without weight whose margin is NaN (every g of its window NaN), which ev_sums carries into MARGIN_MEAN as 0 NaN.  With live null (the
// switch tail_dense) ev_sums itself runs on the tail weights.  With EvArgs::tr set launch_ev_final enqueues tle_final: ev_final with
// FLAG the level's RAT_TR_FLAG and PROB_ROBUST = min(1, (N_VIOL / N_OK) / (TAIL_N / N_OK)) formed in place (never below PROB: where every
// violator lies in the tail the two are the same number, sum y A / sum y and the quotient of the counts, and their roundings may differ
// in the last bit; PROB is returned then).

// ---- rat_policy_sobol: first-order and total Sobol indices of the cost from pick-freeze rollouts (policy_mc.hip) ------------------------------
// Y [d + 2][ldy]: rows A, B and the d groups' AB_i, written by rat_src_sobol_rollout (source_sobol.h).  A base sample is OK when none of
// its d + 2 costs is NaN.  The partials are [2 + 8 d][MC_BLOCKS] doubles, 0.27 MB at d = 16: far below the 64 MiB the other analyses cap
// theirs at, so the call has no cap of that kind; what grows with K is Y itself, which the host bounds (driver.cpp).
#define SB_MAX_GROUPS 16
#define SB_NSUM 8             /* sums per group of sb_pass2: s, s^2, ns, ns^2, ns s, nt, nt^2, nt s */
#define SB_NSTAT 8            /* RAT_SB_NSTAT of the header */
#define SB_FLAG_DEGENERATE 16 /* RAT_SB_DEGENERATE of the header */
// scratch, in doubles: part1 [2][B] | part2 [16][8][B] | summary [8] | rows [16][4]
#define SB_O_P1 0
#define SB_O_P2 (2 * MC_BLOCKS)
#define SB_O_OUT (SB_O_P2 + SB_MAX_GROUPS * SB_NSUM * MC_BLOCKS)
#define SB_O_ROWS (SB_O_OUT + SB_NSTAT)
#define SB_SCRATCH (SB_O_ROWS + SB_MAX_GROUPS * 4)

struct SbArgs {
    const double *y;          // [d + 2][ldy] costs, NaN for a DomainError rollout
    long ldy;
    long K;                   // base samples
    int d;                    // groups, 1 .. SB_MAX_GROUPS
    int *ok;                  // [K] sb_pass1 writes 1 where the base sample is OK
    double *scratch;          // [SB_SCRATCH]
};
// enqueues sb_pass1, sb_pass2 and sb_final on s; the summary is a.scratch + SB_O_OUT, the rows [d][4] a.scratch + SB_O_ROWS
void launch_policy_sobol(const SbArgs &a, hipStream_t s);
