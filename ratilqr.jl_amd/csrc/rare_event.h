// rare_event.h -- rat_policy_rare_event (include/ratilqr.h): the probability of a rare safety event by adaptive importance sampling, on the
// device (rare_event.hip).  The process noise of rollout i is drawn from a shifted proposal, z_k = s_k + xi_k, xi_k ~ N(0, I_n), the
// likelihood ratio rides along as logw_i = sum_k (-s_k' z_k + 1/2 s_k' s_k), and the shift s [N][n] is moved towards the event by the
// multilevel cross-entropy method.  One adaptation iteration is
//   re_rollout   K rollouts under s: margin M_i (rat_policy_events' M of one event), logw_i, the DomainError flag
//   the select   launch_policy_tr (policy_mc.hip) on the margins at alpha = 1 - rho: the ceil((1 - rho) n)-th smallest M, an exact order statistic
//   re_level     gamma = min(0, that M) and the iteration's code (0 go on, 1 gamma == 0, 2 no margin to rank, 3 not finite) -> device memory
//   re_pass_a    n_ok, n_domain, max and min logw                                        (only when the code is 0: the host reads its 4 bytes)
//   re_elite     replays the iteration's Philox stream: per step and component sum_E w_i xi_ik, and sum_E w_i, sum_E w_i^2, |E| over the elite
//                E = { M_i >= gamma }, w_i = exp(logw_i - max logw); gamma and max logw are read from device memory
//   re_update    the slots' partials in index order; s += sum_E w xi / sum_E w (= sum_E w z / sum_E w, z = s + xi); the trace row
// and the final pass is re_rollout on a stream of its own, re_pass_a, re_pass_b (sum_A w, sum_A w^2, N_VIOL over A = { M_i > 0 }) and re_final.
// Every sum runs in a fixed order (policy_mc.hip's: lane g of the grid takes elements g, g + T, ...; the LDS tree; the partials in the same
// tree or in index order at the head of the next launch); no floating-point atomics: the same call returns the same bits.
//
// Keying.  Pass p (the final pass is p = 0, adaptation iteration j is p = j + 1) has the seed seed_p = seed + RE_PASS_STRIDE p (mod 2^64);
// inside a pass the rollouts are keyed as rat_policy_evaluate keys them: chunks of min(K, 2^16) rollouts, chunk c under the Philox key
// seed_p + 0x9E3779B97F4A7C15 c, counter (index within the chunk, 0, t >> 1, component), one Box-Muller transform per step pair.  With
// n_iter == 0 and no shift the final pass therefore draws rat_policy_evaluate's noise at the same seed.
//
// rat_policy_rare_event_noise (a source model under its rat_user_noise) runs the same chain with two kernels of its own: the rollout is
// rat_src_rare_rollout (source_rare.h, a hiprtc module) and the elite sum re_elite_rng.  The shift is [N][P] in the same [N][12] layout,
// P = normals_per_step <= 12, entry (t, i) shifting the i-th rng.normal() of step t; ReArgs.pb.n holds P for re_elite_rng and re_update.
// Its passes have the same seeds seed_p; inside a pass the keying is rat_rng's: the global rollout index in the counter (g lo, g hi, t,
// i >> 1), key seed_p, no chunks -- rat_policy_evaluate_noise's generator at seed_p.
//
// rat_policy_rare_event_params is that call with the normals of rat_user_params shifted as well (source_params.h, RAT_PARAM_SHIFT): the shift
// table has a row N, entry i shifting the i-th parameter normal (ReArgs.pn of them, <= 12), and re_elite_rng has a row N that replays the
// parameter stream -- counter (g lo, g hi, 0xFFFFFFFF, i >> 1), key seed_p -- over the same elite with the same weights, into partials
// behind the three sums.  ReArgs.fix names the part the caller holds still (bit 0 the step rows, bit 1 the parameter row): re_elite_rng
// is launched for the rows that move, re_update checks and moves those alone -- one non-finite entry in either drops the whole update --
// and writes |ps| of the parameter row beside the trace.  With pn == 0 (every other call) no kernel reads row N or the new partials.
#pragma once
#include <hip/hip_runtime.h>

#include "layout.h"
#include "policy_mc.h"

#define RE_NSTAT 12           /* RAT_RE_NSTAT of the header */
#define RE_NTRACE 4           /* RAT_RE_NTRACE */
#define RE_MAX_ITER 32
#define RE_MAX_N 256          /* horizon the shift's LDS copy is sized for: [N][12] doubles beside the kernel's 22 KiB of staging */
#define RE_SLOTS 64           /* workgroups of re_elite per step pair: fixed, so that the summation order depends on K alone */
#define RE_PASS_STRIDE 0xD1B54A32D192ED03ull
#define RE_CHUNK_STRIDE 0x9E3779B97F4A7C15ull
// scratch, in doubles: pass A partials [4][B] | pass B partials [3][B] | stats [12] | level: gamma, - | control: code (int), bad (int) |
// trace [32][4] | the select's scratch [TR_SCRATCH] | |ps| per iteration [32]      (B = MC_BLOCKS)
#define RE_O_PA 0
#define RE_O_PB (4 * MC_BLOCKS)
#define RE_O_STATS (RE_O_PB + 3 * MC_BLOCKS)
#define RE_O_LVL (RE_O_STATS + RE_NSTAT)
#define RE_O_CTL (RE_O_LVL + 2)
#define RE_O_TRACE (RE_O_CTL + 2)
#define RE_O_TR (RE_O_TRACE + RE_MAX_ITER * RE_NTRACE)
#define RE_O_PTRACE (RE_O_TR + TR_SCRATCH)
#define RE_SCRATCH (RE_O_PTRACE + RE_MAX_ITER)

struct ReArgs {
    ProblemDev pb;
    const double *Wchol;      // [Nw][12][16] lower Cholesky factors of W(k), row-major, zero padded (rat_policy_evaluate's pack)
    const double *xnom;       // [(N+1)][12] (open loop: only row 0 is read)
    const double *l;          // [N][4]
    const double *L;          // [N][4][12] or null (open loop)
    long K, chunk;            // chunk = min(K, 2^16)
    unsigned long long seed;  // seed_p of this pass
    double *shift;            // [N][12] s, zero padded; [N + 1][12] with pn > 0: row N is the parameter shift
    const double *Qt;         // [16][16] in the tile as ev_eval reads it (entry (k, i) at k * 16 + i), or unused (linear event)
    const double *at;         // [16] in the tile
    double b;
    int t_lo, t_hi;
    double *margin;           // [K] M, NaN for a DomainError rollout
    double *logw;             // [K]
    int *dom;                 // [K]
    double *scratch;          // [RE_SCRATCH]
    double *part;             // [N * 12 + 3 + 12][RE_SLOTS] re_elite's partials: the step rows, sum w, sum w^2, |E|, the parameter row
    int iter;                 // adaptation iteration (re_level, re_update: the trace row)
    int reached;              // re_final: an iteration found gamma == 0
    int n_run;                // re_final: adaptation iterations that ran
    int pn;                   // rat_policy_rare_event_params: the parameter normals a rollout declares (the width of row N), else 0
    int fix;                  // with pn > 0: bit 0 the step rows, bit 1 the parameter row stay at their shift_in (0: everything is adapted)
};
void launch_re_rollout(const ReArgs &a, bool quad, hipStream_t s);
// the select on the margins and re_level behind it: the code is the int at a.scratch + RE_O_CTL
void launch_re_level(const ReArgs &a, double rho, hipStream_t s);
// re_pass_a, re_elite, re_update
void launch_re_adapt(const ReArgs &a, hipStream_t s);
// the same for rat_policy_rare_event_noise: re_pass_a, re_elite_rng (rat_rng's stream: pb.n holds P, the normals per step; seed is seed_p,
// Wchol / xnom / l / L / chunk are not read), re_update; with pn > 0 the rows of re_elite_rng that a.fix leaves to move
void launch_re_adapt_rng(const ReArgs &a, hipStream_t s);
// re_pass_a, re_pass_b, re_final: the stats are a.scratch + RE_O_STATS
void launch_re_final(const ReArgs &a, hipStream_t s);
