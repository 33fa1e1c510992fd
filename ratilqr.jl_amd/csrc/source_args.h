// source_args.h -- argument blocks of the runtime-compiled model kernels (source_kernels.h), shared with the host driver.
// No HIP include here: under hiprtc <hip/hip_runtime.h> is not found, so the JIT side reaches these definitions through this header and
// layout.h alone.
#pragma once
#include "layout.h"

#define SRC_MAX_N 12          /* the 12 + 4 tile of layout.h */
#define SRC_MAX_M 4
#define SRC_LIN_WAVES 4       /* time steps (waves) per workgroup of rat_src_linearize */

// rat_src_rollout: simulate_dynamics (ileqg.jl:18-38, :62-87), one lane per trajectory
struct SrcRollArgs {
    StateDev st;
    OptsDev op;
    int mode;                 // 0 open loop from (x0, u0) into the nominal slots; 1 closed-loop line-search candidates (what rollout_kernel does)
    int tpw;                  // trajectories per wavefront (lanes 0 .. tpw-1 of each 64-lane workgroup work)
    const double *x0;         // [12]
    const double *u0;         // [N*4]
    const double *p;          // the model's parameters
};

// rat_src_linearize: approximate_model (ileqg.jl:258-322), one wavefront per (trajectory, t), t = N the terminal tile
struct SrcLinArgs {
    StateDev st;
    int mode;                 // 0 nominal slots, 1 candidate slots
    const double *p;
};

// rat_src_pets_rollout (source_pets.h): compute_cost_worker (pets.jl:76-98) of a generative source model, one lane per trajectory
struct SrcPetsArgs {
    const double *x0;         // [12]
    const double *controls;   // [S][N][USTR] padded
    long S, K;
    int N, use_true;
    int tpw;                  // trajectories per wavefront (lanes 0 .. tpw-1 of each 64-lane workgroup work)
    const double *zn, *zu;    // injected draws ([S*K][N][normals], [S*K][N][uniforms]) or both null (Philox keyed by seed)
    unsigned long long seed;
    long traj0;               // global index of this launch's first trajectory (the generator's counter)
    double *traj_cost;        // [S*K]
    const double *p;          // the model's parameters
    int *overdraw;            // set (plain store) when a step draws more than it declared: 1 normals, 2 uniforms
};

// rat_src_noisy_rollout (source_noisy.h): simulate_dynamics with rng (ileqg.jl:44-55, :94-109) + integrate_cost (:115-124) of a source
// model, one lane per Monte-Carlo rollout (rat_policy_evaluate)
struct SrcNoisyArgs {
    const double *Wchol;      // [Nw][12][16] lower Cholesky factors of W(k), row-major, zero padded
    const double *xnom;       // [(N+1)][12] nominal states (open loop: only row 0 is read)
    const double *l;          // [N][4]
    const double *L;          // [N][4][12] or null (open loop)
    const double *z;          // [K][N][n] injected N(0,1) draws or null (Philox keyed by seed)
    long K;
    int N, W_tv;
    int tpw;                  // rollouts per wavefront (lanes 0 .. tpw-1 of each 64-lane workgroup work)
    unsigned long long seed;
    double *cost;             // [K]; NaN where the rollout hit a DomainError
    const double *p;          // the model's parameters
};

// rat_src_user_noisy_rollout (source_user_noise.h): rat_src_noisy_rollout with the disturbance drawn by the user's rat_user_noise from a
// rat_rng, one lane per Monte-Carlo rollout (rat_policy_evaluate_noise)
struct SrcUserNoisyArgs {
    const double *xnom;       // [(N+1)][12] nominal states (open loop: only row 0 is read)
    const double *l;          // [N][4]
    const double *L;          // [N][4][12] or null (open loop)
    const double *zn, *zu;    // injected draws of this launch ([K][N][normals], [K][N][uniforms]) or both null (Philox keyed by seed)
    long K;                   // rollouts of this launch
    long j0;                  // global index of this launch's first rollout (the generator's counter)
    int N;
    int tpw;                  // rollouts per wavefront (lanes 0 .. tpw-1 of each 64-lane workgroup work)
    unsigned long long seed;
    double *cost;             // [K]; NaN where the rollout hit a DomainError
    double *x_out;            // [K][N+1][n] dense, or null
    double *u_out;            // [K][N][m] dense, or null
    const double *p;          // the model's parameters
    int *overdraw;            // set (plain store) when a step draws more than was declared: 1 normals, 2 uniforms
    double *w_out;            // [K][N][n] dense: what rat_user_noise wrote at every step, or null (rat_policy_worst_case_disturbance's replay)
    const double *zpn, *zpu;  // RAT_USER_PARAMS_ON alone (source_params.h): the handle's injected parameter draws, whole ([K_injected][param
                              // normals], [K_injected][param uniforms], indexed by j + j0), or both null (Philox keyed by seed).  Not read otherwise
};

// rat_src_rare_rollout (source_rare.h): rat_src_user_noisy_rollout under a shifted proposal on rng.normal(), with the margin of one event
// in place of the trajectory and the cost (rat_policy_rare_event_noise); the generator only
struct SrcRareArgs {
    const double *xnom;       // [(N+1)][12] nominal states (open loop: only row 0 is read)
    const double *l;          // [N][4]
    const double *L;          // [N][4][12] or null (open loop)
    const double *shift;      // [N][12] s, zero padded: entry i of row t shifts the i-th normal of step t; a module compiled with
                              // RAT_PARAM_SHIFT reads a row N as well: entry i shifts the i-th parameter normal
    const double *Qt;         // [16][16] in the tile as ev_eval reads it, or unused (quad == 0)
    const double *at;         // [16] in the tile
    double b;
    int t_lo, t_hi;
    int quad;                 // the event has a matrix
    long K;
    int N;
    int tpw;                  // rollouts per wavefront (lanes 0 .. tpw-1 of each 64-lane workgroup carry one)
    unsigned long long seed;  // seed_p of this pass: the Philox key; the global rollout index is the counter
    double *margin;           // [K] M, NaN for a DomainError rollout
    double *logw;             // [K]
    int *dom;                 // [K]
    const double *p;          // the model's parameters
    int *overdraw;            // set (plain store) when a step draws more than was declared: 1 normals, 2 uniforms
    int event;                // the RAT_RARE_USER_EVENT variant (rat_policy_rare_event_user): the entry of rat_user_event's g that is the
                              // margin's event; Qt, at, b, quad are not read there and the window is 0 .. N.  Not read otherwise
    const double *zpn, *zpu;  // RAT_USER_PARAMS_ON alone: as SrcUserNoisyArgs' (the rollout index is global here: one launch per pass)
};

// rat_src_user_events (source_events.h): ev_eval (policy_mc.hip) for the user's rat_user_event on the staged trajectories of one replayed
// chunk, one lane per rollout (rat_policy_events_user); the outputs are ev_eval's, so that ev_sums and ev_final run behind it unchanged
struct SrcEventArgs {
    const double *xs, *us;    // staged trajectories of the chunk: [kc][N+1][ldx], [kc][N][ldu]
    int ldx, ldu;
    int N;
    long kc;                  // rollouts of the chunk
    const double *cost;       // [kc] the stored costs of the chunk's rollouts (NaN: DomainError, selected out)
    double *margin;           // [RAT_N_EVENT + 1][ldy] M of the chunk's rollouts, NaN for a DomainError rollout; the last row is "any"
    int *tau;                 // [RAT_N_EVENT + 1][ldy] first violating step, -1: none
    unsigned *mask;           // [N+1][ldy] bit i: g_i > 0 at that step, bit RAT_N_EVENT: any of them; or null (no per-step sums)
    long ldy;
    const double *p;          // the model's parameters
    const double *zpn, *zpu;  // RAT_USER_PARAMS_ON alone: as SrcUserNoisyArgs', with the seed and the global index of the chunk's first rollout
    unsigned long long seed;  // of the replayed evaluation, from which the kernel forms every rollout's parameters again
    long j0;
};

// rat_src_params_sample (source_params.h): rat_user_params alone for rollouts 0 .. K - 1 (rat_policy_params_sample)
struct SrcParamsArgs {
    const double *p;          // the model's nominal parameters
    const double *zpn, *zpu;  // the handle's injected parameter draws, or both null (Philox keyed by seed)
    unsigned long long seed;
    long K;                   // rollouts of this launch
    long j0;                  // global index of this launch's first rollout
    double *q_out;            // [K][RAT_N_PARAMS]
    int *overdraw;            // set (plain store) when the hook draws more than was declared: 4 normals, 8 uniforms
};

// rat_src_sobol_rollout (source_sobol.h): rat_src_user_noisy_rollout's rollout for every (base sample, variant) of rat_policy_sobol, the
// generator only; variant blockIdx.y draws what its masks name from the stream of seed_b and everything else from the stream of seed_a
#define SOBOL_MAX_GROUPS 16
#define SOBOL_MAX_VAR (SOBOL_MAX_GROUPS + 2)   /* A (no bit set), B (every bit set), then the groups */
struct SrcSobolArgs {
    const double *xnom;       // [(N+1)][12] nominal states (open loop: only row 0 is read)
    const double *l;          // [N][4]
    const double *L;          // [N][4][12] or null (open loop)
    long K;                   // base samples of this launch
    long j0;                  // global index of this launch's first base sample (the generator's counter)
    int N;
    int tpw;                  // rollouts per wavefront (lanes 0 .. tpw-1 of each 64-lane workgroup work)
    unsigned long long seed_a, seed_b;
    double *y;                // row v of the costs at y + v ldy, [K] each; NaN where the rollout hit a DomainError
    long ldy;
    const double *p;          // the model's parameters
    int *overdraw;            // set (plain store) as rat_src_user_noisy_rollout sets it: 1, 2 a step's normals / uniforms, 4, 8 the hook's
    unsigned long long pick[SOBOL_MAX_VAR][4];   // per variant: parameter normals, parameter uniforms, step normals, step uniforms
};

// The head of the adjoint kernels' argument blocks (source_adjoint_lanes.h builds its team from it; adjoint_head of driver.cpp fills it):
// one replayed chunk, a team of sixteen lanes per rollout, four rollouts per wavefront
struct SrcAdjointHead {
    const double *xs, *us;    // staged trajectories of the chunk: [kc][N+1][RAT_N], [kc][N][RAT_M] dense
    int N;
    long kc;                  // rollouts of the chunk
    const double *cost;       // [kc] the costs the replay formed (NaN: DomainError, the rollout is passed over)
    const double *L;          // [N][4][12] or null (open loop)
    const double *p;          // the model's parameters
};

// rat_src_adjoint (source_adjoint.h): the adjoint sweep of every rollout of the chunk (rat_policy_gradient / rat_policy_tail_gradient)
struct SrcAdjointArgs : SrcAdjointHead {
    double *gu;               // [kc][N][4] dJ_k / du_t with the loop closed downstream, zero padded; untouched for a rollout without a cost
    int *bad;                 // [kc] 1: the rollout has a cost but a NaN or Inf in its sensitivities; untouched for a rollout without a cost
    int *n_bad;               // the number of those rollouts, added to (an integer atomic: a count has no order)
};

// rat_src_adjoint_p (source_adjoint_params.h): rat_src_adjoint's sweep with the parameter pass and lambda_0 (rat_policy_param_gradient /
// rat_policy_tail_param_gradient)
struct SrcAdjointPArgs : SrcAdjointHead {
    long j0;                  // global index of the chunk's first rollout (parameter sampling: the rollout's own q)
    unsigned long long seed;  // the replayed evaluation's seed
    const double *zpn, *zpu;  // the handle's injected parameter streams (whole, indexed by the global rollout), or both null: the generator
    double *gp;               // [kc][32] dJ_k / dp, zero padded; untouched for a rollout without a cost
    double *lam0;             // [kc][12] dJ_k / dx_0 with the loop closed, zero padded; untouched for a rollout without a cost
    int *bad, *n_bad;         // as SrcAdjointArgs'
};

// rat_src_margin_adjoint (source_margin_adjoint.h): the team sweeping the margins of RAT_N_MARGIN quadratic events jointly
// (rat_policy_margin_gradient); the seed of event i is g_z at the step t* that the margin pass recorded, not the cost
#define SRC_MARGIN_MAX 4      /* events a call sweeps: four lambdas of twelve doubles beside the dual evaluation of f stay in registers */
struct SrcMarginArgs : SrcAdjointHead {
    int quad;                 // 0: every event is linear (g_z = a): Qt is not read
    const double *Qt;         // [RAT_N_MARGIN][16][16] in the tile as ev_eval reads it: entry (k, i) at k * 16 + i is Q's row i, column k
    const double *at;         // [RAT_N_MARGIN][16] in the tile
    const int *tstar;         // [RAT_N_MARGIN][ldt] the chunk's arg-max steps (launch_ev_argmax), -1: the margin is NaN
    long ldt;
    double *gu;               // [kc][RAT_N_MARGIN][N][4] dM_ik / du_t with the loop closed downstream, zero padded; untouched for a rollout without a cost
    int *bad;                 // [RAT_N_MARGIN][ldb] 1: the rollout has a cost but a NaN or Inf in the event's sensitivities; untouched for a rollout without a cost
    long ldb;
    int *n_bad;               // [RAT_N_MARGIN] the number of those rollouts per event, added to (an integer atomic: a count has no order)
};
