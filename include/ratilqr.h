/*
 * ratilqr.h -- C ABI of libratilqr_hip.so: the MI355X (gfx950) implementation of RATiLQR.jl's
 * iLEQG solve and of the Cross-Entropy loop over theta that wraps it.
 *
 * The reference (pure Julia) has no FFI boundary; its operator API for this path is the set of
 * exported functions in /root/reference/src/RATiLQR.jl:20-53.  Each entry point below names the
 * reference function it replaces (file:line into /root/reference/src).  The Julia-side `ccall`
 * bindings a maintainer would add are in INTEGRATION.md and julia/RATiLQRAMD.jl.
 *
 * Conventions
 *   - plain pointers and sizes only; all floating point is fp64 (Float64), counters int32/int64;
 *   - matrices are COLUMN-MAJOR (Julia native), time is the slowest index: a Vector{Matrix}
 *     `L_array` of N (m x n) gains is the flat buffer L[i + m*j + m*n*t];
 *   - the caller owns every host buffer; the library copies in/out and retains no pointer after
 *     return (exception: the standard-normal stream registered with rat_ce_set_stream);
 *   - no exceptions cross the ABI: functions return a rat_rc (API misuse / HIP errors), and every
 *     trajectory carries a per-sample status (RAT_ST_*) with value = +Inf where the reference
 *     would have thrown (cross_entropy_bilevel_optimization.jl:161-165);
 *   - call from one host thread per handle; a handle owns one HIP device and one stream; a rat_multi owns one handle per
 *     device and is driven from one host thread as well (no callbacks, no thread-local state of the caller: @threadcall-safe);
 *   - user closures f/c/h/W cannot cross the ABI: problems are instances of compiled-in model
 *     families (rat_problem_desc.model), or HIP source the library compiles at run time (rat_problem_set_source,
 *     rat_pets_problem_set_source).
 */
#ifndef RATILQR_H
#define RATILQR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAT_VERSION 600

/* ---- return codes (API level) ---------------------------------------------------------------- */
typedef int32_t rat_rc;
#define RAT_OK               0
#define RAT_ERR_ARG          1   /* bad argument / option out of the reference's @assert ranges */
#define RAT_ERR_UNSUPPORTED  2   /* problem size or model outside the compiled kernels (n, m <= 32; power-law family n = m <= 4) */
#define RAT_ERR_HIP          3   /* HIP runtime error (see rat_last_error) */
#define RAT_ERR_NO_PROBLEM   4   /* rat_problem_set was not called */
#define RAT_ERR_STREAM_DRY   5   /* injected N(0,1) stream exhausted */
#define RAT_ERR_DIVERGED     6   /* a loop the reference would spin in forever was cut (App. B.11/B.15) */

/* ---- per-trajectory status (what the reference's exceptions become) -------------------------- */
#define RAT_ST_RUNNING          (-1)
#define RAT_ST_OK                 0  /* converged: d > d_current && mu <= mu_min  (ileqg.jl:642)            */
#define RAT_ST_M_NOT_PD_INIT      1  /* @assert isposdef(M) in initialize!        (ileqg.jl:234,440) -> Inf */
#define RAT_ST_M_NOT_PD_GAIN      2  /* @assert isposdef(M) in solve_approximate_dp! (ileqg.jl:366)  -> Inf */
#define RAT_ST_ITER_MAX           3  /* iter_max reached (ileqg.jl:648); value is valid                     */
#define RAT_ST_DOMAIN             4  /* DomainError / non-finite in rollout or linearisation         -> Inf */
#define RAT_ST_MU_DIVERGED        5  /* mu-restart loop cut                                         -> Inf */
#define RAT_ST_SINGULAR           6  /* reserved (SingularException)                                 -> Inf */
#define RAT_ST_LS_DIVERGED        7  /* line search cut after 4000 DP-failed candidates (App. B.5)  -> Inf */
#define RAT_ST_INTERNAL           8  /* a hand-over between the two workgroups of a sample timed out (never
                                        expected; reported instead of a device hang)                 -> Inf */

/* ---- model families --------------------------------------------------------------------------- */
#define RAT_MODEL_LQ        1  /* f = A x + B u + kappa x.^3 ; c_k, h quadratic (tables below)                */
#define RAT_MODEL_POWERLAW  2  /* f = x.^a + u.^b (n == m) ; c = cx sum(x.^p) + cu sum(u.^pu) ; h = pl_h   */

/* Replaces FiniteHorizonRiskSensitiveOptimalControlProblem(f, c, h, W, N)
 * (optimal_control_problems.jl:67-73).  Field order is shared with oracle/ratilqr_oracle.h. */
typedef struct rat_problem_desc {
    int32_t model;
    int32_t n, m, N;
    int32_t cost_tv;          /* 1: Q,R,P,qv,rv,q0 hold N entries (k = 0..N-1), else one entry */
    int32_t W_tv;             /* 1: W holds N entries, else one entry                            */
    const double *A;          /* n*n                */
    const double *B;          /* n*m                */
    const double *Q;          /* n*n [*N]  c_xx     */
    const double *R;          /* m*m [*N]  c_uu     */
    const double *P;          /* m*n [*N]  c_ux     */
    const double *qv;         /* n   [*N]           */
    const double *rv;         /* m   [*N]           */
    const double *q0;         /* 1   [*N]           */
    const double *Qf;         /* n*n  h_xx          */
    const double *qvf;        /* n                  */
    double q0f;
    double kappa;
    double pl_a, pl_b, pl_p, pl_pu, pl_cx, pl_cu, pl_h;
    const double *W;          /* n*n [*N]  noise covariance W(k) */
} rat_problem_desc;

/* Replaces the keyword arguments of ILEQGSolver(problem; ...)  (ileqg.jl:191-201). */
typedef struct rat_ileqg_opts {
    double mu_min, delta_0, lambda, d;
    int64_t iter_max;
    double eps_init, eps_min;
    int32_t adaptive_eps_init;
} rat_ileqg_opts;

typedef struct rat_handle_s *rat_handle;

int32_t     rat_version(void);
const char *rat_last_error(void);
void        rat_default_ileqg_opts(rat_ileqg_opts *o);                      /* defaults of ileqg.jl:191-194 */

/* Create a solver context on HIP device `device`.
 *   max_batch : largest number of theta-samples one batch call will carry (device buffers are sized once)
 *   spec_eps  : E >= 1, the LARGEST number of line-search step sizes eps_k = eps*lambda^k the library may evaluate
 *               speculatively per (sample, iteration); results are identical for every E.
 *               Speculation only pays where SIMDs would otherwise idle; on this device the sequential rule (E = 1) is at
 *               least as fast at every batch size, so a handle runs E = 1 unless the switch
 *               spec_force = 1 (rat_debug_set / RATILQR_SPEC_FORCE) asks for the requested width (the E > 1 kernels).
 * Replaces the ILEQGSolver constructor (ileqg.jl:191-208); option ranges are validated as its @asserts. */
rat_rc rat_create(const rat_ileqg_opts *opts, int32_t max_batch, int32_t spec_eps, int32_t device, rat_handle *out);
void   rat_destroy(rat_handle h);
rat_rc rat_set_ileqg_opts(rat_handle h, const rat_ileqg_opts *opts);

/* Upload a problem (tables are copied).  Replaces passing `problem` to every call.
 * Sizes: n <= 12, m <= 4 run on the MFMA kernels.  LQ-family problems up to n <= 32, m <= 32 are accepted too (the reference takes its
 * dimensions from the arrays, ileqg.jl:229) and run every entry point in general-size kernels; the power-law family beyond n = m = 4
 * and any larger problem return RAT_ERR_UNSUPPORTED. */
rat_rc rat_problem_set(rat_handle h, const rat_problem_desc *desc);

/* ---- source models: f, c, h written by the user, compiled at run time --------------------------
 * FiniteHorizonRiskSensitiveOptimalControlProblem(f, c, h, W, N) with arbitrary f, c, h (optimal_control_problems.jl:67-73),
 * differentiated by forward-mode AD as the reference does with ForwardDiff (ileqg.jl:265-273).  The source is plain HIP device code
 * that defines, for RAT_N = n and RAT_M = m (compile-time constants) and the user's parameters p (kept on the device):
 *
 *   template <class T> __device__ void rat_user_f(const T *x, const T *u, T *xn, const double *p);   x_{k+1} = f(x_k, u_k)
 *   template <class T> __device__ T    rat_user_c(int k, const T *x, const T *u, const double *p);   c(k, x, u), k = 0 .. N-1
 *   template <class T> __device__ T    rat_user_h(const T *x, const double *p);                      h(x_N)
 *
 * T is double in rollouts, or a forward-mode AD type (rat_ad.h: a dual number for the Jacobian columns of f, a hyper-dual number per
 * upper-triangle pair of z = (x, u) for c and its derivatives; the Hessian is mirrored from the upper triangle like Symmetric(...)).
 * Both support + - * / with double, comparisons on the value, and sin cos tan exp log sqrt pow(T,double) pow(T,T) tanh atan atan2 fabs
 * fmin fmax.  Optionally (the analogue of f_returns_jacobian, ileqg.jl:302-311) the source defines RAT_USER_F_JACOBIAN and
 *
 *   __device__ void rat_user_f_jacobian(const double *x, const double *u, double *xn, double *A, double *B, const double *p);
 *
 * with A n x n and B n x m column-major: exact Jacobians instead of AD for f.  A NaN in x_{t+1} or in a cost whose inputs had none is
 * the reference's DomainError (RAT_ST_DOMAIN, value Inf).  No fast-math.
 * Optionally, for Monte-Carlo evaluation under a disturbance of the user's own (rat_policy_evaluate_noise, below), the source defines
 * RAT_USER_NOISE and
 *
 *   template <class R>
 *   __device__ void rat_user_noise(int k, const double *x, const double *u, R &rng, double *w, const double *p);
 *
 * which writes w[0 .. RAT_N): the rollout is x_{k+1} = f(x_k, u_k) + w.  x and u are the state and control of step k, so the noise may
 * depend on them; w arrives zeroed.  rng is the rat_rng of generative source models (below): rng.normal() is N(0, 1), rng.uniform() is
 * U[0, 1), counted per step against the draw counts the caller declares, which the compile line carries as RAT_PETS_NORMALS and
 * RAT_PETS_UNIFORMS.  A source without RAT_USER_NOISE compiles and behaves exactly as before.
 * Optionally, for safety events of the user's own (rat_policy_events_user, rat_policy_rare_event_user, below), the source defines
 * RAT_USER_EVENT and
 *
 *   __device__ void rat_user_event(int k, const double *x, const double *u, double *g, const double *p);
 *
 * called once per step k = 0 .. N for all events: x has RAT_N entries, u has RAT_M entries and is all zeros at k = N (u_N = 0, as in
 * rat_policy_events).  double only: no AD type is involved.  The caller declares the number of events, n_event in 1 .. 16, which the
 * compile line carries as RAT_N_EVENT.  g[0 .. RAT_N_EVENT) ARRIVES AS NaN: an entry the function leaves alone is "not watched at this
 * step" and is passed over exactly as a NaN g of a quadratic event is -- this is how a window is written.  g_i > 0 means violated.  In
 * the kernel g is a local array of 16 doubles, whatever RAT_N_EVENT is.  RAT_N_EVENT is defined only while an event kernel is compiled
 * (the whole text is compiled when the problem is set, too).  The event reads p like f, c and h: rat_problem_set_params moves an
 * obstacle without a new evaluation, since the replay guard holds the replayed costs against the stored ones and an event parameter
 * moves no cost.  A source without RAT_USER_EVENT compiles and behaves exactly as before.
 * Optionally, for a controller of the user's own in the Monte-Carlo analyses (a saturating or rate-limited actuator behind the affine
 * law, or a baseline controller under the same noise and seeds), the source defines RAT_USER_POLICY and
 *
 *   __device__ void rat_user_policy(int k, const double *x, const double *u_prev, double *u, const double *p);
 *
 * called once per step k = 0 .. N-1 of every MONTE-CARLO ROLLOUT of the source: rat_policy_evaluate, rat_policy_evaluate_noise,
 * rat_policy_rare_event_noise, rat_policy_rare_event_user, and through the replay of rat_policy_evaluate_noise's rollouts
 * rat_policy_worst_case_trajectory, rat_policy_worst_case_disturbance, rat_policy_events and rat_policy_events_user.  The call comes
 * after the library has formed u_k = l_k + L_k (x_k - xbar_k) (l_k open loop, L == NULL) and before anything reads u: the cost, the
 * sampler, f, x_out / u_out / the replayed disturbances, the events.  x: 12 doubles, RAT_N of them live, the rest 0.  u: 4 doubles, RAT_M
 * live, the rest 0; it ARRIVES HOLDING THE AFFINE LAW'S CONTROL and leaves holding the control that is applied -- an entry the function
 * leaves alone stays affine.  u_prev: 4 doubles, the control applied at step k - 1, all zeros at k = 0 (rate limits, actuator lag).  p:
 * the problem's parameters, so rat_problem_set_params moves a limit without recompiling (a replay of an evaluation made under other
 * parameters is refused as ever: the replayed costs differ).  double only: no AD type reaches the hook.  A NaN in u[0 .. RAT_M) after the
 * hook where x and the affine u had none is a DomainError of that rollout, as a NaN from f is: its cost is NaN, it is counted in
 * N_DOMAIN, and dom is set by the rare-event calls.  u_out holds applied controls; rat_user_noise and rat_user_event receive the applied
 * u; the centre (xbar_t, l_t) of the worst-case moment sums stays as it is (it is only a centring).
 * The hook does NOT run in the solver: rat_ileqg_solve / rat_ileqg_solve_batch, their rollouts and linearisation, rat_rollout_open,
 * rat_rollout_feedback and rat_integrate_cost see the affine law alone -- iLEQG remains the reference's algorithm, and the policy it
 * returns is optimal for the unconstrained problem -- nor in PETS, nor for the LQ / power-law families.  A source without RAT_USER_POLICY
 * compiles to what it compiled to before and behaves exactly as before; a source that defines the hook and leaves u alone returns the
 * bits the same source without the hook returns.
 * Optionally, for model parameters that are not known exactly (a mass, a friction coefficient, an obstacle's position to +-20 %), the source
 * defines RAT_USER_PARAMS and
 *
 *   template <class R> __device__ void rat_user_params(R &rng, const double *p, double *q);
 *
 * which draws the parameters of ONE Monte-Carlo rollout.  p: the problem's n_params parameters, the nominal ones, as
 * rat_problem_set_params left them.  q: RAT_N_PARAMS = n_params doubles; it ARRIVES HOLDING A COPY OF p and leaves holding this rollout's
 * parameters -- an entry the function leaves alone stays nominal.  The hook is called once per rollout, in front of step 0; from then on q
 * is what that rollout passes as p to rat_user_c, rat_user_f, rat_user_h, rat_user_noise, rat_user_policy and rat_user_event.  rng is a
 * counted generator with rng.normal() / rng.uniform(), rat_rng's interface with bounds of its own, RAT_PARAM_NORMALS and
 * RAT_PARAM_UNIFORMS: a draw beyond them returns NaN and is an overdraw (RAT_ERR_ARG naming the limits, checked once after the wait; the
 * handle stays usable).  double only: no AD type reaches the hook.  A NaN in q[0 .. n_params) where p had none is a DomainError of that
 * rollout: NaN cost, counted in RAT_MC_N_DOMAIN, dom set by the rare-event calls.
 * The hook runs only where rat_policy_params_sampling has switched parameter sampling on for the handle (below; off is the default, and
 * rat_problem_set_source switches it off again), and then in the kernels that carry a counted rng: rat_policy_evaluate_noise,
 * rat_policy_rare_event_noise, rat_policy_rare_event_user, and through the replay of rat_policy_evaluate_noise's rollouts
 * rat_policy_worst_case_trajectory, rat_policy_worst_case_disturbance, rat_policy_events and rat_policy_events_user -- the replays run
 * the rollouts again under the same seed, so they form the same q; the kernel of rat_policy_events_user forms q once more from the
 * rollout's index and the seed.  Changing the sampling state between an evaluation and its replay is caught by the replay guard like any
 * other change: the replayed costs differ from the stored ones.  With sampling on, a source without the hook is RAT_ERR_ARG, and the
 * message says so.  With sampling off every kernel is compiled without the hook, whether or not the source defines it: a source that
 * defines RAT_USER_PARAMS returns the bits the same source without it returns, and a source without it compiles to what it compiled to
 * before.  With sampling on, a hook that leaves q alone returns the sampling-off bits provided the user's expressions define their bits:
 * a sum of two products may be fused around either product, and the compiler's choice can differ between p in scalar and q in vector
 * registers (a few ulp; '#pragma clang fp contract(off)' in the functions that read p settles it).  NOT covered, all of them on the nominal p always: rat_policy_evaluate under N(0, W) (no counted rng), the solver, its rollouts
 * and its linearisation, PETS, the LQ / power-law families, general sizes.  One GPU.
 * Draw keying: a rollout's parameters depend neither on K nor on how a call is cut into launches.  Injected: the i-th parameter normal /
 * uniform of rollout j is zpn[j * param_normals + i] / zpu[j * param_uniforms + i].  Generator: Philox4x32-10 with the call's seed as key and
 * counter (g lo, g hi, 0xFFFFFFFF, i / 2) for normals, (g lo, g hi, 0xFFFFFFFF, 0x80000000 | i / 2) for uniforms, g the global rollout
 * index; Box-Muller pairing and the 53-bit uniform as for the per-step draws, whose counters (step word t < N) stay bit for bit what they
 * were.  The rare-event calls run every pass under the pass's seed, the final pass under the call's.  Their proposal shifts the per-step
 * normals alone: parameter normals are NOT shifted and add nothing to logw, so an event that a parameter drives cannot be made likelier
 * by these calls (as one driven by a uniform cannot).  rat_policy_rare_event_params (below) shifts the parameter normals as well and is
 * the call for such an event.
 * Limits: n <= 12, m <= 4 (else RAT_ERR_UNSUPPORTED); batches run on the round-based path (rat_set_path FUSED / BLOCK return
 * RAT_ERR_UNSUPPORTED); rat_rollout_noisy and rat_multi are not available for source models: rat_policy_evaluate with cost_out is the way
 * to their Monte-Carlo costs, and rat_policy_evaluate_noise with x_out / u_out the way to Monte-Carlo trajectories (under the user's
 * sampler only).  PETS takes generative source models of its own (rat_pets_problem_set_source, below). */
#define RAT_MODEL_SOURCE    3

/* Compile `source` (NUL-terminated) for the handle's device and make it the handle's problem.  W: n*n column-major, N entries if W_tv
 * (exactly as rat_problem_set takes it).  params: n_params doubles (may be 0 / NULL).  A compile error returns RAT_ERR_ARG with the
 * compiler's log in rat_last_error(); a failed call leaves the previous problem in place.  Code objects are cached per process by
 * (source, n, m, device architecture). */
rat_rc rat_problem_set_source(rat_handle h, const char *source, int32_t n, int32_t m, int32_t N,
                              const double *W, int32_t W_tv, const double *params, int64_t n_params);
/* New values of the source problem's parameters (the same count; no recompilation). */
rat_rc rat_problem_set_params(rat_handle h, const double *params, int64_t n_params);
/* Compile only, for gfx950 (no device needed): RAT_OK, RAT_ERR_ARG with the log in rat_last_error(), or RAT_ERR_UNSUPPORTED. */
rat_rc rat_source_check(const char *source, int32_t n, int32_t m);
/* The same for the kernel of rat_policy_evaluate_noise: `source` must define RAT_USER_NOISE and rat_user_noise (else RAT_ERR_ARG, and the
 * message says so); negative draw counts are RAT_ERR_ARG. */
rat_rc rat_user_noise_check(const char *source, int32_t n, int32_t m, int32_t normals, int32_t uniforms);
/* The same for the kernel of rat_policy_events_user: `source` must define RAT_USER_EVENT and rat_user_event (else RAT_ERR_ARG, and the
 * message says so); n_event outside 1 .. 16 is RAT_ERR_ARG. */
rat_rc rat_user_event_check(const char *source, int32_t n, int32_t m, int32_t n_event);
/* The same for rat_user_policy, in the rollout kernel of rat_policy_evaluate: `source` must define RAT_USER_POLICY and rat_user_policy
 * (else RAT_ERR_ARG, and the message says so; a wrong signature is a compile error). */
rat_rc rat_user_policy_check(const char *source, int32_t n, int32_t m);
/* Parameter sampling of the handle (rat_user_params above): param_normals / param_uniforms are the most rng.normal() / rng.uniform() calls
 * of the hook.  zpn [param_normals x K_injected], zpu [param_uniforms x K_injected] (column-major: rollout slowest): injected draws, every
 * declared stream (else RAT_ERR_ARG), copied by the call -- the library keeps no pointer into the caller's arrays -- and a later call with
 * K > K_injected is RAT_ERR_ARG; both NULL: the device generator, keyed by each call's seed (K_injected is not read).  Counts (0, 0) with
 * both streams NULL switch sampling OFF, the default.  Negative counts: RAT_ERR_ARG.  A problem that is not a source model:
 * RAT_ERR_UNSUPPORTED.  n_params == 0: RAT_ERR_ARG; n_params > 32: RAT_ERR_UNSUPPORTED.  The kernels are compiled for the new state by the
 * next call that needs them (another module per kind, cached like every other). */
rat_rc rat_policy_params_sampling(rat_handle h, int32_t param_normals, int32_t param_uniforms, const double *zpn, const double *zpu,
                                  int64_t K_injected);
/* Compiles the rollout kernel of rat_policy_evaluate_noise with sampling on for gfx950, without a device: `source` must define
 * RAT_USER_PARAMS and rat_user_params (else RAT_ERR_ARG, and the message says so); n_params outside 1 .. 32 and negative counts are refused
 * as rat_policy_params_sampling refuses them. */
rat_rc rat_user_params_check(const char *source, int32_t n, int32_t m, int32_t n_params, int32_t normals, int32_t uniforms,
                             int32_t param_normals, int32_t param_uniforms);
/* The hook alone: q of rollouts 0 .. K - 1 under `seed` (or under the handle's injected draws), q_out [n_params x K] column-major -- the
 * parameters behind the cost_out of rat_policy_evaluate_noise with that seed, and behind the final pass of a rare-event call with it.
 * Sampling must be on (else RAT_ERR_ARG). */
rat_rc rat_policy_params_sample(rat_handle h, int64_t K, uint64_t seed, double *q_out);

/* ---- the hot path ----------------------------------------------------------------------------- */

/* Batched iLEQG: one complete solve!(ileqg, problem, x0, u0; theta_i) per sample, all samples at once.
 * Replaces the fan-out of compute_value_worker (cross_entropy_bilevel_optimization.jl:144-167,186-191):
 * value[i] = solve!(...)[4], or +Inf where the reference would throw.  Optional outputs (may be NULL):
 * status[i] (RAT_ST_*), iters[i] (iLEQG iterations), ls_evals[i] (line-search candidates consumed by the
 * sequential rule of line_search!, ileqg.jl:504-581). x0[n], u0[m*N], theta[B]: host buffers. */
rat_rc rat_ileqg_solve_batch(rat_handle h, const double *x0, const double *u0, const double *theta, int64_t B,
                             double *value, int32_t *status, int32_t *iters, int32_t *ls_evals);

/* Same with theta / value / status / iters / ls_evals resident in device (HBM) memory; x0/u0 are taken
 * from the last rat_set_initial() call.  Asynchronous w.r.t. the host except for the per-round counter
 * read-back; returns after the batch has finished on the handle's stream. */
rat_rc rat_set_initial(rat_handle h, const double *x0, const double *u0);
rat_rc rat_ileqg_solve_batch_dev(rat_handle h, const double *theta_dev, int64_t B, double *value_dev,
                                 int32_t *status_dev, int32_t *iters_dev, int32_t *ls_evals_dev);

/* Single solve with the full policy returned.  Replaces solve!(ileqg, problem, x_0, u_array; theta)
 * (ileqg.jl:635-659): x[n*(N+1)], l[m*N], L[m*n*N], value, eps_history as (eps, new-current) pairs
 * (eps_hist holds 2*hist_cap doubles; *hist_n receives the number of pairs produced). */
rat_rc rat_ileqg_solve(rat_handle h, const double *x0, const double *u0, double theta,
                       double *x, double *l, double *L, double *value, int32_t *status, int32_t *iters,
                       double *eps_hist, int64_t hist_cap, int64_t *hist_n);

/* ---- individual operators (unit parity with test/ileqg_test.jl) -------------------------------- */

/* simulate_dynamics(problem, x_0, u_array)                     ileqg.jl:18-38   -> x[n*(N+1)]; *domain_fail = 1 on DomainError */
rat_rc rat_rollout_open(rat_handle h, const double *x0, const double *u, double *x, int32_t *domain_fail);
/* simulate_dynamics(problem, x_array, l_array, L_array)        ileqg.jl:62-87   -> x_new, u_new */
rat_rc rat_rollout_feedback(rat_handle h, const double *xbar, const double *l, const double *L,
                            double *x_new, double *u_new, int32_t *domain_fail);
/* integrate_cost(problem, x_array, u_array)                    ileqg.jl:115-124 */
rat_rc rat_integrate_cost(rat_handle h, const double *x, const double *u, double *cost);
/* simulate_dynamics(problem, x_0, u_array, rng)  ileqg.jl:44-55  (L == NULL: open loop, only the first column of x_nom is read) and
 * simulate_dynamics(problem, x_array, l_array, L_array, rng)  ileqg.jl:94-109  (affine policy u_k = l_k + L_k (x_k - x_nom_k)):
 * K independent Monte-Carlo rollouts x_{k+1} = f(x_k, u_k) + w_k, w_k ~ N(0, W(k)), drawn as chol_lower(W(k)) z_k (what
 * rand(rng, MvNormal(0, W)) computes).  z: [n x N x K] injected standard-normal draws (column-major, rollout slowest) or NULL for the
 * device generator (Philox4x32-10 keyed by seed; the reference's MersenneTwister stream is not reproducible).
 * Outputs (any may be NULL): x_out [n x (N+1) x K], u_out [m x N x K], cost_out [K] = integrate_cost of each rollout
 * (ileqg.jl:115-124; NaN where a rollout hit a DomainError), *domain_fail = 1 if any rollout did. */
rat_rc rat_rollout_noisy(rat_handle h, const double *x_nom, const double *l, const double *L, int64_t K,
                         const double *z, uint64_t seed, double *x_out, double *u_out, double *cost_out, int32_t *domain_fail);
/* Monte-Carlo policy evaluation: the K rollouts of rat_rollout_noisy (x_nom, l, L, K, z, seed mean exactly what they mean there; L == NULL
 * is an open-loop run) for a problem of any model kind -- the LQ and power-law families, general sizes and source models -- with the
 * statistics of the K costs formed on the device: only these doubles come back, not K of them.
 *   stats[RAT_MC_NSTAT]  the slots below; required
 *   theta[n_theta]       risk parameters, 0 <= n_theta <= 16, every theta[i] >= 0 (else RAT_ERR_ARG)
 *   risk[i]              the entropic risk (1 / theta_i) log mean_k exp(theta_i J_k) that iLEQG minimises, formed as
 *                        Jmax + log(mean_k exp(theta_i (J_k - Jmax))) / theta_i (no overflow for any theta); the mean where theta_i == 0
 *   risk_se[i]           its delta-method standard error sd(y) / (mean(y) theta_i sqrt(N_OK)), y_k = exp(theta_i (J_k - Jmax)); SE_MEAN where
 *                        theta_i == 0.  It is finite only where E exp(2 theta J) is.
 *   cost_out[K]          rat_rollout_noisy's cost_out (bit for bit for the families and general sizes, with the same seed or z), NaN for a
 *                        DomainError rollout
 * risk, risk_se, cost_out may be NULL.  DomainError rollouts are counted and left out of every statistic; with N_OK == 0 the call returns
 * RAT_OK and MEAN, VAR, MIN, MAX, the risks and their errors are NaN.  K < 1 or K > 2^27 is RAT_ERR_ARG, and so is a W(k) that is not
 * positive definite.  The sums run in a fixed order without floating-point atomics: two calls with the same arguments return the same
 * bits.  For a source model the generator is keyed as for the families: a seed names the same noise for a family problem and for the same
 * problem written as source; its rollout kernel is compiled by the first call on the problem (cached per process like the model kernels).
 * The device buffers of the call (8 bytes per rollout, plus 4 for the families) belong to the handle, grow with K and stay until rat_destroy. */
#define RAT_MC_N_OK     0   /* rollouts without a DomainError, as a double */
#define RAT_MC_N_DOMAIN 1   /* rollouts that hit one; they are left out of every statistic */
#define RAT_MC_MEAN     2
#define RAT_MC_VAR      3   /* unbiased; NaN when N_OK < 2 */
#define RAT_MC_MIN      4
#define RAT_MC_MAX      5
#define RAT_MC_SE_MEAN  6   /* sqrt(VAR / N_OK) */
#define RAT_MC_NSTAT    8   /* slot 7 reserved, written as 0 */
rat_rc rat_policy_evaluate(rat_handle h, const double *x_nom, const double *l, const double *L, int64_t K,
                           const double *z, uint64_t seed, const double *theta, int32_t n_theta,
                           double *stats, double *risk, double *risk_se, double *cost_out);
/* rat_policy_evaluate for a source model under the user's own process noise: w_k = rat_user_noise(k, x_k, u_k, rng) ("source models"
 * above) in place of chol_lower(W(k)) z_k.  W is not read: the sampler is the whole disturbance.  x_nom, l, L, K, theta, n_theta, stats,
 * risk, risk_se, cost_out and the range of K mean exactly what they mean for rat_policy_evaluate, and the K costs go through the same
 * fixed-order reduction: two calls with the same arguments return the same bits.
 *   normals_per_step, uniforms_per_step   the most rng.normal() / rng.uniform() calls one step makes (>= 0, else RAT_ERR_ARG); the rollout
 *                         kernel is compiled for them by the first call that names them (cached per process by source, n, m, the two
 *                         counts and the architecture); a step that draws more gets NaN and the call returns RAT_ERR_ARG naming the
 *                         limits (the handle stays usable)
 *   zn, zu                injected draws: the i-th normal / uniform of rollout j at step t is zn[(j N + t) normals_per_step + i] /
 *                         zu[(j N + t) uniforms_per_step + i]; every stream with a positive count must be given (else RAT_ERR_ARG).  Both
 *                         NULL: the device generator, Philox4x32-10 keyed by seed with the rollout's index j in the counter (the keying
 *                         of generative source models, below) -- a rollout's noise does not depend on K
 *   x_out, u_out          [n x (N+1) x K], [m x N x K] dense column-major, rollout slowest (rat_rollout_noisy's layout); either may be
 *                         NULL.  They are staged on the device 2^16 rollouts at a time.  A DomainError rollout holds what was computed
 * The five noise fields are arguments of the call, as in rat_pets_compute_cost, not a descriptor struct.  A NaN in w whose inputs x_k, u_k
 * had none is a DomainError, like a NaN in f or a cost.  Refusals: a problem that is not a source model RAT_ERR_UNSUPPORTED; a source
 * without RAT_USER_NOISE, or one that does not compile, RAT_ERR_ARG with the compiler's log (model.hip:LINE) in rat_last_error(). */
rat_rc rat_policy_evaluate_noise(rat_handle h, const double *x_nom, const double *l, const double *L, int64_t K,
                                 int32_t normals_per_step, int32_t uniforms_per_step, const double *zn, const double *zu, uint64_t seed,
                                 const double *theta, int32_t n_theta, double *stats, double *risk, double *risk_se, double *cost_out,
                                 double *x_out, double *u_out);
/* The worst-case expected cost of a policy within the KL ball, from the K Monte-Carlo costs: sup { E_p[J] : KL(p || q) <= d } over the
 * sample, the quantity rat_ce_solve / rat_nm_solve minimise as value(theta) + d / theta.  The dual is exact and one-dimensional: with
 * y_k = exp(theta (J_k - Jmax)) over the N_OK costs, Z = mean y, m(theta) = sum y J / sum y (the mean under the exponentially tilted, worst-case
 * distribution), KL(theta) = theta (m - Jmax) - log Z (non-decreasing from 0 to log(N_OK / n_max), n_max the rollouts with J == Jmax),
 * bound(d) = min_theta [Jmax + log Z / theta + d / theta], attained where KL(theta*) = d, and there bound = m(theta*).  theta* is searched
 * on the device: 12 passes of 16 points per bound (a geometric grid theta_0 4^(j - 7) around theta_0 = sqrt(2 d) / sd(J), then eleven
 * 17-sections: the last bracket is below 1e-13 relative), no read-back between passes.
 *   cost       NULL: the K costs the last rat_policy_evaluate / rat_policy_evaluate_noise on this handle left on the device -- or the K
 *              costs a later call of this function uploaded; K must be 0 or that K, and RAT_ERR_ARG if no such call has been made.
 *              Otherwise K host doubles (1 <= K <= 2^27), uploaded into the same buffer; NaN entries are DomainError rollouts and are
 *              left out.  No problem needs to be set for this form.
 *   kl_bound   [n_bound], 0 <= n_bound <= 16, every one >= 0 (+Inf allowed; NaN or negative RAT_ERR_ARG)
 *   theta      [n_theta], 0 <= n_theta <= 16, every one >= 0 and finite (else RAT_ERR_ARG); n_bound + n_theta == 0 is RAT_ERR_ARG
 *   out_bound  [n_bound][RAT_WC_NSTAT], out_theta [n_theta][RAT_WC_NSTAT]: a row of the slots below per kl_bound / per theta
 *   weights_out[K] or NULL: y_k / sum y at kl_bound[0]'s theta* (at theta[0] when n_bound == 0), 0 for a DomainError rollout; on a
 *              saturated row 1 / n_max on the maxima and 0 elsewhere.  The importance weights that turn rat_policy_evaluate_noise's
 *              x_out / u_out into worst-case trajectories on the host (rat_policy_worst_case_trajectory forms their moments on the
 *              device instead).
 * Flags: RAT_WC_SATURATED when kl_bound >= log(N_OK / n_max), or when theta_top = 65536 theta_0 still has KL < kl_bound: the row holds the
 * theta -> Inf limits (THETA +Inf, KL log(N_OK / n_max), BOUND = TILT_MEAN = Jmax, TILT_VAR 0, ESS n_max, BOUND_SE NaN).  RAT_WC_EMPTY:
 * N_OK == 0; RAT_WC_NONFINITE: a +-Inf among the costs; every other slot is NaN in both.  kl_bound == 0 is decided first: theta 0, KL 0,
 * BOUND = TILT_MEAN = the mean, ESS N_OK, flag OK.  The sums run in rat_policy_evaluate's fixed order: the same arguments return the same
 * bits, and a row's bits depend neither on the other rows of the call nor on where the costs came from. */
#define RAT_WC_THETA     0   /* bound row: theta*; theta row: the given theta */
#define RAT_WC_KL        1   /* KL(theta) */
#define RAT_WC_BOUND     2   /* Jmax + log Z / theta + d / theta; d = kl_bound[i] on a bound row, the row's own KL on a theta row (so BOUND
                              * equals TILT_MEAN up to rounding there) */
#define RAT_WC_BOUND_SE  3   /* delta method, sd(y) / (mean(y) theta sqrt(N_OK)): risk_se's formula at that theta; SE_MEAN at theta == 0 */
#define RAT_WC_TILT_MEAN 4   /* m(theta) */
#define RAT_WC_TILT_VAR  5   /* sum y (J - m)^2 / sum y */
#define RAT_WC_ESS       6   /* (sum y)^2 / sum y^2: the effective sample size of the tilted estimate */
#define RAT_WC_FLAG      7   /* RAT_WC_OK ... as a double */
#define RAT_WC_NSTAT     8
#define RAT_WC_OK        0
#define RAT_WC_SATURATED 1
#define RAT_WC_EMPTY     2
#define RAT_WC_NONFINITE 3
rat_rc rat_policy_worst_case(rat_handle h, const double *cost, int64_t K, const double *kl_bound, int32_t n_bound,
                             const double *theta, int32_t n_theta, double *out_bound, double *out_theta, double *weights_out);
/* What the worst case looks like: the mean and covariance of (x_t, u_t) at every step under the nominal distribution q (a theta = 0 row)
 * and under the worst-case distribution p* ~ exp(theta* J) q of each kl_bound (and the tilt of each given theta), formed on the device.
 * The call takes no policy and no noise: it REPLAYS the last rat_policy_evaluate / rat_policy_evaluate_noise of the handle -- the same
 * rollout kernel, chunks and seeds, the trajectories staged in buffers of the handle -- and sums, per step and row, S0 = sum y,
 * S1 = sum y D and S2 = sum y D D' of D = (x_t, u_t) - c_t with y = exp(theta (J - Jmax)) from the stored costs (one f64 MFMA per four
 * rollouts, step and row).  c_t is (x_nom[t], l[t]) under a policy and the noise-free open-loop trajectory with L == NULL.  Fixed
 * summation order, no floating-point atomics: the same call returns the same bits, and a row's bits do not depend on the other rows.
 *   kl_bound, theta   as rat_policy_worst_case's (the same refusals)
 *   rows_out  [(n_bound + n_theta)][RAT_WC_NSTAT]: rat_policy_worst_case's rows of the same arguments, bit for bit (bounds, then thetas)
 *   mean_out  [(n_bound + n_theta)][N+1][n+m]: E (x_t, u_t); the u part of step N is 0
 *   cov_out   [(n_bound + n_theta)][N+1][(n+m)^2] column-major, the population form sum y (z - mean)(z - mean)' / sum y (as RAT_WC_TILT_VAR);
 *             rows and columns of u at step N are 0
 * A RAT_WC_SATURATED row holds the moments of the rollouts that attain Jmax; RAT_WC_EMPTY and RAT_WC_NONFINITE rows are NaN.  A
 * DomainError rollout carries no weight.
 * Served: the LQ and power-law families (n <= 12, m <= 4) after rat_policy_evaluate with z == NULL, and source models after
 * rat_policy_evaluate_noise with zn == zu == NULL.  RAT_ERR_UNSUPPORTED: general sizes; a source model evaluated under N(0, W) by
 * rat_policy_evaluate (write the Gaussian as rat_user_noise); an evaluation on injected draws (the caller has x_out: combine it with
 * weights_out on the host); rows x (N + 1) above 3640.  RAT_ERR_ARG, the handle stays usable: no evaluation on the handle yet, or costs
 * uploaded by rat_policy_worst_case(cost != NULL) since; and a replay whose costs are not the stored ones bit for bit (NaN equals NaN):
 * the problem, its parameters or the policy changed since the evaluation. */
rat_rc rat_policy_worst_case_trajectory(rat_handle h, const double *kl_bound, int32_t n_bound, const double *theta, int32_t n_theta,
                                        double *rows_out, double *mean_out, double *cov_out);
/* What the adversary does to the noise: the mean and covariance of the disturbance w_t at every step t = 0 .. N-1, and its covariance with
 * the (x_t, u_t) it acts on, under the nominal distribution q (a theta = 0 row) and under p* ~ exp(theta* J) q of each kl_bound (and the
 * tilt of each given theta).  w_t is what the rollout added: chol_lower(W(t)) z_t for the families, what rat_user_noise wrote for a source
 * model.  The call takes no policy and no noise: it REPLAYS the last evaluation exactly as rat_policy_worst_case_trajectory does -- the
 * same chunks and seeds, the same bit-for-bit check against the stored costs -- with the rollouts keeping w_t in a staging buffer of the
 * handle, and sums per step and row S0, S1 and S2 = sum y Dw Dw' (one f64 MFMA per four rollouts, step and row) and, when cov_wz_out is
 * given, sum y Dw Dz' (a second one) of Dw = w_t - c_w[t], Dz = (x_t, u_t) - c_t.  c_t is the trajectory call's centre; c_w[t] is the w_t
 * of the first rollout whose cost is not NaN among the first min(K, 65536) (0 where that is not finite, or where there is none).  Fixed
 * summation order, no floating-point atomics: the same call returns the same bits, and a row's bits do not depend on the other rows.
 *   kl_bound, theta   as rat_policy_worst_case's (the same refusals)
 *   rows_out   [(n_bound + n_theta)][RAT_WC_NSTAT]: rat_policy_worst_case's rows of the same arguments, bit for bit (bounds, then thetas)
 *   mean_w_out [(n_bound + n_theta)][N][n]: E w_t
 *   cov_w_out  [(n_bound + n_theta)][N][n^2] column-major, the population form sum y (w - mean)(w - mean)' / sum y; exactly symmetric
 *   cov_wz_out [(n_bound + n_theta)][N][n (n+m)] column-major (w's component the row, z = (x_t, u_t) the column), or NULL: the second
 *              product is then not formed.  cov_wz pinv(cov_z) on the x block is the adversary's feedback gain.
 * A RAT_WC_SATURATED row holds the moments of the rollouts that attain Jmax; RAT_WC_EMPTY and RAT_WC_NONFINITE rows are NaN.  A
 * DomainError rollout carries no weight (it is selected out: its w may hold NaN).
 * Served and refused as rat_policy_worst_case_trajectory, with the same codes; the cap of its own is rows x N above 1899 (partial sums of
 * 552 doubles in 8 slots per row and step against 64 MiB): RAT_ERR_UNSUPPORTED. */
rat_rc rat_policy_worst_case_disturbance(rat_handle h, const double *kl_bound, int32_t n_bound, const double *theta, int32_t n_theta,
                                         double *rows_out, double *mean_w_out, double *cov_w_out, double *cov_wz_out);
/* What the adversary picks among the uncertain parameters: the mean and covariance of the parameters q that rat_user_params drew for the
 * rollouts (P = n_params, 1 .. 32), and their covariance with the rollout's cost J, under the nominal distribution (a theta = 0 row) and
 * under p* ~ exp(theta* J) q of each kl_bound (and the tilt of each given theta).  The call takes no policy and no noise: it REPLAYS the
 * last rat_policy_evaluate_noise exactly as rat_policy_worst_case_trajectory does -- the same chunks and seeds, the same bit-for-bit check
 * against the stored costs -- and behind each chunk forms the chunk's q again from the rollout index and the evaluation's seed (the kernel
 * of rat_policy_params_sample; the handle's injected parameter streams are served too) into a staging buffer of the handle.  Per row it
 * sums S0, sum y^2, S1 = sum y Dq, S2 = sum y Dq Dq' (f64 MFMAs: one 16 x 16 block for P <= 16, the blocks (0,0), (0,1), (1,1) above) and,
 * when cov_qJ_out is given, sum y DJ, sum y DJ^2 and sum y DJ Dq, of Dq = q - c_q, DJ = J - c_J.  c_q and c_J are the q and the cost of
 * the first rollout whose stored cost is not NaN among the first min(K, 65536) (0 where that is not finite, or where there is none).
 * Fixed summation order, no floating-point atomics: the same call returns the same bits, and a row's bits do not depend on the other rows.
 *   kl_bound, theta   as rat_policy_worst_case's (the same refusals)
 *   rows_out   [(n_bound + n_theta)][RAT_WC_NSTAT]: rat_policy_worst_case's rows of the same arguments, bit for bit (bounds, then thetas)
 *   mean_q_out [(n_bound + n_theta)][P]: E q
 *   cov_q_out  [(n_bound + n_theta)][P^2] column-major, the population form sum y (q - mean)(q - mean)' / sum y; exactly symmetric
 *   cov_qJ_out [(n_bound + n_theta)][P], or NULL (the cost sums are then not formed): Cov(q_i, J) under the row's distribution, which is
 *              dE_theta[q_i] / dtheta at the row's tilt.  cov_qJ[i]^2 / (cov_q[i,i] RAT_WC_TILT_VAR) is the linear share of Var J that
 *              parameter i explains.
 * A RAT_WC_SATURATED row holds the moments of the rollouts that attain Jmax; RAT_WC_EMPTY and RAT_WC_NONFINITE rows are NaN.  A
 * DomainError rollout carries no weight (it is selected out: its q may hold NaN).
 * Refused, the handle staying usable: parameter sampling off on the handle: RAT_ERR_ARG (call rat_policy_params_sampling, then evaluate);
 * a problem that is not a source model, general sizes: RAT_ERR_UNSUPPORTED; no evaluation, or costs uploaded since: RAT_ERR_ARG; an
 * evaluation under N(0, W) or on injected noise draws: RAT_ERR_UNSUPPORTED; parameters, policy or sampling state changed since the
 * evaluation: RAT_ERR_ARG (the replay guard).  No cap on the rows of its own: the partial sums are 840 doubles in 8 slots per row, 1.7 MB
 * at the 32 rows the arguments allow, against the siblings' 64 MiB. */
rat_rc rat_policy_worst_case_params(rat_handle h, const double *kl_bound, int32_t n_bound, const double *theta, int32_t n_theta,
                                    double *rows_out, double *mean_q_out, double *cov_q_out, double *cov_qJ_out);
/* The tail risk of a policy, from the K Monte-Carlo costs: per level alpha the alpha-quantile of the cost (value at risk: with probability
 * alpha the cost stays below it) and the conditional value at risk, the expected cost of the worst (1 - alpha) share of the rollouts.  With
 * n = N_OK and s_1 <= ... <= s_n the OK costs in ascending order: a = n alpha (one rounded product), k = clamp(ceil(a), 1, n), VAR = s_k (bit
 * for bit an element of the sample; -0.0 counts as +0.0), CVAR = VAR + sum (J - VAR)^+ / (n - a) (Rockafellar-Uryasev: ties and the
 * fractional atom at VAR need no special case).  The tail distribution puts 1 / (n - a) on every rollout above VAR and spreads what is left,
 * r = (n - k - c_gt) + (k - a) rollouts' worth, evenly over the c_eq rollouts at VAR.  alpha == 0 gives VAR = the minimum and CVAR = the mean.
 * VAR is found by a radix select on the device (8 digits of 8 bits over the costs' bit patterns, every level at once, integer histograms;
 * digits the minimum and the maximum share are not swept), the sums in one more sweep in rat_policy_evaluate's fixed order.
 *   cost, K    as rat_policy_worst_case's: NULL for the K costs the last evaluation -- or the last call of either function with host costs --
 *              left on the device (K 0 or that K), otherwise K host doubles (1 <= K <= 2^27), uploaded into the same buffer, NaN entries
 *              left out; no problem needs to be set for that form, and rat_policy_worst_case_trajectory has nothing to replay after it
 *   alpha      [n_alpha], 1 <= n_alpha <= 16, every one in [0, 1) (NaN, negative or >= 1: RAT_ERR_ARG)
 *   rows_out   [n_alpha][RAT_TR_NSTAT]: a row of the slots below per level
 *   weights_out[K] or NULL: the tail distribution at alpha[0] -- 1 / (n - a) where J > VAR, r / (c_eq (n - a)) where J == VAR, 0 elsewhere
 *              and for a DomainError rollout; they sum to one
 * Flags: RAT_TR_SATURATED when n - a < 1, the tail is thinner than one rollout: VAR = CVAR = Jmax, CVAR_SE NaN, ESS n_max, KL
 * log(N_OK / n_max), weights uniform on the maxima.  RAT_TR_EMPTY: N_OK == 0; RAT_TR_NONFINITE: a +-Inf among the costs; every other slot
 * but ALPHA is NaN in both.  ESS and the saturated flag say how far to trust a row: CVAR at ESS of a few rollouts is those rollouts' mean.
 * CVAR is the worst-case expectation over every p with dp/dq <= 1 / (1 - alpha), and the tail distribution has KL(p || q) = KL, so
 * CVAR <= rat_policy_worst_case's BOUND at kl_bound = KL on the same costs.  Integer histograms and fixed-order sums, no floating-point
 * atomics: the same arguments return the same bits, and a row's bits depend neither on the other levels of the call nor on where the costs
 * came from. */
#define RAT_TR_ALPHA     0   /* the level */
#define RAT_TR_VAR       1   /* s_k */
#define RAT_TR_CVAR      2
#define RAT_TR_CVAR_SE   3   /* sd of (J - VAR)^+ over (1 - alpha) sqrt(N_OK) (VAR taken as known); NaN when N_OK < 2 */
#define RAT_TR_TAIL_N    4   /* n - a: the tail's mass in rollouts */
#define RAT_TR_ESS       5   /* (n - a)^2 / (c_gt + r^2 / c_eq): the effective sample size of the tail distribution */
#define RAT_TR_KL        6   /* KL(tail distribution || uniform on the N_OK rollouts) */
#define RAT_TR_FLAG      7   /* RAT_TR_OK ... as a double */
#define RAT_TR_NSTAT     8
#define RAT_TR_OK        0
#define RAT_TR_SATURATED 1
#define RAT_TR_EMPTY     2
#define RAT_TR_NONFINITE 3
rat_rc rat_policy_tail_risk(rat_handle h, const double *cost, int64_t K, const double *alpha, int32_t n_alpha,
                            double *rows_out, double *weights_out);
/* What the tail looks like: the moments of rat_policy_worst_case_trajectory / _disturbance / _params under the CVaR adversary's
 * distribution instead of the KL adversary's -- per level alpha the tail distribution of rat_policy_tail_risk, which puts equal weight on
 * every rollout above VAR, r / c_eq of it on each rollout at VAR and none below: "what do the worst (1 - alpha) of the rollouts look like".
 * Each call REPLAYS the last evaluation exactly as its worst-case sibling does -- the same chunks and seeds, the same bit-for-bit check
 * against the stored costs, the same centres, partial sums and fixed summation order -- with rat_policy_tail_risk's chain on the stored
 * costs as the source of the rows and of the weights.
 *   alpha      [n_alpha], 1 <= n_alpha <= 16, every one in [0, 1): rat_policy_tail_risk's rules (RAT_ERR_ARG)
 *   rows_out   [n_alpha][RAT_TR_NSTAT]: what rat_policy_tail_risk(h, NULL, 0, alpha, n_alpha, ...) returns on the stored costs, bit for bit
 *   the moment outputs: the sibling's layouts with n_alpha rows -- mean_out [n_alpha][N+1][n+m], cov_out [n_alpha][N+1][(n+m)^2]
 *              column-major; mean_w_out [n_alpha][N][n], cov_w_out [n_alpha][N][n^2], cov_wz_out [n_alpha][N][n (n+m)] or NULL;
 *              mean_q_out [n_alpha][P], cov_q_out [n_alpha][P^2], cov_qJ_out [n_alpha][P] or NULL -- in the population form
 *              sum y (. - mean)(. - mean)' / sum y
 * alpha == 0 is the whole sample: the nominal row, bit for bit the theta = 0 row of the sibling.  A RAT_TR_SATURATED level (a tail
 * thinner than one rollout) holds the moments of the rollouts that attain Jmax; RAT_TR_EMPTY and RAT_TR_NONFINITE levels are NaN in every
 * output (the call still returns RAT_OK).  A DomainError rollout carries no weight.  A row's bits do not depend on the other levels of
 * the call.
 * The schedule: at alpha = 0.99 one rollout in a hundred carries weight, so the moment kernels read, per group of four rollouts, one word
 * of "level r has weight here" bits first; a group without weight in a row issues no MFMA for it, a group without weight in any row is
 * not loaded, and a rollout without weight in a row is selected out of that row's operands.  Adding 0 D changes no bit of a sum where D
 * is finite, so on finite data the results are those of the sibling's dense kernels on the same weights, bit for bit.  The one
 * difference: a rollout WITHOUT weight in a row whose trajectory, disturbance or parameters hold Inf or NaN is left out of that row,
 * where the dense kernels form 0 Inf = NaN (the worst-case calls give every rollout with a cost a positive weight, so it cannot arise
 * there).
 * Served and refused as the siblings, with the same codes and caps (rows x (N + 1) above 3640, rows x N above 1899 with n_alpha rows);
 * costs uploaded by rat_policy_tail_risk(cost != NULL) are no evaluation's.  The safety events of the tail: rat_policy_tail_events, below. */
rat_rc rat_policy_tail_trajectory(rat_handle h, const double *alpha, int32_t n_alpha, double *rows_out, double *mean_out, double *cov_out);
rat_rc rat_policy_tail_disturbance(rat_handle h, const double *alpha, int32_t n_alpha, double *rows_out, double *mean_w_out,
                                   double *cov_w_out, double *cov_wz_out);
rat_rc rat_policy_tail_params(rat_handle h, const double *alpha, int32_t n_alpha, double *rows_out, double *mean_q_out,
                              double *cov_q_out, double *cov_qJ_out);
/* Which way to move the policy: the gradient, with respect to the feed-forward terms l and the gains L, of what the Monte-Carlo calls
 * measure on a source model -- the mean cost (theta = 0, alpha = 0), the entropic risk (1 / theta) log mean exp(theta J) of a theta row,
 * sup { E_p[J] : KL(p || q) <= d } of a kl_bound row (envelope theorem: the tilt at theta*, theta* itself is not differentiated) and
 * CVaR_alpha of a level -- by adjoint replay on the device.  The calls take no policy and no noise: they REPLAY the last
 * rat_policy_evaluate_noise exactly as rat_policy_worst_case_trajectory / rat_policy_tail_trajectory do (the same chunks and seeds, the
 * same bit-for-bit check against the stored costs) and sweep every replayed rollout k backwards, the recorded disturbances w_t held fixed:
 *   lambda_N = h_x(x_N)
 *   g_t      = c_z(t, x_t, u_t) + f_z(x_t, u_t)' lambda_{t+1},   z = (x, u),   t = N - 1 .. 0
 *   gu_t     = the u part of g_t                                   (dJ_k / du_t with the loop closed downstream)
 *   lambda_t = (x part of g_t) + L_t' gu_t                          (open loop, L == NULL: the x part alone)
 *   dJ_k / dl_t = gu_t,     dJ_k / dL_t = gu_t (x_t - x_nom_t)'
 * with f_z, c_z, h_x by rat_ad.h's forward mode on the user's rat_user_f / rat_user_c / rat_user_h (f_z from rat_user_f_jacobian where
 * the source defines RAT_USER_F_JACOBIAN).  With y_k the weight of rollout k in a row -- the tilted weights of a theta row, those at
 * theta* of a kl_bound row, the tail distribution of a level, bit for bit the rows' own --
 *   grad_l[t] = sum y_k gu_t^k / sum y_k,      grad_L[t] = sum y_k gu_t^k (x_t^k - x_nom_t)' / sum y_k.
 * What this is and is not:
 *   - A saturated row (RAT_WC_SATURATED, RAT_TR_SATURATED: all weight on the rollouts that attain Jmax) is a SUBGRADIENT of its functional.
 *   - A sampler that reads x or u is differentiated with w FROZEN: rat_user_noise takes double, not T, so the dependence of w_t on
 *     (x_t, u_t) is not seen.  The gradient is exact only for samplers that ignore their state arguments.
 *   - x_nom is not differentiated: it is the point the law is written about, not a decision variable.
 *   rows_out       as rat_policy_worst_case_trajectory's / rat_policy_tail_trajectory's, bit for bit
 *   grad_l_out     [rows][N][m]: one copy per row in the layout rat_policy_evaluate_noise takes l in
 *   grad_L_out     [rows][N][m n] (column-major m x n per step, the layout it takes L in), or NULL; written as zeros after an open-loop
 *                  evaluation
 *   grad_l_se_out  [rows][N][m] or NULL: the self-normalised standard error sqrt(sum p_k^2 (gu - mean)^2), p_k = y_k / sum y, formed
 *                  from the uncentred sums sum y gu, sum y^2 gu, sum y^2 gu^2, sum y^2 and clamped at 0 -- whether an entry of grad_l
 *                  stands out of its own sampling error
 *   n_nonfinite_out  or NULL: rollouts that have a cost but a NaN or Inf somewhere in their sensitivities (h_x or a component of some
 *                  g_t: AD at sqrt(0), say).  They are left out of every gradient sum and of the denominator the gradient is divided
 *                  by; the rows themselves still count them.  The call returns RAT_OK.
 * A DomainError rollout carries no weight.  RAT_WC_EMPTY / RAT_WC_NONFINITE rows (and the tail's) are NaN in every gradient output and the
 * call returns RAT_OK.  Fixed summation order, no floating-point atomics: the same call returns the same bits, and a row's bits do not
 * depend on the other rows of the call.
 * Served: source models after rat_policy_evaluate_noise with zn == zu == NULL -- what the trajectory calls serve for sources.
 * RAT_ERR_UNSUPPORTED, each message naming its reason: the LQ / power-law families and general sizes (write the model as source); a source
 * that defines RAT_USER_POLICY (the hook is not templated, so the law is not differentiable by rat_ad.h); parameter sampling switched
 * on (rat_policy_params_sampling); rows x N above 3360 (64 MiB of partial sums).  Row validation, "no evaluation yet" and the replay
 * guard are the trajectory calls', with their codes. */
rat_rc rat_policy_gradient(rat_handle h, const double *kl_bound, int32_t n_bound, const double *theta, int32_t n_theta,
                           double *rows_out, double *grad_l_out, double *grad_L_out, double *grad_l_se_out, int64_t *n_nonfinite_out);
rat_rc rat_policy_tail_gradient(rat_handle h, const double *alpha, int32_t n_alpha,
                                double *rows_out, double *grad_l_out, double *grad_L_out, double *grad_l_se_out, int64_t *n_nonfinite_out);
/* Compile only, for gfx950 (no device needed), the adjoint kernel of the two calls above.  rat_user_noise_check's codes (a source that
 * does not compile, or one without RAT_USER_NOISE: RAT_ERR_ARG with the compiler's log), and RAT_ERR_UNSUPPORTED for a source that defines
 * RAT_USER_POLICY. */
rat_rc rat_policy_gradient_check(const char *source, int32_t n, int32_t m, int32_t normals, int32_t uniforms);
/* Which way to move the policy so that a safety event becomes less likely: the gradient, with respect to l and L, of the tail mean of an
 * event's margin.  Events are rat_policy_events' quadratic events -- g_i(t, z) = z' Q_i z + a_i' z + b_i of z = (x_t, u_t), the same
 * layouts, the same validation and codes, Q used as given (not symmetrised) or NULL -- and M_ik = max over the window of g_i(t, z_t) is
 * the margin of rollout k, as margin_out has it.  CVaR_alpha(M_i) <= 0 implies P(M_i > 0) <= 1 - alpha, and unlike the indicator it is
 * differentiable almost everywhere: this call is the constraint's gradient beside rat_policy_tail_gradient's, the objective's.
 *   n_event  1 .. 4 (above: RAT_ERR_UNSUPPORTED; the joint sweep below keeps one adjoint per event in registers).  "any" is not served.
 *   alpha    1 .. 16 levels, validated as rat_policy_tail_risk validates them; alpha = 0 is the mean margin.
 * Rows are event-major, row r = i * n_alpha + j.  The sample of event i is its margins over the replayed rollouts (NaN for a DomainError
 * rollout) and row (i, j) is the tail distribution of that sample at alpha_j exactly as rat_policy_tail_risk forms it:
 *   rows_out  [n_event * n_alpha][RAT_TR_NSTAT]: bit for bit rat_policy_tail_risk(cost = row i of rat_policy_events' margin_out).
 * Per replayed rollout k and event i, the recorded disturbances w_t held fixed as in rat_policy_gradient:
 *   t*       = the first step of the window that attains M_ik (only a strictly greater g replaces the running margin; a NaN g is passed
 *              over).  It is recorded by the margin pass itself, not recomputed by the sweep.
 *   at t*      g_z = (Q_i + Q_i') z + a_i with z = (x_t*, u_t*), u_N = 0;  t* < N: gu_t* = its u part, lambda_t* = its x part + L_t*' gu_t*;
 *              t* = N: lambda_N = its x part (there is no u_N)
 *   t > t*     gu_t = 0 exactly
 *   t < t*     g_t = f_z(x_t, u_t)' lambda_{t+1} (no c_z, no h_x);  gu_t = its u part;  lambda_t = its x part + L_t' gu_t (open loop: the
 *              x part alone)
 *   dM_ik / dl_t = gu_t,     dM_ik / dL_t = gu_t (x_t - x_nom_t)'
 * and with y_k the tail weights of the row, self-normalised, grad_l[t] = sum y_k gu_t^k / sum y_k, grad_L[t] likewise:
 *   grad_l_out     [rows][N][m]
 *   grad_L_out     [rows][N][m n] (column-major m x n per step), or NULL; zeros after an open-loop evaluation
 *   grad_l_se_out  [rows][N][m] or NULL: rat_policy_gradient's self-normalised standard error
 *   n_nonfinite_out  [n_event] or NULL: per event, the rollouts that have a cost but a NaN or Inf in that event's sensitivities (g_z at t*
 *                  or a component of some g_t below it); they are left out of the event's gradient sums and of their denominator, the
 *                  rows still count them.  The call returns RAT_OK.
 * A rollout whose margin is NaN carries no weight.  Dead rows (an empty or non-finite sample) are NaN in every gradient output and the call
 * returns RAT_OK.  Fixed summation order, no floating-point atomics: the same call returns the same bits, and a row's bits depend neither
 * on the other levels nor on the other events of the call.
 * What this is and is not:
 *   - A gradient almost everywhere; a SUBGRADIENT where the arg-max step ties (the first one is taken), where the tail's membership ties
 *     (rollouts on the quantile share its weight) and on a saturated row (RAT_TR_SATURATED).
 *   - w is FROZEN: a sampler that reads x or u is not differentiated through (rat_user_noise takes double, not T).
 *   - x_nom is not a decision variable and is not differentiated.
 *   - The value at risk is not differentiated: this is the usual CVaR gradient, the tail mean of the per-rollout gradients.
 * The call REPLAYS the last rat_policy_evaluate_noise twice in one enqueue chain -- once for the margins, once for the adjoints -- in
 * buffers of its own: the handle's recorded evaluation and its stored costs are left as they were, and every other replay call works
 * after it.  Served and refused exactly as rat_policy_gradient is: source models after rat_policy_evaluate_noise with zn == zu == NULL;
 * RAT_ERR_UNSUPPORTED for the families, general sizes, a source that defines RAT_USER_POLICY, parameter sampling switched on, and
 * rows x N above 3360 (64 MiB of partial sums); the same "no evaluation yet" and replay guard. */
rat_rc rat_policy_margin_gradient(rat_handle h, int32_t n_event, const double *Q, const double *a, const double *b,
                                  const int32_t *t_lo, const int32_t *t_hi, const double *alpha, int32_t n_alpha,
                                  double *rows_out, double *grad_l_out, double *grad_L_out, double *grad_l_se_out,
                                  int64_t *n_nonfinite_out);
/* Compile only, for gfx950 (no device needed), the adjoint kernel of the call above for four events.  rat_policy_gradient_check's codes. */
rat_rc rat_policy_margin_gradient_check(const char *source, int32_t n, int32_t m, int32_t normals, int32_t uniforms);
/* How a risk reacts to the model: the gradient of the same functionals -- the mean cost, the entropic risk of a theta row, the KL-robust
 * bound of a kl_bound row (at theta*, envelope theorem), CVaR_alpha of a level -- with respect to the model's parameters p and to the
 * initial state x_0, by the same adjoint replay.  The source opts in: it defines RAT_USER_PARAMS_AD and templates rat_user_f, rat_user_c
 * and rat_user_h on a second type for the parameters,
 *   template <class T, class P> __device__ void rat_user_f(const T *x, const T *u, T *xn, const P *p);
 *   template <class T, class P> __device__ T    rat_user_c(int k, const T *x, const T *u, const P *p);
 *   template <class T, class P> __device__ T    rat_user_h(const T *x, const P *p);
 * (rat_user_noise, rat_user_policy, rat_user_params, rat_user_event and rat_user_f_jacobian keep const double *p).  Every other kernel
 * calls the three with p as double, so P deduces to double and such a source serves every other call unchanged.  Per replayed rollout k,
 * with lambda and g_t as rat_policy_gradient has them:
 *   gp       = h_p(x_N) + sum_t ( c_p(t, x_t, u_t) + f_p(x_t, u_t)' lambda_{t+1} )      (dJ_k / dp)
 *   lambda_0 = (x part of g_0) + L_0' gu_0                                               (dJ_k / dx_0; open loop: the x part alone)
 *   grad_p = sum y_k gp^k / sum y_k,      grad_x0 = sum y_k lambda_0^k / sum y_k
 * with f_p, c_p, h_p by rat_ad.h's forward mode with p seeded (f_p always from rat_user_f, also where RAT_USER_F_JACOBIAN serves f_x, f_u).
 * What this is and is not:
 *   - The noise and the controller are FROZEN: the recorded w_t are held fixed, so a rat_user_noise that scales with a parameter is not
 *     differentiated through, and the law u = l + L (x - x_nom) is a constant -- x_nom and (l, L) do not move with p or x_0.
 *   - grad_x0 answers "the law stays centred on x_nom_0, the true initial state is off by delta": with the loop closed the feedback reacts
 *     to the error; open loop it is the plain shift of x_0.
 *   - theta* of a kl_bound row is not differentiated (envelope theorem); a saturated row is a SUBGRADIENT.
 *   - With parameter sampling on (rat_policy_params_sampling) every rollout is differentiated at its own drawn q: grad_p is the
 *     derivative with respect to a common additive shift of every rollout's drawn parameters, the local counterpart of cov_qJ of
 *     rat_policy_worst_case_params.  rat_user_params itself is not differentiated.
 *   rows_out        as rat_policy_worst_case_trajectory's / rat_policy_tail_trajectory's, bit for bit
 *   grad_p_out      [rows][n_params], or NULL if grad_x0_out is not
 *   grad_x0_out     [rows][n], or NULL if grad_p_out is not
 *   grad_p_se_out, grad_x0_se_out   the same shapes or NULL: the self-normalised standard errors, formed as rat_policy_gradient's grad_l_se
 *   n_nonfinite_out  or NULL: rollouts that have a cost but a NaN or Inf in h_x, some g_t, h_p or some parameter term; they are left out
 *                   of every sum and of the denominator; the rows still count them.  The call returns RAT_OK.
 * Dead rows are NaN; fixed summation order, no floating-point atomics; the replay guard, "no evaluation yet" and the row validation are
 * rat_policy_gradient's.  RAT_ERR_UNSUPPORTED, each message naming its reason: the LQ / power-law families and general sizes; a source
 * without RAT_USER_PARAMS_AD; a source that defines RAT_USER_POLICY; n_params above 32; n_params == 0 together with grad_p_out != NULL.
 * RAT_ERR_ARG with the compiler's log: a source that defines RAT_USER_PARAMS_AD but whose functions do not take const P *.
 * rat_policy_gradient and rat_policy_tail_gradient are unchanged, their refusal of parameter sampling included. */
rat_rc rat_policy_param_gradient(rat_handle h, const double *kl_bound, int32_t n_bound, const double *theta, int32_t n_theta,
                                 double *rows_out, double *grad_p_out, double *grad_p_se_out, double *grad_x0_out, double *grad_x0_se_out,
                                 int64_t *n_nonfinite_out);
rat_rc rat_policy_tail_param_gradient(rat_handle h, const double *alpha, int32_t n_alpha, double *rows_out, double *grad_p_out,
                                      double *grad_p_se_out, double *grad_x0_out, double *grad_x0_se_out, int64_t *n_nonfinite_out);
/* Compile only, for gfx950 (no device needed), the adjoint kernel of the two calls above for n_params parameters (0 .. 32), sampling off.
 * rat_policy_gradient_check's codes; RAT_ERR_UNSUPPORTED also for a source without RAT_USER_PARAMS_AD and for n_params above 32. */
rat_rc rat_policy_param_gradient_check(const char *source, int32_t n, int32_t m, int32_t normals, int32_t uniforms, int32_t n_params);
/* Safety events of a policy: how often it hits an obstacle, leaves the lane or saturates an actuator -- under the nominal distribution q (a
 * theta = 0 row) and under the worst-case distribution p* ~ exp(theta* J) q of each kl_bound (and the tilt of each given theta), formed on
 * the device.  An event is a quadratic function of z_t = (x_t, u_t) in R^d, d = n + m, u_N = 0, watched over a window of steps:
 *   g_i(t, z) = z' Q_i z + a_i' z + b_i,  t_lo_i <= t <= t_hi_i;   M_ik = max over the window of g_i(t, z_t) on rollout k (the margin; a NaN g
 *   is passed over); A_ik = [M_ik > 0] (violated: g == 0 and a NaN g are not); tau_ik = the first step of the window with g_i > 0.
 * Half-spaces and boxes (lane edges, actuator limits) are linear events; a disc or ellipsoid is r^2 - |p - c|^2 (violated inside).  One more
 * event, "any", is formed by the call at index n_event: the union of the given ones (its margin is the largest of theirs, its first step
 * the earliest of theirs).  Like rat_policy_worst_case_trajectory the call takes no policy and no noise: it REPLAYS the last
 * rat_policy_evaluate / rat_policy_evaluate_noise of the handle and checks the replayed costs against the stored ones bit for bit; the
 * same evaluations are served and the same ones refused, with the same codes.  The quadratic part runs on the f64 matrix pipe (sixteen
 * rollouts as the columns of Q Z, four 16 x 16 x 4 MFMAs per event and step); a call with Q == NULL does not pay for it.  Fixed summation
 * order, no floating-point atomics: the same call returns the same bits, and an entry's bits depend neither on the other rows nor on the
 * other events of the call ("any" depends on its events).
 *   n_event   1 .. 16
 *   Q         [n_event][d * d] column-major, used as given (not symmetrised), or NULL: every event is linear
 *   a         [n_event][d];  b [n_event];  t_lo, t_hi [n_event] with 0 <= t_lo <= t_hi <= N
 *   kl_bound, theta   as rat_policy_worst_case's (the same refusals); the rows are the bounds, then the thetas
 *   rows_out  [(n_bound + n_theta)][RAT_WC_NSTAT]: rat_policy_worst_case's rows of the same arguments, bit for bit
 *   event_out [(n_bound + n_theta)][n_event + 1][RAT_EV_NSTAT]: the slots below, y the row's weight of a rollout (0 for a DomainError
 *             rollout, uniform on the maxima for a RAT_WC_SATURATED row).  RAT_WC_EMPTY and RAT_WC_NONFINITE rows are NaN except FLAG.
 *   step_out  [(n_bound + n_theta)][n_event + 1][N+1] or NULL: sum y [g_i(t) > 0] / sum y per step, 0 outside the window: where in the
 *             horizon the risk sits
 *   margin_out[n_event][K] or NULL: M_ik, NaN for a DomainError rollout.  A row of it is a sample like the costs: hand it to
 *             rat_policy_tail_risk(cost = ...) for the quantiles and CVaR of a margin, or to rat_policy_worst_case(cost = ...) for its KL
 *             worst case (either call replaces the costs on the device: evaluate again before the next replay).
 * RAT_ERR_ARG besides: n_event outside 1 .. 16, a NULL a / b / t_lo / t_hi, a window outside 0 <= t_lo <= t_hi <= N, a non-finite entry of
 * Q, a or b.  RAT_ERR_UNSUPPORTED besides: partial sums above 64 MiB (the message says how many rows fit). */
#define RAT_EV_PROB        0   /* sum y A / sum y */
#define RAT_EV_PROB_SE     1   /* sqrt(sum y^2 (A - PROB)^2) / sum y: the self-normalised importance-sampling error; sqrt(p (1 - p) / N_OK) at theta == 0 */
#define RAT_EV_MARGIN_MEAN 2   /* sum y M / sum y */
#define RAT_EV_MARGIN_MAX  3   /* max of M over the OK rollouts: the same on every row */
#define RAT_EV_FIRST_MEAN  4   /* sum y A tau / sum y A; NaN when no weighted rollout violates */
#define RAT_EV_N_VIOL      5   /* the unweighted count of violating OK rollouts */
#define RAT_EV_PROB_ROBUST 6   /* rat_kl_event_bound(N_VIOL / N_OK, d): d the kl_bound on a bound row, the row's own RAT_WC_KL on a theta row.  The
                                * adversary aimed at the event itself, not at the cost: PROB <= PROB_ROBUST on every RAT_WC_OK row */
#define RAT_EV_FLAG        7   /* the row's RAT_WC_FLAG */
#define RAT_EV_NSTAT       8
rat_rc rat_policy_events(rat_handle h, int32_t n_event, const double *Q, const double *a, const double *b,
                         const int32_t *t_lo, const int32_t *t_hi,
                         const double *kl_bound, int32_t n_bound, const double *theta, int32_t n_theta,
                         double *rows_out, double *event_out, double *step_out, double *margin_out);
/* rat_policy_events for events the user writes: g_i(k, x_k, u_k), i < n_event, is what the source's rat_user_event ("source models"
 * above) leaves in g[i] at step k -- a NaN entry is passed over, g_i > 0 is violated, u_N = 0 -- in place of Q, a, b, t_lo, t_hi.  A
 * moving obstacle, an intersection of half-spaces (a min), any function of the state: one call per step serves all events.  M, tau, the
 * event "any" at index n_event, the replay and its guard, kl_bound / theta, rows_out, event_out (RAT_EV_*), step_out, margin_out, the
 * 64 MiB limit on the partial sums and PROB_ROBUST are rat_policy_events' in every respect.  Served: exactly the replays
 * rat_policy_events serves for a source model -- an evaluation recorded by rat_policy_evaluate_noise on the device generator; the rest
 * is refused with that call's codes.  The kernel is compiled by the first call that names this n_event (cached per process by source,
 * n, m, n_event and architecture).  RAT_ERR_UNSUPPORTED: the problem is not a source model.  RAT_ERR_ARG: a source without
 * RAT_USER_EVENT (the message says what to define) or one whose event does not compile, with the compiler's log (model.hip:LINE) in
 * rat_last_error() -- the handle stays usable; n_event outside 1 .. 16. */
rat_rc rat_policy_events_user(rat_handle h, int32_t n_event,
                              const double *kl_bound, int32_t n_bound, const double *theta, int32_t n_theta,
                              double *rows_out, double *event_out, double *step_out, double *margin_out);
/* Safety events under the CVaR adversary: among the worst (1 - alpha) share of the rollouts, how often is an event violated, where in the
 * horizon and by how much.  rat_policy_events / rat_policy_events_user with one row per level of rat_policy_tail_risk in place of the
 * kl_bound / theta rows.  The events, their windows, the extra event "any" at index n_event, M, A, tau and margin_out are the siblings'
 * in every respect; so is the replay: the same guard against the stored costs, the same evaluations served and refused with the same
 * codes, the same 64 MiB limit on the partial sums, with n_alpha rows.
 *   alpha      [n_alpha], 1 <= n_alpha <= 16, every one in [0, 1): rat_policy_tail_risk's rules (RAT_ERR_ARG)
 *   rows_out   [n_alpha][RAT_TR_NSTAT]: what rat_policy_tail_risk(h, NULL, 0, alpha, n_alpha, ...) returns on the stored costs, bit for bit
 *   event_out  [n_alpha][n_event + 1][RAT_EV_NSTAT] and step_out [n_alpha][n_event + 1][N+1] (or NULL): the RAT_EV_* slots with y the
 *              level's tail weight of a rollout -- 1 / (n - a) above VAR, r / (c_eq (n - a)) at VAR, 0 below and for a DomainError rollout,
 *              uniform on the maxima for a RAT_TR_SATURATED level.  Two slots mean something of their own on a tail row:
 *              RAT_EV_FLAG is the row's RAT_TR_FLAG (RAT_TR_EMPTY and RAT_TR_NONFINITE rows are NaN except FLAG; the call still returns
 *              RAT_OK), and RAT_EV_PROB_ROBUST is the CVaR adversary aimed at the event itself, min(1, (N_VIOL / N_OK) / (TAIL_N / N_OK))
 *              in plain double arithmetic on the device: the largest probability of the event under any p with dp/dq <= N_OK / TAIL_N,
 *              hence PROB <= PROB_ROBUST on every RAT_TR_OK row -- where every violator lies in the tail the two are one number whose
 *              two roundings may differ in the last bit: PROB is returned then, so the inequality holds in the bits as well.  N_VIOL
 *              and MARGIN_MAX are unweighted, the same on every row.
 *   margin_out [n_event][K] or NULL: rat_policy_events' bit for bit
 * alpha == 0 is the whole sample: its event_out and step_out rows are the theta = 0 row of rat_policy_events on the same evaluation bit
 * for bit, and PROB_ROBUST equals PROB there.  A row's bits depend neither on the other levels nor on the other events of the call ("any"
 * depends on its events).  No floating-point atomics, a fixed summation order.
 * The schedule is the tail scenarios': at alpha = 0.99 one rollout in a hundred carries weight, so the sums read, per group of four
 * rollouts, the word of "level r has weight here" bits first.  A group without weight in any row of a workgroup is not loaded (the
 * unweighted counts and the largest margin still see every rollout) and a rollout without weight in a row adds nothing to it.  Adding 0
 * changes no bit of a sum, so the results are those of rat_policy_events' own sums on the same weights bit for bit; the one difference: a
 * rollout WITHOUT weight in a row whose margin is NaN (every g of its window NaN) is left out of that row's MARGIN_MEAN, where the dense
 * sums form 0 NaN.  The switch tail_dense runs the dense sums on the tail weights. */
rat_rc rat_policy_tail_events(rat_handle h, int32_t n_event, const double *Q, const double *a, const double *b,
                              const int32_t *t_lo, const int32_t *t_hi,
                              const double *alpha, int32_t n_alpha,
                              double *rows_out, double *event_out, double *step_out, double *margin_out);
rat_rc rat_policy_tail_events_user(rat_handle h, int32_t n_event, const double *alpha, int32_t n_alpha,
                                   double *rows_out, double *event_out, double *step_out, double *margin_out);
/* The largest probability p' an event of probability p can have under any distribution within KL radius d of the sampling one:
 * max { p' : p' log(p' / p) + (1 - p') log((1 - p') / (1 - p)) <= d }, by bisection on [p, 1] until the bracket stops shrinking: two neighbouring doubles, of which the one whose KL is nearer d is returned.  Host
 * only: needs no handle and no GPU.  d == 0 gives p; p == 0 gives 0; p == 1 gives 1; d == +Inf with p > 0 gives 1.  NaN, p outside
 * [0, 1] or d < 0: RAT_ERR_ARG. */
rat_rc rat_kl_event_bound(double p, double d, double *out);
/* The probability of a RARE safety event of a policy, by adaptive importance sampling on the device: where rat_policy_events' plain Monte
 * Carlo returns N_VIOL = 0 (a probability of 1e-8 at K <= 2^27), this call still resolves it.  The rollouts are rat_rollout_noisy's
 * (simulate_dynamics with rng, ileqg.jl:44-55, 94-109): x_{k+1} = f(x_k, u_k) + C_k z_k with C_k = chol_lower(W(k)), under the policy
 * (x_nom, l, L) exactly as rat_policy_evaluate takes it -- but z_k = s_k + xi_k, xi_k ~ N(0, I_n), is drawn from a proposal shifted by
 * s in R^{N x n}, and rollout i carries the log-likelihood ratio logw_i = sum_k (-s_k' z_ik + 1/2 s_k' s_k).  One event
 * g(t, z) = z' Q z + a' z + b of z = (x_t, u_t) over the window t_lo .. t_hi, exactly rat_policy_events' definition: M = max over the
 * window, violated iff M > 0, a NaN g is passed over, u_N = 0.  The shift is adapted by the multilevel cross-entropy method.  Iteration
 * j = 0 .. n_iter - 1 starts from s^(0) = shift_in (0 when NULL):
 *   1. K rollouts under s^(j); M_i, logw_i and the DomainError flag stay on the device;
 *   2. the level gamma_j = min(0, the ceil((1 - rho) n)-th smallest M), n the OK rollouts whose margin is a number, (1 - rho) n one rounded
 *      product: an exact order statistic, by rat_policy_tail_risk's radix select;
 *   3. gamma_j == 0 ends the adaptation (so does a sample with no margin to rank, or with an infinite one).  Otherwise, over the elite
 *      E = { i : M_i >= gamma_j } with w_i = exp(logw_i - max logw), s^(j+1)_k = sum_E w_i z_ik / sum_E w_i, formed as
 *      s^(j)_k + sum_E w_i xi_ik / sum_E w_i with xi replayed from the iteration's Philox stream (no K N n normals are stored), summed in a
 *      fixed order without floating-point atomics.  An update that is not finite is dropped as a whole and flags RAT_RE_NONFINITE.
 * The final pass draws K rollouts under the last shift and returns stats[RAT_RE_NSTAT], the slots below; the weights are NOT
 * self-normalised, the proposal's density is known.  The loop stays on the device; the host reads 4 bytes per iteration (the stop rule).
 * Keying: pass p -- the final pass is p = 0, iteration j is p = j + 1 -- draws under seed_p = seed + 0xD1B54A32D192ED03 p (mod 2^64) the
 * way rat_policy_evaluate draws under its seed (chunks of min(K, 2^16) rollouts, chunk c keyed seed_p + 0x9E3779B97F4A7C15 c, Philox
 * counter (index in the chunk, 0, t >> 1, component)).  So with n_iter == 0 and shift_in == NULL the call is plain Monte Carlo on
 * rat_policy_evaluate's noise at that seed: margin_out is rat_policy_events' bit for bit and every logw is 0.  The same call returns the
 * same bits.
 *   K          1 .. 2^27;  n_iter 0 .. 32;  rho in (0, 0.5]: the elite share
 *   Q          [d * d] column-major, d = n + m, used as given (not symmetrised), or NULL: a linear event (no matrix product)
 *   a [d], b;  t_lo, t_hi with 0 <= t_lo <= t_hi <= N
 *   shift_in   [N][n] (s_k at k n) or NULL;  shift_out [N][n] or NULL: the shift the final pass ran under -- hand it back as shift_in with
 *              n_iter == 0 to estimate again at another K or seed
 *   trace_out  [n_iter][RAT_RE_NTRACE] or NULL: per iteration the level gamma_j, |E|, the elite's effective sample size
 *              (sum_E w)^2 / sum_E w^2 and |s^(j+1)|; the last three are NaN on the iteration that ended the adaptation, all four on
 *              iterations that did not run
 *   margin_out [K], logw_out [K] or NULL: M_i (NaN for a DomainError rollout) and logw_i of the final pass
 * RAT_ERR_ARG: K, n_iter, rho or the window out of range, a non-finite entry of Q, a, b or shift_in, a NULL a or stats, a W(k) that is
 * not positive definite.  RAT_ERR_UNSUPPORTED: general sizes and source models (the shift is defined on the family rollout), N > 256.
 * The device buffers of the call (20 bytes per rollout) belong to the handle, like rat_policy_evaluate's, and are its own: the handle's
 * recorded evaluation is not disturbed, a later rat_policy_events still replays it. */
#define RAT_RE_PROB      0   /* (1 / N_OK) sum_i w_i [M_i > 0], w_i = exp(logw_i) */
#define RAT_RE_PROB_SE   1   /* the sample standard error of that mean: sd(w [M > 0]) / sqrt(N_OK); NaN when N_OK < 2 */
#define RAT_RE_ESS       2   /* (sum_A w)^2 / sum_A w^2 over the violating rollouts A; 0 when none violates */
#define RAT_RE_N_VIOL    3
#define RAT_RE_N_OK      4   /* rollouts without a DomainError */
#define RAT_RE_N_DOMAIN  5
#define RAT_RE_LOGW_MAX  6   /* the largest and ... */
#define RAT_RE_LOGW_MIN  7   /* ... the smallest logw among the OK rollouts */
#define RAT_RE_FLAG      8   /* RAT_RE_OK ... as a double */
#define RAT_RE_N_ITER    9   /* adaptation iterations that ran (the one that found gamma == 0 included) */
#define RAT_RE_LEVEL     10  /* the last gamma_j; NaN when no iteration ran */
#define RAT_RE_NSTAT     12  /* slot 11 reserved, written as 0 */
#define RAT_RE_NTRACE    4
#define RAT_RE_OK          0
#define RAT_RE_NOT_REACHED 1 /* no iteration found gamma == 0 (n_iter == 0 included): PROB is still the weighted estimate, and may be 0 */
#define RAT_RE_EMPTY       2 /* N_OK == 0: PROB, PROB_SE and ESS are NaN */
#define RAT_RE_NONFINITE   3 /* an infinite margin or logw, an overflowing weight or a dropped update: PROB, PROB_SE and ESS are NaN */
rat_rc rat_policy_rare_event(rat_handle h, const double *x_nom, const double *l, const double *L, int64_t K, uint64_t seed,
                             const double *Q, const double *a, double b, int32_t t_lo, int32_t t_hi,
                             const double *shift_in, int32_t n_iter, double rho,
                             double *stats, double *shift_out, double *trace_out, double *margin_out, double *logw_out);
/* rat_policy_rare_event for a source model under the user's own process noise: the rollout is rat_policy_evaluate_noise's,
 * x_{k+1} = f(x_k, u_k) + rat_user_noise(k, x_k, u_k, rng), under the policy (x_nom, l, L) exactly as that call takes it, with its
 * DomainError rule (a NaN from the sampler included) and its overdraw rule (RAT_ERR_ARG naming the limits; the handle stays usable).  W
 * is not read.  The proposal shifts the NORMALS THE SAMPLER DRAWS: the i-th rng.normal() of step t returns z = s[t][i] + xi, xi the
 * generator's N(0, 1) draw, with s in R^{N x P}, P = normals_per_step, and the rollout's log-likelihood ratio logw = sum (-s z + 1/2 s^2)
 * runs over the normals the sampler actually drew, added at the draw, in draw order: a sequential likelihood ratio, valid when the number
 * of draws depends on earlier draws, so the estimate is unbiased for every s and the adaptation only moves its variance.
 * rng.uniform() is NOT shifted (its likelihood ratio is 1): an event that a uniform drives -- the selector of a mixture, a jump that
 * fires with a small probability -- cannot be made likelier by this call; write such a choice through a normal where that matters.
 * The event g(t, z) = z' Q z + a' z + b of z = (x_t, u_t), the window, M, the level gamma_j, the elite, the update
 * s <- s + sum_E w xi / sum_E w, the dropped non-finite update, stats[RAT_RE_NSTAT], the flags, trace_out, margin_out and logw_out are
 * rat_policy_rare_event's, and the weights are NOT self-normalised.  The elite sum runs over all P declared normals of every step,
 * replayed from the pass's stream whether or not that rollout drew them: a component a rollout did not draw moves its shift entry by
 * sampling noise alone, which costs variance and introduces no bias.
 * Keying: pass p -- the final pass is p = 0, iteration j is p = j + 1 -- draws under seed_p = seed + 0xD1B54A32D192ED03 p (mod 2^64) the
 * way rat_policy_evaluate_noise's generator draws under its seed: the global rollout index g in the Philox counter (g lo, g hi, t,
 * i >> 1), key seed_p, no per-chunk keys.  So with n_iter == 0 and shift_in == NULL the call is plain Monte Carlo on
 * rat_policy_evaluate_noise's noise at that seed: margin_out is bit for bit what rat_policy_events returns behind that evaluation, and
 * every logw is 0.  A rollout's noise does not depend on K.  The same call returns the same bits.
 *   normals_per_step   1 .. 12 (0: RAT_ERR_ARG, there is nothing to shift; above 12: RAT_ERR_UNSUPPORTED);  uniforms_per_step >= 0.  The
 *                      kernel is compiled for them by the first call that names them (cached per process, like rat_policy_evaluate_noise's)
 *   shift_in, shift_out   [N][P] (row t at t P) or NULL
 *   K, n_iter, rho, Q, a, b, t_lo, t_hi, trace_out, margin_out, logw_out   as in rat_policy_rare_event
 * There are no injected draws: the device generator only.  RAT_ERR_ARG: what rat_policy_rare_event lists (W apart); a source without
 * RAT_USER_NOISE, or one that does not compile, with the compiler's log in rat_last_error(); an overdraw.  RAT_ERR_UNSUPPORTED: a
 * problem that is not a source model, normals_per_step > 12, N > 256.  The device buffers are rat_policy_rare_event's: the handle's
 * recorded evaluation is not disturbed. */
rat_rc rat_policy_rare_event_noise(rat_handle h, const double *x_nom, const double *l, const double *L, int64_t K,
                                   int32_t normals_per_step, int32_t uniforms_per_step, uint64_t seed,
                                   const double *Q, const double *a, double b, int32_t t_lo, int32_t t_hi,
                                   const double *shift_in, int32_t n_iter, double rho,
                                   double *stats, double *shift_out, double *trace_out, double *margin_out, double *logw_out);
/* Compile only, for gfx950 (no device needed), the kernel of rat_policy_rare_event_noise: RAT_OK; RAT_ERR_ARG with the log in
 * rat_last_error() (a source without RAT_USER_NOISE among them), for negative counts and for normals == 0; RAT_ERR_UNSUPPORTED for
 * normals > 12, n > 12 or m > 4. */
rat_rc rat_rare_event_noise_check(const char *source, int32_t n, int32_t m, int32_t normals, int32_t uniforms);
/* rat_policy_rare_event_noise with entry `event` (0 .. n_event - 1, else RAT_ERR_ARG) of the user's rat_user_event in place of Q, a, b,
 * t_lo, t_hi: M is the largest g[event] over the steps k = 0 .. N at which the function wrote it (NaN where it wrote none: such a
 * rollout is no elite and does not violate), u_N = 0.  Everything else -- the keying, the shifted normals and the sequential likelihood
 * ratio, the level, the elite, the update, stats[RAT_RE_NSTAT] and the flags, the overdraw rule, shift / trace / margin / logw -- is
 * that call's.  With n_iter == 0 and shift_in == NULL margin_out is row `event` of rat_policy_events_user's margin_out behind
 * rat_policy_evaluate_noise at that seed, bit for bit.  The kernel is the rollout kernel's second variant, cached per process by
 * (source, n, m, normals, uniforms, n_event, architecture).  RAT_ERR_ARG besides: n_event outside 1 .. 16, a source without
 * RAT_USER_EVENT.  No user events for the family call rat_policy_rare_event. */
rat_rc rat_policy_rare_event_user(rat_handle h, const double *x_nom, const double *l, const double *L, int64_t K,
                                  int32_t normals_per_step, int32_t uniforms_per_step, uint64_t seed,
                                  int32_t n_event, int32_t event,
                                  const double *shift_in, int32_t n_iter, double rho,
                                  double *stats, double *shift_out, double *trace_out, double *margin_out, double *logw_out);
/* Compile only, for gfx950 (no device needed), the kernel of rat_policy_rare_event_user: rat_rare_event_noise_check's codes, and
 * RAT_ERR_ARG for n_event outside 1 .. 16 or a source without RAT_USER_EVENT. */
rat_rc rat_rare_event_user_check(const char *source, int32_t n, int32_t m, int32_t normals, int32_t uniforms, int32_t n_event);
/* Rare events that an uncertain parameter drives: rat_policy_rare_event_noise (n_event == 0: the quadratic event Q, a, b, t_lo, t_hi) or
 * rat_policy_rare_event_user (n_event in 1 .. 16: entry `event` of rat_user_event; Q, a, b, t_lo, t_hi are not read) with the normals of
 * rat_user_params drawn from a shifted proposal too.  The handle's parameter sampling must be on (rat_policy_params_sampling) with the
 * device generator, PN = its param_normals in 1 .. 12.  The i-th rng.normal() of the hook returns z = ps[i] + xi, xi the N(0, 1) draw of
 * the generator (counter (g lo, g hi, 0xFFFFFFFF, i / 2), key the pass's seed), and adds fma(-ps[i], z, ps[i]^2 / 2) to the rollout's logw
 * at the draw, before step 0; a hook that draws fewer normals than it declared adds fewer terms, so the likelihood ratio stays sequential
 * and the estimate unbiased for every ps.  rng.uniform() of the hook is not shifted.  logw is the whole ratio, parameter part included:
 * the level, the elite E and the weights w_i = exp(logw_i - max logw) are those calls', and with bit 1 of `adapt` the parameter shift
 * moves by ps <- ps + sum_E w_i xi^p_i / sum_E w_i, xi^p replayed from the pass's parameter stream, all PN components whether or not the
 * hook drew them, in the fixed order of the step shift's sums.
 *   adapt        bit 0: adapt the step shift; bit 1: adapt the parameter shift; 1, 2 or 3.  A part whose bit is clear stays at its *_in
 *                (0 when NULL) through every iteration, is still applied and still counted in logw: an event that the parameters alone
 *                drive is estimated with adapt == 2, and pays no variance for step shifts that would move by sampling noise alone.
 *   shift_in, shift_out    [N][P] or NULL, as in rat_policy_rare_event_noise;  pshift_in, pshift_out   [PN] or NULL
 *   trace_out    [n_iter][RAT_RE_NTRACE] as there, |s| over the step shift only;  ptrace_out [n_iter]: |ps^(j+1)|, NaN wherever column 3 of
 *                trace_out is NaN
 *   normals_per_step   1 .. 12 as there: a model without process noise declares one normal and multiplies it by 0
 * A non-finite entry in either adapted part drops the whole update of that iteration, both parts together (RAT_RE_NONFINITE).  Each
 * iteration's rollouts, parameters included, run under that pass's seed, the final pass under the call's.  With pshift_in == NULL (or
 * zeros) and adapt == 1 every output is bit for bit rat_policy_rare_event_noise's / _user's on the same handle at the same seed.
 * RAT_ERR_ARG: what those calls list; parameter sampling off on the handle (the message says to call rat_policy_params_sampling);
 * param_normals == 0 (nothing to shift); adapt outside 1 .. 3; a non-finite pshift_in; n_event outside 0 .. 16; event outside
 * 0 .. n_event - 1.  RAT_ERR_UNSUPPORTED: what those calls list; param_normals > 12 (the width of a shift row); injected parameter
 * streams on the handle (the proposal is defined on the generator, like the step draws); a problem that is not a source model.  The
 * handle stays usable after every refusal and the recorded evaluation is not disturbed. */
rat_rc rat_policy_rare_event_params(rat_handle h, const double *x_nom, const double *l, const double *L, int64_t K,
                                    int32_t normals_per_step, int32_t uniforms_per_step, uint64_t seed,
                                    int32_t n_event, int32_t event,
                                    const double *Q, const double *a, double b, int32_t t_lo, int32_t t_hi,
                                    const double *shift_in, const double *pshift_in, int32_t adapt, int32_t n_iter, double rho,
                                    double *stats, double *shift_out, double *pshift_out, double *trace_out, double *ptrace_out,
                                    double *margin_out, double *logw_out);
/* Compile only, for gfx950 (no device needed), the kernel of rat_policy_rare_event_params with sampling on for n_params parameters:
 * rat_rare_event_noise_check's codes (n_event == 0) or rat_rare_event_user_check's (n_event in 1 .. 16), rat_user_params_check's for the
 * parameter counts (a source without RAT_USER_PARAMS: RAT_ERR_ARG), RAT_ERR_ARG for param_normals == 0 and for n_event outside 0 .. 16,
 * RAT_ERR_UNSUPPORTED for param_normals > 12. */
rat_rc rat_rare_event_params_check(const char *source, int32_t n, int32_t m, int32_t n_params, int32_t normals, int32_t uniforms,
                                   int32_t param_normals, int32_t param_uniforms, int32_t n_event);

/* ---- which uncertainty drives the cost: Sobol indices of a policy ----------------------------------------------------------------
 * How much of Var J of a source model's Monte-Carlo cost comes from which of its independent random inputs: the first-order index
 * S_i = Var(E[J | group i]) / Var J and the total index T_i = E[Var(J | everything but group i)] / Var J of up to sixteen groups of
 * draws, by pick-freeze sampling on the device generator.  T_i - S_i is what group i contributes through interactions alone.
 *
 * Groups.  The caller partitions the declared draws into d = n_groups groups, 1 <= d <= 16.  A group is four 64-bit masks over draw
 * indices, groups[4 i .. 4 i + 3] (RAT_SB_G_*): bit j of the parameter-normal / parameter-uniform word is the j-th rng.normal() /
 * rng.uniform() of rat_user_params, bit j of the step-normal / step-uniform word the j-th rng.normal() / rng.uniform() of rat_user_noise
 * at EVERY step.  Groups are disjoint; a draw in no group belongs
 * to "the rest", which is never frozen: its share shows as 1 - sum S.  A group with four empty masks is allowed (S = T = 0 exactly).
 *
 * Rollouts.  Base sample g = 0 .. K - 1 gets d + 2 rollouts of the policy (x_nom, l, L), each rat_policy_evaluate_noise's rollout
 * (the same feedback law, cost order, DomainError rule, rat_user_policy, parameters drawn in front of step 0):
 *   Y_A[g]   every draw from the generator under seed_a
 *   Y_B[g]   every draw under seed_b
 *   Y_i[g]   the draws of group i under seed_b, all others under seed_a          (Saltelli's AB_i)
 * Draw i taken from a stream is bit for bit the draw i the plain generator yields under that stream's seed for (g, step, i) -- the
 * Box-Muller pairing of normals 2q and 2q + 1 included: where the two lie in different streams each comes from its own stream's block
 * q.  So Y_A is rat_policy_evaluate_noise's cost_out under seed_a bit for bit, Y_B that under seed_b, and no Y depends on K.
 *
 * Estimator.  A base sample is OK when none of its d + 2 costs is NaN.  Over the N_OK OK samples, with mu the mean of Y_A and Y_B pooled,
 * y' = y - mu and s_g = (y'_A^2 + y'_B^2) / 2:
 *   V   = mean(s)
 *   S_i = mean(y'_B (y_i - y_A)) / V                (Saltelli et al. 2010, centred)
 *   T_i = mean((y_A - y_i)^2) / (2 V)               (Jansen 1999)
 * Standard errors by the ratio linearisation: with a_g the numerator's term (y'_B (y_i - y_A), or (y_A - y_i)^2 / 2), R the ratio and
 * e_g = a_g - R s_g (mean zero by construction), SE = sqrt(sum e^2 / (N_OK - 1) / N_OK) / V.  VAR_SE = sd(s) / sqrt(N_OK), sd unbiased.
 * Sums run in a fixed tree: two calls with the same arguments return the same bits, however K was cut into launches.
 *   index_out    [n_groups][RAT_SB_NINDEX] row-major: S, S_SE, T, T_SE
 *   summary_out  [RAT_SB_NSTAT]
 *   y_out        [(n_groups + 2)][K] row-major (rows A, B, then the groups in order), or NULL: the costs stay on the device
 * RAT_SB_FLAG holds the overdraw bits of the rollouts (1, 2: a step's normals / uniforms; 4, 8: the hook's) -- with one set the call
 * returns RAT_ERR_ARG naming the limits, as rat_policy_evaluate_noise does, after writing the summary -- and RAT_SB_DEGENERATE where
 * V == 0, V is not finite or N_OK < 2: every index and standard error is NaN then.
 * Parameter sampling (rat_policy_params_sampling) may be on or off; off, the parameter masks must be zero.  The call leaves the
 * handle's recorded evaluation (its costs, its replay record) as it found it.  One device.
 * RAT_ERR_ARG: null x_nom / l / groups / index_out / summary_out; n_groups outside 1 .. 16; K < 2; (n_groups + 2) K above 2^28 (Y is 8
 * bytes per rollout on the device); seed_a == seed_b; negative draw counts; a mask bit at or beyond its declared count (parameter masks
 * with sampling off included); overlapping groups; a source that does not compile; an overdraw.  RAT_ERR_UNSUPPORTED: a problem that is
 * not a source model, or a source without rat_user_noise; injected parameter streams on the handle (the call is defined on the
 * generator, as rat_policy_rare_event_params is); a declared draw count above 64 (the width of a mask); n > 12 or m > 4. */
#define RAT_SB_G_PARAM_NORMALS  0   /* the words of a group, groups[4 i + word] */
#define RAT_SB_G_PARAM_UNIFORMS 1
#define RAT_SB_G_STEP_NORMALS   2
#define RAT_SB_G_STEP_UNIFORMS  3
#define RAT_SB_NGROUPWORD       4
#define RAT_SB_S        0
#define RAT_SB_S_SE     1
#define RAT_SB_T        2
#define RAT_SB_T_SE     3
#define RAT_SB_NINDEX   4
#define RAT_SB_N_OK     0   /* base samples none of whose d + 2 rollouts hit a DomainError, as a double */
#define RAT_SB_MEAN     1   /* mu */
#define RAT_SB_VAR      2   /* V */
#define RAT_SB_VAR_SE   3
#define RAT_SB_FLAG     4   /* overdraw bits | RAT_SB_DEGENERATE, as a double */
#define RAT_SB_N_DROPPED 5  /* K - N_OK */
#define RAT_SB_NSTAT    8   /* slots 6, 7 reserved, written as 0 */
#define RAT_SB_DEGENERATE 16
rat_rc rat_policy_sobol(rat_handle h, const double *x_nom, const double *l, const double *L, int64_t K,
                        int32_t normals_per_step, int32_t uniforms_per_step,
                        const uint64_t *groups, int32_t n_groups, uint64_t seed_a, uint64_t seed_b,
                        double *index_out, double *summary_out, double *y_out);
/* Compile only, for gfx950 (no device needed), the kernel of rat_policy_sobol; n_params == 0: with parameter sampling off
 * (param_normals, param_uniforms must be 0 then), else with sampling on for n_params parameters.  rat_user_noise_check's codes with
 * RAT_ERR_UNSUPPORTED for a source without RAT_USER_NOISE and for a draw count above 64; rat_user_params_check's for the parameter
 * counts (a source without RAT_USER_PARAMS: RAT_ERR_ARG). */
rat_rc rat_policy_sobol_check(const char *source, int32_t n, int32_t m, int32_t n_params, int32_t normals, int32_t uniforms,
                              int32_t param_normals, int32_t param_uniforms);

/* approximate_model(problem, u_array, x_array)                ileqg.jl:258-322
 * -> q[N+1], qv[n*(N+1)], Q[n*n*(N+1)], r[m*N], R[m*m*N], P[m*n*N], A[n*n*N], B[n*m*N], W[n*n*N] */
rat_rc rat_approximate_model(rat_handle h, const double *u, const double *x,
                             double *q, double *qv, double *Q, double *r, double *R, double *P,
                             double *A, double *B, double *W, int32_t *domain_fail);
/* solve_approximate_dp!(ileqg, approx; theta)                  ileqg.jl:341-406
 * in : the ApproximationResult arrays above (W is taken from the problem),  theta, mu, delta (in/out)
 * out: L[m*n*N], dl[m*N], updated mu / delta (regularisation restarts), status (0 / RAT_ST_M_NOT_PD_GAIN / ...),
 *      and the DynamicProgrammingResult dumps (any may be NULL): s[N+1], sv[n*(N+1)], S[n*n*(N+1)],
 *      g[m*N], G[m*n*N], H[m*m*N]. */
rat_rc rat_dp_gain_sweep(rat_handle h, const double *q, const double *qv, const double *Q, const double *r,
                         const double *R, const double *P, const double *A, const double *B,
                         double theta, double *mu, double *delta, double *L, double *dl, int32_t *status,
                         double *s, double *sv, double *S, double *g, double *G, double *H);
/* solve_approximate_dp(approx, L_array, dl_array; theta, mu)    ileqg.jl:412-465 ; dl may be NULL (zeros);
 * *status = 0 or RAT_ST_M_NOT_PD_GAIN (the @assert at :440). */
rat_rc rat_dp_policy_eval(rat_handle h, const double *q, const double *qv, const double *Q, const double *r,
                          const double *R, const double *P, const double *A, const double *B,
                          const double *L, const double *dl, double theta, double mu, int32_t *status,
                          double *s, double *sv, double *S, double *g, double *G, double *H);

/* Batched forms of the two sweeps on CALLER-SUPPLIED tiles -- the batch path of problems whose f, c, h are arbitrary host closures
 * (optimal_control_problems.jl:67-73; ileqg.jl:265-273, :302-311): the host rolls out and linearises every sample, the device runs the
 * B Riccati sweeps of one CE batch in one launch (one wavefront per sample, the solver's own kernels).  Every array holds B consecutive
 * ApproximationResults / gain histories in the single-sample layouts above (sample slowest); theta[B], mu[B], delta[B] per sample.
 *   rat_dp_gain_sweep_batch  : solve_approximate_dp! per sample (mu restarts inside): in/out mu, delta; out L, dl, status[b]
 *   rat_dp_policy_eval_batch : solve_approximate_dp with dl = nothing per sample (initialize!, line-search candidates): out value[b] =
 *                              s_array[1] (+Inf and status RAT_ST_M_NOT_PD_GAIN where the reference's @assert fires) */
rat_rc rat_dp_gain_sweep_batch(rat_handle h, int64_t B, const double *q, const double *qv, const double *Q, const double *r,
                               const double *R, const double *P, const double *A, const double *Bm, const double *theta,
                               double *mu, double *delta, double *L, double *dl, int32_t *status);
rat_rc rat_dp_policy_eval_batch(rat_handle h, int64_t B, const double *q, const double *qv, const double *Q, const double *r,
                                const double *R, const double *P, const double *A, const double *Bm, const double *L,
                                const double *theta, const double *mu, double *value, int32_t *status);

/* ---- Cross-Entropy loop over theta (RAT iLQR) -------------------------------------------------- */

/* Replaces CrossEntropyBilevelOptimizationSolver (cross_entropy_bilevel_optimization.jl:70-127).
 * The struct is caller-owned plain data: mu_init/sigma_init persist across solves as in the reference. */
typedef struct rat_ce_solver {
    /* parameters */
    int64_t num_samples, num_elite, iter_max;
    double  lambda;
    int32_t use_theta_max;
    /* mutable state */
    double  mu_init, sigma_init, mu, sigma, theta_max, theta_min;
    int64_t iter_current;
    /* bookkeeping (not in the reference) */
    int64_t n_solves, n_redraws;
    int64_t n_final_retries;     /* times the final solve of solve! failed and theta_opt was lowered by sigma (:410-413) */
} rat_ce_solver;

void   rat_ce_default(rat_ce_solver *c);                                     /* ctor defaults :100-127 */
void   rat_ce_initialize(rat_ce_solver *c);                                  /* initialize!   :133-138 */

/* Source of randomness replacing `rng::AbstractRNG`: theta = mu + sigma*z with z drawn in order from a
 * standard-normal stream.  Either inject one (parity runs; the pointer must stay valid while in use) or
 * seed the built-in generator (SplitMix64-seeded xoshiro256++ with Box-Muller; documented in DESIGN.md). */
rat_rc rat_ce_set_stream(rat_handle h, const double *z, int64_t nz);
rat_rc rat_ce_seed(rat_handle h, uint64_t seed);
int64_t rat_ce_stream_pos(rat_handle h);

/* get_positive_samples(mu, sigma, num_samples, rng)             :233-246 */
rat_rc rat_ce_get_positive_samples(rat_handle h, double mu, double sigma, int64_t num, double *theta);
/* compute_cost(ce_solver, problem, x, u_array, theta_array, kl_bound)  :173-195  (cost = value + kl/theta) */
rat_rc rat_ce_compute_cost(rat_handle h, const double *x0, const double *u0, const double *theta, int64_t B,
                           double kl_bound, double *cost);
/* compute_cost with theta_dev / cost_dev resident in device (HBM) memory; x0/u0 from the last rat_set_initial() call.
 * cost = value + kl_bound / theta (:193), +Inf for samples whose solve failed (:163-165).  Returns after the batch has finished. */
rat_rc rat_ce_compute_cost_dev(rat_handle h, const double *theta_dev, int64_t B, double kl_bound, double *cost_dev);
/* the same, stream-ordered: returns once the batch is enqueued on rat_stream(h) (single-launch path; otherwise it behaves like
 * rat_ce_compute_cost_dev).  theta_dev / cost_dev must stay valid, and cost_dev unread, until work ordered after it on that stream
 * (or a synchronisation of it) has passed -- lets a caller chain batch -> cost all-gather -> next batch without host round trips. */
rat_rc rat_ce_compute_cost_enqueue(rat_handle h, const double *theta_dev, int64_t B, double kl_bound, double *cost_dev);
/* the same with the per-sample status (RAT_ST_*), iteration count and line-search evaluation count written beside the costs (device
 * pointers, any of the three may be NULL): what a rank contributes to the cost + status all-gather of a sharded CE batch */
rat_rc rat_ce_compute_cost_enqueue_ex(rat_handle h, const double *theta_dev, int64_t B, double kl_bound, double *cost_dev,
                                      int32_t *status_dev, int32_t *iters_dev, int32_t *ls_evals_dev);
/* The bookkeeping half of step! (:291-334) for hosts that evaluate costs themselves (multi-GPU: the
 * host all-gathers cost shards between rat_ce_draw and rat_ce_update).
 *   rat_ce_draw   : theta[num_samples] for the current iteration (uses mu_init/sigma_init in iteration 1)
 *   rat_ce_update : consumes the costs; *redraw = 1 when the reference would loop and redraw (:293-298, :306) */
rat_rc rat_ce_begin_step(rat_ce_solver *c);
rat_rc rat_ce_draw(rat_handle h, const rat_ce_solver *c, double *theta);
rat_rc rat_ce_update(rat_ce_solver *c, const double *theta, const double *cost, int32_t *redraw);
/* rat_ce_update carried out by the update kernel of the device-resident loop (what rat_ce_solve runs between two batches) on
 * host-supplied thetas / costs: same arithmetic, same elite order -- sort(by = cost) under Julia's isless (NaN last, -0.0 before
 * +0.0, ties in input order; :326-328).  num_samples <= 1024. */
rat_rc rat_ce_update_dev(rat_handle h, rat_ce_solver *c, const double *theta, const double *cost, int32_t *redraw);
/* handle-free form of rat_ce_draw over an explicit stream (pure host code; usable before any device exists):
 * consumes z[*zpos..] and advances *zpos. */
rat_rc rat_ce_draw_stream(const rat_ce_solver *c, const double *z, int64_t nz, int64_t *zpos, double *theta);
/* step!(ce_solver, problem, x, u_array, kl_bound, rng)          :252-335 ; theta_out/cost_out may be NULL */
rat_rc rat_ce_step(rat_handle h, rat_ce_solver *c, const double *x0, const double *u0, double kl_bound,
                   double *theta_out, double *cost_out);
/* solve!(ce_solver, problem, x_0, u_array, rng; kl_bound)       :364-415 */
rat_rc rat_ce_solve(rat_handle h, rat_ce_solver *c, const double *x0, const double *u0, double kl_bound,
                    double *theta_opt, double *x, double *l, double *L, double *value,
                    double *theta_min, double *theta_max);

/* ---- RAT iLQR++: Nelder-Mead over theta ---------------------------------- */

/* Replaces NelderMeadBilevelOptimizationSolver (nelder_mead_bilevel_optimization.jl:72-128).  Caller-owned plain data.
 * c_high / c_low are Union{Nothing,Float64} in the reference and are NOT reset by initialize! (:164-168): they persist
 * across solve! calls, as do theta_high_init / theta_low_init when they were shrunk (:290-303).  Reproduced as is. */
typedef struct rat_nm_solver {
    double  alpha, beta, gamma, eps, lambda;
    int64_t iter_max;
    double  theta_high_init, theta_low_init;
    int64_t iter_current;
    double  theta_high, theta_low;
    int32_t has_c_high, has_c_low;
    double  c_high, c_low;
    int64_t n_solves;           /* iLEQG solves the SEQUENTIAL algorithm would have made (bookkeeping) */
    int64_t n_batches;          /* batched device calls actually made */
} rat_nm_solver;

void   rat_nm_default(rat_nm_solver *s);                                     /* ctor defaults :102-128 */
void   rat_nm_initialize(rat_nm_solver *s);                                  /* initialize!   :164-168 */
/* compute_cost_worker(nm_solver, problem, x, u_array, theta, kl_bound)        :134-158 */
rat_rc rat_nm_compute_cost(rat_handle h, const double *x0, const double *u0, double theta, double kl_bound, double *cost);
/* step! :174-252.  Every theta the sequential logic can ask for -- this iteration's reflection, expansion, two possible
 * contraction and two possible shrink points and, as far as the handle's max_batch allows (80 samples), the six points of
 * each state the iteration can end in -- is solved ahead in ONE batch (a batch of <= 512 samples takes one solve's time); the
 * reflect / expand / contract / shrink decisions are then replayed on the host against the table of (theta, cost), so the
 * outcome is the sequential one and the next call usually needs no device call.  The table is kept between calls while
 * (problem, x0, u0, kl_bound) are unchanged.  Switch nm_depth (rat_debug_set) limits the speculation. */
rat_rc rat_nm_step(rat_handle h, rat_nm_solver *s, const double *x0, const double *u0, double kl_bound);
/* solve!(nm_solver, problem, x_0, u_array; kl_bound)                           :276-352 ; *status = final iLEQG status
 * (a failure there is an uncaught exception in the reference).  Both initial vertices and the first two iterations under
 * either ordering go into the first device call (158 samples; three iterations, 1022 samples, on a handle that large), later calls
 * cover two iterations each, and the final
 * solve at theta_opt is read out of the last batch's device state instead of being run again. */
rat_rc rat_nm_solve(rat_handle h, rat_nm_solver *s, const double *x0, const double *u0, double kl_bound,
                    double *theta_opt, double *x, double *l, double *L, double *value, int32_t *status);

/* ---- PETS: cross-entropy over control sequences with stochastic rollouts ---------- */

/* Replaces FiniteHorizonGenerativeOptimalControlProblem(f_stochastic, c, h, N) (optimal_control_problems.jl:126-131) by a
 * device model family:  f_stochastic(x, u, rng, use_true_model) = A x + B u + kappa x.^3 + w
 *   w : noise_kind 0 -> N(nmean, nchol nchol') ; 1 -> uniform on [nlo, nhi)^n (test/pets_test.jl:15)
 *   use_true_model : with probability tw2 the noise is N(tmean2, tchol2 tchol2') instead (2-component mixture of the docs
 *                    example, optimal_control_problems.jl:103-110); tw2 = 0 disables it
 *   c(k, x, u) = the LQ quadratic form of `lq` (time-varying tables allowed) + l1u * sum(abs.(u)) ; h quadratic (lq.Qf ...). */
typedef struct rat_gen_problem_desc {
    rat_problem_desc lq;        /* model must be RAT_MODEL_LQ; lq.W is ignored (may be NULL) */
    double l1u;
    int32_t noise_kind;
    const double *nmean;        /* n        */
    const double *nchol;        /* n*n column-major, lower triangular */
    double nlo, nhi;
    double tw2;
    const double *tmean2;       /* n        */
    const double *tchol2;       /* n*n      */
} rat_gen_problem_desc;

/* Replaces CrossEntropyDirectOptimizationSolver (pets.jl:36-68).  Caller-owned; the mu and Sigma pointers are caller-owned buffers
 * [N][m] and [N][m*m] (column-major blocks, time slowest). */
typedef struct rat_pets_solver {
    int64_t num_control_samples, num_trajectory_samples, num_elite, iter_max;
    double  smoothing_factor;
    int64_t N, m, iter_current;
    double *mu_init, *Sigma_init, *mu, *Sigma;
} rat_pets_solver;

rat_rc rat_pets_problem_set(rat_handle h, const rat_gen_problem_desc *desc);
void   rat_pets_initialize(rat_pets_solver *s);                               /* initialize!  pets.jl:70-74 */
/* compute_cost_serial(direct_solver, problem, x, control_sequence_array, rng, use_true_model)  pets.jl:128-157
 *   controls[S][N][m] (time-major, m fastest), cost[S] = mean over K stochastic rollouts of sum c + h.
 * Randomness, serial semantics: trajectory j = ii*K + kk consumes zn[(j*N + t)*n .. +n) at step t (N(0,1) draws for Gaussian
 * noise, U[0,1) draws for uniform noise) and zu[j*N + t] (mixture choice; may be NULL when tw2 = 0).  zn = NULL selects the
 * device generator (Philox4x32-10 keyed by `seed`, counter = (trajectory, step / 2, lane); both Box-Muller outputs are used, for steps 2i and 2i + 1): statistical parity only. */
rat_rc rat_pets_compute_cost(rat_handle h, const double *x0, const double *controls, int64_t S, int64_t K,
                             int32_t use_true_model, const double *zn, const double *zu, uint64_t seed, double *cost);
/* draw the control sequences of one step! (pets.jl:206-216): controls[ii][t] = mu_t + chol(Sigma_t) * zc[(ii*N + t)*m ..] */
rat_rc rat_pets_sample_controls(const rat_pets_solver *s, const double *zc, double *controls);
/* get_elite_samples + compute_new_distribution (pets.jl:159-191); elite_idx[num_elite] may be NULL */
rat_rc rat_pets_update(rat_pets_solver *s, const double *controls, const double *cost, int64_t *elite_idx);
/* step! (pets.jl:193-245): sample, evaluate, elites, smoothed update.  zc: S*N*m normals; zn/zu/seed as above. */
rat_rc rat_pets_step(rat_handle h, rat_pets_solver *s, const double *x0, int32_t use_true_model, const double *zc,
                     const double *zn, const double *zu, uint64_t seed, double *controls_out, double *cost_out);
/* solve! (pets.jl:270-281): iter_max steps from (mu_init, Sigma_init); streams hold iter_max consecutive step blocks
 * (zn NULL -> device generator with seed + iteration).  With zn NULL and <= 1024 control samples the whole loop stays on the device
 * (switch pets_device): sampling, rollouts, elite selection and the smoothed update are one enqueue chain, one host wait per solve!;
 * mu / Sigma equal the host loop's bit for bit.  zc NULL (device-resident loop only): the control normals are drawn on the device too. */
rat_rc rat_pets_solve(rat_handle h, rat_pets_solver *s, const double *x0, int32_t use_true_model, const double *zc,
                      const double *zn, const double *zu, uint64_t seed);

/* ---- generative source models: f_stochastic, c, h written by the user, compiled at run time ------------------------------------------
 * FiniteHorizonGenerativeOptimalControlProblem(f_stochastic, c, h, N) with user device code (pets.jl / optimal_control_problems.jl:77-131).
 * After success, rat_pets_compute_cost / rat_pets_step / rat_pets_solve (host loop and device-resident loop) run this model;
 * rat_pets_problem_set switches the handle back to the family.  The handle's iLEQG problem is not touched, and vice versa.
 * The source defines, for the compile-time constants RAT_N = n, RAT_M = m, RAT_PETS_NORMALS = normals_per_step and
 * RAT_PETS_UNIFORMS = uniforms_per_step, and the user's parameters p (kept on the device):
 *
 *   __device__ void rat_user_f_stochastic(const double *x, const double *u, rat_rng &rng, int use_true_model, double *xn, const double *p);
 *   template <class T> __device__ T rat_user_c(int k, const T *x, const T *u, const double *p);   c(k, x, u), k = 0 .. N-1 (T = double)
 *   template <class T> __device__ T rat_user_h(const T *x, const double *p);                      h(x_N)
 *
 * rat_rng provides double normal() (N(0,1)) and double uniform() (U[0,1)).  rat_user_f is not needed; a source that defines all four
 * functions works with rat_problem_set_source and rat_pets_problem_set_source alike.  Each step's draws are counted, i = 0, 1, ...:
 *   injected (zn or zu non-NULL; every stream whose count is nonzero must be given, else RAT_ERR_ARG): the i-th normal() of trajectory
 *     j = ii*K + kk at step t reads zn[(j*N + t)*normals_per_step + i], the i-th uniform() zu[(j*N + t)*uniforms_per_step + i]; slots are
 *     fixed per (j, t, i) -- a draw the model skips leaves its slot unread.  normals_per_step = n is the family's zn layout.
 *   generator (zn and zu NULL): Philox4x32-10 with key (seed lo, seed hi) and g = the global trajectory index (rat_pets_enqueue's
 *     sample0 * K + j): normal pair q = i / 2 from counter (g lo, g hi, t, q) -- two 53-bit uniforms (r0:r1, r2:r3) >> 11 * 2^-53, the
 *     Box-Muller transform of csrc/rat_normal.h, normal 2q its cosine output, 2q + 1 its sine output; uniform pair q from counter
 *     (g lo, g hi, t, 0x80000000 | q), uniform 2q = (r0:r1), 2q + 1 = (r2:r3).  Results do not depend on how a batch is split.
 *   overdraw: a draw beyond the declared count is NaN and the call returns RAT_ERR_ARG naming the limits (rat_pets_solve checks once,
 *     after its single wait).  NaN costs otherwise propagate as in the reference (PETS has no DomainError).
 * Limits as rat_problem_set_source: n <= 12, m <= 4 (else RAT_ERR_UNSUPPORTED); negative counts RAT_ERR_ARG; a compile error RAT_ERR_ARG
 * with the compiler's log (model.hip:LINE) and the handle's previous generative problem in place; hiprtc missing RAT_ERR_UNSUPPORTED.
 * Code objects are cached per process by (source, kind, n, m, the two counts, device architecture).  rat_multi_pets_* take the family only. */
rat_rc rat_pets_problem_set_source(rat_handle h, const char *source, int32_t n, int32_t m, int32_t N,
                                   int32_t normals_per_step, int32_t uniforms_per_step,
                                   const double *params, int64_t n_params);
/* New values of the generative source problem's parameters (the same count; no recompilation). */
rat_rc rat_pets_set_params(rat_handle h, const double *params, int64_t n_params);
/* Compile only, for gfx950 (no device needed): RAT_OK, RAT_ERR_ARG with the log in rat_last_error(), or RAT_ERR_UNSUPPORTED. */
rat_rc rat_pets_source_check(const char *source, int32_t n, int32_t m,
                             int32_t normals_per_step, int32_t uniforms_per_step);

/* ---- several devices behind one object -----------------------------------------------------------------
 * Replaces the process fan-out of compute_cost (cross_entropy_bilevel_optimization.jl:180-192: `@sync ... @async remotecall_fetch(
 * compute_value_worker, 2 + mod(i, nprocs - 1), ...)` over `addprocs` workers) and of the PETS cost (pets.jl:108-124): ONE host
 * thread drives n_devices GPUs.  theta-samples are split in contiguous blocks (rat_shard_bounds), every device solves its block in
 * one launch on its own HIP stream, and ONE ncclAllGather (RCCL over xGMI) of the per-sample costs, ordered on those streams, leaves
 * cost[B] on every device; device 0's copy returns to the host.  Elite selection stays host arithmetic (rat_ce_update), the final
 * solve at theta_opt runs on device 0.  Results do not depend on n_devices. */
typedef struct rat_multi_s *rat_multi;
/* contiguous block [lo, hi) of `rank` among `world` (blocks differ by at most one sample; device-free) */
rat_rc  rat_shard_bounds(int64_t B, int32_t world, int32_t rank, int64_t *lo, int64_t *hi);
/* devices: n_devices distinct HIP device indices, or NULL for 0 .. n_devices-1.  max_batch is the whole CE batch. */
rat_rc  rat_create_multi(const rat_ileqg_opts *opts, int32_t max_batch, int32_t spec_eps, int32_t n_devices,
                         const int32_t *devices, rat_multi *out);
void    rat_multi_destroy(rat_multi m);
int32_t rat_multi_n_devices(rat_multi m);
rat_handle rat_multi_handle(rat_multi m, int32_t i);        /* the single-device handle of device i (e.g. rat_ce_set_stream on i = 0) */
int32_t rat_multi_uses_rccl(rat_multi m);                   /* 1 when the costs travel through ncclAllGather */
int64_t rat_multi_allgathers(rat_multi m);                  /* collectives issued so far (one per compute_cost batch) */
rat_rc  rat_multi_problem_set(rat_multi m, const rat_problem_desc *desc);
rat_rc  rat_multi_set_initial(rat_multi m, const double *x0, const double *u0);
/* compute_cost (:173-195) on all devices; x0/u0 may be NULL (keep the last rat_multi_set_initial) */
rat_rc  rat_multi_ce_compute_cost(rat_multi m, const double *x0, const double *u0, const double *theta, int64_t B,
                                  double kl_bound, double *cost);
/* the same with the gathered per-sample status (RAT_ST_*), iLEQG iteration count and line-search evaluation count of every shard
 * (the all-gather carries cost + status); any of the three may be NULL */
rat_rc  rat_multi_ce_compute_cost_ex(rat_multi m, const double *x0, const double *u0, const double *theta, int64_t B,
                                     double kl_bound, double *cost, int32_t *status, int32_t *iters, int32_t *ls_evals);
/* rat_ileqg_solve_batch (compute_value_worker over a batch, :144-167) on all devices: value (+Inf for failures) and the per-sample counters */
rat_rc  rat_multi_ileqg_solve_batch(rat_multi m, const double *x0, const double *u0, const double *theta, int64_t B,
                                    double *value, int32_t *status, int32_t *iters, int32_t *ls_evals);
/* 1 when the devices are logical (test hook RATILQR_MULTI_LOGICAL=1: device index d runs on physical device d mod the visible count
 * and the all-gather is carried out by stream-ordered device copies: the G > 1 code on a one-GPU box) */
int32_t rat_multi_is_logical(rat_multi m);
/* step! (:252-335) / solve! (:364-415) with the cost evaluation on all devices; draws come from rat_multi_handle(m, 0) */
rat_rc  rat_multi_ce_step(rat_multi m, rat_ce_solver *c, const double *x0, const double *u0, double kl_bound,
                          double *theta_out, double *cost_out);
rat_rc  rat_multi_ce_solve(rat_multi m, rat_ce_solver *c, const double *x0, const double *u0, double kl_bound,
                           double *theta_opt, double *x, double *l, double *L, double *value,
                           double *theta_min, double *theta_max);
/* PETS on all devices (pets.jl:100-126, the `remotecall_fetch(compute_cost_worker, ...)` fan-out :108-124): the S control samples in
 * contiguous blocks, all K stochastic rollouts of a sample on one device, costs straight to the host; arguments as rat_pets_compute_cost.
 * Costs do not depend on n_devices (injected noise is addressed by global sample index, the device generator by global trajectory). */
rat_rc  rat_multi_pets_problem_set(rat_multi m, const rat_gen_problem_desc *desc);
rat_rc  rat_multi_pets_compute_cost(rat_multi m, const double *x0, const double *controls, int64_t S, int64_t K,
                                    int32_t use_true_model, const double *zn, const double *zu, uint64_t seed, double *cost);

/* ---- execution path of the batched solves of a handle ------------------------------------------
 * Results are identical on every path (tested bit for bit); AUTO picks by batch size, speculation width E and the device's CU count:
 *   E = 1: BLOCK up to 2 n_cu samples (a sample's evaluation and gain recursions side by side on two SIMDs), FUSED beyond (in-wave
 *          pairing; batches beyond one sample per SIMD run that kernel in generations of workgroups);
 *   E = 2 / 4 / 8: BLOCK while the batch fits one generation of workgroups (n_cu * floor(8 / (E + 1)) samples; E = 8: n_cu), ROUNDS beyond;
 *   any other E, and the operator entry points: ROUNDS.
 * rat_set_path fixes the path of the handle (RAT_ERR_UNSUPPORTED when the handle's E has no such kernel) and overrides the `block` /
 * `fused` switches below; RAT_PATH_AUTO returns to what those switches say (a handle created on the round-based path stays there). */
#define RAT_PATH_AUTO   0
#define RAT_PATH_ROUNDS 1   /* one launch per phase, rounds polled by the host */
#define RAT_PATH_FUSED  2   /* one persistent wavefront per sample: whole solve! in one launch (E = 1) */
#define RAT_PATH_BLOCK  3   /* one workgroup per sample: whole solve! in one launch (E = 1, 2, 4, 8) */
rat_rc  rat_set_path(rat_handle h, int32_t path);
/* the path (RAT_PATH_ROUNDS / _FUSED / _BLOCK; 4 = general-size kernel) a batch of B samples takes on this handle, or -1 */
int32_t rat_get_path(rat_handle h, int64_t B);

/* ---- execution switches: ONE entry point for tests, A/B tools and bench.py's contract leg ------------------------------------------
 * Results never depend on a switch, except `wdiag` and `block_acl` (another rounding order: ~1e-13 relative).  At rat_create every switch also takes
 * the value of the environment variable RATILQR_<KEY IN CAPITALS> when that is set (the library reads no other environment variable
 * besides RATILQR_MULTI_LOGICAL / RATILQR_MULTI_FORCE_RCCL of rat_create_multi).  A switch that changes the HBM layout of the handle's
 * state (`fused`, `dual`, `speculate` on an E = 1 handle) re-lays it: give rat_set_initial again, as after rat_set_path.
 *   key             values   meaning (default)
 *   fused           0 / 1    E = 1: single-launch solves (1) or one launch per phase, "round-based path" (0)            (1)
 *   block           -1/0/1   workgroup-per-sample kernel: by batch size (-1), never (0), whenever it exists (1)          (-1)
 *   block_max_b     B        E = 1: largest batch the workgroup-per-sample kernel takes under block = -1                 (2 n_cu)
 *   block_shape     0 / 1    two-wave workgroups padded to one wave per SIMD with ticketed SIMD pairs                   (1)
 *   block_helpers   0 / 1    spare waves of a padded workgroup linearise (one workgroup per CU)                          (1)
 *   block_acl       0 / 1    E = 1 workgroup-per-sample kernel: closed-loop rollouts in deviation form (3 MFMAs on the recursion's
 *                            chain; values agree with the other paths to rounding, ~1e-15, not bit for bit; opt-in)      (0)
 *   fused_dual      (read)   policy evaluation + following gain sweep as two recursions of one wavefront: always on (the separate-sweep
 *                            instantiations of rounds 1-5 were retired in round 6; writes are ignored)                    (1)
 *   fused_occ2      B0       batches of >= B0 samples: the 256-register one-recursion kernel, two samples per SIMD       (0 = never;
 *                            -1, the default: LQ-family batches of more samples than the device has SIMDs)
 *   spec_force      0 / 1    run the speculation width rat_create was given (kernels for E = 2, 4, 8 in one launch, any E on the
 *                            round-based path) instead of the sequential rule; re-lays the handle's state like `fused`         (0)
 *   spec_width      (read)   the width the handle runs: 1, or rat_create's spec_eps under spec_force
 *   prune           0 / 1    round-based path, E > 1, tile-free candidates: the evaluations of candidates 1 .. E-1 of a sample stop once
 *                            candidate 0 is known to be the line search's choice (identical outputs)                      (1)
 *   wide16          0 / 1    general sizes with 12 <= n <= 16, m <= 4 (beyond the 12 + 4 tile): sweeps and rollouts of the solve kernel in
 *                            registers on the matrix pipe (wide16.h); 0 = the general LDS sweep.  rat_debug_get: 1 only where the
 *                            problem set on the handle really runs that form                                              (1)
 *   wide32          0 / 1    every other general size (n <= 32, m <= 32): the same in block form on 16 x 16 tiles, tables as register images
 *                            (wide32.h: one wavefront per SIMD instead of one per compute unit); 0 = the general LDS sweep      (1)
 *   init_share      0 / 1    initialize!'s rollout (independent of theta) rolled out once per (x_0, u_array) and copied   (1)
 *   init_lazy       0 / 1    ... except for the FIRST batch on a new (x_0, u_array) while a sample has a compute unit to itself (<= n_cu samples):
 *                            the samples roll it out inside the solve kernel and the shared rollout's launch (19 us) stays off the
 *                            critical path of one-shot callers -- receding-horizon solves, a single rat_ileqg_solve               (1)
 *   materialize     0 / 1    one-wavefront-per-sample kernel, LQ family, time-invariant cost: tile records written by the
 *                            rollouts and loaded by the sweeps (SURVEY 8d's wording) instead of formed in registers      (0)
 *   lq_replay       0 / 1    one-wavefront-per-sample kernel, LQ family with kappa = 0, diagonal time-invariant W and cost: every full paired
 *                            gain sweep records its Riccati matrices (-M^-1, [G | H + mu I]: 2 KB per step and sample) and a later pair
 *                            that would recompute them -- the evaluation of the gains it solved beside the next gain sweep, both at
 *                            mu = 0 -- runs only the vector half of both recursions over the record (csrc/sweep_dual.h:
 *                            replay_dual_body); identical outputs                                                        (1)
 *   lq_replay_count (read)   sweeps of this handle replayed so far, two per replayed pair (rat_debug_set clears it)
 *   lq_replay_last  0 / 1    ... and the evaluation that ends a solve (d < d_tol or iter_max), whose gains came from the record, runs only
 *                            its vector half over it as well (replay_eval_body); 0 = that evaluation runs in full; identical outputs  (1)
 *   lq_replay_last_count (read)  evaluations of this handle replayed that way so far, one each; not part of lq_replay_count
 *                            (rat_debug_set clears it)
 *   lq_replay_stack 0 / 1    the replayed pair forms row 12 of T for both recursions in one stacked chain of three MFMAs (column 12 of the gain
 *                            recursion's V in column 4 of the evaluation's operand); 0 = one chain each; identical outputs   (1)
 *   lq_replay_factor 0 / 1   the replayed pair takes the LDL' factor of H from the record (the recording pass stores it in lanes of the
 *                            -M^-1 words that hold no matrix data); 0 = every step factors the recorded H again; identical outputs  (1)
 *   fly             0 / 1    round-based path, E > 1: line-search candidates without tile records                         (1)
 *   fly_multi       0 / 1    ... and all candidates of a sample rolled out by one wavefront                               (1)
 *   dual            0 / 1    round-based path: candidate 0 paired with the next gain sweep in one wavefront              (E > 1)
 *   speculate       0 / 1    round-based path: speculative gain sweeps on a second stream                                (0)
 *   nm_depth        0 .. 3   Nelder-Mead speculation: 0 the six vertices of the iteration per device call; 1 also the two current vertices (the
 *                            final solve is read out of the last batch) and both initial vertices with the first iteration in one call; 2 also
 *                            the vertices of the iteration after (two iterations per device call); 3 also a third iteration in the first call
 *                            of rat_nm_solve (handles of >= 1022 samples).  Results do not depend on it  (3)
 *   pets_wave16     0 .. 3   PETS rollouts: 0 four per wavefront; 1 sixteen per wavefront as MFMA columns, the noise drawn by three generator
 *                            wavefronts per workgroup while the launch is small (<= 1536 wavefronts), by the recursion's own beyond; 2 never
 *                            split; 3 always split.  1-3 are bit-identical, 0 agrees to rounding  (1)
 *   ce_device       0 / 1    rat_ce_solve keeps the CE loop on the device: draw / update kernels, one host wait per solve!        (1)
 *   pets_device     0 / 1    rat_pets_solve keeps the CE loop over control sequences on the device (one host wait per solve!)      (1)
 *   block_psw       0 / 1    E = 1 batches of at most one sample per compute unit (LQ family): the workgroup-per-sample solve with every Riccati
 *                            sweep TIME-PARALLEL over the sample's four SIMDs (solve_block_psw_kernel, csrc/psweep.h); status / iteration /
 *                            line-search counts as on every other path, values equal to rounding (~1e-15), not bit for bit          (1)
 *   psw_acl         0 / 1    ... its closed-loop rollouts in deviation form (3 MFMAs on the recursion's chain)                      (1)
 *   psw_duo         0 / 1    ... with TWO workgroups (compute units) per sample while the batch leaves half the device dark (<= n_cu / 2
 *                            samples): the policy evaluations as four-wave teams on one, every gain sweep as a four-wave team on the
 *                            other, hand-overs through the XCD's L2 (counts identical, values to rounding: other segment cuts)         (1)
 *   psw_duo_count   (read)   samples of this handle that have run that way so far (rat_debug_set clears it)
 *   psw_prl         0 / 1    ... and the candidate's closed-loop rollout (simulate_dynamics, ileqg.jl:62-87) TIME-PARALLEL over the four
 *                            wavefronts where the deviation from the nominal trajectory is affine (kappa == 0, time-invariant cost,
 *                            N >= 16): four segments, the deviation at each cut from the composed maps of the segments before it
 *                            (rollprl_body; counts identical, values to ~1e-15 against the one-wave recursion)                         (1)
 *   prl_elem, prl_hop, prl_epi   its cost model in hundredths of an ordinary rollout step -- one step of a segment map, one hop, the
 *                            terminal tile: where the three cuts go (any model gives the same results)                      (45, 90, 100)
 *   prl_cuts        (read)   the cuts of the last launch that ran it: cut_1 | cut_2 << 16 | cut_3 << 32 (0: it did not apply)
 *   psweep          0, 2..4  the batched sweep operators (rat_dp_gain_sweep_batch / rat_dp_policy_eval_batch) run the TIME-PARALLEL sweep:
 *                            that many wavefronts per trajectory over that many + 1 horizon segments (csrc/psweep.h); results agree with the
 *                            sequential sweep to rounding (not bit for bit); values above 4 mean 4 (one wave per SIMD)             (0)
 *   psw_hop, psw_hop_e, psw_comp   its cost model in hundredths of an ordinary step -- one hop of a gain sweep, one hop of an evaluation, one
 *                            element step: where the segment cuts go                                                      (120, 140, 125)
 *   src_tpw         16 / 32 / 64   source models: trajectories per wavefront of the rollout kernel (16: measured faster at 1024
 *                            trajectories, profiles/source_model.md)                                                        (16)
 *   src_pets_tpw    16 / 32 / 64   generative source models: trajectories per wavefront of the PETS rollout kernel (64: 3.7x 16's
 *                            rollouts/s at 10^6 trajectories, equal at 10 k; profiles/source_pets.md)                     (64)
 *   mc_cost_K       read-only      costs the last rat_policy_evaluate / _noise (or rat_policy_worst_case / rat_policy_tail_risk with host costs) left on the device (0: none)
 *   src_mc_tpw      16 / 32 / 64   source models: rollouts per wavefront of rat_policy_evaluate's rollout kernel (profiles/policy_mc.md) (64)
 *   tail_dense      0 / 1    rat_policy_tail_trajectory / _disturbance / _params run the worst-case calls' dense moment kernels on the tail
 *                            weights instead of the liveness schedule: what that schedule is measured against (profiles/policy_tail_scenarios.md) (0);
 *                            rat_policy_tail_events / _user likewise run rat_policy_events' dense sums (profiles/policy_tail_events.md)
 *   wdiag           0 / 1    diagonal time-invariant W: inv(W) folded into M^-1's operand (takes effect at the next rat_problem_set) (1) */
rat_rc  rat_debug_set(rat_handle h, const char *key, int64_t value);
rat_rc  rat_debug_get(rat_handle h, const char *key, int64_t *value);      /* the EFFECTIVE value on this handle */

/* ---- measurement hooks (bench.py) -------------------------------------------------------------- */
#define RAT_K_ROLLOUT   0
#define RAT_K_LINEARIZE 1
#define RAT_K_SWEEP_EVAL 2
#define RAT_K_SWEEP_GAIN 3
#define RAT_K_SELECT    4
#define RAT_K_SWEEP_INIT 5   /* open-loop policy evaluation of initialize! (no gains read) */
#define RAT_K_SWEEP_DUAL 6   /* fused wavefront: policy evaluation + the next step!'s gain sweep over one pass of the tiles */
#define RAT_K_SOLVE_FUSED 7  /* one persistent wavefront per sample runs the whole solve! (E = 1): every phase above in one launch */
#define RAT_K_SOLVE_BLOCK 8  /* one workgroup per sample runs the whole solve!: a wavefront per line-search candidate + a gain-sweep wavefront */
#define RAT_K_SOLVE_WIDE  9  /* general-size solve kernel (n <= 32, m <= 32 beyond the 12 + 4 tile): a workgroup per sample, whole solve! */
#define RAT_K_PETS       10  /* PETS stochastic rollouts (pets_rollout_kernel + the per-sample mean) */
#define RAT_K_CE         11  /* draw + update kernels of the device-resident Cross-Entropy loops: rat_ce_solve (one workgroup each), rat_pets_solve (one per time step) */
#define RAT_K_COUNT     12
/* When enabled, kernel launches are bracketed by HIP events on the handle's stream.
 * on = 0: off; on = 1: every kernel kind; otherwise on = (mask << 1) | 1 with bit k of mask selecting kind RAT_K_k.
 * Launches of a surplus round (no live sample left) are not counted. */
rat_rc rat_profile_enable(rat_handle h, int32_t on);
rat_rc rat_profile_reset(rat_handle h);
/* launches[k], trajectories[k] (units processed), total_ms[k] for k < RAT_K_COUNT */
rat_rc rat_profile_get(rat_handle h, int64_t *launches, int64_t *trajectories, double *total_ms);
/* the handle's HIP stream as an opaque pointer (hipStream_t), and its device index */
void  *rat_stream(rat_handle h);
/* bytes of one trajectory's tile bundle as laid out in HBM, and of the per-trajectory L/x/u arrays */
rat_rc rat_layout_info(rat_handle h, int64_t *tile_bytes, int64_t *L_bytes, int64_t *x_bytes, int64_t *u_bytes);

#ifdef __cplusplus
}
#endif
#endif
