// source_model.h -- host side of the runtime-compiled model family (RAT_MODEL_SOURCE): hiprtc, loaded with dlopen, and a process-wide
// cache of the code objects it produced.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ratilqr.h"

// The modules a source can be compiled into.  (The numbers are part of the cache key.)
enum SrcKind {
    SRC_MODEL = 0,       // the risk-sensitive model's rollout and linearisation (rat_problem_set_source)
    SRC_PETS,            // a generative source's PETS rollout (rat_pets_problem_set_source)
    SRC_NOISY,           // the Monte-Carlo rollout under N(0, W) (rat_policy_evaluate)
    SRC_USER_NOISE,      // that rollout under the user's rat_user_noise (rat_policy_evaluate_noise)
    SRC_RARE,            // that under a shifted proposal, with a quadratic event's margin (rat_policy_rare_event_noise)
    SRC_EVENTS,          // the user's rat_user_event on replayed trajectories (rat_policy_events_user)
    SRC_RARE_USER,       // SRC_RARE with entry `event` of rat_user_event for the margin (rat_policy_rare_event_user)
    SRC_PARAMS,          // the user's rat_user_params alone (rat_policy_params_sample)
    SRC_SOBOL,           // SRC_USER_NOISE's rollout with every draw picked from one of two streams (rat_policy_sobol)
    SRC_ADJOINT,         // the adjoint sweep on replayed trajectories (rat_policy_gradient, rat_policy_tail_gradient)
    SRC_ADJOINT_P,       // that sweep with the parameter pass and lambda_0 (rat_policy_param_gradient, rat_policy_tail_param_gradient)
    SRC_MARGIN_ADJOINT,  // the adjoint sweep seeded by quadratic events' margins, the events of a call jointly (rat_policy_margin_gradient)
    SRC_NKIND
};
// One row per kind: what its translation unit is made of and what the module exports.  Every kind is the user's text behind
// source_args.h, rat_ad.h and rat_rng.h, then `header` (under a #line of its own), compiled for `arch` with -O3 -std=c++17 -DRAT_N=n
// -DRAT_M=m -DRAT_PETS_NORMALS=npn -DRAT_PETS_UNIFORMS=npu (0 where the kind takes no draws).  A kind that takes parameter draws gets
// -DRAT_USER_PARAMS_ON=1 -DRAT_N_PARAMS=npar -DRAT_PARAM_NORMALS=ppn -DRAT_PARAM_UNIFORMS=ppu as well when the shape has npar > 0
// (parameter sampling is on, rat_policy_params_sampling); with npar == 0 its command line is what it was without the feature.  The two
// rng_shift kinds get -DRAT_PARAM_SHIFT=1 besides when the shape has pshift (rat_policy_rare_event_params: source_params.h).  SRC_SOBOL
// alone gets -DRAT_RNG_PICK=1 (rat_rng.h, source_params.h: a second key and the masks that pick a draw's stream).  A params_ad kind gets
// -DRAT_N_PARAMS=nap, the problem's parameter count, whether or not sampling is on (with sampling on npar == nap).  A margins kind gets
// -DRAT_N_MARGIN=nev: the quadratic events its kernel sweeps jointly (they are data, not source: nothing is asked of the user's text).
struct SrcKindRow {
    const char *header;          // embedded header with the kind's kernels
    const char *entry, *entry2;  // kernels the module exports (entry2: NULL but for SRC_MODEL's linearisation)
    bool rng_shift;              // "#define RAT_RNG_SHIFT 1" in front of everything
    bool draws;                  // takes npn, npu (a sampler's source must define RAT_USER_NOISE: the header refuses it otherwise)
    bool events;                 // takes nev: -DRAT_N_EVENT=nev (the source must define RAT_USER_EVENT)
    bool rare_user_event;        // -DRAT_RARE_USER_EVENT=1
    bool param_draws;            // takes npar, ppn, ppu: the kernels that call rat_user_params once per rollout (source_params.h)
    bool params_ad;              // takes nap: the kernel seeds rat_dual[RAT_N_PARAMS] (the source must define RAT_USER_PARAMS_AD)
    bool margins;                // takes nev as -DRAT_N_MARGIN=nev
};
const SrcKindRow &src_kind(SrcKind kind);
struct SrcShape {                                        // (fields a kind does not take are read as 0)
    int npn = 0, npu = 0, nev = 0;
    int npar = 0, ppn = 0, ppu = 0;                      // parameter sampling: RAT_N_PARAMS (0: off), parameter normals / uniforms per rollout
    int pshift = 0;                                      // 1: -DRAT_PARAM_SHIFT=1, the parameter normals are shifted too (rat_policy_rare_event_params);
                                                         // read by the rng_shift kinds alone (SRC_RARE, SRC_RARE_USER), which need npar > 0 with it
    int nap = 0;                                         // the problem's parameter count, read by the params_ad kind alone (SRC_ADJOINT_P)
};

// Compiles `source` as `kind`.  RAT_OK: *code holds the code object (shared with the cache, which keys on source, n, m, kind, shape and
// arch).  RAT_ERR_ARG: *log holds the compiler's log.  RAT_ERR_UNSUPPORTED: hiprtc is not available in this process.  *ms (if not null):
// wall time of the call; *cached: whether the code object came from the cache.
rat_rc src_compile(SrcKind kind, const char *source, int n, int m, const SrcShape &shape, const std::string &arch,
                   std::shared_ptr<const std::vector<char>> *code, std::string *log, double *ms = nullptr, bool *cached = nullptr);
// The offload-arch string for the device's reported gcnArchName (an xnack+ feature is never passed on).
std::string src_arch(const char *gcn_arch_name);
