// source_model.h -- host side of the runtime-compiled model family (RAT_MODEL_SOURCE): hiprtc, loaded with dlopen, and a process-wide
// cache of the code objects it produced.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ratilqr.h"

// Compiles the user's source behind the embedded headers (rat_ad.h, rat_rng.h, source_args.h, layout.h; source_kernels.h after it) for
// `arch` with -O3 -std=c++17 -DRAT_N=n -DRAT_M=m -DRAT_PETS_NORMALS=0 -DRAT_PETS_UNIFORMS=0.  RAT_OK: *code holds the code object (shared with the cache).  RAT_ERR_ARG: *log holds the
// compiler's log.  RAT_ERR_UNSUPPORTED: hiprtc is not available in this process.  *ms (if not null): wall time of the call; *cached:
// whether the code object came from the cache.
rat_rc src_compile(const char *source, int n, int m, const std::string &arch, std::shared_ptr<const std::vector<char>> *code,
                   std::string *log, double *ms = nullptr, bool *cached = nullptr);
// The same for a generative source (PETS): source_pets.h after it, -DRAT_PETS_NORMALS=npn -DRAT_PETS_UNIFORMS=npu.  Cached apart from
// risk-sensitive compiles of the same text.
rat_rc src_compile_gen(const char *source, int n, int m, int npn, int npu, const std::string &arch,
                       std::shared_ptr<const std::vector<char>> *code, std::string *log, double *ms = nullptr, bool *cached = nullptr);
// The Monte-Carlo rollout kernel of a risk-sensitive source (rat_policy_evaluate): source_noisy.h after it.  A third kind with a cache key
// of its own, compiled on the first evaluation of a source problem, not when the problem is set.
rat_rc src_compile_noisy(const char *source, int n, int m, const std::string &arch, std::shared_ptr<const std::vector<char>> *code,
                         std::string *log, double *ms = nullptr, bool *cached = nullptr);
// That rollout under the user's noise sampler (rat_policy_evaluate_noise): source_user_noise.h after the source, which must define
// RAT_USER_NOISE and rat_user_noise; -DRAT_PETS_NORMALS=npn -DRAT_PETS_UNIFORMS=npu.  A fourth kind, compiled on the first such evaluation.
rat_rc src_compile_user_noise(const char *source, int n, int m, int npn, int npu, const std::string &arch,
                              std::shared_ptr<const std::vector<char>> *code, std::string *log, double *ms = nullptr, bool *cached = nullptr);
// That rollout under a shifted proposal with the margin of one event (rat_policy_rare_event_noise): source_rare.h after the source, and
// "#define RAT_RNG_SHIFT 1" in front of rat_rng.h -- the only kind that defines it.  A fifth kind, compiled on the first such call.
rat_rc src_compile_rare(const char *source, int n, int m, int npn, int npu, const std::string &arch,
                        std::shared_ptr<const std::vector<char>> *code, std::string *log, double *ms = nullptr, bool *cached = nullptr);
// The user's events on replayed trajectories (rat_policy_events_user): source_events.h after the source, which must define RAT_USER_EVENT
// and rat_user_event; -DRAT_N_EVENT=n_event, no draws.  A sixth kind, compiled by the first call that names this n_event.
rat_rc src_compile_events(const char *source, int n, int m, int n_event, const std::string &arch,
                          std::shared_ptr<const std::vector<char>> *code, std::string *log, double *ms = nullptr, bool *cached = nullptr);
// src_compile_rare with the user's event for the margin (rat_policy_rare_event_user): the same text with -DRAT_RARE_USER_EVENT=1
// -DRAT_N_EVENT=n_event.  A seventh kind.
rat_rc src_compile_rare_user(const char *source, int n, int m, int npn, int npu, int n_event, const std::string &arch,
                             std::shared_ptr<const std::vector<char>> *code, std::string *log, double *ms = nullptr, bool *cached = nullptr);
// The offload-arch string for the device's reported gcnArchName (an xnack+ feature is never passed on).
std::string src_arch(const char *gcn_arch_name);
