// source_model.h -- host side of the runtime-compiled model family (RAT_MODEL_SOURCE): hiprtc, loaded with dlopen, and a process-wide
// cache of the code objects it produced.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ratilqr.h"

// Compiles the user's source behind the embedded headers (rat_ad.h, source_args.h, layout.h, source_kernels.h) for `arch` with
// -O3 -std=c++17 -DRAT_N=n -DRAT_M=m.  RAT_OK: *code holds the code object (shared with the cache).  RAT_ERR_ARG: *log holds the
// compiler's log.  RAT_ERR_UNSUPPORTED: hiprtc is not available in this process.  *ms (if not null): wall time of the call; *cached:
// whether the code object came from the cache.
rat_rc src_compile(const char *source, int n, int m, const std::string &arch, std::shared_ptr<const std::vector<char>> *code,
                   std::string *log, double *ms = nullptr, bool *cached = nullptr);
// The offload-arch string for the device's reported gcnArchName (an xnack+ feature is never passed on).
std::string src_arch(const char *gcn_arch_name);
