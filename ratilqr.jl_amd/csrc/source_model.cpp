// source_model.cpp -- hiprtc (through dlopen: the library loads, and every other path works, where hiprtc is missing) and the process-wide
// code-object cache of the runtime-compiled model family.
#include "source_model.h"

#include <dlfcn.h>

#include <chrono>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>

#include <hip/hiprtc.h>

namespace {

// the embedded headers (Makefile: source_embed.inc, raw string literals of the files)
#include "source_embed.inc"

struct Rtc {
    bool tried = false, ok = false;
    std::string why;
    hiprtcResult (*create)(hiprtcProgram *, const char *, const char *, int, const char *const *, const char *const *) = nullptr;
    hiprtcResult (*compile)(hiprtcProgram, int, const char *const *) = nullptr;
    hiprtcResult (*destroy)(hiprtcProgram *) = nullptr;
    hiprtcResult (*log_size)(hiprtcProgram, size_t *) = nullptr;
    hiprtcResult (*log)(hiprtcProgram, char *) = nullptr;
    hiprtcResult (*code_size)(hiprtcProgram, size_t *) = nullptr;
    hiprtcResult (*code)(hiprtcProgram, char *) = nullptr;
};

std::mutex g_mu;
Rtc g_rtc;
// key: (source, n, m, kind (0 risk-sensitive, 1 generative, 2 the risk-sensitive model's Monte-Carlo rollout, 3 that rollout under the
// user's noise sampler, 4 that rollout under a shifted proposal with an event's margin: source_rare.h, 5 the user's events on replayed
// trajectories: source_events.h, 6 kind 4 with the user's event for the margin: source_rare.h under RAT_RARE_USER_EVENT), normals per step,
// uniforms per step, events of rat_user_event (0 where the kind has none), architecture)
std::map<std::tuple<std::string, int, int, int, int, int, int, std::string>, std::shared_ptr<const std::vector<char>>> g_cache;

bool rtc_load(std::string *why) {           // (g_mu held)
    if (!g_rtc.tried) {
        g_rtc.tried = true;
        void *so = dlopen("libhiprtc.so", RTLD_NOW | RTLD_LOCAL);
        if (!so) so = dlopen("libhiprtc.so.7", RTLD_NOW | RTLD_LOCAL);
        if (!so) g_rtc.why = std::string("hiprtc is not available: ") + dlerror();
        else {
#define SYM(field, name) g_rtc.field = reinterpret_cast<decltype(g_rtc.field)>(dlsym(so, name))
            SYM(create, "hiprtcCreateProgram"); SYM(compile, "hiprtcCompileProgram"); SYM(destroy, "hiprtcDestroyProgram");
            SYM(log_size, "hiprtcGetProgramLogSize"); SYM(log, "hiprtcGetProgramLog");
            SYM(code_size, "hiprtcGetCodeSize"); SYM(code, "hiprtcGetCode");
#undef SYM
            g_rtc.ok = g_rtc.create && g_rtc.compile && g_rtc.destroy && g_rtc.log_size && g_rtc.log && g_rtc.code_size && g_rtc.code;
            if (!g_rtc.ok) g_rtc.why = "hiprtc is not available: a symbol is missing from libhiprtc.so";
        }
    }
    if (!g_rtc.ok) *why = g_rtc.why;
    return g_rtc.ok;
}

}  // namespace

std::string src_arch(const char *gcn_arch_name) {
    std::string in = gcn_arch_name ? gcn_arch_name : "", out;
    size_t pos = 0;
    while (pos <= in.size()) {
        size_t e = in.find(':', pos);
        if (e == std::string::npos) e = in.size();
        const std::string tok = in.substr(pos, e - pos);
        if (!tok.empty() && tok != "xnack+") out += (out.empty() ? "" : ":") + tok;
        pos = e + 1;
    }
    return out.empty() ? std::string("gfx950") : out;
}

static rat_rc compile_impl(const char *source, int n, int m, int kind, int npn, int npu, int nev, const std::string &arch,
                          std::shared_ptr<const std::vector<char>> *code, std::string *log, double *ms, bool *cached) {
    const auto t0 = std::chrono::steady_clock::now();
    auto done = [&](rat_rc rc) {
        if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return rc;
    };
    std::lock_guard<std::mutex> lk(g_mu);
    if (cached) *cached = false;
    const auto key = std::make_tuple(std::string(source), n, m, kind, npn, npu, nev, arch);
    auto it = g_cache.find(key);
    if (it != g_cache.end()) {
        if (code) *code = it->second;
        if (cached) *cached = true;
        return done(RAT_OK);
    }
    std::string why;
    if (!rtc_load(&why)) { if (log) *log = why; return done(RAT_ERR_UNSUPPORTED); }
    // the user's source between the AD and rat_rng headers and the kernels (a source that defines all four functions compiles as either
    // kind); #line makes the compiler's messages name lines of the user's text.  A generative source does not define rat_user_f:
    // source_kernels.h is not part of its text
    const std::string text = std::string(kind == 4 || kind == 6 ? "#define RAT_RNG_SHIFT 1\n" : "") + "#include \"source_args.h\"\n#include \"rat_ad.h\"\n#include \"rat_rng.h\"\n#line 1 \"model.hip\"\n" +
                             source + (kind == 0 ? "\n#line 1 \"source_kernels.h\"\n#include \"source_kernels.h\"\n"
                                      : kind == 2 ? "\n#line 1 \"source_noisy.h\"\n#include \"source_noisy.h\"\n"
                                      : kind == 3 ? "\n#line 1 \"source_user_noise.h\"\n#include \"source_user_noise.h\"\n"
                                      : kind == 4 || kind == 6 ? "\n#line 1 \"source_rare.h\"\n#include \"source_rare.h\"\n"
                                      : kind == 5 ? "\n#line 1 \"source_events.h\"\n#include \"source_events.h\"\n"
                                                  : "\n#line 1 \"source_pets.h\"\n#include \"source_pets.h\"\n");
    const char *hdr[] = {k_embed_layout_h, k_embed_source_args_h, k_embed_rat_ad_h, k_embed_source_kernels_h, k_embed_rat_normal_h,
                         k_embed_rat_philox_h, k_embed_rat_rng_h, k_embed_source_pets_h, k_embed_source_noisy_h, k_embed_source_user_noise_h,
                         k_embed_source_rare_h, k_embed_source_events_h};
    const char *hdr_names[] = {"layout.h", "source_args.h", "rat_ad.h", "source_kernels.h", "rat_normal.h", "rat_philox.h", "rat_rng.h",
                               "source_pets.h", "source_noisy.h", "source_user_noise.h", "source_rare.h", "source_events.h"};
    hiprtcProgram prog = nullptr;
    if (g_rtc.create(&prog, text.c_str(), "model.hip", 12, hdr, hdr_names) != HIPRTC_SUCCESS) {
        if (log) *log = "hiprtcCreateProgram failed";
        return done(RAT_ERR_ARG);
    }
    const std::string dn = "-DRAT_N=" + std::to_string(n), dm = "-DRAT_M=" + std::to_string(m), oa = "--offload-arch=" + arch;
    const std::string dpn = "-DRAT_PETS_NORMALS=" + std::to_string(npn), dpu = "-DRAT_PETS_UNIFORMS=" + std::to_string(npu);
    const std::string dne = "-DRAT_N_EVENT=" + std::to_string(nev);
    const char *opts[] = {"-O3", "-std=c++17", dn.c_str(), dm.c_str(), oa.c_str(), dpn.c_str(), dpu.c_str(), dne.c_str(), "-DRAT_RARE_USER_EVENT=1"};
    const hiprtcResult rc = g_rtc.compile(prog, kind == 6 ? 9 : kind == 5 ? 8 : 7, opts);   // (the kinds from before see the options from before)
    size_t ls = 0;
    std::string lg;
    if (g_rtc.log_size(prog, &ls) == HIPRTC_SUCCESS && ls > 1) {
        lg.resize(ls);
        g_rtc.log(prog, &lg[0]);
        lg.resize(strnlen(lg.c_str(), ls));
    }
    if (rc != HIPRTC_SUCCESS) {
        g_rtc.destroy(&prog);
        if (log) *log = "source model does not compile:\n" + lg;
        return done(RAT_ERR_ARG);
    }
    size_t cs = 0;
    auto obj = std::make_shared<std::vector<char>>();
    if (g_rtc.code_size(prog, &cs) != HIPRTC_SUCCESS || cs == 0) {
        g_rtc.destroy(&prog);
        if (log) *log = "hiprtc produced no code object";
        return done(RAT_ERR_ARG);
    }
    obj->resize(cs);
    g_rtc.code(prog, obj->data());
    g_rtc.destroy(&prog);
    g_cache[key] = obj;
    if (code) *code = obj;
    if (log) *log = lg;
    return done(RAT_OK);
}

rat_rc src_compile(const char *source, int n, int m, const std::string &arch, std::shared_ptr<const std::vector<char>> *code,
                   std::string *log, double *ms, bool *cached) {
    return compile_impl(source, n, m, 0, 0, 0, 0, arch, code, log, ms, cached);
}

rat_rc src_compile_gen(const char *source, int n, int m, int npn, int npu, const std::string &arch,
                       std::shared_ptr<const std::vector<char>> *code, std::string *log, double *ms, bool *cached) {
    return compile_impl(source, n, m, 1, npn, npu, 0, arch, code, log, ms, cached);
}

rat_rc src_compile_noisy(const char *source, int n, int m, const std::string &arch, std::shared_ptr<const std::vector<char>> *code,
                         std::string *log, double *ms, bool *cached) {
    return compile_impl(source, n, m, 2, 0, 0, 0, arch, code, log, ms, cached);
}

rat_rc src_compile_user_noise(const char *source, int n, int m, int npn, int npu, const std::string &arch,
                              std::shared_ptr<const std::vector<char>> *code, std::string *log, double *ms, bool *cached) {
    return compile_impl(source, n, m, 3, npn, npu, 0, arch, code, log, ms, cached);
}

rat_rc src_compile_rare(const char *source, int n, int m, int npn, int npu, const std::string &arch,
                        std::shared_ptr<const std::vector<char>> *code, std::string *log, double *ms, bool *cached) {
    return compile_impl(source, n, m, 4, npn, npu, 0, arch, code, log, ms, cached);
}

rat_rc src_compile_events(const char *source, int n, int m, int n_event, const std::string &arch,
                          std::shared_ptr<const std::vector<char>> *code, std::string *log, double *ms, bool *cached) {
    return compile_impl(source, n, m, 5, 0, 0, n_event, arch, code, log, ms, cached);
}

rat_rc src_compile_rare_user(const char *source, int n, int m, int npn, int npu, int n_event, const std::string &arch,
                             std::shared_ptr<const std::vector<char>> *code, std::string *log, double *ms, bool *cached) {
    return compile_impl(source, n, m, 6, npn, npu, n_event, arch, code, log, ms, cached);
}
