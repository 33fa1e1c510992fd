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

// the embedded headers (Makefile: source_embed.inc, raw string literals of the files of EMBED_H, then k_embed_texts and k_embed_names)
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
// key: (source, n, m, SrcKind, normals per step, uniforms per step, events of rat_user_event (0 where the kind takes none), parameters
// drawn per rollout (0: sampling off) with their normals and uniforms, whether the parameter normals are shifted (0 where the kind has
// no shifted proposal), the parameter count of a params_ad kind (0 elsewhere), architecture)
std::map<std::tuple<std::string, int, int, int, int, int, int, int, int, int, int, int, std::string>, std::shared_ptr<const std::vector<char>>> g_cache;

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

// indexed by SrcKind:  header                 entry                         entry2               rng_shift draws events rare_user_event param_draws params_ad margins
static const SrcKindRow k_kinds[SRC_NKIND] = {
    /* SRC_MODEL      */ {"source_kernels.h",    "rat_src_rollout",            "rat_src_linearize", false,    false, false, false, false, false, false},
    /* SRC_PETS       */ {"source_pets.h",       "rat_src_pets_rollout",       nullptr,             false,    true,  false, false, false, false, false},
    /* SRC_NOISY      */ {"source_noisy.h",      "rat_src_noisy_rollout",      nullptr,             false,    false, false, false, false, false, false},
    /* SRC_USER_NOISE */ {"source_user_noise.h", "rat_src_user_noisy_rollout", nullptr,             false,    true,  false, false, true,  false, false},
    /* SRC_RARE       */ {"source_rare.h",       "rat_src_rare_rollout",       nullptr,             true,     true,  false, false, true,  false, false},
    /* SRC_EVENTS     */ {"source_events.h",     "rat_src_user_events",        nullptr,             false,    false, true,  false, true,  false, false},
    /* SRC_RARE_USER  */ {"source_rare.h",       "rat_src_rare_rollout",       nullptr,             true,     true,  true,  true,  true,  false, false},
    /* SRC_PARAMS     */ {"source_params.h",     "rat_src_params_sample",      nullptr,             false,    false, false, false, true,  false, false},
    /* SRC_SOBOL      */ {"source_sobol.h",      "rat_src_sobol_rollout",      nullptr,             false,    true,  false, false, true,  false, false},
    /* SRC_ADJOINT    */ {"source_adjoint.h",    "rat_src_adjoint",            nullptr,             false,    true,  false, false, false, false, false},
    /* SRC_ADJOINT_P  */ {"source_adjoint_params.h", "rat_src_adjoint_p",   nullptr,             false,    true,  false, false, true,  true, false},
    /* SRC_MARGIN_ADJOINT */ {"source_margin_adjoint.h", "rat_src_margin_adjoint", nullptr,      false,    true,  false, false, false, false, true},
};

const SrcKindRow &src_kind(SrcKind kind) { return k_kinds[kind]; }

rat_rc src_compile(SrcKind kind, const char *source, int n, int m, const SrcShape &shape, const std::string &arch,
                   std::shared_ptr<const std::vector<char>> *code, std::string *log, double *ms, bool *cached) {
    const SrcKindRow &row = k_kinds[kind];
    const int npn = row.draws ? shape.npn : 0, npu = row.draws ? shape.npu : 0, nev = (row.events || row.margins) ? shape.nev : 0;
    const int npar = row.param_draws ? shape.npar : 0, ppn = npar > 0 ? shape.ppn : 0, ppu = npar > 0 ? shape.ppu : 0;
    const int pshift = row.rng_shift ? shape.pshift : 0, nap = row.params_ad ? shape.nap : 0;
    const auto t0 = std::chrono::steady_clock::now();
    auto done = [&](rat_rc rc) {
        if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return rc;
    };
    std::lock_guard<std::mutex> lk(g_mu);
    if (cached) *cached = false;
    const auto key = std::make_tuple(std::string(source), n, m, (int)kind, npn, npu, nev, npar, ppn, ppu, pshift, nap, arch);
    auto it = g_cache.find(key);
    if (it != g_cache.end()) {
        if (code) *code = it->second;
        if (cached) *cached = true;
        return done(RAT_OK);
    }
    std::string why;
    if (!rtc_load(&why)) { if (log) *log = why; return done(RAT_ERR_UNSUPPORTED); }
    // the user's source between the AD and rat_rng headers and the kind's kernels (a source that defines all four functions compiles as
    // either of the first two kinds); #line makes the compiler's messages name lines of the user's text
    const std::string text = std::string(row.rng_shift ? "#define RAT_RNG_SHIFT 1\n" : "") +
                             "#include \"source_args.h\"\n#include \"rat_ad.h\"\n#include \"rat_rng.h\"\n#line 1 \"model.hip\"\n" + source +
                             "\n#line 1 \"" + row.header + "\"\n#include \"" + row.header + "\"\n";
    hiprtcProgram prog = nullptr;
    if (g_rtc.create(&prog, text.c_str(), "model.hip", (int)(sizeof(k_embed_texts) / sizeof(k_embed_texts[0])), k_embed_texts,
                     k_embed_names) != HIPRTC_SUCCESS) {
        if (log) *log = "hiprtcCreateProgram failed";
        return done(RAT_ERR_ARG);
    }
    const std::string dn = "-DRAT_N=" + std::to_string(n), dm = "-DRAT_M=" + std::to_string(m), oa = "--offload-arch=" + arch;
    const std::string dpn = "-DRAT_PETS_NORMALS=" + std::to_string(npn), dpu = "-DRAT_PETS_UNIFORMS=" + std::to_string(npu);
    const std::string dne = "-DRAT_N_EVENT=" + std::to_string(nev);
    std::vector<const char *> opts = {"-O3", "-std=c++17", dn.c_str(), dm.c_str(), oa.c_str(), dpn.c_str(), dpu.c_str()};
    if (row.events) opts.push_back(dne.c_str());
    const std::string dnm = "-DRAT_N_MARGIN=" + std::to_string(nev);
    if (row.margins) opts.push_back(dnm.c_str());
    if (row.rare_user_event) opts.push_back("-DRAT_RARE_USER_EVENT=1");
    const std::string dnp = "-DRAT_N_PARAMS=" + std::to_string(npar), dppn = "-DRAT_PARAM_NORMALS=" + std::to_string(ppn),
                      dppu = "-DRAT_PARAM_UNIFORMS=" + std::to_string(ppu);
    if (npar > 0) {                                                   // parameter sampling is on
        opts.push_back("-DRAT_USER_PARAMS_ON=1");
        opts.push_back(dnp.c_str()); opts.push_back(dppn.c_str()); opts.push_back(dppu.c_str());
    }
    const std::string dnap = "-DRAT_N_PARAMS=" + std::to_string(nap);
    if (row.params_ad && npar == 0) opts.push_back(dnap.c_str());     // (with sampling on npar == nap is already there)
    if (pshift) opts.push_back("-DRAT_PARAM_SHIFT=1");
    if (kind == SRC_PARAMS) opts.push_back("-DRAT_PARAMS_SAMPLE_KERNEL=1");
    if (kind == SRC_SOBOL) opts.push_back("-DRAT_RNG_PICK=1");
    const hiprtcResult rc = g_rtc.compile(prog, (int)opts.size(), opts.data());
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
