"""rat_policy_rare_event_params without a device: the NumPy model of the whole call (tests/rare_event_params_model.py) against two closed
forms and against a plain count, the compile-only check, the exported symbols and their prototypes, and the code-object cache
(csrc/source_model.cpp: pshift in the key of SRC_RARE and SRC_RARE_USER alone; with pshift = 0 every module is what it was).

Closed forms (n = m = 1, N = 1, x0 = 1, one parameter normal, one step normal), beta = 6, P = Phi(-6) = 9.87e-10:
  (a) user_params_model.SCALAR, x1 = (a0 + s z_p) x0, event x1 > c; adapt = "params"
  (b) the same with w = sigma z, x1 ~ N(a0 x0, s^2 x0^2 + sigma^2); adapt = "both"
asserted as |PROB - exact| <= 4 PROB_SE under the condition PROB_SE / PROB <= 0.10 at K = 2^14, n_iter = 8, rho = 0.1.  The condition is
no measurement: the mean shift by beta leaves a per-sample relative variance of e^(beta^2) Phi(-2 beta) / Phi(-beta)^2 - 1, about
sqrt(2 pi) beta / 2 - 1 = 6.5 at beta = 6, hence about 2 % at 2^14 (the shift the iterations stop at is a little short of beta: 3.3 %
here); the test confirms that the seeds the device tests use (rare_event_params_model.SEED_A, SEED_B) meet it."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import rare_event_model as rm
import rare_event_params_model as rp
import ratilqr.jl_amd as rat
import user_event_model as ue
import user_params_model as pm
from ratilqr.jl_amd import _native as nv
from source_pets_models import PENDULUM
from test_cpu_julia_shim import PROTOS
from test_cpu_source_kinds import CSRC, ROCM_INC, embed_inc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = 1, 2


# ---- 1. the model against the closed forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,adapt,seed", [("a", "params", rp.SEED_A), ("b", "both", rp.SEED_B)])
def test_the_model_meets_the_closed_form_at_beta_six(which, adapt, seed):
    _, _, mod, exact = rp.closed_case(which)
    x, l, L = rp.closed_policy()
    r = rp.rare_event_params(mod, x, l, L, None, rp.K_CLOSED, seed=seed, adapt_mode=adapt, n_iter=rp.N_ITER_CLOSED, rho=rp.RHO_CLOSED)
    print(f"({which}) exact {exact:.6e}: PROB {r['prob']:.6e} SE {r['prob_se']:.3e} ({abs(r['prob'] - exact) / r['prob_se']:.2f} sigma), "
          f"SE/PROB {r['prob_se'] / r['prob']:.3e}, {r['n_iter']} iterations, ps {r['param_shift']}, s {r['shift'].ravel()}")
    assert abs(exact - 9.8659e-10) < 1e-13
    assert r["flag"] == rm.OK
    assert r["prob_se"] / r["prob"] <= 0.10                           # the cap: a condition on the seed, confirmed here
    assert abs(r["prob"] - exact) <= 4.0 * r["prob_se"]
    if which == "a":
        # the level reaches 0 once a tenth of the rollouts pass beta: the shift is then within the upper decile's 1.28 (and noise) of it
        assert np.all(r["shift"] == 0.0) and rp.BETA - 2.0 < r["param_shift"][0] < rp.BETA + 1.0
        assert np.array_equal(np.isnan(r["param_trace"]), np.isnan(r["trace"][:, 3]))
    # what the existing calls can do: the same model with nothing shifted sees no violation at all
    plain = rp.rare_event_params(mod, x, l, L, None, rp.K_CLOSED, seed=seed, n_iter=0)
    assert plain["n_viol"] == 0 and plain["prob"] == 0.0 and plain["flag"] == rm.NOT_REACHED


# ---- 2. unbiased under an arbitrary fixed parameter shift ------------------------------------------------------------------------------------
def test_a_fixed_parameter_shift_leaves_the_estimate_unbiased():
    """the pendulum whose obstacle radius the hook draws, an event of probability about 1e-2, n_iter = 0: PROB under a random parameter
    shift (and a random step shift) against the plain count of another seed, within 4 combined standard errors"""
    c = rp.ParityCase("pend")
    K = 1 << 14
    mod = c.model(c.rarefied(K, 3, q=0.99))
    x, l, L = c.policy
    plain = rp.rare_event_params(mod, x, l, L, None, K, seed=5, n_iter=0)
    assert 3e-3 < plain["prob"] < 3e-2 and plain["prob"] == plain["n_viol"] / K and np.all(plain["logw"] == 0.0)
    r = np.random.default_rng(8)
    for ps, s in ((0.8 * r.standard_normal(2), None), (0.8 * r.standard_normal(2), 0.1 * r.standard_normal((c.N, c.npn)))):
        got = rp.rare_event_params(mod, x, l, L, None, K, seed=6, shift=s, param_shift=ps, n_iter=0)
        se = float(np.hypot(got["prob_se"], plain["prob_se"]))
        print(f"ps {ps}: PROB {got['prob']:.5e} SE {got['prob_se']:.2e}; plain {plain['prob']:.5e} SE {plain['prob_se']:.2e}: "
              f"{abs(got['prob'] - plain['prob']) / se:.2f} sigma")
        assert np.array_equal(got["param_shift"], ps) and np.any(got["logw"] != 0.0)
        assert abs(got["prob"] - plain["prob"]) <= 4.0 * se


def test_the_parameter_part_of_logw_follows_the_draws():
    """logw of a pass is the parameter terms in draw order, then the step terms: against the sum written out"""
    c = rp.ParityCase("pend")
    mod, K = c.model(), 64
    r = np.random.default_rng(1)
    ps, s = r.standard_normal(2), 0.2 * r.standard_normal((c.N, c.npn))
    x, l, L = c.policy
    _, logw, _, xi, xip = rp.one_pass(mod, x, l, L, None, 9, 0, K, s, ps)
    want = np.zeros(K)
    for i in range(2):
        want = want + (-ps[i] * (ps[i] + xip[:, i]) + 0.5 * ps[i] * ps[i])
    for t in range(c.N):
        for i in range(c.npn):
            want = want + (-s[t, i] * (s[t, i] + xi[:, t, i]) + 0.5 * s[t, i] * s[t, i])
    assert np.array_equal(logw, want)
    # the parameter stream is user_params_model.gen_draws' at the pass's seed (NumPy's sin and cos: to rounding)
    assert np.allclose(xip, pm.gen_draws(9, K, 2, 0)[0], rtol=0, atol=1e-14)


# ---- 3. the compile-only check and the exports ----------------------------------------------------------------------------------------------
def _check_rc(src, n, m, npar, npn, npu, ppn, ppu, nev):
    return nv.lib().rat_rare_event_params_check(src.encode(), n, m, npar, npn, npu, ppn, ppu, nev)


@pytest.mark.parametrize("name", ["pend", "lq12"])
def test_the_check_compiles_both_variants_of_the_cases(name):
    c = pm.case(name)
    np_ = len(c.p)
    assert _check_rc(c.source("scale"), c.n, c.m, np_, c.npn, c.npu, 2, 1, 0) == 0
    assert _check_rc(c.source("scale", event=True), c.n, c.m, np_, c.npn, c.npu, 2, 1, 1) == 0
    rat.rare_event_params_check(c.source("scale", event=True), c.n, c.m, np_, c.npn, c.npu, param_normals=2, param_uniforms=1, n_event=1)


def test_the_check_refuses_what_the_call_refuses():
    c = pm.case("pend")
    np_ = len(c.p)
    assert _check_rc(c.source(None), c.n, c.m, np_, c.npn, c.npu, 2, 1, 0) == ARG     # no hook
    assert "RAT_USER_PARAMS" in nv.lib().rat_last_error().decode()
    assert _check_rc(c.source("scale"), c.n, c.m, np_, c.npn, c.npu, 0, 1, 0) == ARG
    assert "param_normals is 0" in nv.lib().rat_last_error().decode()
    assert _check_rc(c.source("scale"), c.n, c.m, np_, c.npn, c.npu, 13, 1, 0) == UNSUPPORTED
    assert _check_rc(c.source("scale"), c.n, c.m, np_, c.npn, c.npu, 2, 1, 17) == ARG
    assert _check_rc(c.source("scale"), c.n, c.m, np_, c.npn, c.npu, 2, 1, -1) == ARG
    assert _check_rc(c.source("scale"), c.n, c.m, np_, c.npn, c.npu, 2, 1, 1) == ARG  # no rat_user_event
    assert _check_rc(c.source("scale"), c.n, c.m, np_, 0, c.npu, 2, 1, 0) == ARG      # no step normal to shift
    assert _check_rc(c.source("scale"), c.n, c.m, np_, 13, c.npu, 2, 1, 0) == UNSUPPORTED
    assert _check_rc(c.source("scale"), c.n, c.m, 0, c.npn, c.npu, 2, 1, 0) == ARG    # no parameters
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED.*param_normals is above 12"):
        rat.rare_event_params_check(c.source("scale"), c.n, c.m, np_, c.npn, c.npu, param_normals=13)


def _canon(t):
    if t is C.c_void_p:
        return "p:void"
    if t is C.c_char_p:
        return "cstr"
    if t is nv._dp:
        return "p:f64"
    return {C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_double: "f64"}[t]


def test_the_library_exports_both_symbols_with_the_declared_prototypes():
    lib = nv.lib()
    for name in ("rat_policy_rare_event_params", "rat_rare_event_params_check"):
        assert name in nv.EXPORTS and hasattr(lib, name) and name in PROTOS, name
        ret, args = PROTOS[name]
        assert ret == "i32" and [_canon(t) for t in getattr(lib, name).argtypes] == args, name
    assert len(PROTOS["rat_policy_rare_event_params"][1]) == 27 and len(PROTOS["rat_rare_event_params_check"][1]) == 9
    # no device: a null handle is an argument error, as for the other calls
    assert lib.rat_policy_rare_event_params(None, None, None, None, 64, 1, 0, 1, 0, 0, None, None, 0.0, 0, 0, None, None, 3, 1, 0.1,
                                            None, None, None, None, None, None, None) == ARG


def test_the_python_surface():
    import dataclasses
    import inspect
    names = [f.name for f in dataclasses.fields(rat.RareEventResult)]
    assert "param_shift" in names and "param_trace" in names
    sig = inspect.signature(rat.Context.policy_rare_event_params)
    for k in ("noise", "seed", "shift", "param_shift", "adapt", "n_iter", "rho", "n_event", "want_margins", "want_logw"):
        assert k in sig.parameters, k
    assert sig.parameters["adapt"].default == "both" and sig.parameters["n_iter"].default == 8 and sig.parameters["rho"].default == 0.1
    assert callable(rat.rare_event_probability_params)
    from ratilqr.jl_amd import generic                                # the pass-through of the general-size carrier
    assert any("policy_rare_event_params" in getattr(v, "__dict__", {}) for v in vars(generic).values() if inspect.isclass(v))


# ---- 4. code-object digests ------------------------------------------------------------------------------------------------------------------
# one request per line: kind n m npn npu nev npar ppn ppu pshift source-file; the answers are "R rc cached object digest" and the log, as
# test_cpu_source_kinds.PROBE gives them, the digest over the sections that hold what a kernel is (code_digest below).  Built without
# PROBE_PSHIFT the program reads the column and leaves SrcShape as it is: the program that recorded tests/golden/rare_event_params_digests.json
# on the parent commit, whose SrcShape has no such field.
PROBE = r"""
#include "source_model.h"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
// FNV-1a over the sections .note, .rodata and .text of an ELF64 code object: the kernels' metadata (registers, scratch, arguments), their
// descriptors and their instructions.  Not over the symbol tables: the compiler names a symbol __hip_cuid_<hash of everything it was
// given>, headers the translation unit never includes among them, so the whole file's bytes change with a comment in any embedded header.
template <class T> static T rd(const std::vector<char> &o, size_t at) {
    T v = 0;
    if (at + sizeof(T) <= o.size()) std::memcpy(&v, o.data() + at, sizeof(T));
    return v;
}
static unsigned long long code_digest(const std::vector<char> &o) {
    unsigned long long fnv = 1469598103934665603ull;
    const size_t shoff = rd<unsigned long long>(o, 0x28), entsize = rd<unsigned short>(o, 0x3A), shnum = rd<unsigned short>(o, 0x3C);
    const size_t strsec = shoff + entsize * rd<unsigned short>(o, 0x3E), stroff = rd<unsigned long long>(o, strsec + 0x18);
    int found = 0;
    for (size_t i = 0; i < shnum; ++i) {
        const size_t sh = shoff + i * entsize, name = stroff + rd<unsigned>(o, sh), off = rd<unsigned long long>(o, sh + 0x18),
                     size = rd<unsigned long long>(o, sh + 0x20);
        if (name >= o.size() || rd<unsigned>(o, sh + 4) == 8 /* SHT_NOBITS */ || off + size > o.size()) continue;
        const char *nm = o.data() + name;
        if (std::strncmp(nm, ".note", 6) && std::strncmp(nm, ".rodata", 8) && std::strncmp(nm, ".text", 6)) continue;
        ++found;
        for (size_t k = 0; k < size; ++k) fnv = (fnv ^ (unsigned char)o[off + k]) * 1099511628211ull;
    }
    return found == 3 ? fnv : 0;
}
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream req(argv[1]);
    std::vector<const void *> seen;
    int kind, n, m, pshift;
    SrcShape shape;
    std::string path;
    while (req >> kind >> n >> m >> shape.npn >> shape.npu >> shape.nev >> shape.npar >> shape.ppn >> shape.ppu >> pshift >> path) {
#ifdef PROBE_PSHIFT
        shape.pshift = pshift;
#endif
        std::ifstream f(path);
        std::stringstream text;
        text << f.rdbuf();
        std::shared_ptr<const std::vector<char>> code;
        std::string log;
        bool cached = false;
        const rat_rc rc = src_compile((SrcKind)kind, text.str().c_str(), n, m, shape, "gfx950", &code, &log, nullptr, &cached);
        int id = -1;
        unsigned long long fnv = 0;
        if (code) {
            for (id = 0; id < (int)seen.size() && seen[id] != code.get(); ++id) {}
            if (id == (int)seen.size()) seen.push_back(code.get());
            fnv = code_digest(*code);
        }
        for (char &c : log) if (c == '\n') c = '|';
        std::printf("R %d %d %d %016llx\nL %s\n", (int)rc, cached ? 1 : 0, id, fnv, log.c_str());
        std::fflush(stdout);
    }
    return 0;
}
"""
# every function a kind can ask for in one text (test_cpu_source_kinds.ALL), and a hook that draws two normals and a uniform
ALL_P = (ue.source(ue.DI, "half", len(ue.DI_P)) + PENDULUM.split("template <class T> __device__ T rat_user_c")[0] +
         pm.source("", "scale", pi0=0, pi1=1, pi2=2, psh=0.1))
NPAR = len(ue.DI_P)
KIND_NAMES = ("SRC_MODEL", "SRC_PETS", "SRC_NOISY", "SRC_USER_NOISE", "SRC_RARE", "SRC_EVENTS", "SRC_RARE_USER", "SRC_PARAMS")
OFF = [(k, 0, 0, 0, 0) for k in range(7)]                             # sampling off: seven kinds (SRC_PARAMS is compiled with sampling on)
ON = [(k, NPAR, 2, 1, 0) for k in range(8)]                           # sampling on, pshift = 0: all eight
SHIFTED = [(k, NPAR, 2, 1, 1) for k in range(8)]                      # sampling on, pshift = 1
REQUESTS = OFF + ON + SHIFTED + [(4, 0, 0, 0, 1)]                     # ... and pshift = 1 with sampling off: refused by the header
GOLDEN = os.path.join(ROOT, "tests", "golden", "rare_event_params_digests.json")


def compiler_id():
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    out = subprocess.run([hipcc, "--version"], capture_output=True, text=True, timeout=60).stdout
    return " | ".join(ln.strip() for ln in out.split("\n") if ln.startswith(("HIP version", "AMD clang version")))


def run_digest_probe(tmp, csrc=CSRC, flags=("-DPROBE_PSHIFT=1",), requests=REQUESTS):
    embed_inc(os.path.join(tmp, "source_embed.inc")) if csrc == CSRC else None
    with open(os.path.join(tmp, "probe.cpp"), "w") as f:
        f.write(PROBE)
    with open(os.path.join(tmp, "all_p.hip"), "w") as f:
        f.write(ALL_P)
    with open(os.path.join(tmp, "requests.txt"), "w") as f:
        for kind, npar, ppn, ppu, pshift in requests:
            f.write(f"{kind} 2 1 2 0 1 {npar} {ppn} {ppu} {pshift} {os.path.join(tmp, 'all_p.hip')}\n")
    exe = os.path.join(tmp, "probe")
    subprocess.run(["c++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", *flags, "-I", ROCM_INC, "-I", csrc, "-I", tmp,
                    os.path.join(tmp, "probe.cpp"), os.path.join(csrc, "source_model.cpp"), "-o", exe, "-ldl", "-pthread"], check=True, timeout=300)
    out = subprocess.run([exe, os.path.join(tmp, "requests.txt")], check=True, capture_output=True, text=True, timeout=900).stdout.split("\n")
    answers = []
    for r, l in zip(out[0::2], out[1::2]):
        rc, cached, obj, digest = r.split()[1:]
        answers.append(dict(rc=int(rc), cached=int(cached), obj=int(obj), digest=digest, log=l[2:]))
    assert len(answers) == len(requests), out
    return answers


@pytest.fixture(scope="module")
def digests(tmp_path_factory):
    if shutil.which("c++") is None or not os.path.exists(os.path.join(ROCM_INC, "hip", "hiprtc.h")):
        pytest.skip("no host C++ compiler or no hiprtc.h")
    return run_digest_probe(str(tmp_path_factory.mktemp("rare_event_params_digests")))


def test_pshift_is_another_cache_entry_for_the_two_rare_kinds_alone(digests):
    off, on, shifted, refused = digests[:7], digests[7:15], digests[15:23], digests[23]
    for name, a in zip(KIND_NAMES, off + on[7:]):
        assert a["rc"] == 0 and int(a["digest"], 16) != 0, (name, a)
    for k, (a, b) in enumerate(zip(on, shifted)):
        assert a["rc"] == 0 and b["rc"] == 0, (KIND_NAMES[k], a, b)
        if k in (4, 6):                                               # SRC_RARE, SRC_RARE_USER: another entry, another module
            assert not b["cached"] and b["obj"] != a["obj"] and b["digest"] != a["digest"], (KIND_NAMES[k], a, b)
        else:                                                         # no part of the key: the entry of pshift = 0 again
            assert b["cached"] == 1 and b["obj"] == a["obj"], (KIND_NAMES[k], a, b)
    for k in (0, 1, 2):                                               # kinds without parameter draws: sampling is no part of their key either
        assert on[k]["cached"] == 1 and on[k]["obj"] == off[k]["obj"], KIND_NAMES[k]
    assert refused["rc"] == ARG and refused["obj"] == -1 and "RAT_PARAM_SHIFT needs parameter sampling on" in refused["log"]


def test_with_pshift_zero_every_module_is_what_the_parent_commit_compiled(digests):
    """the digests of the seven kinds with sampling off and of all eight with sampling on, pshift = 0, against the ones the same program
    recorded on the parent commit (profiles/policy_rare_event_params.md has both lists).  A code object's bytes belong to a compiler: the
    recorded list names its own, and another compiler's objects cannot be held against it."""
    gold = json.load(open(GOLDEN))
    if gold["compiler"] != compiler_id():
        pytest.skip(f"the digests were recorded with {gold['compiler']!r}; this is {compiler_id()!r}")
    got = {"off": [a["digest"] for a in digests[:7]], "on": [a["digest"] for a in digests[7:15]]}
    for part in ("off", "on"):
        for name, a, b in zip(KIND_NAMES, got[part], gold[part]):
            assert a == b, (part, name, a, b)
