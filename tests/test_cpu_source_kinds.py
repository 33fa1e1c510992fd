"""The table of source-model kinds (csrc/source_model.h: SrcKind, src_kind, src_compile) without a device and without the library: a
stand-alone program linked against csrc/source_model.cpp compiles one source for gfx950 as every kind and reports, per request, the return
code, whether the code object came from the process-wide cache, which object it is, whether it holds the entry names of its table row, and
the log.  Nothing here looks at a code object's size or bytes beyond those names: they depend on the compiler's version."""
import os
import re
import shutil
import subprocess

import pytest

import user_event_model as ue
from source_pets_models import PENDULUM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ratilqr.jl_amd", "csrc")
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
KINDS = ("SRC_MODEL", "SRC_PETS", "SRC_NOISY", "SRC_USER_NOISE", "SRC_RARE", "SRC_EVENTS", "SRC_RARE_USER")
ARG = 1

# one request per line of the file argv[1]: kind n m npn npu nev source-file.  One answer per request:
# "R rc cached object size digest entries" (object: 0, 1, ... in order of first appearance, -1 without one; digest: FNV-1a of the bytes),
# then "L " and the log with its line ends as '|'
PROBE = r"""
#include "source_model.h"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
static bool holds(const std::vector<char> &obj, const char *name) {
    const size_t k = std::strlen(name);
    for (size_t i = 0; i + k <= obj.size(); ++i) if (!std::memcmp(obj.data() + i, name, k)) return true;
    return false;
}
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream req(argv[1]);
    std::vector<const void *> seen;
    int kind, n, m;
    SrcShape shape;
    std::string path;
    while (req >> kind >> n >> m >> shape.npn >> shape.npu >> shape.nev >> path) {
        std::ifstream f(path);
        std::stringstream text;
        text << f.rdbuf();
        std::shared_ptr<const std::vector<char>> code;
        std::string log;
        bool cached = false;
        const rat_rc rc = src_compile((SrcKind)kind, text.str().c_str(), n, m, shape, "gfx950", &code, &log, nullptr, &cached);
        int id = -1, entries = 0;
        unsigned long long fnv = 1469598103934665603ull;
        if (code) {
            for (id = 0; id < (int)seen.size() && seen[id] != code.get(); ++id) {}
            if (id == (int)seen.size()) seen.push_back(code.get());
            for (char c : *code) fnv = (fnv ^ (unsigned char)c) * 1099511628211ull;
            const SrcKindRow &row = src_kind((SrcKind)kind);
            entries = holds(*code, row.entry) && (!row.entry2 || holds(*code, row.entry2));
        }
        for (char &c : log) if (c == '\n') c = '|';
        std::printf("R %d %d %d %zu %016llx %d\nL %s\n", (int)rc, cached ? 1 : 0, id, code ? code->size() : (size_t)0, fnv, entries, log.c_str());
        std::fflush(stdout);
    }
    return 0;
}
"""

# every function a kind can ask for in one text (n = 2, m = 1): f, c, h, the sampler, the event "half", and a generative f
ALL = ue.source(ue.DI, "half", len(ue.DI_P)) + PENDULUM.split("template <class T> __device__ T rat_user_c")[0]
NO_EVENT = ue.DI
NO_NOISE = ue.source(ue.DI.split("#define RAT_USER_NOISE")[0], "half", len(ue.DI_P))
# (kind, npn, npu, nev, source): every kind once, every kind again, then one field changed at a time, then the refusals
FIRST = [(k, 2, 0, 1, "all") for k in range(7)]
CHANGED = [(3, 3, 0, 0, "all"), (3, 2, 1, 0, "all"), (5, 0, 0, 2, "all"), (6, 2, 0, 2, "all")]
IGNORED = [(2, 5, 5, 5, "all"), (4, 2, 0, 9, "all"), (5, 7, 7, 1, "all")]       # fields the kind does not take: the first entries again
REFUSED = [(5, 0, 0, 1, "no_event"), (6, 2, 0, 1, "no_event"), (3, 2, 0, 0, "no_noise"), (4, 2, 0, 0, "no_noise")]
REQUESTS = FIRST + FIRST + CHANGED + IGNORED + REFUSED


def embed_inc(path):
    """csrc/Makefile's rule for source_embed.inc: the headers of EMBED_H as raw string literals, then the arrays of their texts and names"""
    names = re.search(r"^EMBED_H = (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    with open(path, "w") as out:
        for name in names:
            out.write('static const char k_embed_%s[] = R"RATEMBED(' % name.replace(".", "_"))
            out.write(open(os.path.join(CSRC, name)).read())
            out.write(')RATEMBED";\n')
        out.write("static const char *const k_embed_texts[] = {%s};\n" % "".join("k_embed_%s, " % name.replace(".", "_") for name in names))
        out.write("static const char *const k_embed_names[] = {%s};\n" % "".join('"%s", ' % name for name in names))


def build_probe(tmp, flags=()):
    """the probe as a plain executable in `tmp`"""
    embed_inc(os.path.join(tmp, "source_embed.inc"))
    with open(os.path.join(tmp, "probe.cpp"), "w") as f:
        f.write(PROBE)
    exe = os.path.join(tmp, "probe")
    subprocess.run(["c++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", *flags, "-I", ROCM_INC, "-I", CSRC, "-I", tmp,
                    os.path.join(tmp, "probe.cpp"), os.path.join(CSRC, "source_model.cpp"), "-o", exe, "-ldl", "-pthread"],
                   check=True, timeout=300)
    return exe


def run_probe(exe, tmp, requests, sources):
    for name, text in sources.items():
        with open(os.path.join(tmp, name + ".hip"), "w") as f:
            f.write(text)
    with open(os.path.join(tmp, "requests.txt"), "w") as f:
        for kind, npn, npu, nev, name in requests:
            f.write(f"{kind} 2 1 {npn} {npu} {nev} {os.path.join(tmp, name + '.hip')}\n")
    out = subprocess.run([exe, os.path.join(tmp, "requests.txt")], check=True, capture_output=True, text=True, timeout=600).stdout.split("\n")
    answers = []
    for r, l in zip(out[0::2], out[1::2]):
        rc, cached, obj, size, digest, entries = r.split()[1:]
        answers.append(dict(rc=int(rc), cached=int(cached), obj=int(obj), size=int(size), digest=digest, entries=int(entries), log=l[2:]))
    assert len(answers) == len(requests), out
    return answers


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    if shutil.which("c++") is None or not os.path.exists(os.path.join(ROCM_INC, "hip", "hiprtc.h")):
        pytest.skip("no host C++ compiler or no hiprtc.h")
    tmp = str(tmp_path_factory.mktemp("source_kinds"))
    return run_probe(build_probe(tmp), tmp, REQUESTS, {"all": ALL, "no_event": NO_EVENT, "no_noise": NO_NOISE})


def test_every_kind_compiles_the_all_in_one_source_and_exports_its_entries(answers):
    for kind, a in zip(KINDS, answers[:7]):
        assert a["rc"] == 0 and not a["cached"] and a["entries"] == 1, (kind, a)
    assert [a["obj"] for a in answers[:7]] == list(range(7))          # seven kinds, seven cache entries


def test_the_same_key_comes_from_the_cache_as_the_same_object(answers):
    for kind, a, b in zip(KINDS, answers[:7], answers[7:14]):
        assert b["rc"] == 0 and b["cached"] == 1 and b["obj"] == a["obj"], (kind, a, b)


def test_another_draw_count_or_n_event_is_another_entry(answers):
    for i, a in enumerate(answers[14:18]):
        assert a["rc"] == 0 and not a["cached"] and a["obj"] == 7 + i and a["entries"] == 1, (CHANGED[i], a)


def test_a_field_the_kind_does_not_take_is_no_part_of_the_key(answers):
    for req, a in zip(IGNORED, answers[18:21]):
        assert a["rc"] == 0 and a["cached"] == 1 and a["obj"] == req[0], (req, a)


def test_a_source_without_the_event_or_the_sampler_is_refused_by_the_kinds_that_need_it(answers):
    for req, a in zip(REFUSED, answers[21:25]):
        want = "RAT_USER_EVENT" if req[4] == "no_event" else "RAT_USER_NOISE"
        assert a["rc"] == ARG and a["obj"] == -1 and "does not define " + want in a["log"], (req, a)
