"""csrc/rat_ad.h on the host at domain edges, kinks, ties, branch switches and extreme scales: the table of tests/ad_edge_cases.py, every case
under rat_dual seeded on each variable in turn and under rat_hdual seeded on every pair (i <= j) -- what rat_src_linearize does -- against
mpmath at the regular points and against the table's classes at the singular ones.  tests/test_gpu_ad_edges.py runs the same table on
the device."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import ad_edge_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AD_H = os.path.join(ROOT, "ratilqr.jl_amd", "csrc", "rat_ad.h")


def test_every_declared_family_has_a_regular_and_an_edge_case():
    declared = T.declared_families(open(AD_H).read())
    # the parse found what the header has: the arithmetic forms, the compound assignments, the comparisons, the functions
    assert {"operator+:TT", "operator/:dT", "operator-:T", "operator*=:Td", "operator<=:dT", "operator!=:TT", "sin:T", "pow:Td", "pow:TT",
            "pow:dT", "fmin:dT", "atan2:Td", "fabs:T"} <= declared and len(declared) == 57, sorted(declared)
    regular = {f for c in T.CASES for f in c.fams if any(p.kind == "regular" for p in c.points)}
    edges = {f for c in T.CASES for f in c.fams if any(p.kind == "singular" or p.edge for p in c.points)}
    assert not declared - regular, sorted(declared - regular)
    assert not declared - edges, sorted(declared - edges)
    assert not (regular | edges) - declared, sorted((regular | edges) - declared)      # no case names a family the header lacks


def test_regular_points_are_finite_and_well_conditioned():
    """Moving any argument by one ulp moves every reference number by less than a tenth of the (host) bound."""
    n = 0
    for k, (c, p) in enumerate(T.ITEMS):
        if p.kind != "regular":
            continue
        n += 1
        v, g, H = T.item_reference(k)
        base = np.array([v, *g, *[H[ij] for ij in T.PAIRS]])
        assert np.all(np.isfinite(base)), (c.name, p.z)
        for q in range(3):
            for to in (-np.inf, np.inf):
                z = list(p.z)
                z[q] = float(np.nextafter(z[q], to))
                v2, g2, H2 = T.reference(c.ref, z)
                moved = np.array([v2, *g2, *[H2[ij] for ij in T.PAIRS]])
                worst = np.max(np.abs(moved - base) / np.maximum(1.0, np.abs(base)))
                assert worst < 0.1 * T.HOST_BOUND, (c.name, p.z, q, worst)
    assert n == sum(p.kind == "regular" for _, p in T.ITEMS) and n > 150


def test_the_pinned_tokens_are_used_where_the_table_says():
    """`fin` (finite, number reported) stands in one place only: the curvature of x / x at 1e-100."""
    fin = [(c.name, p.z[0]) for c, p in T.ITEMS if p.kind == "singular" and " fin" in p.expect]
    assert fin == [("xoverx@", 1e-100)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if shutil.which("c++") is None:
        pytest.fail("no host C++ compiler: the AD header cannot be checked")
    d = tmp_path_factory.mktemp("ad_edges")
    src, exe = d / "ad_edges.cpp", d / "ad_edges"
    src.write_text(T.host_program())
    subprocess.run(["c++", "-std=c++17", "-O2", "-I", os.path.dirname(AD_H), str(src), "-o", str(exe)], check=True, timeout=300)
    return T.parse_host_output(subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout)


def host_outputs(r):
    """(what, index, got) for every output of one item on the host; the hyper-dual outputs of every pair, the dual ones of every seed."""
    for (i, j), (v, e1, e2, e12) in r["hd"].items():
        yield "v", None, v
        yield "g", i, e1
        yield "g", j, e2
        yield "H", (i, j), e12
    for i in range(3):
        yield "v", None, r["dual"][i][0]
        yield "dual", i, r["dual"][i][1]
    yield "v", None, r["dual"][3][0]
    yield "unused", None, r["dual"][3][1]


def test_ad_header_on_the_host_over_the_table(host):
    assert sorted(host) == list(range(len(T.ITEMS)))                   # every item ran, none twice
    bad, ran, worst, worst_rel = [], 0, {}, {}
    for k, (c, p) in enumerate(T.ITEMS):
        r, want, ref = host[k], T.expected(k), T.item_reference(k)
        assert len(r["hd"]) == 6 and len(r["dual"]) == 4
        ran += 1
        for what, idx, got in host_outputs(r):
            token = T.expected_dual(k)[idx] if what == "dual" else want[what] if idx is None else want[what][idx]
            w = T.resolve(token, k, "g" if what == "dual" else what, idx)
            msg = T.check_token(got, token, w, T.HOST_BOUND)
            if msg:
                bad.append(f"{c.name} at {p.z} {what}{'' if idx is None else idx}: {msg}")
            if what != "unused" and ref is not None and math.isfinite(got):     # the report: against mpmath wherever there is a reference
                m = float(ref[0] if what == "v" else ref[1][idx] if what in ("g", "dual") else ref[2][idx])
                worst[c.fn] = max(worst.get(c.fn, 0.0), T.err(got, m))
                if m != 0:
                    worst_rel[c.fn] = max(worst_rel.get(c.fn, 0.0), abs(got - m) / abs(m))
        if p.kind == "singular" and not p.dual:                        # the two types agree in the class of every first partial
            for i in range(3):
                assert T.same_class(r["dual"][i][1], r["hd"][(i, i)][1]), (c.name, p.z, i)
    print("function            worst |err| / max(1, |want|)   worst |err| / |want|   (host)")
    for fn in sorted(worst):
        print(f"{fn:18s}  {worst[fn]:.2e}                       {worst_rel.get(fn, 0.0):.2e}")
    assert ran == len(T.ITEMS)
    assert not bad, "\n".join(bad)


def test_the_two_types_agree_on_x_over_x_inside_the_documented_range(host):
    """Denominators in [1e-100, 1e100]: the same value and the same first partial from rat_dual and rat_hdual."""
    seen = 0
    for k, (c, p) in enumerate(T.ITEMS):
        if c.fn == "self_quot" and 1e-100 <= abs(p.z[0]) <= 1e100:
            seen += 1
            for i in range(3):
                d, h = host[k]["dual"][i], host[k]["hd"][(i, i)]
                assert d[0] == h[0] and abs(d[1] - h[1]) <= T.HOST_BOUND, (p.z, i, d, h)
    assert seen >= 4
