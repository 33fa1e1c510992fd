"""The reference of tests/test_gpu_source_shapes.py, pinned without a device.  The generated source (tests/source_shapes_model.py) is
compiled as host C++ against csrc/rat_ad.h and its AD derivatives are compared with the hand-written NumPy closed forms: two independent
derivations.  rat_source_check cross-compiles it for gfx950 at every shape, and the oracle's closure path solves every solve case."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ratilqr.jl_amd as rat
from oracle import oracle as orc

import source_shapes_model as ssm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ratilqr.jl_amd", "csrc")
K_VALUES = (0, 3)

HOST_MAIN = r"""
static void line(double v) { std::printf("%.17g\n", v); }
int main() {
    const int n = RAT_N, m = RAT_M, nz = RAT_N + RAT_M;
    for (int pt = 0; pt < NPT; ++pt) {
        const double *x = PTS[pt], *u = PTS[pt] + n;
        for (int kk = 0; kk < NK; ++kk) {                                // c, grad c, hess c (row-major over z = (x, u))
            line(rat_user_c<double>(KS[kk], x, u, P));
            for (int i = 0; i < nz; ++i)
                for (int j = 0; j < nz; ++j) {
                    rat_hdual xh[RAT_N], uh[RAT_M];
                    for (int q = 0; q < n; ++q) xh[q] = rat_hdual(x[q], q == i, q == j, 0.0);
                    for (int q = 0; q < m; ++q) uh[q] = rat_hdual(u[q], n + q == i, n + q == j, 0.0);
                    const rat_hdual r = rat_user_c<rat_hdual>(KS[kk], xh, uh, P);
                    if (j == 0) line(r.e1);
                    line(r.e12);
                }
        }
        line(rat_user_h<double>(x, P));                                  // h, grad h, hess h
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                rat_hdual xh[RAT_N];
                for (int q = 0; q < n; ++q) xh[q] = rat_hdual(x[q], q == i, q == j, 0.0);
                const rat_hdual r = rat_user_h<rat_hdual>(xh, P);
                if (j == 0) line(r.e1);
                line(r.e12);
            }
        double xn[RAT_N];                                                // f, then the columns of [f_x | f_u]
        rat_user_f<double>(x, u, xn, P);
        for (int i = 0; i < n; ++i) line(xn[i]);
        for (int col = 0; col < nz; ++col) {
            rat_dual xd[RAT_N], ud[RAT_M], xo[RAT_N];
            for (int q = 0; q < n; ++q) xd[q] = rat_dual(x[q], q == col);
            for (int q = 0; q < m; ++q) ud[q] = rat_dual(u[q], n + q == col);
            rat_user_f<rat_dual>(xd, ud, xo, P);
            for (int i = 0; i < n; ++i) line(xo[i].d);
        }
    }
    return 0;
}
"""


def c_array(name, a):
    a = np.atleast_2d(np.asarray(a, float))
    rows = ",\n".join("{" + ", ".join(float(v).hex() for v in r) + "}" for r in a)
    return f"static const double {name}[{a.shape[0]}][{a.shape[1]}] = {{\n{rows}}};\n"


def want_lines(mdl, pts):
    n = mdl.n
    out = []
    for z in pts:
        x, u = z[:n], z[n:]
        for k in K_VALUES:
            val, (qv, Q, rv, R, P) = mdl.c_all(k, x, u)
            g, H = np.concatenate([qv, rv]), np.block([[Q, P.T], [P, R]])
            out.append(val)
            for i in range(mdl.nz):
                out.append(g[i]); out.extend(H[i])
        val, (qv, Q) = mdl.h_all(x)
        out.append(val)
        for i in range(n):
            out.append(qv[i]); out.extend(Q[i])
        xn, A, B = mdl.f(x, u, True)
        out.extend(xn); out.extend(np.hstack([A, B]).T.ravel())
    return np.array(out)


@pytest.mark.skipif(shutil.which("c++") is None, reason="no host C++ compiler")
@pytest.mark.parametrize("n,m", [(12, 4), (10, 1), (1, 4)])
def test_host_compiled_source_matches_the_numpy_closed_forms(tmp_path, n, m):
    mdl = ssm.model(n, m, ssm.SEED[(n, m)])
    pts = 0.7 * np.random.default_rng(11).standard_normal((2, n + m))
    assert min(mdl.margin(z[:n], z[n:]) for z in pts) > 0.1              # every argument inside its domain and off the kinks
    text = ('#include "rat_ad.h"\n#include <cstdio>\n' + mdl.source + f"#define NPT {len(pts)}\n#define NK {len(K_VALUES)}\n"
            + "static const int KS[NK] = {" + ", ".join(map(str, K_VALUES)) + "};\n"
            + c_array("PP", mdl.p) + "static const double *P = PP[0];\n" + c_array("PTS", pts) + HOST_MAIN)
    src, exe = tmp_path / "shapes.cpp", tmp_path / "shapes"
    src.write_text(text)
    subprocess.run(["c++", "-std=c++17", "-O2", "-D__device__=", f"-DRAT_N={n}", f"-DRAT_M={m}", "-I", CSRC, str(src), "-o", str(exe)],
                   check=True, timeout=300)
    got = np.array(subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split(), float)
    want = want_lines(mdl, pts)
    assert got.shape == want.shape
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"({n}, {m}): worst scaled error {err.max():.3e} over {want.size} numbers")
    assert err.max() < 1e-13, (int(err.argmax()), got[err.argmax()], want[err.argmax()])


def test_reference_is_not_degenerate():
    """What lets the GPU comparison see a transposition or a dropped pair: no structural zero anywhere, P not symmetric."""
    for (n, m) in ssm.SHAPES:
        mdl = ssm.model(n, m, ssm.SEED[(n, m)])
        z = 0.7 * np.random.default_rng(3).standard_normal(n + m)
        _, (qv, Q, rv, R, P) = mdl.c_all(1, z[:n], z[n:])
        _, (_, Qf) = mdl.h_all(z[:n])
        A, B = mdl.jac(z[:n], z[n:])
        assert np.all(P != 0) and np.all(A != 0) and np.all(B != 0) and np.all(Q != 0) and np.all(R != 0) and np.all(Qf != 0)
        assert np.array_equal(Q, Q.T) and np.array_equal(R, R.T)


@pytest.mark.parametrize("n,m", ssm.SHAPES)
def test_source_check_accepts_the_generated_source(n, m):
    rat.native.source_check(ssm.source(), n, m)
    if (n, m) == (3, 2):
        rat.native.source_check(ssm.source(domain_variant=True), n, m)


_SOLVES = {}


def oracle_solve(n, m, theta):
    if (n, m, theta) not in _SOLVES:
        mdl, x0, u0 = ssm.solve_case(n, m)
        cp = orc.ClosureProblem(mdl.f, mdl.c, mdl.h, ssm.noise(n), ssm.SOLVE_N, n, m, mdl.jac, mdl.c_derivatives, mdl.h_derivatives)
        _SOLVES[(n, m, theta)] = (mdl, orc.closure_solve(cp, x0, u0, theta))
    return _SOLVES[(n, m, theta)]


@pytest.mark.parametrize("theta", ssm.SOLVE_THETAS)
@pytest.mark.parametrize("n,m", ssm.SOLVE_SHAPES)
def test_oracle_solves_the_reference_model(n, m, theta):
    mdl, r = oracle_solve(n, m, theta)
    assert r["status"] == 0 and r["iters"] >= 2, (r["status"], r["iters"])
    assert mdl.margin(r["x"], r["l"]) > 0.1


def test_a_line_search_rejects_a_candidate():
    """One line-search evaluation per iteration means every first candidate was accepted; more means a rejection (or a sweep that failed)."""
    runs = {(n, m, th): oracle_solve(n, m, th)[1] for (n, m) in ssm.SOLVE_SHAPES for th in ssm.SOLVE_THETAS}
    rejected = [k for k, r in runs.items() if r["ls_evals"] > r["iters"] and any(e[1] > 0 for e in r["eps_history"])]
    print("solve cases with a rejected candidate:", rejected)
    assert rejected
