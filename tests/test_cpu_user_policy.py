"""The controller the user writes (rat_user_policy, include/ratilqr.h "source models"): what can be checked without a device -- the NumPy
model of tests/user_policy_model.py against the models it restates and its own claims (the clamp bites, the rate limiter reads u_prev),
the compile-only entry point rat_user_policy_check (hiprtc for gfx950) and every other module kind on the test sources, the export and
its mirrors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ratilqr.jl_amd as rat
import user_noise_model as um
import user_policy_model as up
from ratilqr.jl_amd import _native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED = 0, 1, 2


def last_error():
    return nv.lib().rat_last_error().decode()


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("name", up.CASE_NAMES)
def test_the_hookless_model_is_the_existing_model(name, closed):
    """without a hook, and with the identity hook: user_noise_model.np_rollouts' numbers on its inputs, bit for bit -- under the sampler
    and under chol(W) z written as a sampler"""
    c = up.case(name)
    f, cc, h, noise = c.fns
    x_nom, l, L = c.args(closed)
    zu = None if c.zu is None else c.zu.ravel()
    ref = um.np_rollouts(f, cc, h, noise, c.params(), x_nom, l, L, c.K, c.zn.ravel(), zu, c.npn, c.npu)
    gauss = lambda k, x, u, rng, p: c.Wchol @ np.array([rng.normal() for _ in range(c.n)])
    ref_g = um.np_rollouts(f, cc, h, gauss, c.params(), x_nom, l, L, c.K, c.z.ravel(), None, c.n, 0)
    for hook in (None, "identity"):
        for got, want in ((c.model(hook, closed), ref), (c.model(hook, closed, gaussian=True), ref_g)):
            for a, b in zip(got, want):
                assert np.array_equal(a, b)


@pytest.mark.parametrize("name", up.CASE_NAMES)
def test_the_clamp_bites_and_the_rate_limiter_reads_u_prev(name):
    c = up.case(name)
    clamp, rate = c.q[0], c.q[1]
    # the hookless policy leaves the limits in more than a quarter of the (rollout, step) pairs, under either disturbance
    for gaussian in (False, True):
        _, _, us = c.model(None, True, gaussian=gaussian)
        share = up.beyond(us, clamp)
        print(f"{name} gaussian={gaussian}: the hookless policy is beyond the clamp {clamp:.4f} in {share:.3f} of the pairs")
        assert share > 0.25
    assert (np.abs(c.policy[1]) > clamp).any()                       # open loop too: some l_t is beyond it
    for closed in (False, True):
        cost0, _, _ = c.model(None, closed)
        cost, xs, us = c.model("clamp", closed)
        assert np.abs(us).max() == clamp and not np.array_equal(cost, cost0)
        # every entry is the affine law of the state the clamped loop reached, clamped
        x_nom, l, L = c.args(closed)
        aff = np.broadcast_to(l, us.shape) if L is None else l + np.einsum("tij,ktj->kti", L, xs[:, :-1] - x_nom[:-1])
        assert np.allclose(us, np.clip(aff, -clamp, clamp), rtol=0, atol=1e-13 * clamp)    # (einsum sums in another order than @)
        _, _, ur = c.model("rate", closed)
        steps = np.diff(np.concatenate([np.zeros_like(ur[:, :1]), ur], axis=1), axis=1)
        assert np.abs(ur).max() <= clamp and np.abs(steps).max() <= rate * (1 + 1e-15)
        assert (np.abs(steps) >= rate * (1 - 1e-15)).mean() > 0.1 and not np.array_equal(ur, us)      # the rate limit bites as well


def test_a_nan_from_the_hook_is_a_nan_cost_in_the_model():
    c = up.case("pend")
    _, xs, _ = c.model("clamp", True)
    j = int(np.argmax(xs[:, 1:-1, 0].max(axis=1)))
    top = np.sort(xs[:, 1:-1, 0].max(axis=1))                        # (x_0 is the same point on every rollout, and below these)
    q = c.q.copy()
    q[2] = 0.5 * (top[-1] + top[-2])                                 # between the largest and the second largest: rollout j alone crosses
    cost, _, us = c.model("nan", True, q=q)
    assert np.array_equal(np.isnan(cost), np.arange(c.K) == j) and np.isnan(us[j]).any()


# ---- the kernels compile without a device -------------------------------------------------------------------------------------------------
def sources(name):
    """every hook on the case's source: (text, n, m, normals, uniforms); with the pendulum, the sampler that reads u as well"""
    c = up.case(name)
    out = [(up.source(c.base, c.poff, hook), c.n, c.m, c.npn, c.npu) for hook in up.BODIES]
    if name == "pend":
        out.append((up.source(up.PEND_UDEP, 3, "clamp"), 2, 1, 2, 0))
    return out


@pytest.mark.parametrize("name", up.CASE_NAMES)
def test_every_test_source_compiles_as_every_module_kind(name):
    lib = nv.lib()
    for text, n, m, npn, npu in sources(name):
        ev = up.with_u_event(text, 900).encode()                     # (the kinds with events need rat_user_event)
        assert lib.rat_user_policy_check(text.encode(), n, m) == OK, last_error()
        assert lib.rat_source_check(text.encode(), n, m) == OK, last_error()
        assert lib.rat_user_noise_check(text.encode(), n, m, npn, npu) == OK, last_error()
        assert lib.rat_rare_event_noise_check(text.encode(), n, m, npn, npu) == OK, last_error()
        assert lib.rat_user_event_check(ev, n, m, 1) == OK, last_error()
        assert lib.rat_rare_event_user_check(ev, n, m, npn, npu, 1) == OK, last_error()


def test_what_the_check_returns():
    chk = nv.lib().rat_user_policy_check
    c = up.case("pend")
    good = up.source(c.base, c.poff, "rate")
    assert chk(good.encode(), 2, 1) == OK, last_error()
    # a source without the hook: the message says what to define -- also after the same text was compiled as the hookless kernel
    for _ in range(2):
        assert chk(c.base.encode(), 2, 1) == ARG
        assert "does not define RAT_USER_POLICY" in last_error() and "rat_user_policy(k, x, u_prev, u, p)" in last_error()
    # a wrong signature: the compiler's log, with the line of the user's text
    bad = c.base + "#define POFF 3\n" + up.WRONG_SIGNATURE + up.BODIES["clamp"] + "}\n"
    line = bad[:bad.index("__device__ void rat_user_policy")].count("\n") + 1
    assert chk(bad.encode(), 2, 1) == ARG
    assert "no matching function for call to 'rat_user_policy'" in last_error() and re.search(rf"model\.hip:{line}:", last_error()), last_error()
    # a syntax error inside the hook
    syn = good.replace("fmin(fmax(u_prev[i] + d, -q[0]), q[0]);", "fmin(fmax(u_prev[i] + d, -q[0]), q[0])")
    line = syn[:syn.index("u[i] = fmin(fmax(u_prev[i] + d")].count("\n") + 1
    assert chk(syn.encode(), 2, 1) == ARG and re.search(rf"model\.hip:{line}:", last_error()), last_error()
    big = up.source(um.LQ_MIX, "ohi + 1", "clamp").encode()
    assert chk(big, 13, 4) == UNSUPPORTED and chk(big, 12, 5) == UNSUPPORTED
    assert chk(None, 2, 1) == ARG and chk(good.encode(), 0, 1) == ARG
    # the Python mirror raises on a refusal
    rat.user_policy_check(good, 2, 1)
    with pytest.raises(rat.RatError, match="(?s)RAT_ERR_ARG.*does not define RAT_USER_POLICY"):
        rat.user_policy_check(c.base, 2, 1)
    with pytest.raises(rat.RatError, match="RAT_ERR_UNSUPPORTED"):
        nv.user_policy_check(big.decode(), 13, 4)


def test_a_source_with_the_hook_still_passes_source_check():
    """the solver's module (rat_src_rollout, rat_src_linearize) compiles the text and never calls the hook: even a hook whose signature
    the Monte-Carlo kernels refuse passes, as any unused function does"""
    c = up.case("lq5")
    assert nv.lib().rat_source_check(up.source(c.base, c.poff, "rate").encode(), 5, 3) == OK, last_error()
    bad = c.base + "#define POFF (ohi + 1)\n" + up.WRONG_SIGNATURE + up.BODIES["clamp"] + "}\n"
    assert nv.lib().rat_source_check(bad.encode(), 5, 3) == OK, last_error()
    assert nv.lib().rat_user_noise_check(bad.encode(), 5, 3, 5, 1) == ARG and "rat_user_policy" in last_error()


def test_abi_export_and_prototype():
    lib = C.CDLL(nv.SO_PATH)
    hdr = open(os.path.join(ROOT, "include", "ratilqr.h")).read()
    name = "rat_user_policy_check"
    assert name in nv.EXPORTS and hasattr(lib, name)
    args = re.search(r"rat_rc " + name + r"\(([^;]*)\);", hdr).group(1)
    assert [" ".join(a.split()) for a in args.split(",")] == ["const char *source", "int32_t n", "int32_t m"]
    assert list(getattr(nv.lib(), name).argtypes) == [C.c_char_p, C.c_int32, C.c_int32]
    assert callable(rat.user_policy_check) and rat.user_policy_check is nv.user_policy_check
    julia = open(os.path.join(ROOT, "julia", "RATiLQRAMD.jl")).read()
    assert f"(:{name}, LIB)" in julia and re.search(r"\nexport\b.*[\s,]user_policy_check[,\n]", julia, flags=re.S)
    # the contract is in the header, with what the hook does not touch
    assert "__device__ void rat_user_policy(int k, const double *x, const double *u_prev, double *u, const double *p);" in hdr
    assert "The hook does NOT run in the solver" in hdr
