"""rat_policy_rare_event_noise on the host: tests/rare_event_noise_model.py, the NumPy model of the whole call, against the closed form of
tests/test_cpu_rare_event.py, and the compile-only check of the kernel -- no GPU.

The closed form's problem is linear_case() of tests/test_cpu_rare_event.py written as a source model whose sampler is chol(W) z (two
normals a step): (x_t, u_t) stays Gaussian, so the half-space of linear_event(p) has P(violated) = p exactly.

The seed.  SEED was fixed here, on the model alone, before the device ran: the first one tried (tests/test_cpu_rare_event.py's).  At it
the model meets both conditions of test_closed_form at all three probabilities: 0.68, 0.70 and 1.22 standard errors off at 1e-3, 1e-6 and
1e-9, the relative error 17, 429 and 7684 times below plain Monte Carlo's."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import rare_event_model as rm
import rare_event_noise_model as nm
from ratilqr.jl_amd import _native as nv
from test_cpu_rare_event import K_CLOSED, N_ITER_CLOSED, QUANTILES, RHO, linear_case, linear_event
from user_noise_model import LQ_GAUSS, PEND_PLAIN, PEND_STATE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261019
OK, ARG, UNSUPPORTED = 0, 1, 2


def linear_model():
    prob, x, l, L = linear_case()
    return nm.Model(nm.lin_f, nm.lin_noise, nm.lin_params(prob), 2, 1, prob.N, 2), x, l, L


@pytest.fixture(scope="module")
def closed():
    mod, x, l, L = linear_model()
    out = {}
    for p in QUANTILES:
        ev, exact = linear_event(p)
        out[p] = (nm.rare_event_noise(mod, x, l, L, ev, K_CLOSED, seed=SEED, n_iter=N_ITER_CLOSED, rho=RHO), exact)
    return out


@pytest.mark.parametrize("p", sorted(QUANTILES))
def test_closed_form(closed, p):
    r, exact = closed[p]
    plain = math.sqrt((1.0 - exact) / (exact * K_CLOSED))            # plain Monte Carlo's relative error at the same K: derivable
    print(f"p = {exact:.6e}: PROB {r['prob']:.6e} SE {r['prob_se']:.3e} ({abs(r['prob'] - exact) / r['prob_se']:.2f} sigma), "
          f"SE/PROB {r['prob_se'] / r['prob']:.3e} against plain {plain:.3e}, {r['n_iter']} iterations, ESS {r['ess']:.0f}")
    assert r["flag"] == rm.OK
    assert r["shift"].shape == (4, 2)
    assert abs(r["prob"] - exact) <= 5.0 * r["prob_se"]
    assert r["prob_se"] / r["prob"] < plain


def test_the_estimate_is_unbiased_under_an_arbitrary_shift():
    """n_iter = 0 under a fixed random shift that no adaptation produced: the likelihood ratio alone makes the estimate right"""
    mod, x, l, L = linear_model()
    ev, exact = linear_event(1e-3)
    shift = 0.25 * np.random.default_rng(3).standard_normal((mod.N, mod.P))
    r = nm.rare_event_noise(mod, x, l, L, ev, K_CLOSED, seed=SEED, shift=shift, n_iter=0)
    print(f"p = {exact:.6e}: PROB {r['prob']:.6e} SE {r['prob_se']:.3e} ({abs(r['prob'] - exact) / r['prob_se']:.2f} sigma), N_VIOL {r['n_viol']}")
    assert r["flag"] == rm.NOT_REACHED and r["n_iter"] == 0 and np.array_equal(r["shift"], shift)
    assert np.any(r["logw"] != 0.0) and r["n_viol"] > 0
    assert abs(r["prob"] - exact) <= 5.0 * r["prob_se"]


def test_without_a_shift_the_normals_are_rat_rngs_at_the_seed():
    """pass 0 without a shift: the generator of rat_policy_evaluate_noise at the same seed (tests/source_pets_models documents its keying:
    counter (g lo, g hi, t, i >> 1)), an odd count uses the first output of the last block only, and the noise of a rollout does not depend on K"""
    a, b = nm.normals(5, 0, 7, 3, 3), nm.normals(5, 0, 100, 3, 3)
    assert np.array_equal(a, b[:7])
    assert np.array_equal(nm.normals(5, 0, 7, 3, 4)[:, :, :3], a)
    assert not np.array_equal(nm.normals(5, 1, 7, 3, 3), a)


def test_the_kernel_compiles_without_a_device_and_refuses_what_it_cannot_shift():
    chk = nv.lib().rat_rare_event_noise_check
    assert chk(PEND_STATE.encode(), 2, 1, 3, 0) == OK, nv.lib().rat_last_error().decode()
    assert chk(LQ_GAUSS.encode(), 12, 4, 12, 0) == OK, nv.lib().rat_last_error().decode()
    assert chk(PEND_PLAIN.encode(), 2, 1, 2, 0) == ARG and "RAT_USER_NOISE" in nv.lib().rat_last_error().decode()
    assert chk(PEND_STATE.encode(), 2, 1, 13, 0) == UNSUPPORTED
    assert chk(PEND_STATE.encode(), 2, 1, 0, 0) == ARG
    assert chk(PEND_STATE.encode(), 2, 1, 3, -1) == ARG
    assert chk(LQ_GAUSS.encode(), 13, 4, 12, 0) == UNSUPPORTED
    nv.rare_event_noise_check(PEND_STATE, 2, 1, 3)                    # the Python wrapper: raises on a refusal
    with pytest.raises(nv.RatError):
        nv.rare_event_noise_check(PEND_PLAIN, 2, 1, 2)


def test_abi_export_and_prototype():
    lib = C.CDLL(nv.SO_PATH)
    hdr = open(os.path.join(ROOT, "include", "ratilqr.h")).read()
    ctype = {"rat_handle": C.c_void_p, "const double *": nv._dp, "double *": nv._dp, "int64_t": C.c_int64, "int32_t": C.c_int32,
             "uint64_t": C.c_uint64, "double": C.c_double, "const char *": C.c_char_p}
    for name in ("rat_policy_rare_event_noise", "rat_rare_event_noise_check"):
        assert name in nv.EXPORTS and hasattr(lib, name)
        args = re.search(r"rat_rc " + name + r"\(([^;]*)\);", hdr).group(1)
        want = [ctype[re.sub(r"\s*\w+$", "", " ".join(a.split())).replace(" *", " *").strip()] for a in args.split(",")]
        assert list(getattr(nv.lib(), name).argtypes) == want, name
