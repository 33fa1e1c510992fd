"""ctypes binding of csrc/libratilqr_hip.so (C ABI: include/ratilqr.h).

There is deliberately NO fallback: if the HIP library is missing or no GPU is visible, every
compute entry point raises.  (The CPU oracle lives under oracle/ and is never imported here.)
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("RATILQR_SO", os.path.join(_HERE, "csrc", "libratilqr_hip.so"))   # override: diagnostic builds only

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_up = C.POINTER(C.c_uint64)

RC_NAMES = {0: "RAT_OK", 1: "RAT_ERR_ARG", 2: "RAT_ERR_UNSUPPORTED", 3: "RAT_ERR_HIP", 4: "RAT_ERR_NO_PROBLEM",
            5: "RAT_ERR_STREAM_DRY", 6: "RAT_ERR_DIVERGED"}
ST_RUNNING, ST_OK, ST_M_NOT_PD_INIT, ST_M_NOT_PD_GAIN, ST_ITER_MAX, ST_DOMAIN, ST_MU_DIVERGED, ST_SINGULAR, \
    ST_LS_DIVERGED = -1, 0, 1, 2, 3, 4, 5, 6, 7
K_NAMES = ("rollout", "linearize", "sweep_eval", "sweep_gain", "select", "sweep_init", "sweep_dual", "solve_fused", "solve_block", "solve_wide",
           "pets", "ce_bookkeeping")


class RatError(RuntimeError):
    pass


class ProblemDesc(C.Structure):
    _fields_ = [("model", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("N", C.c_int32),
                ("cost_tv", C.c_int32), ("W_tv", C.c_int32),
                ("A", _dp), ("B", _dp), ("Q", _dp), ("R", _dp), ("P", _dp), ("qv", _dp), ("rv", _dp), ("q0", _dp),
                ("Qf", _dp), ("qvf", _dp), ("q0f", C.c_double), ("kappa", C.c_double),
                ("pl_a", C.c_double), ("pl_b", C.c_double), ("pl_p", C.c_double), ("pl_pu", C.c_double),
                ("pl_cx", C.c_double), ("pl_cu", C.c_double), ("pl_h", C.c_double),
                ("W", _dp)]


class IleqgOpts(C.Structure):
    _fields_ = [("mu_min", C.c_double), ("delta_0", C.c_double), ("lam", C.c_double), ("d", C.c_double),
                ("iter_max", C.c_int64), ("eps_init", C.c_double), ("eps_min", C.c_double),
                ("adaptive_eps_init", C.c_int32)]


class CeSolver(C.Structure):
    _fields_ = [("num_samples", C.c_int64), ("num_elite", C.c_int64), ("iter_max", C.c_int64),
                ("lam", C.c_double), ("use_theta_max", C.c_int32),
                ("mu_init", C.c_double), ("sigma_init", C.c_double), ("mu", C.c_double), ("sigma", C.c_double),
                ("theta_max", C.c_double), ("theta_min", C.c_double), ("iter_current", C.c_int64),
                ("n_solves", C.c_int64), ("n_redraws", C.c_int64), ("n_final_retries", C.c_int64)]


class GenProblemDesc(C.Structure):
    _fields_ = [("lq", ProblemDesc), ("l1u", C.c_double), ("noise_kind", C.c_int32), ("nmean", _dp), ("nchol", _dp),
                ("nlo", C.c_double), ("nhi", C.c_double), ("tw2", C.c_double), ("tmean2", _dp), ("tchol2", _dp)]


class PetsSolver(C.Structure):
    _fields_ = [("num_control_samples", C.c_int64), ("num_trajectory_samples", C.c_int64), ("num_elite", C.c_int64),
                ("iter_max", C.c_int64), ("smoothing_factor", C.c_double), ("N", C.c_int64), ("m", C.c_int64),
                ("iter_current", C.c_int64), ("mu_init", _dp), ("Sigma_init", _dp), ("mu", _dp), ("Sigma", _dp)]


class NmSolver(C.Structure):
    _fields_ = [("alpha", C.c_double), ("beta", C.c_double), ("gamma", C.c_double), ("eps", C.c_double), ("lam", C.c_double),
                ("iter_max", C.c_int64), ("theta_high_init", C.c_double), ("theta_low_init", C.c_double),
                ("iter_current", C.c_int64), ("theta_high", C.c_double), ("theta_low", C.c_double),
                ("has_c_high", C.c_int32), ("has_c_low", C.c_int32), ("c_high", C.c_double), ("c_low", C.c_double),
                ("n_solves", C.c_int64), ("n_batches", C.c_int64)]


EXPORTS = [
    "rat_version", "rat_last_error", "rat_default_ileqg_opts", "rat_create", "rat_destroy", "rat_set_ileqg_opts",
    "rat_problem_set", "rat_ileqg_solve_batch", "rat_set_initial", "rat_ileqg_solve_batch_dev", "rat_ileqg_solve",
    "rat_rollout_open", "rat_rollout_feedback", "rat_rollout_noisy", "rat_integrate_cost", "rat_approximate_model", "rat_dp_gain_sweep",
    "rat_dp_policy_eval", "rat_ce_default", "rat_ce_initialize", "rat_ce_set_stream", "rat_ce_seed",
    "rat_ce_stream_pos", "rat_ce_get_positive_samples", "rat_ce_compute_cost", "rat_ce_compute_cost_dev", "rat_ce_compute_cost_enqueue", "rat_ce_begin_step", "rat_ce_draw",
    "rat_ce_update", "rat_ce_draw_stream", "rat_ce_step", "rat_ce_solve", "rat_nm_default", "rat_nm_initialize",
    "rat_nm_compute_cost", "rat_nm_step", "rat_nm_solve", "rat_pets_problem_set", "rat_pets_initialize",
    "rat_pets_compute_cost", "rat_pets_sample_controls", "rat_pets_update", "rat_pets_step", "rat_pets_solve", "rat_profile_enable", "rat_profile_reset", "rat_profile_get",
    "rat_stream", "rat_layout_info",
    "rat_dp_gain_sweep_batch", "rat_dp_policy_eval_batch",
    "rat_shard_bounds", "rat_create_multi", "rat_multi_destroy", "rat_multi_n_devices", "rat_multi_handle", "rat_multi_uses_rccl",
    "rat_multi_allgathers", "rat_multi_problem_set", "rat_multi_set_initial", "rat_multi_ce_compute_cost", "rat_multi_ce_step",
    "rat_multi_ce_solve", "rat_multi_pets_problem_set", "rat_multi_pets_compute_cost",
    "rat_multi_ce_compute_cost_ex", "rat_multi_ileqg_solve_batch", "rat_multi_is_logical", "rat_set_path", "rat_get_path", "rat_ce_compute_cost_enqueue_ex",
    "rat_debug_set", "rat_debug_get", "rat_ce_update_dev",
    "rat_problem_set_source", "rat_problem_set_params", "rat_source_check",
    "rat_pets_problem_set_source", "rat_pets_set_params", "rat_pets_source_check",
    "rat_policy_evaluate",
    "rat_policy_evaluate_noise", "rat_user_noise_check",
    "rat_policy_worst_case",
    "rat_policy_worst_case_trajectory",
    "rat_policy_worst_case_disturbance",
    "rat_policy_worst_case_params",
    "rat_policy_tail_risk",
    "rat_policy_tail_trajectory", "rat_policy_tail_disturbance", "rat_policy_tail_params",
    "rat_policy_events", "rat_kl_event_bound",
    "rat_policy_rare_event",
    "rat_policy_rare_event_noise", "rat_rare_event_noise_check",
    "rat_policy_events_user", "rat_user_event_check", "rat_policy_rare_event_user", "rat_rare_event_user_check",
    "rat_user_policy_check",
    "rat_policy_params_sampling", "rat_user_params_check", "rat_policy_params_sample",
    "rat_policy_rare_event_params", "rat_rare_event_params_check",
    "rat_policy_tail_events", "rat_policy_tail_events_user",
    "rat_policy_sobol", "rat_policy_sobol_check",
    "rat_policy_gradient", "rat_policy_tail_gradient", "rat_policy_gradient_check",
    "rat_policy_param_gradient", "rat_policy_tail_param_gradient", "rat_policy_param_gradient_check",
    "rat_policy_margin_gradient", "rat_policy_margin_gradient_check",
]
MC_N_OK, MC_N_DOMAIN, MC_MEAN, MC_VAR, MC_MIN, MC_MAX, MC_SE_MEAN, MC_NSTAT = 0, 1, 2, 3, 4, 5, 6, 8      # RAT_MC_* of the header
WC_SLOTS = ("theta", "kl", "bound", "bound_se", "tilt_mean", "tilt_var", "ess", "flag")      # RAT_WC_* slots of the header, in order
WC_NSTAT, WC_OK, WC_SATURATED, WC_EMPTY, WC_NONFINITE = 8, 0, 1, 2, 3
TR_SLOTS = ("alpha", "var", "cvar", "cvar_se", "tail_n", "ess", "kl", "flag")                # RAT_TR_* slots of the header, in order
TR_NSTAT, TR_OK, TR_SATURATED, TR_EMPTY, TR_NONFINITE = 8, 0, 1, 2, 3
EV_SLOTS = ("prob", "prob_se", "margin_mean", "margin_max", "first_mean", "n_viol", "prob_robust", "flag")   # RAT_EV_* slots of the header, in order
EV_NSTAT, EV_MAX = 8, 16
RE_SLOTS = ("prob", "prob_se", "ess", "n_viol", "n_ok", "n_domain", "logw_max", "logw_min", "flag", "n_iter", "level")   # RAT_RE_* slots of the header, in order
RE_NSTAT, RE_NTRACE, RE_OK, RE_NOT_REACHED, RE_EMPTY, RE_NONFINITE = 12, 4, 0, 1, 2, 3
SB_S, SB_S_SE, SB_T, SB_T_SE, SB_NINDEX = 0, 1, 2, 3, 4                                      # RAT_SB_* of the header: an index row ...
SB_N_OK, SB_MEAN, SB_VAR, SB_VAR_SE, SB_FLAG, SB_N_DROPPED, SB_NSTAT = 0, 1, 2, 3, 4, 5, 8  # ... the summary ...
SB_NGROUPWORD, SB_MAX_GROUPS, SB_DEGENERATE = 4, 16, 16                                      # ... a group's words, the cap, the flag bit

_lib = None


def lib():
    """Load the HIP library; raise loudly if it is not built (run `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RatError(f"{SO_PATH} is missing: build it with `make -C {os.path.dirname(SO_PATH)}` "
                           "(there is no CPU fallback)")
        _lib = C.CDLL(SO_PATH)
        _lib.rat_last_error.restype = C.c_char_p
        _lib.rat_stream.restype = C.c_void_p
        _lib.rat_ce_stream_pos.restype = C.c_int64
        _lib.rat_stream.argtypes = [C.c_void_p]
        _lib.rat_destroy.argtypes = [C.c_void_p]
        _lib.rat_destroy.restype = None
        _lib.rat_multi_destroy.argtypes = [C.c_void_p]
        _lib.rat_multi_destroy.restype = None
        _lib.rat_multi_handle.argtypes = [C.c_void_p, C.c_int32]
        _lib.rat_multi_handle.restype = C.c_void_p
        _lib.rat_multi_allgathers.argtypes = [C.c_void_p]
        _lib.rat_multi_allgathers.restype = C.c_int64
        _lib.rat_set_path.argtypes = [C.c_void_p, C.c_int32]
        _lib.rat_get_path.argtypes = [C.c_void_p, C.c_int64]
        _lib.rat_get_path.restype = C.c_int32
        _lib.rat_debug_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        _lib.rat_debug_get.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]
        _lib.rat_problem_set_source.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int32, _dp, C.c_int64]
        _lib.rat_problem_set_params.argtypes = [C.c_void_p, _dp, C.c_int64]
        _lib.rat_source_check.argtypes = [C.c_char_p, C.c_int32, C.c_int32]
        _lib.rat_pets_problem_set_source.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int64]
        _lib.rat_pets_set_params.argtypes = [C.c_void_p, _dp, C.c_int64]
        _lib.rat_pets_source_check.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        _lib.rat_policy_evaluate.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int64, _dp, C.c_uint64, _dp, C.c_int32, _dp, _dp, _dp, _dp]
        _lib.rat_policy_evaluate_noise.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int64, C.c_int32, C.c_int32, _dp, _dp, C.c_uint64, _dp,
                                                   C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp]
        _lib.rat_user_noise_check.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        _lib.rat_policy_worst_case.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp]
        _lib.rat_policy_worst_case_trajectory.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp]
        _lib.rat_policy_worst_case_disturbance.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp, _dp]
        _lib.rat_policy_worst_case_params.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp, _dp]
        _lib.rat_policy_tail_risk.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, C.c_int32, _dp, _dp]
        _lib.rat_policy_tail_trajectory.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, _dp, _dp]
        _lib.rat_policy_tail_disturbance.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, _dp, _dp, _dp]
        _lib.rat_policy_tail_params.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, _dp, _dp, _dp]
        _lib.rat_policy_events.argtypes = [C.c_void_p, C.c_int32, _dp, _dp, _dp, _ip, _ip, _dp, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp, _dp]
        _lib.rat_kl_event_bound.argtypes = [C.c_double, C.c_double, _dp]
        _lib.rat_policy_rare_event.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int64, C.c_uint64, _dp, _dp, C.c_double, C.c_int32, C.c_int32, _dp,
                                               C.c_int32, C.c_double, _dp, _dp, _dp, _dp, _dp]
        _lib.rat_policy_rare_event_noise.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int64, C.c_int32, C.c_int32, C.c_uint64, _dp, _dp, C.c_double,
                                                     C.c_int32, C.c_int32, _dp, C.c_int32, C.c_double, _dp, _dp, _dp, _dp, _dp]
        _lib.rat_rare_event_noise_check.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        _lib.rat_policy_events_user.argtypes = [C.c_void_p, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp, _dp]
        _lib.rat_user_event_check.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32]
        _lib.rat_policy_tail_events.argtypes = [C.c_void_p, C.c_int32, _dp, _dp, _dp, _ip, _ip, _dp, C.c_int32, _dp, _dp, _dp, _dp]
        _lib.rat_policy_tail_events_user.argtypes = [C.c_void_p, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp, _dp]
        _lib.rat_policy_rare_event_user.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int64, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_int32,
                                                    _dp, C.c_int32, C.c_double, _dp, _dp, _dp, _dp, _dp]
        _lib.rat_rare_event_user_check.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        _lib.rat_user_policy_check.argtypes = [C.c_char_p, C.c_int32, C.c_int32]
        _lib.rat_policy_params_sampling.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp, C.c_int64]
        _lib.rat_user_params_check.argtypes = [C.c_char_p] + [C.c_int32] * 7
        _lib.rat_policy_params_sample.argtypes = [C.c_void_p, C.c_int64, C.c_uint64, _dp]
        _lib.rat_policy_rare_event_params.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int64, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_int32,
                                                      _dp, _dp, C.c_double, C.c_int32, C.c_int32, _dp, _dp, C.c_int32, C.c_int32, C.c_double,
                                                      _dp, _dp, _dp, _dp, _dp, _dp, _dp]
        _lib.rat_rare_event_params_check.argtypes = [C.c_char_p] + [C.c_int32] * 8
        _lib.rat_policy_sobol.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int64, C.c_int32, C.c_int32, _up, C.c_int32, C.c_uint64, C.c_uint64,
                                          _dp, _dp, _dp]
        _lib.rat_policy_sobol_check.argtypes = [C.c_char_p] + [C.c_int32] * 7
        _lib.rat_policy_gradient.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp, _dp, C.POINTER(C.c_int64)]
        _lib.rat_policy_tail_gradient.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, _dp, _dp, _dp, C.POINTER(C.c_int64)]
        _lib.rat_policy_gradient_check.argtypes = [C.c_char_p] + [C.c_int32] * 4
        _lib.rat_policy_margin_gradient.argtypes = [C.c_void_p, C.c_int32, _dp, _dp, _dp, _ip, _ip, _dp, C.c_int32, _dp, _dp, _dp, _dp, C.POINTER(C.c_int64)]
        _lib.rat_policy_margin_gradient_check.argtypes = [C.c_char_p] + [C.c_int32] * 4
        _lib.rat_policy_param_gradient.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_int64)]
        _lib.rat_policy_tail_param_gradient.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_int64)]
        _lib.rat_policy_param_gradient_check.argtypes = [C.c_char_p] + [C.c_int32] * 5
    return _lib


def check(rc):
    if rc != 0:
        raise RatError(f"{RC_NAMES.get(rc, rc)}: {lib().rat_last_error().decode()}")


def P(a):
    return None if a is None else a.ctypes.data_as(_dp)


def PI(a):
    return None if a is None else a.ctypes.data_as(_ip)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def cm3(a):
    """(T, rows, cols) -> flat buffer, time slowest, column-major inside (Vector{Matrix} of Julia)."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).transpose(0, 2, 1)).ravel()


def from_cm3(buf, T, rows, cols):
    return np.asarray(buf, dtype=np.float64).reshape(T, cols, rows).transpose(0, 2, 1).copy()


def set_source(h, prob):
    """rat_problem_set_source for a DeviceSourceProblem; returns the arrays the call read (kept alive by the caller)."""
    W, p = f64(_wbuf(prob)), f64(prob.params)
    check(lib().rat_problem_set_source(h, prob.source.encode(), int(prob.n), int(prob.m), int(prob.N), P(W), int(bool(prob.W_tv)),
                                       P(p) if p.size else None, C.c_int64(p.size)))
    return {"W": W, "params": p}


def _wbuf(prob):
    from .problems import _colmajor
    return _colmajor(prob.Wtab)


def source_check(source, n, m):
    """rat_source_check: compile only (gfx950, no device needed); raises RatError with the compiler's log."""
    check(lib().rat_source_check(str(source).encode(), int(n), int(m)))


def user_noise_check(source, n, m, normals_per_step=0, uniforms_per_step=0):
    """rat_user_noise_check: compile a source's rollout kernel under its own rat_user_noise only (gfx950, no device needed); raises
    RatError with the compiler's log, or saying that the source does not define RAT_USER_NOISE."""
    check(lib().rat_user_noise_check(str(source).encode(), int(n), int(m), int(normals_per_step), int(uniforms_per_step)))


def rare_event_noise_check(source, n, m, normals_per_step=1, uniforms_per_step=0):
    """rat_rare_event_noise_check: compile the rollout kernel of rat_policy_rare_event_noise only (gfx950, no device needed); raises
    RatError with the compiler's log, saying that the source does not define RAT_USER_NOISE, or naming the limit on normals_per_step."""
    check(lib().rat_rare_event_noise_check(str(source).encode(), int(n), int(m), int(normals_per_step), int(uniforms_per_step)))


def user_event_check(source, n, m, n_event=1):
    """rat_user_event_check: compile the kernel of rat_policy_events_user only (gfx950, no device needed); raises RatError with the
    compiler's log, or saying that the source does not define RAT_USER_EVENT."""
    check(lib().rat_user_event_check(str(source).encode(), int(n), int(m), int(n_event)))


def user_policy_check(source, n, m):
    """rat_user_policy_check: compile the Monte-Carlo rollout kernel with the source's rat_user_policy only (gfx950, no device needed);
    raises RatError with the compiler's log, or saying that the source does not define RAT_USER_POLICY."""
    check(lib().rat_user_policy_check(str(source).encode(), int(n), int(m)))


def user_params_check(source, n, m, n_params, normals_per_step=0, uniforms_per_step=0, param_normals=0, param_uniforms=0):
    """rat_user_params_check: compile the rollout kernel of rat_policy_evaluate_noise with parameter sampling on (gfx950, no device
    needed); raises RatError with the compiler's log, saying that the source does not define RAT_USER_PARAMS, or naming the limit on
    n_params (1 .. 32) or the counts."""
    check(lib().rat_user_params_check(str(source).encode(), int(n), int(m), int(n_params), int(normals_per_step), int(uniforms_per_step),
                                      int(param_normals), int(param_uniforms)))


def rare_event_user_check(source, n, m, normals_per_step=1, uniforms_per_step=0, n_event=1):
    """rat_rare_event_user_check: compile the rollout kernel of rat_policy_rare_event_user only (gfx950, no device needed); raises RatError
    with the compiler's log, saying what the source does not define, or naming the limit on normals_per_step or n_event."""
    check(lib().rat_rare_event_user_check(str(source).encode(), int(n), int(m), int(normals_per_step), int(uniforms_per_step), int(n_event)))


def rare_event_params_check(source, n, m, n_params, normals_per_step=1, uniforms_per_step=0, param_normals=1, param_uniforms=0, n_event=0):
    """rat_rare_event_params_check: compile the rollout kernel of rat_policy_rare_event_params only (gfx950, no device needed) -- the
    quadratic event's variant with n_event=0, rat_user_event's with n_event in 1 .. 16; raises RatError with the compiler's log, saying
    what the source does not define, or naming the limit on the counts (param_normals in 1 .. 12)."""
    check(lib().rat_rare_event_params_check(str(source).encode(), int(n), int(m), int(n_params), int(normals_per_step), int(uniforms_per_step),
                                            int(param_normals), int(param_uniforms), int(n_event)))


def policy_sobol_check(source, n, m, n_params=0, normals_per_step=0, uniforms_per_step=0, param_normals=0, param_uniforms=0):
    """rat_policy_sobol_check: compile the rollout kernel of rat_policy_sobol only (gfx950, no device needed), with parameter sampling
    off (n_params=0) or on; raises RatError with the compiler's log, saying what the source does not define, or naming the limit on
    the counts (at most 64 each)."""
    check(lib().rat_policy_sobol_check(str(source).encode(), int(n), int(m), int(n_params), int(normals_per_step), int(uniforms_per_step),
                                       int(param_normals), int(param_uniforms)))


def policy_margin_gradient_check(source, n, m, normals_per_step=0, uniforms_per_step=0):
    """rat_policy_margin_gradient_check: compile the adjoint kernel of rat_policy_margin_gradient only (gfx950, four events, no device
    needed); raises RatError with the compiler's log, RAT_ERR_UNSUPPORTED for a source that defines RAT_USER_POLICY."""
    check(lib().rat_policy_margin_gradient_check(str(source).encode(), int(n), int(m), int(normals_per_step), int(uniforms_per_step)))


def policy_gradient_check(source, n, m, normals_per_step=0, uniforms_per_step=0):
    """rat_policy_gradient_check: compile the adjoint kernel of rat_policy_gradient / rat_policy_tail_gradient only (gfx950, no device
    needed); raises RatError with the compiler's log, or saying that the source defines RAT_USER_POLICY (RAT_ERR_UNSUPPORTED)."""
    check(lib().rat_policy_gradient_check(str(source).encode(), int(n), int(m), int(normals_per_step), int(uniforms_per_step)))


def policy_param_gradient_check(source, n, m, normals_per_step=0, uniforms_per_step=0, n_params=0):
    """rat_policy_param_gradient_check: compile the adjoint kernel of rat_policy_param_gradient / rat_policy_tail_param_gradient only
    (gfx950, no device needed) for n_params parameters; raises RatError with the compiler's log, or saying that the source lacks
    RAT_USER_PARAMS_AD, defines RAT_USER_POLICY or has more than 32 parameters (RAT_ERR_UNSUPPORTED)."""
    check(lib().rat_policy_param_gradient_check(str(source).encode(), int(n), int(m), int(normals_per_step), int(uniforms_per_step), int(n_params)))


def pets_set_source(h, prob):
    """rat_pets_problem_set_source for a DeviceGenerativeSourceProblem; returns the parameter array the call read."""
    p = f64(prob.params)
    check(lib().rat_pets_problem_set_source(h, prob.source.encode(), int(prob.n), int(prob.m), int(prob.N), int(prob.normals_per_step),
                                            int(prob.uniforms_per_step), P(p) if p.size else None, C.c_int64(p.size)))
    return p


def pets_source_check(source, n, m, normals_per_step=None, uniforms_per_step=0):
    """rat_pets_source_check: compile a generative source only (gfx950, no device needed); raises RatError with the compiler's log.
    normals_per_step defaults to n."""
    npn = int(n) if normals_per_step is None else int(normals_per_step)
    check(lib().rat_pets_source_check(str(source).encode(), int(n), int(m), npn, int(uniforms_per_step)))


def make_desc(prob):
    t = prob.c_tables()
    keep = {k: f64(v) for k, v in t.items() if isinstance(v, np.ndarray)}
    d = ProblemDesc()
    for k in ("model", "n", "m", "N", "cost_tv", "W_tv"):
        setattr(d, k, int(t[k]))
    for k in ("q0f", "kappa", "pl_a", "pl_b", "pl_p", "pl_pu", "pl_cx", "pl_cu", "pl_h"):
        setattr(d, k, float(t[k]))
    for k, v in keep.items():
        setattr(d, k, P(v))
    return d, keep
