"""ctypes binding of libflowfusion_amd.so and the PyTorch custom op that fronts it.

The shared library (C ABI: include/flowfusion_amd.h) is the product; this module only moves
pointers: tensors are torch-allocated device memory, the launch goes onto torch's current HIP
stream.  There is deliberately no fallback: a missing library or a tensor that is not on the
GPU is an error.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import List, Optional, Tuple

import torch

FF_OK = 0
FF_ERR_BADARG = -1
FF_ERR_UNSUPPORTED = -2
FF_ERR_HIP = -3
FF_ERR_EXCHANGE = -4

MODE_STATE = 0
MODE_HUTCH = 1
MODE_EXACT = 2

# FF_PREC_* of include/flowfusion_amd.h
PREC_F32, PREC_BF16X3, PREC_BF16X2 = 0, 1, 2
PRECISIONS = {"f32": PREC_F32, "bf16x3": PREC_BF16X3, "bf16x2": PREC_BF16X2}

# FF_ACT_* of include/flowfusion_amd.h
ACT_SILU, ACT_TANH, ACT_SIGMOID, ACT_RELU, ACT_LEAKY_RELU, ACT_ELU, ACT_SOFTPLUS, ACT_GELU, ACT_GELU_TANH = range(9)

_LIB_PATH = Path(__file__).resolve().parent / "lib" / "libflowfusion_amd.so"


class PlanStruct(ctypes.Structure):
    _fields_ = [
        ("dim", ctypes.c_int32),
        ("cond_dim", ctypes.c_int32),
        ("n_hidden", ctypes.c_int32),
        ("width", ctypes.c_int32),
        ("dregs", ctypes.c_int32),
        ("cregs", ctypes.c_int32),
        ("kernel_id", ctypes.c_int32),
        ("tile", ctypes.c_int32),
        ("activation", ctypes.c_int32),
        ("act_param", ctypes.c_float * 2),
        ("precision", ctypes.c_int32),
    ]


class OdeArgs(ctypes.Structure):
    _fields_ = [
        ("x_in", ctypes.c_void_p),
        ("x_out", ctypes.c_void_p),
        ("cond", ctypes.c_void_p),
        ("probe", ctypes.c_void_p),
        ("dlogp_out", ctypes.c_void_p),
        ("noise", ctypes.c_void_p),
        ("wpack", ctypes.c_void_p),
        ("etab", ctypes.c_void_p),
        ("in_shift", ctypes.c_void_p),
        ("in_scale", ctypes.c_void_p),
        ("out_scale", ctypes.c_void_p),
        ("out_shift", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
        ("batch", ctypes.c_int64),
        ("noise_stride", ctypes.c_int64),
        ("n_evals", ctypes.c_int32),
        ("mode", ctypes.c_int32),
        ("tangent_first", ctypes.c_int32),
        ("tangent_count", ctypes.c_int32),
        ("k1_in", ctypes.c_void_p),
        ("kl1_in", ctypes.c_void_p),
        ("dlogp_in", ctypes.c_void_p),
        ("aux_out", ctypes.c_void_p * 4),
        ("aux_lp_out", ctypes.c_void_p * 4),
        ("n_aux", ctypes.c_int32),
        ("rng_noise_base", ctypes.c_int32),
        ("rng_seed", ctypes.c_uint64),
        ("rng_sample_offset", ctypes.c_int64),
        ("jac_out", ctypes.c_void_p),
        ("jac_all", ctypes.c_int32),
        ("stage_slots", ctypes.c_int32),
        ("gate", ctypes.c_void_p),
    ]


STATUS_NAN, STATUS_BAD_SLOT = 1, 2          # FF_STATUS_*
SCHED_FLOW, SCHED_VE, SCHED_VP, SCHED_SUBVP, SCHED_FOURIER = 0, 1, 2, 3, 4     # FF_SCHED_*
PAIR_KERNEL_BASE = 0x10000                                  # FF_PAIR_KERNEL_BASE
PAIR_SELECT_KERNEL_BASE = 0x20000                           # FF_PAIR_SELECT_KERNEL_BASE
PUSH_KERNEL_BASE = 0x40000                                  # FF_PUSH_KERNEL_BASE
STATUS_NOISE_ROW = 4                                        # FF_STATUS_NOISE_ROW
MAX_PUSH_TANGENTS = 15                                      # tangent columns beside the value column of a 16-column tile
PULL_KERNEL_BASE = 0x50000                                  # FF_PULL_KERNEL_BASE
PULL_SELECT_KERNEL_BASE = 0xA0000                           # FF_PULL_SELECT_KERNEL_BASE
PUSH_SELECT_KERNEL_BASE = 0xB0000                           # FF_PUSH_SELECT_KERNEL_BASE
MAX_PULL_COTANGENTS = 15                                    # cotangent columns beside the value column of a 16-column tile
VJP_KERNEL_BASE = 0x60000                                   # FF_VJP_KERNEL_BASE
MAX_VJP_SEEDS = 15                                          # seed columns beside the value column of a 16-column tile
REC_KERNEL_BASE = 0x70000                                   # FF_REC_KERNEL_BASE
DADJ_KERNEL_BASE = 0x80000                                  # FF_DADJ_KERNEL_BASE
LGRAD_KERNEL_BASE = 0x90000                                 # FF_LGRAD_KERNEL_BASE
ADAPT_START, ADAPT_FINISH = 1, 2            # FF_ADAPT_START / FF_ADAPT_FINISH
ADAPT_ERR_UNDERFLOW, ADAPT_ERR_NONFINITE, ADAPT_ERR_MAXSTEPS = 1, 2, 3
ADAPT_MAX_PASSES = 8
MAX_SLOTS, MAX_AUX = 7, 4


class AdaptState(ctypes.Structure):       # ff_adapt_state (128 bytes of device memory)
    _fields_ = [
        ("t", ctypes.c_double), ("dt", ctypes.c_double), ("t_prev", ctypes.c_double), ("dt_prev", ctypes.c_double),
        ("t_end", ctypes.c_double), ("h0", ctypes.c_double), ("d0", ctypes.c_double), ("d1", ctypes.c_double),
        ("active", ctypes.c_int32), ("commit", ctypes.c_int32), ("done", ctypes.c_int32), ("error", ctypes.c_int32),
        ("n_attempts", ctypes.c_int32), ("n_accepted", ctypes.c_int32), ("n_steps", ctypes.c_int32),
        ("reserved0", ctypes.c_int32), ("last_ratio", ctypes.c_float), ("reserved1", ctypes.c_float * 7),
    ]


class AdaptConfig(ctypes.Structure):      # ff_adapt_config
    _fields_ = [
        ("n_stages", ctypes.c_int32), ("order", ctypes.c_int32),
        ("alpha", ctypes.c_float * (MAX_SLOTS - 1)), ("beta", (ctypes.c_float * 8) * (MAX_SLOTS - 1)),
        ("c_sol", ctypes.c_float * 8), ("c_mid", ctypes.c_float * 8), ("c_err", ctypes.c_float * 8),
        ("rtol", ctypes.c_float), ("atol", ctypes.c_float),
        ("min_step", ctypes.c_double), ("max_step", ctypes.c_double), ("first_step", ctypes.c_double),
        ("max_num_steps", ctypes.c_int32), ("sched", ctypes.c_int32), ("no_sigma", ctypes.c_int32), ("sign", ctypes.c_float),
        ("p", ctypes.c_double * 4),
        ("emb_w", ctypes.c_void_p), ("n_emb", ctypes.c_int32), ("pi", ctypes.c_float),
        ("w0t", ctypes.c_void_p), ("b0", ctypes.c_void_p), ("h_real", ctypes.c_int32), ("n_tcols", ctypes.c_int32),
    ]


class AdaptBuffers(ctypes.Structure):     # ff_adapt_buffers
    _fields_ = [
        ("y", ctypes.c_void_p), ("f0", ctypes.c_void_p), ("lp", ctypes.c_void_p), ("fl0", ctypes.c_void_p),
        ("aux", ctypes.c_void_p * MAX_AUX), ("aux_lp", ctypes.c_void_p * MAX_AUX), ("aux_lp_pass", ctypes.c_void_p),
        ("scratch_x", ctypes.c_void_p), ("scratch_lp", ctypes.c_void_p), ("etab", ctypes.c_void_p),
        ("out_y", ctypes.c_void_p), ("out_lp", ctypes.c_void_p), ("state", ctypes.c_void_p),
        ("norm_workspace", ctypes.c_void_p), ("norm_only", ctypes.c_void_p * 2), ("norm_only_n", ctypes.c_int64 * 2),
        ("n_passes", ctypes.c_int32), ("pass_first", ctypes.c_int32 * ADAPT_MAX_PASSES),
        ("pass_count", ctypes.c_int32 * ADAPT_MAX_PASSES),
        ("exchange_sums", ctypes.c_void_p), ("exchange", ctypes.c_void_p), ("exchange_user", ctypes.c_void_p),
        ("est_kind", ctypes.c_int32), ("est_r", ctypes.c_int32), ("est_m", ctypes.c_int32), ("est_reserved", ctypes.c_int32),
        ("est_probes0", ctypes.c_void_p), ("est_probes1", ctypes.c_void_p), ("est_jac", ctypes.c_void_p),
        ("est_div", ctypes.c_void_p), ("est_workspace", ctypes.c_void_p),
    ]


TRACE_HUTCHPP, TRACE_XTRACE = 1, 2        # FF_TRACE_*


class TraceArgs(ctypes.Structure):        # ff_trace_args
    _fields_ = [
        ("kind", ctypes.c_int32), ("dim", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("r", ctypes.c_int32),
        ("m", ctypes.c_int32), ("reserved", ctypes.c_int32), ("batch", ctypes.c_int64),
        ("jac", ctypes.c_void_p), ("probes0", ctypes.c_void_p), ("probes1", ctypes.c_void_p), ("out", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p), ("gate", ctypes.c_void_p),
    ]


class TraceProdArgs(ctypes.Structure):    # ff_trace_prod_args
    _fields_ = [
        ("kind", ctypes.c_int32), ("dim", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("r", ctypes.c_int32),
        ("m", ctypes.c_int32), ("reserved", ctypes.c_int32), ("batch", ctypes.c_int64),
        ("probes0", ctypes.c_void_p), ("probes1", ctypes.c_void_p), ("y", ctypes.c_void_p), ("basis", ctypes.c_void_p),
        ("rfac", ctypes.c_void_p), ("prod", ctypes.c_void_p), ("out", ctypes.c_void_p), ("workspace", ctypes.c_void_p),
        ("gate", ctypes.c_void_p),
    ]


EXCHANGE_DOUBLES = 8                      # FF_EXCHANGE_DOUBLES
EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)      # int (*exchange)(void* user, void* stream)


class CombineArgs(ctypes.Structure):      # ff_combine_args
    _fields_ = [
        ("x", ctypes.c_void_p),
        ("k", ctypes.c_void_p * 7),
        ("coef", ctypes.c_float * 7),
        ("x_coef", ctypes.c_float),
        ("out", ctypes.c_void_p),
        ("n", ctypes.c_int64),
    ]


class NormTerm(ctypes.Structure):         # ff_norm_term
    _fields_ = [
        ("num", ctypes.c_void_p),
        ("sub", ctypes.c_void_p),
        ("scale0", ctypes.c_void_p),
        ("scale1", ctypes.c_void_p),
        ("n", ctypes.c_int64),
    ]


NORM_TERMS = 3                      # FF_NORM_TERMS
PRIOR_NOISE_INDEX = 0xFFFFFFFF     # FF_PRIOR_NOISE_INDEX
PROBE_NOISE_INDEX = 0xFFFFFFFE     # FF_PROBE_NOISE_INDEX
TRACE_PROBE_NOISE_BASE = 0xFFFE0000  # FF_TRACE_PROBE_NOISE_BASE (second probe set: + 0x8000)
MOMENTUM_NOISE_BASE = 0xFFFD0000   # FF_MOMENTUM_NOISE_BASE (+ k: momentum k of a data point, ff_marginal_expand / _reduce)
MAX_MOMENTA = 4096                 # 1 <= K <= 4096
HUTCH_PROBE_NOISE_BASE = 0xFFFC0000  # FF_HUTCH_PROBE_NOISE_BASE (+ k: probe k >= 1 of a K-probe Hutchinson launch, ff_probe_fill)
MAX_HUTCH_PROBES = 65535           # FF_MAX_HUTCH_PROBES
OBS_NOISE_BASE = 0xFFFB0000        # FF_OBS_NOISE_BASE (+ k: noise draw k of an observation, ff_observe_expand)
MAX_OBS_DRAWS = 4096               # FF_MAX_OBS_DRAWS
OBS_RESAMPLE_NOISE_INDEX = 0xFFFA0000  # FF_OBS_RESAMPLE_NOISE_INDEX (the uniforms of ff_weighted_resample: block m >> 2, word m & 3)
MAX_OBS_SAMPLES = 4096             # FF_MAX_OBS_SAMPLES

_lib = None


def library_path() -> Path:
    return Path(os.environ.get("FLOWFUSION_AMD_LIB", _LIB_PATH))


def lib() -> ctypes.CDLL:
    """Load libflowfusion_amd.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not path.exists():
        raise RuntimeError(
            f"{path} not found: the HIP library is not built. Run `python -m flowfusion_amd.build` "
            "(needs hipcc; cross-compiles gfx950 without a GPU). There is no CPU fallback.")
    _lib = _bind(ctypes.CDLL(str(path)))
    return _lib


def load_library(path) -> ctypes.CDLL:
    """A library with this ABI other than the product -- the test-only builds of flowfusion_amd/build.py VARIANTS
    (tests/test_gpu_skew.py) -- bound like the product library, NOT installed as the one the package launches through."""
    path = Path(path)
    if not path.exists():
        raise RuntimeError(f"{path} not found: run `python -m flowfusion_amd.build`")
    return _bind(ctypes.CDLL(str(path)))


def _bind(L: ctypes.CDLL) -> ctypes.CDLL:
    L.ff_version.restype = ctypes.c_char_p
    L.ff_kernel_count.restype = ctypes.c_int
    L.ff_kernel_name.restype = ctypes.c_char_p
    L.ff_kernel_name.argtypes = [ctypes.c_int]
    L.ff_mlp_plan.restype = ctypes.c_int
    L.ff_mlp_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                              ctypes.c_int, ctypes.POINTER(PlanStruct)]
    L.ff_mlp_plan_act.restype = ctypes.c_int
    L.ff_mlp_plan_act.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                  ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                                  ctypes.POINTER(PlanStruct)]
    L.ff_mlp_plan_prec.restype = ctypes.c_int
    L.ff_mlp_plan_prec.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                   ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_int,
                                   ctypes.POINTER(PlanStruct)]
    L.ff_plan_kernel_name.restype = ctypes.c_char_p
    L.ff_plan_kernel_name.argtypes = [ctypes.POINTER(PlanStruct)]
    L.ff_mlp_wpack_floats.restype = ctypes.c_size_t
    L.ff_mlp_wpack_floats.argtypes = [ctypes.POINTER(PlanStruct)]
    L.ff_mlp_wpack.restype = ctypes.c_int
    L.ff_mlp_wpack.argtypes = [ctypes.POINTER(PlanStruct), ctypes.POINTER(ctypes.c_void_p),
                               ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int),
                               ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.ff_mlp_ode_launch.restype = ctypes.c_int
    L.ff_mlp_ode_launch.argtypes = [ctypes.POINTER(PlanStruct), ctypes.POINTER(OdeArgs), ctypes.c_void_p]
    L.ff_mlp_ode_launch_probes.restype = ctypes.c_int
    L.ff_mlp_ode_launch_probes.argtypes = [ctypes.POINTER(PlanStruct), ctypes.POINTER(OdeArgs), ctypes.c_void_p, ctypes.c_void_p]
    L.ff_push_kernel_count.restype = ctypes.c_int
    L.ff_push_kernel_name.restype = ctypes.c_char_p
    L.ff_push_kernel_name.argtypes = [ctypes.c_int]
    L.ff_mlp_push_plan.restype = ctypes.c_int
    L.ff_mlp_push_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                   ctypes.c_int, ctypes.POINTER(PlanStruct)]
    L.ff_mlp_ode_launch_push.restype = ctypes.c_int
    L.ff_mlp_ode_launch_push.argtypes = [ctypes.POINTER(PlanStruct), ctypes.POINTER(OdeArgs), ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]
    L.ff_pull_kernel_count.restype = ctypes.c_int
    L.ff_pull_kernel_name.restype = ctypes.c_char_p
    L.ff_pull_kernel_name.argtypes = [ctypes.c_int]
    L.ff_mlp_pull_plan.restype = ctypes.c_int
    L.ff_mlp_pull_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                   ctypes.c_int, ctypes.POINTER(PlanStruct)]
    L.ff_mlp_pull_wpack_floats.restype = ctypes.c_size_t
    L.ff_mlp_pull_wpack_floats.argtypes = [ctypes.POINTER(PlanStruct)]
    L.ff_mlp_pull_wpack.restype = ctypes.c_int
    L.ff_mlp_pull_wpack.argtypes = L.ff_mlp_wpack.argtypes
    L.ff_mlp_ode_launch_pull.restype = ctypes.c_int
    L.ff_mlp_ode_launch_pull.argtypes = [ctypes.POINTER(PlanStruct), ctypes.POINTER(OdeArgs), ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p]
    L.ff_pullsel_kernel_count.restype = ctypes.c_int
    L.ff_pullsel_kernel_name.restype = ctypes.c_char_p
    L.ff_pullsel_kernel_name.argtypes = [ctypes.c_int]
    L.ff_mlp_pull_select_plan.restype = ctypes.c_int
    L.ff_mlp_pull_select_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(PlanStruct)]
    L.ff_mlp_pull_select_wpack_floats.restype = ctypes.c_size_t
    L.ff_mlp_pull_select_wpack_floats.argtypes = [ctypes.POINTER(PlanStruct)]
    L.ff_mlp_pull_select_wpack.restype = ctypes.c_int
    L.ff_mlp_pull_select_wpack.argtypes = [ctypes.POINTER(PlanStruct)] + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    L.ff_mlp_ode_launch_pull_select.restype = ctypes.c_int
    L.ff_mlp_ode_launch_pull_select.argtypes = L.ff_mlp_ode_launch_pull.argtypes
    L.ff_pushsel_kernel_count.restype = ctypes.c_int
    L.ff_pushsel_kernel_name.restype = ctypes.c_char_p
    L.ff_pushsel_kernel_name.argtypes = [ctypes.c_int]
    L.ff_mlp_push_select_plan.restype = ctypes.c_int
    L.ff_mlp_push_select_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(PlanStruct)]
    L.ff_mlp_push_select_wpack_floats.restype = ctypes.c_size_t
    L.ff_mlp_push_select_wpack_floats.argtypes = [ctypes.POINTER(PlanStruct)]
    L.ff_mlp_push_select_wpack.restype = ctypes.c_int
    L.ff_mlp_push_select_wpack.argtypes = [ctypes.POINTER(PlanStruct)] + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    L.ff_mlp_ode_launch_push_select.restype = ctypes.c_int
    L.ff_mlp_ode_launch_push_select.argtypes = L.ff_mlp_ode_launch_push.argtypes
    L.ff_vjp_kernel_count.restype = ctypes.c_int
    L.ff_vjp_kernel_name.restype = ctypes.c_char_p
    L.ff_vjp_kernel_name.argtypes = [ctypes.c_int]
    L.ff_mlp_ode_launch_vjp.restype = ctypes.c_int
    L.ff_mlp_ode_launch_vjp.argtypes = [ctypes.POINTER(PlanStruct), ctypes.POINTER(OdeArgs), ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_void_p, ctypes.c_void_p]
    for fam in ("rec", "dadj"):
        getattr(L, f"ff_{fam}_kernel_count").restype = ctypes.c_int
        getattr(L, f"ff_{fam}_kernel_name").restype = ctypes.c_char_p
        getattr(L, f"ff_{fam}_kernel_name").argtypes = [ctypes.c_int]
    L.ff_mlp_record_floats.restype = ctypes.c_size_t
    L.ff_mlp_record_floats.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    L.ff_mlp_ode_launch_record.restype = ctypes.c_int
    L.ff_mlp_ode_launch_record.argtypes = [ctypes.POINTER(PlanStruct), ctypes.POINTER(OdeArgs), ctypes.c_void_p, ctypes.c_void_p]
    L.ff_mlp_ode_launch_pull_discrete.restype = ctypes.c_int
    L.ff_mlp_ode_launch_pull_discrete.argtypes = [ctypes.POINTER(PlanStruct), ctypes.POINTER(OdeArgs), ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.ff_lgrad_kernel_count.restype = ctypes.c_int
    L.ff_lgrad_kernel_name.restype = ctypes.c_char_p
    L.ff_lgrad_kernel_name.argtypes = [ctypes.c_int]
    L.ff_mlp_ode_launch_logp_grad.restype = ctypes.c_int
    L.ff_mlp_ode_launch_logp_grad.argtypes = [ctypes.POINTER(PlanStruct), ctypes.POINTER(OdeArgs)] + [ctypes.c_void_p] * 7
    L.ff_mlp_samples_per_workgroup.restype = ctypes.c_int
    L.ff_mlp_samples_per_workgroup.argtypes = [ctypes.POINTER(PlanStruct), ctypes.c_int]
    L.ff_last_hip_error.restype = ctypes.c_int
    L.ff_mlp_launch_kind.restype = ctypes.c_int
    L.ff_mlp_launch_kind.argtypes = [ctypes.POINTER(PlanStruct), ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    L.ff_normal_fill.restype = ctypes.c_int
    L.ff_normal_fill.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64,
                                 ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p]
    probe_fill = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_float]
    L.ff_probe_fill.restype = L.ff_probe_fill_host.restype = ctypes.c_int
    L.ff_probe_fill.argtypes, L.ff_probe_fill_host.argtypes = probe_fill + [ctypes.c_void_p], probe_fill
    L.ff_scaled_rms_workspace_bytes.restype = ctypes.c_size_t
    L.ff_scaled_rms.restype = ctypes.c_int
    L.ff_scaled_rms.argtypes = [ctypes.POINTER(NormTerm), ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_void_p,
                                ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.ff_stage_combine.restype = ctypes.c_int
    L.ff_stage_combine.argtypes = [ctypes.POINTER(CombineArgs), ctypes.c_void_p]
    expand = [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64,
                                      ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    reduce = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64,
              ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    L.ff_marginal_expand.restype = L.ff_marginal_expand_host.restype = ctypes.c_int
    L.ff_marginal_reduce.restype = L.ff_marginal_reduce_host.restype = ctypes.c_int
    L.ff_marginal_expand.argtypes, L.ff_marginal_expand_host.argtypes = expand + [ctypes.c_void_p], expand
    L.ff_marginal_reduce.argtypes, L.ff_marginal_reduce_host.argtypes = reduce + [ctypes.c_void_p], reduce
    weigh = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_double,
             ctypes.c_double] + [ctypes.c_void_p] * 4
    mgrad = [ctypes.c_void_p] * 6 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                     ctypes.c_void_p]
    L.ff_marginal_weigh.restype = L.ff_marginal_weigh_host.restype = ctypes.c_int
    L.ff_marginal_grad_reduce.restype = L.ff_marginal_grad_reduce_host.restype = ctypes.c_int
    L.ff_marginal_weigh.argtypes, L.ff_marginal_weigh_host.argtypes = weigh + [ctypes.c_void_p], weigh
    L.ff_marginal_grad_reduce.argtypes, L.ff_marginal_grad_reduce_host.argtypes = mgrad + [ctypes.c_void_p], mgrad
    obs_expand = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                  ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lme = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    L.ff_observe_expand.restype = L.ff_observe_expand_host.restype = ctypes.c_int
    L.ff_logmeanexp.restype = L.ff_logmeanexp_host.restype = ctypes.c_int
    L.ff_observe_expand.argtypes, L.ff_observe_expand_host.argtypes = obs_expand + [ctypes.c_void_p], obs_expand
    L.ff_logmeanexp.argtypes, L.ff_logmeanexp_host.argtypes = lme + [ctypes.c_void_p], lme
    resample = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.ff_weighted_resample.restype = L.ff_weighted_resample_host.restype = ctypes.c_int
    L.ff_weighted_resample.argtypes, L.ff_weighted_resample_host.argtypes = resample + [ctypes.c_void_p], resample
    obs_keep = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double, ctypes.c_void_p]
    grad_reduce = [ctypes.c_void_p] * 5 + [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                           ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.ff_observe_keep.restype = L.ff_observe_keep_host.restype = ctypes.c_int
    L.ff_observe_grad_reduce.restype = L.ff_observe_grad_reduce_host.restype = ctypes.c_int
    L.ff_observe_keep.argtypes, L.ff_observe_keep_host.argtypes = obs_keep + [ctypes.c_void_p], obs_keep
    L.ff_observe_grad_reduce.argtypes, L.ff_observe_grad_reduce_host.argtypes = grad_reduce + [ctypes.c_void_p], grad_reduce
    mobs_expand = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 3 + \
                  [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64,
                   ctypes.c_void_p, ctypes.c_void_p]
    mobs_grad = [ctypes.c_void_p] * 7 + [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                         ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.ff_marginal_observe_expand.restype = L.ff_marginal_observe_expand_host.restype = ctypes.c_int
    L.ff_marginal_observe_grad_reduce.restype = L.ff_marginal_observe_grad_reduce_host.restype = ctypes.c_int
    L.ff_marginal_observe_expand.argtypes, L.ff_marginal_observe_expand_host.argtypes = mobs_expand + [ctypes.c_void_p], mobs_expand
    L.ff_marginal_observe_grad_reduce.argtypes, L.ff_marginal_observe_grad_reduce_host.argtypes = \
        mobs_grad + [ctypes.c_void_p], mobs_grad
    mobs_resample = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                     ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64] + [ctypes.c_void_p] * 4
    L.ff_marginal_observe_resample.restype = L.ff_marginal_observe_resample_host.restype = ctypes.c_int
    L.ff_marginal_observe_resample.argtypes, L.ff_marginal_observe_resample_host.argtypes = \
        mobs_resample + [ctypes.c_void_p], mobs_resample
    L.ff_mlp_ode_adaptive.restype = ctypes.c_int
    L.ff_mlp_ode_adaptive.argtypes = [ctypes.POINTER(PlanStruct), ctypes.POINTER(OdeArgs), ctypes.POINTER(AdaptConfig),
                                      ctypes.POINTER(AdaptBuffers), ctypes.c_double, ctypes.c_double, ctypes.c_int32,
                                      ctypes.c_int32, ctypes.c_void_p]
    L.ff_trace_workspace_floats.restype = ctypes.c_size_t
    L.ff_trace_workspace_floats.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]
    L.ff_trace_estimate.restype = ctypes.c_int
    L.ff_trace_estimate.argtypes = [ctypes.POINTER(TraceArgs), ctypes.c_void_p]
    L.ff_trace_estimate_host.restype = ctypes.c_int
    L.ff_trace_estimate_host.argtypes = [ctypes.POINTER(TraceArgs)]
    L.ff_trace_prod_workspace_floats.restype = ctypes.c_size_t
    L.ff_trace_prod_workspace_floats.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]
    for fn in (L.ff_trace_basis, L.ff_trace_combine):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.POINTER(TraceProdArgs), ctypes.c_void_p]
    for fn in (L.ff_trace_basis_host, L.ff_trace_combine_host):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.POINTER(TraceProdArgs)]
    L.ff_adapt_host_row.restype = ctypes.c_int
    L.ff_adapt_host_row.argtypes = [ctypes.POINTER(AdaptConfig), ctypes.c_float, ctypes.POINTER(ctypes.c_float),
                                    ctypes.POINTER(ctypes.c_float), ctypes.c_void_p]
    L.ff_pair_kernel_count.restype = ctypes.c_int
    L.ff_pair_kernel_name.restype = ctypes.c_char_p
    L.ff_pair_kernel_name.argtypes = [ctypes.c_int]
    L.ff_mlp_pair_plan.restype = ctypes.c_int
    L.ff_mlp_pair_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                   ctypes.POINTER(PlanStruct)]
    L.ff_mlp_pair_select_plan.restype = ctypes.c_int
    L.ff_mlp_pair_select_plan.argtypes = L.ff_mlp_pair_plan.argtypes
    L.ff_mlp_pair_wpack_floats.restype = ctypes.c_size_t
    L.ff_mlp_pair_wpack_floats.argtypes = [ctypes.POINTER(PlanStruct)]
    L.ff_mlp_pair_wpack.restype = ctypes.c_int
    L.ff_mlp_pair_wpack.argtypes = [ctypes.POINTER(PlanStruct)] + [ctypes.POINTER(ctypes.c_void_p)] * 4 + [
        ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.ff_mlp_row_width.restype = ctypes.c_int
    L.ff_mlp_row_width.argtypes = [ctypes.POINTER(PlanStruct)]
    L.ff_adapt_host_transition.restype = ctypes.c_int
    L.ff_adapt_host_transition.argtypes = [ctypes.POINTER(AdaptConfig), ctypes.POINTER(AdaptState), ctypes.c_int32,
                                           ctypes.POINTER(ctypes.c_float)]
    return L


def _err(rc: int, what: str) -> RuntimeError:
    names = {FF_ERR_BADARG: "FF_ERR_BADARG", FF_ERR_UNSUPPORTED: "FF_ERR_UNSUPPORTED", FF_ERR_HIP: "FF_ERR_HIP",
             FF_ERR_EXCHANGE: "FF_ERR_EXCHANGE"}
    extra = f" (hipError {lib().ff_last_hip_error()})" if rc == FF_ERR_HIP else ""
    return RuntimeError(f"{what} failed: {names.get(rc, rc)}{extra}")


def make_plan(dim: int, cond_dim: int, hidden: List[int], mode: int,
              act: Tuple[int, float, float] = (ACT_SILU, 0.0, 0.0), precision: int = PREC_F32) -> PlanStruct:
    """ff_mlp_plan_prec: pick the compiled kernel for this network shape (raises if none fits)."""
    p = PlanStruct()
    arr = (ctypes.c_int * len(hidden))(*hidden)
    prm = (ctypes.c_float * 2)(float(act[1]), float(act[2]))
    rc = lib().ff_mlp_plan_prec(dim, cond_dim, len(hidden), arr, mode, int(act[0]), prm, int(precision), ctypes.byref(p))
    if rc == FF_ERR_UNSUPPORTED and precision in (PREC_BF16X3, PREC_BF16X2):
        name = "bf16x3" if precision == PREC_BF16X3 else "bf16x2"
        raise NotImplementedError(
            f"precision='{name}' (one of the split-precision options 'bf16x3' / 'bf16x2') has no kernel for dim={dim}, cond_dim={cond_dim}, hidden={hidden}, mode={mode}, "
            f"activation={act[0]}: the split-precision family covers SiLU networks of 1-4 hidden layers up to 256 wide, "
            "cond_dim <= 16, dim <= 16: bf16x3 state-only solves (sampling, Euler-Maruyama; fixed grids and the adaptive "
            "methods); bf16x2 also Hutchinson and exact-trace log-densities and, state-only with at most 4 Runge-Kutta "
            "stages, dim <= 32; use precision='f32'")
    if rc == FF_ERR_UNSUPPORTED:
        raise NotImplementedError(
            f"no gfx950 kernel instantiation for dim={dim}, cond_dim={cond_dim}, hidden={hidden}, mode={mode}, "
            f"activation={act[0]}: "
            "compiled shapes cover dim<=128, cond_dim<=64, hidden width<=1024 (SiLU; other activations: dim<=64, "
            "cond_dim<=16, width<=512)")
    if rc != FF_OK:
        raise _err(rc, "ff_mlp_plan")
    return p


def pack_weights(plan: PlanStruct, weights: List[torch.Tensor], biases: List[Optional[torch.Tensor]],
                 hidden: List[int], x_col0: int, c_col0: int) -> torch.Tensor:
    """ff_mlp_wpack on host copies of the nn.Linear parameters; returns the packed CPU tensor.  A pull plan
    (``make_pull_plan``): ff_mlp_pull_wpack, the forward network's pack followed by the transposed network's."""
    L = lib()
    pull = is_pull_plan(plan)
    n = (L.ff_mlp_pull_wpack_floats if pull else L.ff_mlp_wpack_floats)(ctypes.byref(plan))
    out = torch.empty(n, dtype=torch.float32)
    ws = [f32_on(w, "cpu") for w in weights]
    bs = [f32_on(b, "cpu") for b in biases]
    wp = (ctypes.c_void_p * len(ws))(*[w.data_ptr() for w in ws])
    bp = (ctypes.c_void_p * len(bs))(*[0 if b is None else b.data_ptr() for b in bs])
    hw = (ctypes.c_int * len(hidden))(*hidden)
    rc = (L.ff_mlp_pull_wpack if pull else L.ff_mlp_wpack)(ctypes.byref(plan), wp, bp, hw, int(ws[0].shape[1]), x_col0, c_col0,
                                                           out.data_ptr())
    if rc != FF_OK:
        raise _err(rc, "ff_mlp_pull_wpack" if pull else "ff_mlp_wpack")
    return out


def kernel_name(plan: PlanStruct) -> str:
    """ff_plan_kernel_name: the instantiation a plan selects."""
    n = lib().ff_plan_kernel_name(ctypes.byref(plan))
    return n.decode() if n else "?"


def make_pair_plan(dim: int, cond_dim: int, hidden: List[int], select: bool = False) -> PlanStruct:
    """ff_mlp_pair_plan: the two-network kernel for a state of ``dim`` = 2D dimensions (raises if none holds it);
    ``select``: ff_mlp_pair_select_plan, its row-select variant (one network per evaluation row)."""
    p = PlanStruct()
    arr = (ctypes.c_int * len(hidden))(*hidden)
    rc = (lib().ff_mlp_pair_select_plan if select else lib().ff_mlp_pair_plan)(dim, cond_dim, len(hidden), arr, ctypes.byref(p))
    if rc == FF_ERR_UNSUPPORTED:
        raise NotImplementedError(
            f"no gfx950 two-network kernel for a state of {dim} dimensions, cond_dim={cond_dim}, units={hidden}: the "
            "compiled pair kernels hold states of up to 32 dimensions (16 per half), up to 16 conditional inputs and "
            "hidden widths up to 256 (SiLU)")
    if rc != FF_OK:
        raise _err(rc, "ff_mlp_pair_plan")
    return p


def is_pair_plan(plan: PlanStruct) -> bool:
    return PAIR_KERNEL_BASE <= int(plan.kernel_id) < PUSH_KERNEL_BASE


def is_select_plan(plan: PlanStruct) -> bool:
    return PAIR_SELECT_KERNEL_BASE <= int(plan.kernel_id) < PUSH_KERNEL_BASE


PUSH_ENVELOPE = ("the push-forward kernels (flow_jvp / flow_jacobian) hold SiLU networks in f32 with hidden widths up to 256, "
                 "up to 32 state dimensions and up to 16 conditional inputs, and up to 15 tangents per sample")


def make_push_plan(dim: int, cond_dim: int, hidden: List[int], act: Tuple[int, float, float] = (ACT_SILU, 0.0, 0.0),
                   precision: int = PREC_F32) -> PlanStruct:
    """ff_mlp_push_plan: the smallest push-forward unit that holds the network (NotImplementedError with the envelope if
    none does)."""
    p = PlanStruct()
    arr = (ctypes.c_int * len(hidden))(*hidden)
    rc = lib().ff_mlp_push_plan(dim, cond_dim, len(hidden), arr, int(act[0]), int(precision), ctypes.byref(p))
    if rc == FF_ERR_UNSUPPORTED:
        raise NotImplementedError(f"no gfx950 push-forward kernel for dim={dim}, cond_dim={cond_dim}, hidden={hidden}, "
                                  f"activation={act[0]}: {PUSH_ENVELOPE}")
    if rc != FF_OK:
        raise _err(rc, "ff_mlp_push_plan")
    return p


def is_push_plan(plan: PlanStruct) -> bool:
    return PUSH_KERNEL_BASE <= int(plan.kernel_id) < PULL_KERNEL_BASE


PULL_ENVELOPE = ("the pull-back kernels (flow_vjp) hold SiLU networks in f32 with hidden widths up to 256, up to 32 state "
                 "dimensions and up to 16 conditional inputs, up to 15 cotangents per sample, and as many hidden layers as "
                 "leave the stash of their slopes inside 160 KiB of LDS: 18 at width 256 (17 beyond 16 dimensions), 36 at "
                 "width 128")


def make_pull_plan(dim: int, cond_dim: int, hidden: List[int], act: Tuple[int, float, float] = (ACT_SILU, 0.0, 0.0),
                   precision: int = PREC_F32) -> PlanStruct:
    """ff_mlp_pull_plan: the smallest pull-back unit that holds the network (NotImplementedError with the envelope if
    none does, or if its depth overflows the stash)."""
    p = PlanStruct()
    arr = (ctypes.c_int * len(hidden))(*hidden)
    rc = lib().ff_mlp_pull_plan(dim, cond_dim, len(hidden), arr, int(act[0]), int(precision), ctypes.byref(p))
    if rc == FF_ERR_UNSUPPORTED:
        raise NotImplementedError(f"no gfx950 pull-back kernel for dim={dim}, cond_dim={cond_dim}, hidden={hidden}, "
                                  f"activation={act[0]}: {PULL_ENVELOPE}")
    if rc != FF_OK:
        raise _err(rc, "ff_mlp_pull_plan")
    return p


def is_pull_plan(plan: PlanStruct) -> bool:
    return PULL_KERNEL_BASE <= int(plan.kernel_id) < PULL_SELECT_KERNEL_BASE


def row_width(plan: PlanStruct) -> int:
    """ff_mlp_row_width: first-layer bias words per evaluation row (2 x width for a pair plan, width for a select plan)."""
    return int(lib().ff_mlp_row_width(ctypes.byref(plan)))


def pack_pair_weights(plan: PlanStruct, q_layers, p_layers, hidden: List[int], x_col0: int, c_col0: int) -> torch.Tensor:
    """ff_mlp_pair_wpack on host copies of the two networks' nn.Linear parameters; returns the packed CPU tensor."""
    L = lib()
    n = L.ff_mlp_pair_wpack_floats(ctypes.byref(plan))
    out = torch.empty(n, dtype=torch.float32)
    keep, ptrs = [], []
    for layers in (q_layers, p_layers):
        ws = [f32_on(l.weight, "cpu") for l in layers]
        bs = [f32_on(l.bias, "cpu") for l in layers]
        keep += ws + bs
        ptrs.append((ctypes.c_void_p * len(ws))(*[w.data_ptr() for w in ws]))
        ptrs.append((ctypes.c_void_p * len(bs))(*[b.data_ptr() for b in bs]))
    hw = (ctypes.c_int * len(hidden))(*hidden)
    rc = L.ff_mlp_pair_wpack(ctypes.byref(plan), ptrs[0], ptrs[1], ptrs[2], ptrs[3], hw, int(q_layers[0].weight.shape[1]),
                             x_col0, c_col0, out.data_ptr())
    if rc != FF_OK:
        raise _err(rc, "ff_mlp_pair_wpack")
    return out


PULL_SELECT_ENVELOPE = ("the row-select pull-back kernels (sample_leapfrog_vjp / log_prob_leapfrog_grad) hold two SiLU networks of one "
                        "shape in f32 with hidden widths up to 256, joint states [q | p] of up to 32 dimensions (16 per half) and up "
                        "to 16 conditional inputs, up to 15 cotangents per sample, and as many hidden layers as leave the stash of "
                        "their slopes inside 160 KiB of LDS: 18 at width 256 (17 beyond 16 joint dimensions), 36 at width 128")


def make_pull_select_plan(dim: int, cond_dim: int, hidden: List[int]) -> PlanStruct:
    """ff_mlp_pull_select_plan: the row-select pull-back unit for a joint state of ``dim`` = 2D dimensions
    (NotImplementedError with the envelope if none holds it, or if its depth overflows the stash)."""
    p = PlanStruct()
    arr = (ctypes.c_int * len(hidden))(*hidden)
    rc = lib().ff_mlp_pull_select_plan(dim, cond_dim, len(hidden), arr, ctypes.byref(p))
    if rc == FF_ERR_UNSUPPORTED:
        raise NotImplementedError(f"no gfx950 row-select pull-back kernel for a joint state of {dim} dimensions, cond_dim={cond_dim}, "
                                  f"units={hidden}: {PULL_SELECT_ENVELOPE}")
    if rc != FF_OK:
        raise _err(rc, "ff_mlp_pull_select_plan")
    return p


def is_pull_select_plan(plan: PlanStruct) -> bool:
    return PULL_SELECT_KERNEL_BASE <= int(plan.kernel_id) < PUSH_SELECT_KERNEL_BASE


def pack_pull_select_weights(plan: PlanStruct, q_layers, p_layers, hidden: List[int], x_col0: int, c_col0: int) -> torch.Tensor:
    """ff_mlp_pull_select_wpack on host copies of the two networks' nn.Linear parameters: two pull packs, mlp_q's then mlp_p's;
    returns the packed CPU tensor."""
    L = lib()
    n = L.ff_mlp_pull_select_wpack_floats(ctypes.byref(plan))
    out = torch.empty(n, dtype=torch.float32)
    keep, ptrs = [], []
    for layers in (q_layers, p_layers):
        ws = [f32_on(l.weight, "cpu") for l in layers]
        bs = [f32_on(l.bias, "cpu") for l in layers]
        keep += ws + bs
        ptrs.append((ctypes.c_void_p * len(ws))(*[w.data_ptr() for w in ws]))
        ptrs.append((ctypes.c_void_p * len(bs))(*[b.data_ptr() for b in bs]))
    hw = (ctypes.c_int * len(hidden))(*hidden)
    rc = L.ff_mlp_pull_select_wpack(ctypes.byref(plan), ptrs[0], ptrs[1], ptrs[2], ptrs[3], hw, int(q_layers[0].weight.shape[1]),
                                    x_col0, c_col0, out.data_ptr())
    if rc != FF_OK:
        raise _err(rc, "ff_mlp_pull_select_wpack")
    return out


PUSH_SELECT_ENVELOPE = ("the row-select push-forward kernels (sample_leapfrog_jvp / sample_leapfrog_jacobian) hold two SiLU networks "
                        "of one shape in f32 with hidden widths up to 256, joint states [q | p] of up to 32 dimensions (16 per half) "
                        "and up to 16 conditional inputs, and up to 15 tangents per sample")


def make_push_select_plan(dim: int, cond_dim: int, hidden: List[int]) -> PlanStruct:
    """ff_mlp_push_select_plan: the row-select push-forward unit for a joint state of ``dim`` = 2D dimensions
    (NotImplementedError with the envelope if none holds it)."""
    p = PlanStruct()
    arr = (ctypes.c_int * len(hidden))(*hidden)
    rc = lib().ff_mlp_push_select_plan(dim, cond_dim, len(hidden), arr, ctypes.byref(p))
    if rc == FF_ERR_UNSUPPORTED:
        raise NotImplementedError(f"no gfx950 row-select push-forward kernel for a joint state of {dim} dimensions, cond_dim={cond_dim}, "
                                  f"units={hidden}: {PUSH_SELECT_ENVELOPE}")
    if rc != FF_OK:
        raise _err(rc, "ff_mlp_push_select_plan")
    return p


def is_push_select_plan(plan: PlanStruct) -> bool:
    return int(plan.kernel_id) >= PUSH_SELECT_KERNEL_BASE


def pack_push_select_weights(plan: PlanStruct, q_layers, p_layers, hidden: List[int], x_col0: int, c_col0: int) -> torch.Tensor:
    """ff_mlp_push_select_wpack on host copies of the two networks' nn.Linear parameters: two forward packs, mlp_q's then
    mlp_p's; returns the packed CPU tensor."""
    L = lib()
    n = L.ff_mlp_push_select_wpack_floats(ctypes.byref(plan))
    out = torch.empty(n, dtype=torch.float32)
    keep, ptrs = [], []
    for layers in (q_layers, p_layers):
        ws = [f32_on(l.weight, "cpu") for l in layers]
        bs = [f32_on(l.bias, "cpu") for l in layers]
        keep += ws + bs
        ptrs.append((ctypes.c_void_p * len(ws))(*[w.data_ptr() for w in ws]))
        ptrs.append((ctypes.c_void_p * len(bs))(*[b.data_ptr() for b in bs]))
    hw = (ctypes.c_int * len(hidden))(*hidden)
    rc = L.ff_mlp_push_select_wpack(ctypes.byref(plan), ptrs[0], ptrs[1], ptrs[2], ptrs[3], hw, int(q_layers[0].weight.shape[1]),
                                    x_col0, c_col0, out.data_ptr())
    if rc != FF_OK:
        raise _err(rc, "ff_mlp_push_select_wpack")
    return out


LAUNCH_ONE_WAVE, LAUNCH_TWIN, LAUNCH_ONE_WAVE_AND_TWIN = 0, 1, 2      # FF_LAUNCH_*


def launch_kind(plan: PlanStruct, batch: int, mode: int, tangent_count: int = 0, jac_out: bool = False) -> int:
    """ff_mlp_launch_kind: which kernel(s) a launch of ``batch`` samples takes (LAUNCH_*)."""
    rc = int(lib().ff_mlp_launch_kind(ctypes.byref(plan), batch, mode, tangent_count, int(jac_out)))
    if rc < 0:
        raise _err(rc, "ff_mlp_launch_kind")
    return rc


def samples_per_workgroup(plan: PlanStruct, mode: int) -> int:
    return int(lib().ff_mlp_samples_per_workgroup(ctypes.byref(plan), mode))


def normal_fill(batch: int, dim: int, seed: int, sample_offset: int, device, noise_index: int = PRIOR_NOISE_INDEX,
                scale: float = 1.0) -> torch.Tensor:
    """ff_normal_fill: [batch, dim] normals of the counter-based stream for global rows
    sample_offset .. sample_offset + batch - 1 (the prior draw of the sharded Euler-Maruyama sampler)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("flowfusion_amd: ff_normal_fill fills device memory (there is no CPU path)")
    out = torch.empty(batch, dim, dtype=torch.float32, device=device)
    if batch == 0:
        return out
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        rc = lib().ff_normal_fill(out.data_ptr(), batch, dim, seed & 0xFFFFFFFFFFFFFFFF, sample_offset,
                                  noise_index & 0xFFFFFFFF, float(scale), ctypes.c_void_p(stream))
    if rc != FF_OK:
        raise _err(rc, "ff_normal_fill")
    return out


def probe_fill(batch: int, num_probes: int, dim: int, seed: int, sample_offset: int, device, scale: float = 1.0) -> torch.Tensor:
    """ff_probe_fill: the [batch, K, dim] probes (+-``scale``) of a K-probe Hutchinson launch for global rows
    sample_offset .. sample_offset + batch - 1 -- probe 0 under the single-probe stream's index, probe k >= 1 under
    HUTCH_PROBE_NOISE_BASE + k.  On a CUDA device on the current stream; ``device="cpu"`` goes to ff_probe_fill_host."""
    device = torch.device(device)
    K = int(num_probes)
    if not 1 <= K <= MAX_HUTCH_PROBES:
        raise ValueError(f"num_probes={num_probes}: 1 .. {MAX_HUTCH_PROBES} probes per sample")
    if batch < 0 or dim < 1:
        raise ValueError(f"probe_fill: batch={batch}, dim={dim}")
    out = torch.empty(batch, K, dim, dtype=torch.float32, device=device)
    if batch == 0:
        return out
    L = lib()
    rc = _on_stream(device, L.ff_probe_fill, L.ff_probe_fill_host,
                    (out.data_ptr(), batch, K, dim, int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_offset), float(scale)))
    if rc != FF_OK:
        raise _err(rc, "ff_probe_fill")
    return out


def stage_combine(out: torch.Tensor, x: Optional[torch.Tensor], ks, coefs, x_coef: float = 1.0) -> torch.Tensor:
    """ff_stage_combine: out = x_coef * x + sum_s coefs[s] * ks[s] in one pass (flat fp32 device tensors of
    equal numel; `out` may alias an input).  Terms with a zero coefficient are not read, `x` with a zero `x_coef` included."""
    if not out.is_cuda:
        raise RuntimeError("flowfusion_amd: ff_stage_combine works on device memory (there is no CPU path)")
    dev = out.device
    a = CombineArgs()
    n = out.numel()
    a.out = _chk(out, "out", dev)
    a.x = _chk(x, "x", dev)
    if x is not None and x.numel() != n:
        raise RuntimeError("stage_combine: x and out differ in size")
    if len(ks) > 7 or len(ks) != len(coefs):
        raise RuntimeError("stage_combine: at most FF_MAX_SLOTS = 7 terms, one coefficient each")
    for s, (k, c) in enumerate(zip(ks, coefs)):
        c = float(c)
        if k is None or c == 0.0:
            continue
        if k.numel() != n:
            raise RuntimeError("stage_combine: term and out differ in size")
        a.k[s] = _chk(k, f"k[{s}]", dev)
        a.coef[s] = c
    a.x_coef = float(x_coef)
    a.n = n
    if n == 0:
        return out
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib().ff_stage_combine(ctypes.byref(a), ctypes.c_void_p(stream))
    if rc != FF_OK:
        raise _err(rc, "ff_stage_combine")
    return out


def _on_stream(dev, device_fn, host_fn, args):
    """One call of a kernel entry point on torch's current stream of ``dev``, or of its host twin for CPU tensors."""
    if dev.type != "cuda":
        return host_fn(*args)
    with torch.cuda.device(dev):
        return device_fn(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))


def marginal_expand(x: torch.Tensor, num_momenta: int, seed: int, sample_offset: int = 0,
                    shift: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
                    cond: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """ff_marginal_expand: (z0 [B K, 2 D], cond_out [B K, C] or None) from ``x`` [B, D]: row r K + k is
    [(x[r] - shift) / scale | momentum k of global row sample_offset + r] and the (already normalised) ``cond[r]``.
    Device tensors on the current stream; CPU tensors go to ff_marginal_expand_host."""
    dev = x.device
    B, D = x.shape
    K = int(num_momenta)
    if not 1 <= K <= MAX_MOMENTA:
        raise ValueError(f"num_momenta={num_momenta}: 1 .. {MAX_MOMENTA} momentum draws per data point")
    for t, name in ((shift, "shift"), (scale, "scale")):
        if t is not None and t.numel() != D:
            raise RuntimeError(f"marginal_expand: {name} has {t.numel()} elements, x has {D} columns")
    if cond is not None and (cond.dim() != 2 or cond.shape[0] != B or cond.shape[1] < 1):
        raise RuntimeError(f"marginal_expand: cond has shape {tuple(cond.shape)}, expected [{B}, C >= 1]")
    C = 0 if cond is None else int(cond.shape[1])
    z0 = torch.empty(B * K, 2 * D, dtype=torch.float32, device=dev)
    cond_out = None if cond is None else torch.empty(B * K, C, dtype=torch.float32, device=dev)
    if B == 0:
        return z0, cond_out
    L = lib()
    rc = _on_stream(dev, L.ff_marginal_expand, L.ff_marginal_expand_host,
                    (_chk(x, "x", dev), _chk(shift, "shift", dev), _chk(scale, "scale", dev), _chk(cond, "cond", dev), B, D, C, K,
                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_offset), z0.data_ptr(), 0 if cond is None else cond_out.data_ptr()))
    if rc != FF_OK:
        raise _err(rc, "ff_marginal_expand")
    return z0, cond_out


def marginal_reduce(z1: torch.Tensor, num_momenta: int, seed: int, sample_offset: int = 0, log_det: float = 0.0,
                    out: Optional[torch.Tensor] = None, ess: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ff_marginal_reduce: ``out`` [B] = logsumexp over the K rows of a data point of log N(z1) - log N(p0), - log K -
    log_det, from ``z1`` [B K, 2 D] (the solution from ``marginal_expand``'s z0; p0 regenerated from ``seed`` and
    ``sample_offset``); ``ess`` [B], if given, takes the effective sample size.  ``out`` is allocated if None.  Device
    tensors on the current stream; CPU tensors go to ff_marginal_reduce_host."""
    dev = z1.device
    K = int(num_momenta)
    if not 1 <= K <= MAX_MOMENTA:
        raise ValueError(f"num_momenta={num_momenta}: 1 .. {MAX_MOMENTA} momentum draws per data point")
    rows, D2 = z1.shape
    if rows % K or D2 % 2 or D2 < 2:
        raise RuntimeError(f"marginal_reduce: z1 has shape {tuple(z1.shape)}, expected [B * {K}, 2 D]")
    B = rows // K
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    for t, name in ((out, "out"), (ess, "ess")):
        if t is not None and t.numel() != B:
            raise RuntimeError(f"marginal_reduce: {name} has {t.numel()} elements for {B} data points")
    if B == 0:
        return out
    L = lib()
    rc = _on_stream(dev, L.ff_marginal_reduce, L.ff_marginal_reduce_host,
                    (_chk(z1, "z1", dev), B, D2 // 2, K, int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_offset), float(log_det),
                     _chk(out, "out", dev), _chk(ess, "ess", dev)))
    if rc != FF_OK:
        raise _err(rc, "ff_marginal_reduce")
    return out


def marginal_weigh(z1: torch.Tensor, num_momenta: int, seed: int, sample_offset: int = 0, log_det: float = 0.0,
                   min_weight: float = 0.0, out: Optional[torch.Tensor] = None, ess: Optional[torch.Tensor] = None):
    """ff_marginal_weigh: ``(out [B], lw [B K] float64, keep [B K] int32)`` from ``z1`` [B K, 2 D]: ``out`` (and ``ess`` [B],
    if given) bit for bit what ``marginal_reduce`` writes, every row's log-weight in double, and ``keep`` = 1 where draw k of
    its point has a normalised weight ``exp(lw - max) / W`` that is > 0 and >= ``min_weight`` (0 <= min_weight < 1); a
    degenerate point (a NaN among its ``lw``, or all -inf) keeps nothing.  ``out`` is allocated if None.  Device tensors on
    the current stream; CPU tensors go to ff_marginal_weigh_host."""
    dev = z1.device
    K = int(num_momenta)
    if not 1 <= K <= MAX_MOMENTA:
        raise ValueError(f"num_momenta={num_momenta}: 1 .. {MAX_MOMENTA} momentum draws per data point")
    m = float(min_weight)
    if not 0.0 <= m < 1.0:
        raise ValueError(f"min_weight={min_weight}: a normalised weight, 0 <= min_weight < 1 (0 keeps every draw of non-zero weight)")
    if z1.dim() != 2 or z1.shape[0] % K or z1.shape[1] % 2 or z1.shape[1] < 2:
        raise RuntimeError(f"marginal_weigh: z1 has shape {tuple(z1.shape)}, expected [B * {K}, 2 D]")
    rows, D2 = z1.shape
    B = rows // K
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    for t, name in ((out, "out"), (ess, "ess")):
        if t is not None and t.numel() != B:
            raise RuntimeError(f"marginal_weigh: {name} has {t.numel()} elements for {B} data points")
    lw = torch.empty(rows, dtype=torch.float64, device=dev)
    keep = torch.empty(rows, dtype=torch.int32, device=dev)
    ptrs = (_chk(z1, "z1", dev), _chk(out, "out", dev), _chk(ess, "ess", dev))
    if B == 0:
        return out, lw, keep
    L = lib()
    rc = _on_stream(dev, L.ff_marginal_weigh, L.ff_marginal_weigh_host,
                    (ptrs[0], B, D2 // 2, K, int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_offset), float(log_det), m, ptrs[1],
                     ptrs[2], lw.data_ptr(), keep.data_ptr()))
    if rc != FF_OK:
        raise _err(rc, "ff_marginal_weigh")
    return out, lw, keep


def marginal_grad_reduce(lw: torch.Tensor, row_of: torch.Tensor, gz_rows: torch.Tensor, gc_rows: Optional[torch.Tensor],
                         num_momenta: int, scale: Optional[torch.Tensor] = None, cond_scale: Optional[torch.Tensor] = None,
                         grad_x: Optional[torch.Tensor] = None, grad_c: Optional[torch.Tensor] = None):
    """ff_marginal_grad_reduce: ``(grad_x [B, D], grad_c [B, C] or None)``, the gradient of ``marginal_weigh``'s ``out`` from
    the kept rows' pull-backs of ``-z1``: ``sum_k wn_k gz_rows[row_of[r K + k]][:D] / scale`` and ``sum_k wn_k
    gc_rows[row_of[r K + k]] / cond_scale``; ``wn`` the normalised weights of the full sum, recomputed from ``lw`` [B K]
    float64.  ``row_of`` [B K] int32: the row of a draw in ``gz_rows`` [n, 2 D] / ``gc_rows`` [n, C], < 0 for a draw that is
    skipped (checked here to stay below n).  ``scale`` [D] / ``cond_scale`` [C]: None for 1.  The outputs are allocated where
    not given.  Device tensors on the current stream; CPU tensors go to ff_marginal_grad_reduce_host."""
    dev = lw.device
    K = int(num_momenta)
    if not 1 <= K <= MAX_MOMENTA:
        raise ValueError(f"num_momenta={num_momenta}: 1 .. {MAX_MOMENTA} momentum draws per data point")
    if lw.dtype != torch.float64 or lw.dim() != 1 or lw.numel() % K or not lw.is_contiguous():
        raise RuntimeError(f"marginal_grad_reduce: lw must be a contiguous float64 tensor [B * {K}], got {lw.dtype} "
                           f"{tuple(lw.shape)}")
    B = lw.numel() // K
    if gz_rows.dim() != 2 or gz_rows.shape[1] % 2 or gz_rows.shape[1] < 2:
        raise RuntimeError(f"marginal_grad_reduce: gz_rows has shape {tuple(gz_rows.shape)}, expected [n, 2 D]")
    n, D = int(gz_rows.shape[0]), int(gz_rows.shape[1]) // 2
    if gc_rows is not None and (gc_rows.dim() != 2 or gc_rows.shape[0] != n or gc_rows.shape[1] < 1):
        raise RuntimeError(f"marginal_grad_reduce: gc_rows has shape {tuple(gc_rows.shape)}, expected [{n}, C >= 1]")
    C = 0 if gc_rows is None else int(gc_rows.shape[1])
    if row_of.dtype != torch.int32 or row_of.numel() != B * K or not row_of.is_contiguous() or row_of.device != dev:
        raise RuntimeError(f"marginal_grad_reduce: row_of must be a contiguous int32 tensor of {B * K} elements on {dev}")
    if B > 0 and int(row_of.max()) >= n:
        raise RuntimeError(f"marginal_grad_reduce: row_of points at row {int(row_of.max())}, gz_rows has {n} rows")
    if gc_rows is None:
        cond_scale = None
    for t, name, cols in ((scale, "scale", D), (cond_scale, "cond_scale", C)):
        if t is not None and t.numel() != cols:
            raise RuntimeError(f"marginal_grad_reduce: {name} has {t.numel()} elements for {cols} columns")
    if grad_x is None:
        grad_x = torch.empty(B, D, dtype=torch.float32, device=dev)
    if grad_c is None and gc_rows is not None:
        grad_c = torch.empty(B, C, dtype=torch.float32, device=dev)
    for t, name, cols in ((grad_x, "grad_x", D), (grad_c, "grad_c", C)):
        if t is not None and t.numel() != B * cols:
            raise RuntimeError(f"marginal_grad_reduce: {name} has {t.numel()} elements for [{B}, {cols}]")
    if n == 0:                                              # nothing was kept: no row is read, but the pointer is mandatory
        gz_rows = torch.zeros(1, 2 * D, dtype=torch.float32, device=dev)
        gc_rows = None if gc_rows is None else torch.zeros(1, C, dtype=torch.float32, device=dev)
    ptrs = (_chk(gz_rows, "gz_rows", dev), _chk(gc_rows, "gc_rows", dev), _chk(scale, "scale", dev),
            _chk(cond_scale, "cond_scale", dev), _chk(grad_x, "grad_x", dev),
            _chk(grad_c if gc_rows is not None else None, "grad_c", dev))
    if B == 0:
        return grad_x, grad_c
    L = lib()
    rc = _on_stream(dev, L.ff_marginal_grad_reduce, L.ff_marginal_grad_reduce_host,
                    (lw.data_ptr(), row_of.data_ptr(), ptrs[0], ptrs[1], ptrs[2], ptrs[3], B, D, C, K, ptrs[4], ptrs[5]))
    if rc != FF_OK:
        raise _err(rc, "ff_marginal_grad_reduce")
    return grad_x, grad_c


def observe_expand(x: torch.Tensor, noise_std: torch.Tensor, num_draws: int, seed: int, sample_offset: int = 0,
                   cond: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """ff_observe_expand: (y [B K, D], cond_out [B K, C] or None) from ``x`` [B, D]: row r K + k is
    ``x[r] - noise_std[r] * z`` with z noise draw k of global row sample_offset + r (two fp32 roundings), and ``cond[r]``.
    ``noise_std``: [D] (one vector for every row) or [B, D].  Device tensors on the current stream; CPU tensors go to
    ff_observe_expand_host."""
    dev = x.device
    if x.dim() != 2 or x.shape[1] < 1:
        raise RuntimeError(f"observe_expand: x has shape {tuple(x.shape)}, expected [B, D >= 1]")
    B, D = x.shape
    K = int(num_draws)
    if not 1 <= K <= MAX_OBS_DRAWS:
        raise ValueError(f"num_draws={num_draws}: 1 .. {MAX_OBS_DRAWS} noise draws per data point")
    if tuple(noise_std.shape) == (D,):
        stride = 0
    elif tuple(noise_std.shape) == (B, D):
        stride = D
    else:
        raise RuntimeError(f"observe_expand: noise_std has shape {tuple(noise_std.shape)}, expected [{D}] or [{B}, {D}]")
    if cond is not None and (cond.dim() != 2 or cond.shape[0] != B or cond.shape[1] < 1):
        raise RuntimeError(f"observe_expand: cond has shape {tuple(cond.shape)}, expected [{B}, C >= 1]")
    C = 0 if cond is None else int(cond.shape[1])
    y = torch.empty(B * K, D, dtype=torch.float32, device=dev)
    cond_out = None if cond is None else torch.empty(B * K, C, dtype=torch.float32, device=dev)
    ptrs = (_chk(x, "x", dev), _chk(noise_std, "noise_std", dev), _chk(cond, "cond", dev))
    if B == 0:
        return y, cond_out
    L = lib()
    rc = _on_stream(dev, L.ff_observe_expand, L.ff_observe_expand_host,
                    (ptrs[0], ptrs[1], stride, ptrs[2], B, D, C, K, int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_offset),
                     y.data_ptr(), 0 if cond is None else cond_out.data_ptr()))
    if rc != FF_OK:
        raise _err(rc, "ff_observe_expand")
    return y, cond_out


def logmeanexp(lp: torch.Tensor, num_draws: int, out: Optional[torch.Tensor] = None,
               ess: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ff_logmeanexp: ``out`` [B] = logsumexp over the K consecutive entries of a data point in ``lp`` (B K elements:
    [B K] or [B K, 1]) - log K, in double, rounded once; ``ess`` [B], if given, takes the effective sample size of the K
    weights.  ``out`` is allocated if None.  Device tensors on the current stream; CPU tensors go to ff_logmeanexp_host."""
    dev = lp.device
    K = int(num_draws)
    if not 1 <= K <= MAX_OBS_DRAWS:
        raise ValueError(f"num_draws={num_draws}: 1 .. {MAX_OBS_DRAWS} noise draws per data point")
    if lp.numel() % K or lp.dim() > 2 or (lp.dim() == 2 and lp.shape[1] != 1):
        raise RuntimeError(f"logmeanexp: lp has shape {tuple(lp.shape)}, expected [B * {K}] or [B * {K}, 1]")
    B = lp.numel() // K
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    for t, name in ((out, "out"), (ess, "ess")):
        if t is not None and t.numel() != B:
            raise RuntimeError(f"logmeanexp: {name} has {t.numel()} elements for {B} data points")
    ptrs = (_chk(lp, "lp", dev), _chk(out, "out", dev), _chk(ess, "ess", dev))
    if B == 0:
        return out
    L = lib()
    rc = _on_stream(dev, L.ff_logmeanexp, L.ff_logmeanexp_host, (ptrs[0], B, K, ptrs[1], ptrs[2]))
    if rc != FF_OK:
        raise _err(rc, "ff_logmeanexp")
    return out


def weighted_resample(y: torch.Tensor, lp: torch.Tensor, num_draws: int, num_samples: int, seed: int, sample_offset: int = 0,
                      want_index: bool = True, want_moments: bool = True):
    """ff_weighted_resample: ``(samples [B, M, D], index [B, M] int32, mean [B, D], var [B, D])`` from the particles ``y``
    [B K, D] and their log-weights ``lp`` (B K elements: [B K] or [B K, 1]): M = ``num_samples`` multinomial draws of
    every point's K rows by the weights ``exp(lp - max lp)`` (uniforms of global row sample_offset + r from the
    counter-based stream), and the weighted mean and variance, in double.  ``index`` is None without ``want_index``,
    ``mean`` and ``var`` without ``want_moments``.  Device tensors on the current stream; CPU tensors go to
    ff_weighted_resample_host."""
    dev = y.device
    K, M = int(num_draws), int(num_samples)
    if not 1 <= K <= MAX_OBS_DRAWS:
        raise ValueError(f"num_draws={num_draws}: 1 .. {MAX_OBS_DRAWS} noise draws per data point")
    if not 0 <= M <= MAX_OBS_SAMPLES:
        raise ValueError(f"num_samples={num_samples}: 0 .. {MAX_OBS_SAMPLES} posterior draws per data point")
    if y.dim() != 2 or y.shape[1] < 1 or y.shape[0] % K:
        raise RuntimeError(f"weighted_resample: y has shape {tuple(y.shape)}, expected [B * {K}, D >= 1]")
    rows, D = y.shape
    if lp.numel() != rows or lp.dim() > 2 or (lp.dim() == 2 and lp.shape[1] != 1):
        raise RuntimeError(f"weighted_resample: lp has shape {tuple(lp.shape)}, expected [{rows}] or [{rows}, 1]")
    B = rows // K
    samples = torch.empty(B, M, D, dtype=torch.float32, device=dev)
    index = torch.empty(B, M, dtype=torch.int32, device=dev) if want_index else None
    mean = torch.empty(B, D, dtype=torch.float32, device=dev) if want_moments else None
    var = torch.empty(B, D, dtype=torch.float32, device=dev) if want_moments else None
    ptrs = (_chk(y, "y", dev), _chk(lp, "lp", dev))
    if B == 0 or (M == 0 and not want_moments):             # nothing to compute
        return samples, index, mean, var
    L = lib()
    rc = _on_stream(dev, L.ff_weighted_resample, L.ff_weighted_resample_host,
                    (ptrs[0], ptrs[1], B, D, K, M, int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_offset), samples.data_ptr(),
                     0 if index is None else index.data_ptr(), 0 if mean is None else mean.data_ptr(),
                     0 if var is None else var.data_ptr()))
    if rc != FF_OK:
        raise _err(rc, "ff_weighted_resample")
    return samples, index, mean, var


def _lp_points(lp: torch.Tensor, num_draws: int, what: str) -> Tuple[int, int]:
    """(B, K) of the B K log-densities ``lp`` ([B K] or [B K, 1]) of an observe reduction."""
    K = int(num_draws)
    if not 1 <= K <= MAX_OBS_DRAWS:
        raise ValueError(f"num_draws={num_draws}: 1 .. {MAX_OBS_DRAWS} noise draws per data point")
    if lp.numel() % K or lp.dim() > 2 or (lp.dim() == 2 and lp.shape[1] != 1):
        raise RuntimeError(f"{what}: lp has shape {tuple(lp.shape)}, expected [B * {K}] or [B * {K}, 1]")
    return lp.numel() // K, K


def observe_keep(lp: torch.Tensor, num_draws: int, min_weight: float = 0.0) -> torch.Tensor:
    """ff_observe_keep: ``keep`` [B K] int32, 1 where draw k of its point has a normalised weight ``exp(lp - max) / W`` that
    is > 0 and >= ``min_weight`` (0 <= min_weight < 1), in double; a degenerate point (a NaN or +inf among its ``lp``, or
    all -inf) keeps nothing.  ``lp``: B K elements, [B K] or [B K, 1].  Device tensors on the current stream; CPU tensors
    go to ff_observe_keep_host."""
    dev = lp.device
    B, K = _lp_points(lp, num_draws, "observe_keep")
    m = float(min_weight)
    if not 0.0 <= m < 1.0:
        raise ValueError(f"min_weight={min_weight}: a normalised weight, 0 <= min_weight < 1 (0 keeps every draw of non-zero weight)")
    keep = torch.empty(B * K, dtype=torch.int32, device=dev)
    ptr = _chk(lp, "lp", dev)
    if B == 0:
        return keep
    L = lib()
    rc = _on_stream(dev, L.ff_observe_keep, L.ff_observe_keep_host, (ptr, B, K, m, keep.data_ptr()))
    if rc != FF_OK:
        raise _err(rc, "ff_observe_keep")
    return keep


def observe_grad_reduce(lp: torch.Tensor, row_of: torch.Tensor, gx_rows: torch.Tensor, gc_rows: Optional[torch.Tensor],
                        noise_std: torch.Tensor, num_draws: int, seed: int, sample_offset: int = 0,
                        want_noise_grad: bool = True, grad_x: Optional[torch.Tensor] = None,
                        grad_c: Optional[torch.Tensor] = None, grad_noise_std: Optional[torch.Tensor] = None):
    """ff_observe_grad_reduce: ``(grad_x [B, D], grad_c [B, C] or None, grad_noise_std [B, D] or None)``, the gradient of
    ff_logmeanexp of ``lp`` (B K elements) from the kept rows' own gradients: ``sum_k wn_k gx_rows[row_of[r K + k]]``,
    likewise ``gc_rows``, and ``-sum_k wn_k z_k gx_rows[row_of[r K + k]]`` with the noise draws regenerated from ``seed`` and
    global row ``sample_offset + r``; ``wn`` the normalised weights of the full sum, in double.  ``row_of`` [B K] int32: the
    row of a draw's gradient in ``gx_rows`` [n, D] / ``gc_rows`` [n, C], < 0 for a draw that is skipped (checked here to stay
    below n).  ``noise_std`` [D] or [B, D] as ff_observe_expand took it.  The outputs are allocated where not given.  Device
    tensors on the current stream; CPU tensors go to ff_observe_grad_reduce_host."""
    dev = lp.device
    B, K = _lp_points(lp, num_draws, "observe_grad_reduce")
    if gx_rows.dim() != 2 or gx_rows.shape[1] < 1:
        raise RuntimeError(f"observe_grad_reduce: gx_rows has shape {tuple(gx_rows.shape)}, expected [n, D >= 1]")
    n, D = gx_rows.shape
    if gc_rows is not None and (gc_rows.dim() != 2 or gc_rows.shape[0] != n or gc_rows.shape[1] < 1):
        raise RuntimeError(f"observe_grad_reduce: gc_rows has shape {tuple(gc_rows.shape)}, expected [{n}, C >= 1]")
    C = 0 if gc_rows is None else int(gc_rows.shape[1])
    if row_of.dtype != torch.int32 or row_of.numel() != B * K or not row_of.is_contiguous() or row_of.device != dev:
        raise RuntimeError(f"observe_grad_reduce: row_of must be a contiguous int32 tensor of {B * K} elements on {dev}")
    if B > 0 and int(row_of.max()) >= n:
        raise RuntimeError(f"observe_grad_reduce: row_of points at row {int(row_of.max())}, gx_rows has {n} rows")
    if tuple(noise_std.shape) == (D,):
        stride = 0
    elif tuple(noise_std.shape) == (B, D):
        stride = D
    else:
        raise RuntimeError(f"observe_grad_reduce: noise_std has shape {tuple(noise_std.shape)}, expected [{D}] or [{B}, {D}]")
    if grad_x is None:
        grad_x = torch.empty(B, D, dtype=torch.float32, device=dev)
    if grad_c is None and gc_rows is not None:
        grad_c = torch.empty(B, C, dtype=torch.float32, device=dev)
    if grad_noise_std is None and want_noise_grad:
        grad_noise_std = torch.empty(B, D, dtype=torch.float32, device=dev)
    for t, name, cols in ((grad_x, "grad_x", D), (grad_c, "grad_c", C), (grad_noise_std, "grad_noise_std", D)):
        if t is not None and t.numel() != B * cols:
            raise RuntimeError(f"observe_grad_reduce: {name} has {t.numel()} elements for [{B}, {cols}]")
    if n == 0:                                              # nothing was kept: no row is read, but the pointer is mandatory
        gx_rows = torch.zeros(1, D, dtype=torch.float32, device=dev)
        gc_rows = None if gc_rows is None else torch.zeros(1, C, dtype=torch.float32, device=dev)
    ptrs = (_chk(lp, "lp", dev), _chk(gx_rows, "gx_rows", dev), _chk(gc_rows, "gc_rows", dev), _chk(noise_std, "noise_std", dev),
            _chk(grad_x, "grad_x", dev), _chk(grad_c if gc_rows is not None else None, "grad_c", dev),
            _chk(grad_noise_std, "grad_noise_std", dev))
    if B == 0:
        return grad_x, grad_c, grad_noise_std
    L = lib()
    rc = _on_stream(dev, L.ff_observe_grad_reduce, L.ff_observe_grad_reduce_host,
                    (ptrs[0], row_of.data_ptr(), ptrs[1], ptrs[2], ptrs[3], stride, B, D, C, K, int(seed) & 0xFFFFFFFFFFFFFFFF,
                     int(sample_offset), ptrs[4], ptrs[5], ptrs[6]))
    if rc != FF_OK:
        raise _err(rc, "ff_observe_grad_reduce")
    return grad_x, grad_c, grad_noise_std


def _std_stride(noise_std: torch.Tensor, B: int, D: int, what: str) -> int:
    """std_row_stride of a ``noise_std`` [D] (0) or [B, D] (D)."""
    if tuple(noise_std.shape) == (D,):
        return 0
    if tuple(noise_std.shape) == (B, D):
        return D
    raise RuntimeError(f"{what}: noise_std has shape {tuple(noise_std.shape)}, expected [{D}] or [{B}, {D}]")


def marginal_observe_expand(x: torch.Tensor, noise_std: torch.Tensor, num_draws: int, seed: int, sample_offset: int = 0,
                            shift: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
                            cond: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """ff_marginal_observe_expand: (z0 [B K, 2 D], cond_out [B K, C] or None) from ``x`` [B, D]: row r K + k is
    [((x[r] - noise_std[r] * z_k) - shift) / scale | momentum k] and the (already normalised) ``cond[r]``, noise draw k and
    momentum k both of global row sample_offset + r (noise indices OBS_NOISE_BASE + k and MOMENTUM_NOISE_BASE + k).
    ``noise_std``: [D] (one vector for every row) or [B, D].  Device tensors on the current stream; CPU tensors go to
    ff_marginal_observe_expand_host."""
    dev = x.device
    if x.dim() != 2 or x.shape[1] < 1:
        raise RuntimeError(f"marginal_observe_expand: x has shape {tuple(x.shape)}, expected [B, D >= 1]")
    B, D = x.shape
    K = int(num_draws)
    if not 1 <= K <= min(MAX_MOMENTA, MAX_OBS_DRAWS):
        raise ValueError(f"num_draws={num_draws}: 1 .. {min(MAX_MOMENTA, MAX_OBS_DRAWS)} joint draws per data point")
    stride = _std_stride(noise_std, B, D, "marginal_observe_expand")
    for t, name in ((shift, "shift"), (scale, "scale")):
        if t is not None and t.numel() != D:
            raise RuntimeError(f"marginal_observe_expand: {name} has {t.numel()} elements, x has {D} columns")
    if cond is not None and (cond.dim() != 2 or cond.shape[0] != B or cond.shape[1] < 1):
        raise RuntimeError(f"marginal_observe_expand: cond has shape {tuple(cond.shape)}, expected [{B}, C >= 1]")
    C = 0 if cond is None else int(cond.shape[1])
    z0 = torch.empty(B * K, 2 * D, dtype=torch.float32, device=dev)
    cond_out = None if cond is None else torch.empty(B * K, C, dtype=torch.float32, device=dev)
    ptrs = (_chk(x, "x", dev), _chk(noise_std, "noise_std", dev), _chk(shift, "shift", dev), _chk(scale, "scale", dev),
            _chk(cond, "cond", dev))
    if B == 0:
        return z0, cond_out
    L = lib()
    rc = _on_stream(dev, L.ff_marginal_observe_expand, L.ff_marginal_observe_expand_host,
                    (ptrs[0], ptrs[1], stride, ptrs[2], ptrs[3], ptrs[4], B, D, C, K, int(seed) & 0xFFFFFFFFFFFFFFFF,
                     int(sample_offset), z0.data_ptr(), 0 if cond is None else cond_out.data_ptr()))
    if rc != FF_OK:
        raise _err(rc, "ff_marginal_observe_expand")
    return z0, cond_out


def marginal_observe_grad_reduce(lw: torch.Tensor, row_of: torch.Tensor, gz_rows: torch.Tensor, gc_rows: Optional[torch.Tensor],
                                 noise_std: torch.Tensor, num_draws: int, seed: int, sample_offset: int = 0,
                                 scale: Optional[torch.Tensor] = None, cond_scale: Optional[torch.Tensor] = None,
                                 want_noise_grad: bool = True, grad_x: Optional[torch.Tensor] = None,
                                 grad_c: Optional[torch.Tensor] = None, grad_noise_std: Optional[torch.Tensor] = None):
    """ff_marginal_observe_grad_reduce: ``(grad_x [B, D], grad_c [B, C] or None, grad_noise_std [B, D] or None)``:
    ``grad_x`` and ``grad_c`` bit for bit what ``marginal_grad_reduce`` writes for the same ``lw`` [B K] float64, ``row_of``
    [B K] int32, ``gz_rows`` [n, 2 D], ``gc_rows`` [n, C], ``scale`` and ``cond_scale``, and ``grad_noise_std = -sum_k wn_k z_k
    gz_rows[row_of[r K + k]][:D] / scale`` with the noise draws regenerated from ``seed`` and global row ``sample_offset + r``.
    ``noise_std`` [D] or [B, D] as ``marginal_observe_expand`` took it (its values are not read).  ``row_of`` is checked here
    to stay below n.  The outputs are allocated where not given.  Device tensors on the current stream; CPU tensors go to
    ff_marginal_observe_grad_reduce_host."""
    dev = lw.device
    K = int(num_draws)
    what = "marginal_observe_grad_reduce"
    if not 1 <= K <= min(MAX_MOMENTA, MAX_OBS_DRAWS):
        raise ValueError(f"num_draws={num_draws}: 1 .. {min(MAX_MOMENTA, MAX_OBS_DRAWS)} joint draws per data point")
    if lw.dtype != torch.float64 or lw.dim() != 1 or lw.numel() % K or not lw.is_contiguous():
        raise RuntimeError(f"{what}: lw must be a contiguous float64 tensor [B * {K}], got {lw.dtype} {tuple(lw.shape)}")
    B = lw.numel() // K
    if gz_rows.dim() != 2 or gz_rows.shape[1] % 2 or gz_rows.shape[1] < 2:
        raise RuntimeError(f"{what}: gz_rows has shape {tuple(gz_rows.shape)}, expected [n, 2 D]")
    n, D = int(gz_rows.shape[0]), int(gz_rows.shape[1]) // 2
    if gc_rows is not None and (gc_rows.dim() != 2 or gc_rows.shape[0] != n or gc_rows.shape[1] < 1):
        raise RuntimeError(f"{what}: gc_rows has shape {tuple(gc_rows.shape)}, expected [{n}, C >= 1]")
    C = 0 if gc_rows is None else int(gc_rows.shape[1])
    if row_of.dtype != torch.int32 or row_of.numel() != B * K or not row_of.is_contiguous() or row_of.device != dev:
        raise RuntimeError(f"{what}: row_of must be a contiguous int32 tensor of {B * K} elements on {dev}")
    if B > 0 and int(row_of.max()) >= n:
        raise RuntimeError(f"{what}: row_of points at row {int(row_of.max())}, gz_rows has {n} rows")
    stride = _std_stride(noise_std, B, D, what)
    if gc_rows is None:
        cond_scale = None
    for t, name, cols in ((scale, "scale", D), (cond_scale, "cond_scale", C)):
        if t is not None and t.numel() != cols:
            raise RuntimeError(f"{what}: {name} has {t.numel()} elements for {cols} columns")
    if grad_x is None:
        grad_x = torch.empty(B, D, dtype=torch.float32, device=dev)
    if grad_c is None and gc_rows is not None:
        grad_c = torch.empty(B, C, dtype=torch.float32, device=dev)
    if grad_noise_std is None and want_noise_grad:
        grad_noise_std = torch.empty(B, D, dtype=torch.float32, device=dev)
    for t, name, cols in ((grad_x, "grad_x", D), (grad_c, "grad_c", C), (grad_noise_std, "grad_noise_std", D)):
        if t is not None and t.numel() != B * cols:
            raise RuntimeError(f"{what}: {name} has {t.numel()} elements for [{B}, {cols}]")
    if n == 0:                                              # nothing was kept: no row is read, but the pointer is mandatory
        gz_rows = torch.zeros(1, 2 * D, dtype=torch.float32, device=dev)
        gc_rows = None if gc_rows is None else torch.zeros(1, C, dtype=torch.float32, device=dev)
    ptrs = (_chk(gz_rows, "gz_rows", dev), _chk(gc_rows, "gc_rows", dev), _chk(scale, "scale", dev),
            _chk(cond_scale, "cond_scale", dev), _chk(noise_std, "noise_std", dev), _chk(grad_x, "grad_x", dev),
            _chk(grad_c if gc_rows is not None else None, "grad_c", dev), _chk(grad_noise_std, "grad_noise_std", dev))
    if B == 0:
        return grad_x, grad_c, grad_noise_std
    L = lib()
    rc = _on_stream(dev, L.ff_marginal_observe_grad_reduce, L.ff_marginal_observe_grad_reduce_host,
                    (lw.data_ptr(), row_of.data_ptr(), ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], stride, B, D, C, K,
                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_offset), ptrs[5], ptrs[6], ptrs[7]))
    if rc != FF_OK:
        raise _err(rc, "ff_marginal_observe_grad_reduce")
    return grad_x, grad_c, grad_noise_std


def marginal_observe_resample(x: torch.Tensor, noise_std: torch.Tensor, lw: torch.Tensor, num_draws: int, num_samples: int,
                              seed: int, sample_offset: int = 0, samples: Optional[torch.Tensor] = None,
                              index: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None,
                              var: Optional[torch.Tensor] = None):
    """ff_marginal_observe_resample: ``(samples [B, M, D], index [B, M] int32, mean [B, D], var [B, D])``, the posterior of
    every observation ``x`` [B, D] from the K = ``num_draws`` joint draws of its noisy marginal: M = ``num_samples``
    multinomial draws of the candidates ``x[r] - noise_std[r] * z_k`` by the weights ``exp(lw - max lw)`` (``lw`` [B K]
    float64, ``marginal_weigh``'s), and their weighted mean and variance, in double.  No particle buffer: the candidates are
    regenerated from ``seed`` and global row ``sample_offset + r`` (noise indices OBS_NOISE_BASE + k), the uniforms are
    ``weighted_resample``'s.  ``noise_std``: [D] or [B, D], as ``marginal_observe_expand`` took it.  The outputs are allocated
    where not given.  Device tensors on the current stream; CPU tensors go to ff_marginal_observe_resample_host."""
    dev = x.device
    what = "marginal_observe_resample"
    if x.dim() != 2 or x.shape[1] < 1:
        raise RuntimeError(f"{what}: x has shape {tuple(x.shape)}, expected [B, D >= 1]")
    B, D = x.shape
    K, M = int(num_draws), int(num_samples)
    if not 1 <= K <= min(MAX_MOMENTA, MAX_OBS_DRAWS):
        raise ValueError(f"num_draws={num_draws}: 1 .. {min(MAX_MOMENTA, MAX_OBS_DRAWS)} joint draws per data point")
    if not 0 <= M <= MAX_OBS_SAMPLES:
        raise ValueError(f"num_samples={num_samples}: 0 .. {MAX_OBS_SAMPLES} posterior draws per data point")
    stride = _std_stride(noise_std, B, D, what)
    if lw.dtype != torch.float64 or lw.dim() != 1 or lw.numel() != B * K or not lw.is_contiguous() or lw.device != dev:
        raise RuntimeError(f"{what}: lw must be a contiguous float64 tensor [{B} * {K}] on {dev}, got {lw.dtype} "
                           f"{tuple(lw.shape)} on {lw.device}")
    if samples is None:
        samples = torch.empty(B, M, D, dtype=torch.float32, device=dev)
    if index is None:
        index = torch.empty(B, M, dtype=torch.int32, device=dev)
    if mean is None:
        mean = torch.empty(B, D, dtype=torch.float32, device=dev)
    if var is None:
        var = torch.empty(B, D, dtype=torch.float32, device=dev)
    for t, name, n in ((samples, "samples", B * M * D), (index, "index", B * M), (mean, "mean", B * D), (var, "var", B * D)):
        if t.numel() != n:
            raise RuntimeError(f"{what}: {name} has {t.numel()} elements, expected {n}")
    if index.dtype != torch.int32 or index.device != dev or not index.is_contiguous():
        raise RuntimeError(f"{what}: index must be a contiguous int32 tensor on {dev}")
    ptrs = (_chk(x, "x", dev), _chk(noise_std, "noise_std", dev), _chk(samples, "samples", dev), _chk(mean, "mean", dev),
            _chk(var, "var", dev))
    if B == 0:
        return samples, index, mean, var
    L = lib()
    rc = _on_stream(dev, L.ff_marginal_observe_resample, L.ff_marginal_observe_resample_host,
                    (ptrs[0], ptrs[1], stride, lw.data_ptr(), B, D, K, M, int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_offset),
                     ptrs[2], index.data_ptr(), ptrs[3], ptrs[4]))
    if rc != FF_OK:
        raise _err(rc, "ff_marginal_observe_resample")
    return samples, index, mean, var


def trace_kind_and_probes(kind: str, probes):
    """(FF_TRACE_*, probes0, probes1, r, m) from ``kind`` ("hutchpp": probes = (S, G); "xtrace": probes = (O,)), each
    probe tensor [n, B, D] as the reference stores them (diffusion.py:708-719)."""
    if kind == "hutchpp":
        S, G = probes
        return TRACE_HUTCHPP, S, G, int(S.shape[0]), int(G.shape[0])
    if kind == "xtrace":
        (O,) = probes
        return TRACE_XTRACE, O, None, int(O.shape[0]), 0
    raise ValueError(f"trace estimator {kind!r}: expected 'hutchpp' or 'xtrace'")


def trace_estimate(jac: torch.Tensor, kind: str, probes, host: bool = False) -> torch.Tensor:
    """ff_trace_estimate: Hutch++ / XTrace divergence estimates [n_rows, B] from recorded Jacobians ``jac``
    [n_rows, B, D, D] (A = J^T per evaluation row and sample) in ONE launch; ``host=True`` runs the same arithmetic on CPU
    tensors through ff_trace_estimate_host (tests without a GPU)."""
    n_rows, B, D, D2 = jac.shape
    code, p0, p1, r, m = trace_kind_and_probes(kind, probes)
    if D != D2 or tuple(p0.shape) != (r, B, D) or (p1 is not None and tuple(p1.shape) != (m, B, D)):
        raise RuntimeError(f"trace_estimate: jac {tuple(jac.shape)} and probes {tuple(p0.shape)} do not match")
    dev = jac.device
    if host != (dev.type == "cpu"):
        raise RuntimeError("flowfusion_amd: ff_trace_estimate works on device memory (host=True: CPU tensors, tests only)")
    jac, p0, p1 = f32_on(jac, dev), f32_on(p0, dev), f32_on(p1, dev)
    out = torch.empty(n_rows, B, dtype=torch.float32, device=dev)
    items = 1 if host else n_rows * B
    ws = torch.empty(max(1, int(lib().ff_trace_workspace_floats(code, D, r, items))), dtype=torch.float32, device=dev)
    a = TraceArgs()
    a.kind, a.dim, a.n_rows, a.r, a.m, a.batch = code, D, n_rows, r, m, B
    a.jac, a.probes0, a.probes1 = jac.data_ptr(), p0.data_ptr(), (0 if p1 is None else p1.data_ptr())
    a.out, a.workspace = out.data_ptr(), ws.data_ptr()
    if host:
        rc = lib().ff_trace_estimate_host(ctypes.byref(a))
    else:
        with torch.cuda.device(dev):
            rc = lib().ff_trace_estimate(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != FF_OK:
        raise _err(rc, "ff_trace_estimate")
    return out


def _trace_prod(second: bool, kind: str, probes, y, basis, rfac, prod, host: bool):
    """The one call behind ``trace_basis`` / ``trace_combine``: checks the layouts of ff_trace_prod_args, allocates what the
    launch writes, runs it on torch's current stream (``host``: the _host twin on CPU tensors)."""
    code, p0, p1, r, m = trace_kind_and_probes(kind, probes)
    K2 = r + m if code == TRACE_HUTCHPP else r
    lead = y if not second else prod
    what = "ff_trace_combine" if second else "ff_trace_basis"
    if lead.dim() != 4:
        raise RuntimeError(f"{what}: products [n_rows, B, K, D], got {tuple(lead.shape)}")
    n_rows, B, _, D = lead.shape
    if tuple(lead.shape) != (n_rows, B, K2 if second else r, D) or tuple(p0.shape) != (r, B, D) or \
            (p1 is not None and tuple(p1.shape) != (m, B, D)):
        raise RuntimeError(f"{what}: products {tuple(lead.shape)} and probes {tuple(p0.shape)} do not match")
    dev = lead.device
    if host != (dev.type == "cpu"):
        raise RuntimeError(f"flowfusion_amd: {what} works on device memory (host=True: CPU tensors, tests only)")
    lead, p0, p1 = f32_on(lead, dev), f32_on(p0, dev), f32_on(p1, dev)
    if second:
        basis, rfac = f32_on(basis, dev), f32_on(rfac, dev)
        if tuple(basis.shape) != (n_rows, B, K2, D) or (code == TRACE_XTRACE and (rfac is None or tuple(rfac.shape) != (n_rows, B, r, r))):
            raise RuntimeError(f"{what}: basis {tuple(basis.shape)} does not match products {tuple(lead.shape)}")
        out = torch.empty(n_rows, B, dtype=torch.float32, device=dev)
    else:
        basis = torch.empty(n_rows, B, K2, D, dtype=torch.float32, device=dev)
        rfac = torch.empty(n_rows, B, r, r, dtype=torch.float32, device=dev) if code == TRACE_XTRACE else None
        out = None
    items = 1 if host else n_rows * B
    ws = torch.empty(max(1, int(lib().ff_trace_prod_workspace_floats(code, D, r, items))), dtype=torch.float32, device=dev)
    a = TraceProdArgs()
    a.kind, a.dim, a.n_rows, a.r, a.m, a.batch = code, D, n_rows, r, m, B
    a.probes0, a.probes1 = p0.data_ptr(), (0 if p1 is None else p1.data_ptr())
    a.basis, a.rfac, a.workspace = basis.data_ptr(), (0 if rfac is None else rfac.data_ptr()), ws.data_ptr()
    if second:
        a.prod, a.out = lead.data_ptr(), out.data_ptr()
    else:
        a.y = lead.data_ptr()
    if host:
        rc = (lib().ff_trace_combine_host if second else lib().ff_trace_basis_host)(ctypes.byref(a))
    else:
        with torch.cuda.device(dev):
            rc = (lib().ff_trace_combine if second else lib().ff_trace_basis)(
                ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != FF_OK:
        raise _err(rc, what)
    return out if second else (basis, rfac)


def trace_basis(y: torch.Tensor, kind: str, probes, host: bool = False):
    """ff_trace_basis: from the first sweep's products ``y`` [n_rows, B, r, D] (``A p_c`` for the sketch probes S / O of
    ``probes``, laid out as for ``trace_estimate``) the second sweep's seeds ``basis`` [n_rows, B, K2, D] -- Hutch++:
    ``q_0 .. q_{r-1}, u_0 .. u_{m-1}``, K2 = r + m; XTrace: ``q_0 .. q_{r-1}``, K2 = r -- and ``rfac`` [n_rows, B, r, r]
    (XTrace; else None).  ``host=True``: CPU tensors through ff_trace_basis_host (tests without a GPU)."""
    return _trace_prod(False, kind, probes, y, None, None, None, host)


def trace_combine(basis: torch.Tensor, rfac: Optional[torch.Tensor], prod: torch.Tensor, kind: str, probes,
                  host: bool = False) -> torch.Tensor:
    """ff_trace_combine: the Hutch++ / XTrace estimates [n_rows, B] from ``trace_basis``'s output and the second sweep's
    products ``prod`` [n_rows, B, K2, D] = ``A basis``: ``trace_estimate``'s arithmetic with every matrix-vector product
    read instead of summed.  ``host=True``: ff_trace_combine_host."""
    return _trace_prod(True, kind, probes, None, basis, rfac, prod, host)


_norm_ws = {}     # (device index, stream) -> (workspace, out) of ff_scaled_rms


def scaled_rms(terms, atol: float, rtol: float, check: Optional[torch.Tensor] = None, read: bool = True):
    """ff_scaled_rms: ``terms`` = up to 3 tuples (num, sub or None, scale0, scale1 or None) of equal-sized fp32 device
    tensors; returns [rms_0, .., rms_{n-1}, nonfinite(check)] as Python floats -- one launch, one read-back (the single
    host synchronisation of an attempted step under the host controller).  ``read=False`` returns the device tensor the
    kernel wrote instead (no synchronisation; valid until the next call on this stream)."""
    dev = terms[0][0].device
    if dev.type != "cuda":
        raise RuntimeError("flowfusion_amd: ff_scaled_rms works on device memory (there is no CPU path)")
    if not 1 <= len(terms) <= NORM_TERMS:
        raise RuntimeError(f"scaled_rms: 1..{NORM_TERMS} terms")
    arr = (NormTerm * NORM_TERMS)()
    keep = []
    for i, (num, sub, s0, s1) in enumerate(terms):
        for t in (num, sub, s0, s1):
            if t is not None and t.numel() != num.numel():
                raise RuntimeError("scaled_rms: the arrays of a term differ in size")
        arr[i].num, arr[i].sub = _chk(num, "num", dev), _chk(sub, "sub", dev)
        arr[i].scale0, arr[i].scale1 = _chk(s0, "scale0", dev), _chk(s1, "scale1", dev)
        arr[i].n = num.numel()
        keep.append((num, sub, s0, s1))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        ws, out = norm_workspace(dev, stream)
        rc = lib().ff_scaled_rms(arr, len(terms), float(atol), float(rtol), _chk(check, "check", dev),
                                 0 if check is None else check.numel(), out.data_ptr(), ws.data_ptr(), ctypes.c_void_p(stream))
    if rc != FF_OK:
        ws[:4].zero_()      # whatever happened to the launch, the arrival counter starts the next one from zero
        raise _err(rc, "ff_scaled_rms")
    return out[: len(terms) + 1].tolist() if read else out[: len(terms) + 1]


def norm_workspace(dev, stream: int):
    """(workspace, out) of the norm reductions for this device and stream: the kernels leave the arrival counter at
    zero, so sequential launches on one stream share a workspace (ff_scaled_rms, the adaptive controller)."""
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (index, stream)
    if key not in _norm_ws:
        nbytes = int(lib().ff_scaled_rms_workspace_bytes())
        _norm_ws[key] = (torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=dev),
                         torch.empty(NORM_TERMS + 1, dtype=torch.float32, device=dev))
    return _norm_ws[key]


_PLAN_WORDS = ctypes.sizeof(PlanStruct) // 4


def _plan_from_words(words: List[int]) -> PlanStruct:
    return PlanStruct.from_buffer_copy((ctypes.c_int32 * _PLAN_WORDS)(*words[:_PLAN_WORDS]))


def _slots_hint(words: List[int]) -> int:
    """ff_ode_args.stage_slots travelling behind the plan's words (0 = unknown)."""
    return int(words[_PLAN_WORDS]) if len(words) > _PLAN_WORDS else 0


def plan_words(plan: PlanStruct, stage_slots: int = 0) -> List[int]:
    """The plan as 32-bit words (how it travels through the custom op's integer-list argument), followed by the number of
    stage slots the launch's table uses (ff_ode_args.stage_slots; 0 = unknown)."""
    return list((ctypes.c_int32 * _PLAN_WORDS).from_buffer_copy(plan)) + [int(stage_slots)]


def _chk(t: Optional[torch.Tensor], name: str, dev) -> int:
    if t is None:
        return 0
    if t.device != dev:
        raise RuntimeError(f"{name} is on {t.device}, expected {dev}")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous float32")
    return t.data_ptr()


def probe_count(probe: Optional[torch.Tensor]) -> int:
    """ff_ode_args.tangent_count of a Hutchinson launch with this probe: K for [B, K, D], 0 (one probe) for [B, D] / None."""
    return int(probe.shape[1]) if probe is not None and probe.dim() == 3 else 0


def _chk_probe(probe: Optional[torch.Tensor], B: int, D: int, mode: int, tangent_count: int) -> None:
    """The probe's shape: [B, D], or [B, K, D] in MODE_HUTCH with tangent_count = K (ff_ode_args.tangent_count)."""
    if probe is None:
        return
    K = max(int(tangent_count), 1) if mode == MODE_HUTCH else 1
    want = (B, K, D) if (probe.dim() == 3 or K > 1) else (B, D)
    if tuple(probe.shape) != want:
        raise RuntimeError(f"probe has shape {tuple(probe.shape)}, expected {want}" +
                           (f" (tangent_count={tangent_count})" if len(want) == 3 else ""))


def f32_on(t: Optional[torch.Tensor], dev) -> Optional[torch.Tensor]:
    """``t`` (or None) detached, on ``dev``, contiguous float32: the form in which every C call takes a tensor."""
    return None if t is None else t.detach().to(dev, torch.float32).contiguous()


# the caller's tensors among the ff_ode_args fields -> the name the ops' signatures (and so _chk's messages) give each
_ARG_NAMES = {"x_in": "x", "cond": "cond", "probe": "probe", "noise": "noise", "wpack": "wpack", "etab": "etab",
              "in_shift": "in_shift", "in_scale": "in_scale", "out_scale": "out_scale", "out_shift": "out_shift",
              "k1_in": "k1", "kl1_in": "kl1", "dlogp_in": "dlogp0", "jac_out": "jac"}      # (mlp_ode_push: probe = its `tangents`)
_AuxPtrs = ctypes.c_void_p * MAX_AUX


def _row_ptrs(t: torch.Tensor) -> ctypes.Array:
    """ff_ode_args.aux_out / aux_lp_out: the addresses of t[0], t[1], .. of a contiguous fp32 tensor the op allocated
    (NULL throughout for one without elements: the state-only modes' aux_lp)."""
    if t.numel() == 0:
        return _AuxPtrs()
    step = t.numel() // t.shape[0] * 4
    return _AuxPtrs(*range(t.data_ptr(), t.data_ptr() + t.shape[0] * step, step))


def _launch_ode(p: PlanStruct, dev, tensors: dict, per_probe: Optional[torch.Tensor] = None, push=None, pull=None, vjp=None,
                record=None, discrete=None, logp_grad=None, pull_select=None, push_select=None, **fields) -> None:
    """The one launch of the twelve ops below, on torch's current stream of ``dev``: ff_mlp_ode_launch,
    ff_mlp_ode_launch_probes where the op allocated a ``per_probe`` [B, K] buffer, ff_mlp_ode_launch_push with
    ``push = (cond_tangents [B, K, C] or None, tangent_out [B, K, D])`` (ff_mlp_ode_launch_push_select with the same pair as
    ``push_select``, on a push-select plan), ff_mlp_ode_launch_pull with
    ``pull = (cotangents [B, K, D], cot_x_out [B, K, D], cot_cond_out [B, K, C] or None)``, or ff_mlp_ode_launch_vjp with
    ``vjp = (seeds, seed_row_stride, prod_out [n_evals, B, K, D])``, ff_mlp_ode_launch_record with ``record = record_out
    [n_evals, B, D]``, or ff_mlp_ode_launch_pull_discrete with ``discrete = (record [n_evals, B, D], cotangents [B, K, D],
    cot_x_out [B, K, D], cot_cond_out [B, K, C] or None)``, or ff_mlp_ode_launch_logp_grad with ``logp_grad = (record, probes
    [B, D], weight [B] or None, cotangent [B, D], grad_x_out [B, D], grad_cond_out [B, C] or None)``.  ``tensors``: the caller's
    tensors (or None) by ff_ode_args field name, each checked by ``_chk``; ``fields``: the scalar fields and the addresses
    of what the op allocated itself.  A field named in neither stays zero."""
    a = OdeArgs(**fields)
    for field, t in tensors.items():
        if t is not None:
            setattr(a, field, _chk(t, _ARG_NAMES[field], dev))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if record is not None:
            what = "ff_mlp_ode_launch_record"
            rc = lib().ff_mlp_ode_launch_record(ctypes.byref(p), ctypes.byref(a), _chk(record, "record_out", dev),
                                                ctypes.c_void_p(stream))
        elif logp_grad is not None:
            what = "ff_mlp_ode_launch_logp_grad"
            rc = lib().ff_mlp_ode_launch_logp_grad(ctypes.byref(p), ctypes.byref(a), _chk(logp_grad[0], "record", dev),
                                                   _chk(logp_grad[1], "probes", dev), _chk(logp_grad[2], "weight", dev),
                                                   _chk(logp_grad[3], "cotangent", dev), _chk(logp_grad[4], "grad_x_out", dev),
                                                   _chk(logp_grad[5], "grad_cond_out", dev), ctypes.c_void_p(stream))
        elif discrete is not None:
            what = "ff_mlp_ode_launch_pull_discrete"
            rc = lib().ff_mlp_ode_launch_pull_discrete(ctypes.byref(p), ctypes.byref(a), _chk(discrete[0], "record", dev),
                                                       _chk(discrete[1], "cotangents", dev), _chk(discrete[2], "cot_x_out", dev),
                                                       _chk(discrete[3], "cot_cond_out", dev), ctypes.c_void_p(stream))
        elif vjp is not None:
            what = "ff_mlp_ode_launch_vjp"
            rc = lib().ff_mlp_ode_launch_vjp(ctypes.byref(p), ctypes.byref(a), _chk(vjp[0], "seeds", dev), int(vjp[1]),
                                             _chk(vjp[2], "prod_out", dev), ctypes.c_void_p(stream))
        elif pull_select is not None:       # (pull's triple, on a pull-select plan)
            what = "ff_mlp_ode_launch_pull_select"
            rc = lib().ff_mlp_ode_launch_pull_select(ctypes.byref(p), ctypes.byref(a), _chk(pull_select[0], "cotangents", dev),
                                                     _chk(pull_select[1], "cot_x_out", dev), _chk(pull_select[2], "cot_cond_out", dev),
                                                     ctypes.c_void_p(stream))
        elif pull is not None:
            what = "ff_mlp_ode_launch_pull"
            rc = lib().ff_mlp_ode_launch_pull(ctypes.byref(p), ctypes.byref(a), _chk(pull[0], "cotangents", dev),
                                              _chk(pull[1], "cot_x_out", dev), _chk(pull[2], "cot_cond_out", dev),
                                              ctypes.c_void_p(stream))
        elif push_select is not None:       # (push's pair, on a push-select plan)
            what = "ff_mlp_ode_launch_push_select"
            rc = lib().ff_mlp_ode_launch_push_select(ctypes.byref(p), ctypes.byref(a), _chk(push_select[0], "cond_tangents", dev),
                                                     _chk(push_select[1], "tangent_out", dev), ctypes.c_void_p(stream))
        elif push is not None:
            what = "ff_mlp_ode_launch_push"
            rc = lib().ff_mlp_ode_launch_push(ctypes.byref(p), ctypes.byref(a), _chk(push[0], "cond_tangents", dev),
                                              _chk(push[1], "tangent_out", dev), ctypes.c_void_p(stream))
        elif per_probe is None:
            what = "ff_mlp_ode_launch"
            rc = lib().ff_mlp_ode_launch(ctypes.byref(p), ctypes.byref(a), ctypes.c_void_p(stream))
        else:
            what = "ff_mlp_ode_launch_probes"
            rc = lib().ff_mlp_ode_launch_probes(ctypes.byref(p), ctypes.byref(a), _chk(per_probe, "per_probe", dev),
                                                ctypes.c_void_p(stream))
    if rc != FF_OK:
        raise _err(rc, what)


@torch.library.custom_op("flowfusion_amd::mlp_ode", mutates_args=())
def mlp_ode(x: torch.Tensor, cond: Optional[torch.Tensor], probe: Optional[torch.Tensor],
            noise: Optional[torch.Tensor], wpack: torch.Tensor, etab: torch.Tensor,
            in_shift: Optional[torch.Tensor], in_scale: Optional[torch.Tensor],
            out_scale: Optional[torch.Tensor], out_shift: Optional[torch.Tensor],
            plan: List[int], mode: int, tangent_first: int = 0, tangent_count: int = 0,
            rng_seed: int = 0, rng_sample_offset: int = 0, rng_noise_base: int = 0
            ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Fused integration on the GPU: returns (final state [B,D], integrated divergence [B], status[1]).
    With `noise=None`, rows flagged FF_ROW_NOISE draw their normals in the kernel (Philox4x32-10 keyed by
    `rng_seed` and the global sample index `rng_sample_offset + row`; see ff_ode_args)."""
    if not x.is_cuda:
        raise RuntimeError("flowfusion_amd::mlp_ode needs tensors on the GPU (there is no CPU path)")
    dev = x.device
    p = _plan_from_words(plan)
    B, D = x.shape
    if D != p.dim:
        raise RuntimeError(f"state has {D} columns, plan was made for {p.dim}")
    x_out = torch.empty_like(x)
    dlogp = torch.zeros(B if mode != MODE_STATE else 0, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if B == 0:                      # nothing to integrate (zero-size tensors have no storage to point at)
        return x_out, dlogp, status
    if cond is not None and tuple(cond.shape) != (B, p.cond_dim):
        raise RuntimeError(f"cond has shape {tuple(cond.shape)}, expected {(B, p.cond_dim)}")
    _chk_probe(probe, B, D, mode, tangent_count)
    if etab.shape[1] != 32 + row_width(p):
        raise RuntimeError("evaluation table width does not match the plan")
    _launch_ode(p, dev, {"x_in": x, "cond": cond, "probe": probe, "noise": noise, "wpack": wpack, "etab": etab,
                         "in_shift": in_shift, "in_scale": in_scale, "out_scale": out_scale, "out_shift": out_shift},
                x_out=x_out.data_ptr(), dlogp_out=dlogp.data_ptr() if mode != MODE_STATE else 0, status=status.data_ptr(),
                batch=B, noise_stride=B * D, n_evals=etab.shape[0], mode=mode,
                tangent_first=tangent_first, tangent_count=tangent_count, rng_seed=rng_seed & 0xFFFFFFFFFFFFFFFF,
                rng_sample_offset=rng_sample_offset, rng_noise_base=rng_noise_base, stage_slots=_slots_hint(plan))
    return x_out, dlogp, status


@mlp_ode.register_fake
def _(x, cond, probe, noise, wpack, etab, in_shift, in_scale, out_scale, out_shift, plan, mode,
      tangent_first=0, tangent_count=0, rng_seed=0, rng_sample_offset=0, rng_noise_base=0):
    B = x.shape[0]
    return (torch.empty_like(x), x.new_empty(B if mode != MODE_STATE else 0),
            torch.empty(1, dtype=torch.int32, device=x.device))


@torch.library.custom_op("flowfusion_amd::mlp_ode_probes", mutates_args=())
def mlp_ode_probes(x: torch.Tensor, cond: Optional[torch.Tensor], probe: torch.Tensor, wpack: torch.Tensor,
                   etab: torch.Tensor, in_shift: Optional[torch.Tensor], in_scale: Optional[torch.Tensor],
                   out_scale: Optional[torch.Tensor], out_shift: Optional[torch.Tensor], plan: List[int],
                   tangent_count: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``mlp_ode`` in MODE_HUTCH with the divergence of every probe on its own (ff_mlp_ode_launch_probes): returns (final
    state [B, D], integrated divergence [B], per-probe divergences [B, K], status [1]), K = max(1, tangent_count); the
    first two are bitwise ``mlp_ode``'s, row k of the third is the integral of p_k^T J p_k for probe k as given."""
    if not x.is_cuda:
        raise RuntimeError("flowfusion_amd::mlp_ode_probes needs tensors on the GPU (there is no CPU path)")
    dev = x.device
    p = _plan_from_words(plan)
    B, D = x.shape
    if D != p.dim:
        raise RuntimeError(f"state has {D} columns, plan was made for {p.dim}")
    K = max(int(tangent_count), 1)
    x_out = torch.empty_like(x)
    dlogp = torch.zeros(B, dtype=torch.float32, device=dev)
    per_probe = torch.zeros(B, K, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if B == 0:
        return x_out, dlogp, per_probe, status
    if cond is not None and tuple(cond.shape) != (B, p.cond_dim):
        raise RuntimeError(f"cond has shape {tuple(cond.shape)}, expected {(B, p.cond_dim)}")
    _chk_probe(probe, B, D, MODE_HUTCH, tangent_count)
    if etab.shape[1] != 32 + row_width(p):
        raise RuntimeError("evaluation table width does not match the plan")
    _launch_ode(p, dev, {"x_in": x, "cond": cond, "probe": probe, "wpack": wpack, "etab": etab,
                         "in_shift": in_shift, "in_scale": in_scale, "out_scale": out_scale, "out_shift": out_shift},
                per_probe=per_probe, x_out=x_out.data_ptr(), dlogp_out=dlogp.data_ptr(), status=status.data_ptr(),
                batch=B, n_evals=etab.shape[0], mode=MODE_HUTCH, tangent_count=tangent_count,
                stage_slots=_slots_hint(plan))
    return x_out, dlogp, per_probe, status


@mlp_ode_probes.register_fake
def _(x, cond, probe, wpack, etab, in_shift, in_scale, out_scale, out_shift, plan, tangent_count=0):
    B = x.shape[0]
    return (torch.empty_like(x), x.new_empty(B), x.new_empty(B, max(int(tangent_count), 1)),
            torch.empty(1, dtype=torch.int32, device=x.device))


@torch.library.custom_op("flowfusion_amd::mlp_ode_push", mutates_args=())
def mlp_ode_push(x: torch.Tensor, cond: Optional[torch.Tensor], tangents: Optional[torch.Tensor],
                 cond_tangents: Optional[torch.Tensor], wpack: torch.Tensor, etab: torch.Tensor,
                 in_shift: Optional[torch.Tensor], in_scale: Optional[torch.Tensor], out_scale: Optional[torch.Tensor],
                 out_shift: Optional[torch.Tensor], plan: List[int], unit: bool, tangent_first: int,
                 tangent_count: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The fused fixed-grid solve with K = ``tangent_count`` tangents per sample pushed through it
    (ff_mlp_ode_launch_push): returns (final state [B, D], tangent_out [B, K, D], status [1]) with
    ``tangent_out[b, k] = d x_out[b] / d (x[b], cond[b]) . (v_k, c_k)``, the derivative of the discrete solver map.
    ``unit=False``: v = ``tangents`` [B, K, D] (None = zero), c = ``cond_tangents`` [B, K, C] (None = zero).
    ``unit=True``: the unit vectors ``tangent_first .. tangent_first + K - 1`` of the combined space [0, D + C)."""
    if not x.is_cuda:
        raise RuntimeError("flowfusion_amd::mlp_ode_push needs tensors on the GPU (there is no CPU path)")
    dev = x.device
    p = _plan_from_words(plan)
    B, D = x.shape
    K = int(tangent_count)
    if D != p.dim:
        raise RuntimeError(f"state has {D} columns, plan was made for {p.dim}")
    if K < 1:
        raise RuntimeError(f"tangent_count={tangent_count}: at least one tangent per sample")
    x_out = torch.empty_like(x)
    t_out = torch.empty(B, K, D, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if B == 0:
        return x_out, t_out, status
    if cond is not None and tuple(cond.shape) != (B, p.cond_dim):
        raise RuntimeError(f"cond has shape {tuple(cond.shape)}, expected {(B, p.cond_dim)}")
    if unit and (tangents is not None or cond_tangents is not None):
        raise RuntimeError("unit tangents take no tangent buffers")
    if tangents is not None and tuple(tangents.shape) != (B, K, D):
        raise RuntimeError(f"tangents has shape {tuple(tangents.shape)}, expected {(B, K, D)}")
    if cond_tangents is not None and tuple(cond_tangents.shape) != (B, K, p.cond_dim):
        raise RuntimeError(f"cond_tangents has shape {tuple(cond_tangents.shape)}, expected {(B, K, p.cond_dim)}")
    if etab.shape[1] != 32 + row_width(p):
        raise RuntimeError("evaluation table width does not match the plan")
    _launch_ode(p, dev, {"x_in": x, "cond": cond, "probe": tangents, "wpack": wpack, "etab": etab,
                         "in_shift": in_shift, "in_scale": in_scale, "out_scale": out_scale, "out_shift": out_shift},
                push=(cond_tangents, t_out), x_out=x_out.data_ptr(), status=status.data_ptr(), batch=B,
                n_evals=etab.shape[0], mode=MODE_EXACT if unit else MODE_HUTCH, tangent_first=tangent_first if unit else 0,
                tangent_count=K, stage_slots=_slots_hint(plan))
    return x_out, t_out, status


@mlp_ode_push.register_fake
def _(x, cond, tangents, cond_tangents, wpack, etab, in_shift, in_scale, out_scale, out_shift, plan, unit, tangent_first,
      tangent_count):
    return (torch.empty_like(x), x.new_empty(x.shape[0], int(tangent_count), x.shape[1]),
            torch.empty(1, dtype=torch.int32, device=x.device))


@torch.library.custom_op("flowfusion_amd::mlp_ode_push_select", mutates_args=())
def mlp_ode_push_select(x: torch.Tensor, cond: Optional[torch.Tensor], tangents: Optional[torch.Tensor],
                        cond_tangents: Optional[torch.Tensor], wpack: torch.Tensor, etab: torch.Tensor,
                        in_shift: Optional[torch.Tensor], in_scale: Optional[torch.Tensor], out_scale: Optional[torch.Tensor],
                        out_shift: Optional[torch.Tensor], plan: List[int], unit: bool, tangent_first: int,
                        tangent_count: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The fused push-forward through select rows (ff_mlp_ode_launch_push_select) over the rows ``etab`` of a leapfrog grid, from
    the joint state ``x`` [B, 2D]: returns what ``mlp_ode_push`` returns -- (final state [B, 2D], tangent_out [B, K, 2D], status
    [1]) -- with ``tangent_out[b, k] = d x_out[b] / d (x[b], cond[b]) . (v_k, c_k)``, the derivative of the discrete leapfrog.
    ``unit`` / ``tangents`` / ``cond_tangents`` as there.  ``wpack``: the push-select plan's two forward packs
    (``pack_push_select_weights``)."""
    if not x.is_cuda:
        raise RuntimeError("flowfusion_amd::mlp_ode_push_select needs tensors on the GPU (there is no CPU path)")
    dev = x.device
    p = _plan_from_words(plan)
    if not is_push_select_plan(p):
        raise RuntimeError("flowfusion_amd::mlp_ode_push_select needs a push-select plan")
    B, D = x.shape
    K = int(tangent_count)
    if D != p.dim:
        raise RuntimeError(f"state has {D} columns, plan was made for {p.dim}")
    if K < 1:
        raise RuntimeError(f"tangent_count={tangent_count}: at least one tangent per sample")
    x_out = torch.empty_like(x)
    t_out = torch.empty(B, K, D, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if B == 0:
        return x_out, t_out, status
    if cond is not None and tuple(cond.shape) != (B, p.cond_dim):
        raise RuntimeError(f"cond has shape {tuple(cond.shape)}, expected {(B, p.cond_dim)}")
    if unit and (tangents is not None or cond_tangents is not None):
        raise RuntimeError("unit tangents take no tangent buffers")
    if tangents is not None and tuple(tangents.shape) != (B, K, D):
        raise RuntimeError(f"tangents has shape {tuple(tangents.shape)}, expected {(B, K, D)}")
    if cond_tangents is not None and tuple(cond_tangents.shape) != (B, K, p.cond_dim):
        raise RuntimeError(f"cond_tangents has shape {tuple(cond_tangents.shape)}, expected {(B, K, p.cond_dim)}")
    if etab.shape[1] != 32 + row_width(p):
        raise RuntimeError("evaluation table width does not match the plan")
    _launch_ode(p, dev, {"x_in": x, "cond": cond, "probe": tangents, "wpack": wpack, "etab": etab,
                         "in_shift": in_shift, "in_scale": in_scale, "out_scale": out_scale, "out_shift": out_shift},
                push_select=(cond_tangents, t_out), x_out=x_out.data_ptr(), status=status.data_ptr(), batch=B,
                n_evals=etab.shape[0], mode=MODE_EXACT if unit else MODE_HUTCH, tangent_first=tangent_first if unit else 0,
                tangent_count=K, stage_slots=_slots_hint(plan))
    return x_out, t_out, status


@mlp_ode_push_select.register_fake
def _(x, cond, tangents, cond_tangents, wpack, etab, in_shift, in_scale, out_scale, out_shift, plan, unit, tangent_first,
      tangent_count):
    return (torch.empty_like(x), x.new_empty(x.shape[0], int(tangent_count), x.shape[1]),
            torch.empty(1, dtype=torch.int32, device=x.device))


@torch.library.custom_op("flowfusion_amd::mlp_ode_pull", mutates_args=())
def mlp_ode_pull(x: torch.Tensor, cond: Optional[torch.Tensor], cotangents: torch.Tensor, wpack: torch.Tensor, etab: torch.Tensor,
                 in_shift: Optional[torch.Tensor], in_scale: Optional[torch.Tensor], out_scale: Optional[torch.Tensor],
                 out_shift: Optional[torch.Tensor], plan: List[int], want_cond: bool
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The fused continuous-adjoint solve (ff_mlp_ode_launch_pull) over the rows ``etab`` of the REVERSED span, from
    ``x`` = the forward solve's result: returns (retraced state [B, D], cot_x [B, K, D], cot_cond [B, K, C] -- [B, K, 0]
    unless ``want_cond`` --, status [1]) with ``cot_x[b, k] = cotangents[b, k]^T d x[b] / d (retraced state[b])`` and
    ``cot_cond[b, k]`` likewise for ``cond[b]``.  ``wpack``: the pull plan's two packs (``pack_weights``)."""
    if not x.is_cuda:
        raise RuntimeError("flowfusion_amd::mlp_ode_pull needs tensors on the GPU (there is no CPU path)")
    dev = x.device
    p = _plan_from_words(plan)
    B, D = x.shape
    if D != p.dim:
        raise RuntimeError(f"state has {D} columns, plan was made for {p.dim}")
    if cotangents.dim() != 3 or cotangents.shape[0] != B or cotangents.shape[2] != D or cotangents.shape[1] < 1:
        raise RuntimeError(f"cotangents has shape {tuple(cotangents.shape)}, expected [{B}, K >= 1, {D}]")
    K = int(cotangents.shape[1])
    C = int(p.cond_dim) if want_cond else 0
    if want_cond and p.cond_dim == 0:
        raise RuntimeError("want_cond on a plan without conditional inputs")
    x_out = torch.empty_like(x)
    gx = torch.empty(B, K, D, dtype=torch.float32, device=dev)
    gc = torch.empty(B, K, C, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if B == 0:
        return x_out, gx, gc, status
    if cond is not None and tuple(cond.shape) != (B, p.cond_dim):
        raise RuntimeError(f"cond has shape {tuple(cond.shape)}, expected {(B, p.cond_dim)}")
    if etab.shape[1] != 32 + row_width(p):
        raise RuntimeError("evaluation table width does not match the plan")
    _launch_ode(p, dev, {"x_in": x, "cond": cond, "wpack": wpack, "etab": etab,
                         "in_shift": in_shift, "in_scale": in_scale, "out_scale": out_scale, "out_shift": out_shift},
                pull=(cotangents, gx, gc if want_cond else None), x_out=x_out.data_ptr(), status=status.data_ptr(), batch=B,
                n_evals=etab.shape[0], mode=MODE_HUTCH, tangent_count=K, stage_slots=_slots_hint(plan))
    return x_out, gx, gc, status


@mlp_ode_pull.register_fake
def _(x, cond, cotangents, wpack, etab, in_shift, in_scale, out_scale, out_shift, plan, want_cond):
    B, K = x.shape[0], cotangents.shape[1]
    C = _plan_from_words(plan).cond_dim if want_cond else 0
    return (torch.empty_like(x), x.new_empty(B, K, x.shape[1]), x.new_empty(B, K, C),
            torch.empty(1, dtype=torch.int32, device=x.device))


@torch.library.custom_op("flowfusion_amd::mlp_ode_pull_select", mutates_args=())
def mlp_ode_pull_select(x: torch.Tensor, cond: Optional[torch.Tensor], cotangents: torch.Tensor, wpack: torch.Tensor, etab: torch.Tensor,
                        in_shift: Optional[torch.Tensor], in_scale: Optional[torch.Tensor], out_scale: Optional[torch.Tensor],
                        out_shift: Optional[torch.Tensor], plan: List[int], want_cond: bool
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The fused pull-back through select rows (ff_mlp_ode_launch_pull_select) over the rows ``etab`` of the REVERSED leapfrog
    grid, from ``x`` = the forward leapfrog's result [B, 2D]: returns what ``mlp_ode_pull`` returns -- (retraced state, cot_x
    [B, K, 2D], cot_cond [B, K, C] ([B, K, 0] unless ``want_cond``), status [1]) -- with ``cot_x`` / ``cot_cond`` the exact
    transpose of the forward leapfrog.  ``wpack``: the pull-select plan's two pull packs (``pack_pull_select_weights``)."""
    if not x.is_cuda:
        raise RuntimeError("flowfusion_amd::mlp_ode_pull_select needs tensors on the GPU (there is no CPU path)")
    dev = x.device
    p = _plan_from_words(plan)
    if not is_pull_select_plan(p):
        raise RuntimeError("flowfusion_amd::mlp_ode_pull_select needs a pull-select plan")
    B, D = x.shape
    if D != p.dim:
        raise RuntimeError(f"state has {D} columns, plan was made for {p.dim}")
    if cotangents.dim() != 3 or cotangents.shape[0] != B or cotangents.shape[2] != D or cotangents.shape[1] < 1:
        raise RuntimeError(f"cotangents has shape {tuple(cotangents.shape)}, expected [{B}, K >= 1, {D}]")
    K = int(cotangents.shape[1])
    C = int(p.cond_dim) if want_cond else 0
    if want_cond and p.cond_dim == 0:
        raise RuntimeError("want_cond on a plan without conditional inputs")
    x_out = torch.empty_like(x)
    gx = torch.empty(B, K, D, dtype=torch.float32, device=dev)
    gc = torch.empty(B, K, C, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if B == 0:
        return x_out, gx, gc, status
    if cond is not None and tuple(cond.shape) != (B, p.cond_dim):
        raise RuntimeError(f"cond has shape {tuple(cond.shape)}, expected {(B, p.cond_dim)}")
    if etab.shape[1] != 32 + row_width(p):
        raise RuntimeError("evaluation table width does not match the plan")
    _launch_ode(p, dev, {"x_in": x, "cond": cond, "wpack": wpack, "etab": etab,
                         "in_shift": in_shift, "in_scale": in_scale, "out_scale": out_scale, "out_shift": out_shift},
                pull_select=(cotangents, gx, gc if want_cond else None), x_out=x_out.data_ptr(), status=status.data_ptr(), batch=B,
                n_evals=etab.shape[0], mode=MODE_HUTCH, tangent_count=K, stage_slots=_slots_hint(plan))
    return x_out, gx, gc, status


@mlp_ode_pull_select.register_fake
def _(x, cond, cotangents, wpack, etab, in_shift, in_scale, out_scale, out_shift, plan, want_cond):
    B, K = x.shape[0], cotangents.shape[1]
    C = _plan_from_words(plan).cond_dim if want_cond else 0
    return (torch.empty_like(x), x.new_empty(B, K, x.shape[1]), x.new_empty(B, K, C),
            torch.empty(1, dtype=torch.int32, device=x.device))


@torch.library.custom_op("flowfusion_amd::mlp_ode_vjp_products", mutates_args=())
def mlp_ode_vjp_products(x: torch.Tensor, cond: Optional[torch.Tensor], seeds: torch.Tensor, wpack: torch.Tensor, etab: torch.Tensor,
                         in_shift: Optional[torch.Tensor], in_scale: Optional[torch.Tensor], out_scale: Optional[torch.Tensor],
                         out_shift: Optional[torch.Tensor], plan: List[int]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The fused fixed-grid solve of the state over the (forward) rows ``etab`` with K products per evaluation row
    (ff_mlp_ode_launch_vjp): returns (x_out [B, D], prod [n_evals, B, K, D], status [1]) with
    ``prod[e, b, k] = a_e seed + b_e J_net(y_e)^T seed`` at the stage state ``y_e`` of row e.  ``seeds`` [B, K, D]: the same
    seeds on every row; [n_evals, B, K, D]: seeds per row.  ``plan`` / ``wpack``: the PULL plan and its two packs."""
    if not x.is_cuda:
        raise RuntimeError("flowfusion_amd::mlp_ode_vjp_products needs tensors on the GPU (there is no CPU path)")
    dev = x.device
    p = _plan_from_words(plan)
    B, D = x.shape
    n = int(etab.shape[0])
    if D != p.dim:
        raise RuntimeError(f"state has {D} columns, plan was made for {p.dim}")
    per_row = seeds.dim() == 4
    if seeds.dim() not in (3, 4) or tuple(seeds.shape[-3::2]) != (B, D) or seeds.shape[-2] < 1 or (per_row and seeds.shape[0] != n):
        raise RuntimeError(f"seeds has shape {tuple(seeds.shape)}, expected [{B}, K >= 1, {D}] or [{n}, {B}, K >= 1, {D}]")
    K = int(seeds.shape[-2])
    x_out = torch.empty_like(x)
    prod = torch.empty(n, B, K, D, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if B == 0:
        return x_out, prod, status
    if cond is not None and tuple(cond.shape) != (B, p.cond_dim):
        raise RuntimeError(f"cond has shape {tuple(cond.shape)}, expected {(B, p.cond_dim)}")
    if etab.shape[1] != 32 + row_width(p):
        raise RuntimeError("evaluation table width does not match the plan")
    _launch_ode(p, dev, {"x_in": x, "cond": cond, "wpack": wpack, "etab": etab,
                         "in_shift": in_shift, "in_scale": in_scale, "out_scale": out_scale, "out_shift": out_shift},
                vjp=(seeds, B * K * D if per_row else 0, prod), x_out=x_out.data_ptr(), status=status.data_ptr(), batch=B,
                n_evals=n, mode=MODE_HUTCH, tangent_count=K, stage_slots=_slots_hint(plan))
    return x_out, prod, status


@mlp_ode_vjp_products.register_fake
def _(x, cond, seeds, wpack, etab, in_shift, in_scale, out_scale, out_shift, plan):
    return (torch.empty_like(x), x.new_empty(etab.shape[0], x.shape[0], seeds.shape[-2], x.shape[1]),
            torch.empty(1, dtype=torch.int32, device=x.device))


@torch.library.custom_op("flowfusion_amd::mlp_ode_record", mutates_args=())
def mlp_ode_record(x: torch.Tensor, cond: Optional[torch.Tensor], wpack: torch.Tensor, etab: torch.Tensor,
                   in_shift: Optional[torch.Tensor], in_scale: Optional[torch.Tensor], out_scale: Optional[torch.Tensor],
                   out_shift: Optional[torch.Tensor], plan: List[int]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The fused fixed-grid solve of the state over the (forward) rows ``etab`` that writes every stage state down
    (ff_mlp_ode_launch_record): returns (x_out [B, D], record [n_evals, B, D], status [1]) with ``record[e, b]`` = the stage
    state y_e of row e in the integrated state's units (after the input map).  ``plan`` / ``wpack``: the PULL plan and its
    two packs."""
    if not x.is_cuda:
        raise RuntimeError("flowfusion_amd::mlp_ode_record needs tensors on the GPU (there is no CPU path)")
    dev = x.device
    p = _plan_from_words(plan)
    B, D = x.shape
    n = int(etab.shape[0])
    if D != p.dim:
        raise RuntimeError(f"state has {D} columns, plan was made for {p.dim}")
    x_out = torch.empty_like(x)
    rec = torch.empty(n, B, D, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if B == 0:
        return x_out, rec, status
    if cond is not None and tuple(cond.shape) != (B, p.cond_dim):
        raise RuntimeError(f"cond has shape {tuple(cond.shape)}, expected {(B, p.cond_dim)}")
    if etab.shape[1] != 32 + row_width(p):
        raise RuntimeError("evaluation table width does not match the plan")
    _launch_ode(p, dev, {"x_in": x, "cond": cond, "wpack": wpack, "etab": etab,
                         "in_shift": in_shift, "in_scale": in_scale, "out_scale": out_scale, "out_shift": out_shift},
                record=rec, x_out=x_out.data_ptr(), status=status.data_ptr(), batch=B, n_evals=n, mode=MODE_STATE,
                stage_slots=_slots_hint(plan))
    return x_out, rec, status


@mlp_ode_record.register_fake
def _(x, cond, wpack, etab, in_shift, in_scale, out_scale, out_shift, plan):
    return (torch.empty_like(x), x.new_empty(etab.shape[0], x.shape[0], x.shape[1]),
            torch.empty(1, dtype=torch.int32, device=x.device))


@torch.library.custom_op("flowfusion_amd::mlp_ode_pull_discrete", mutates_args=())
def mlp_ode_pull_discrete(record: torch.Tensor, cond: Optional[torch.Tensor], cotangents: torch.Tensor, wpack: torch.Tensor,
                          etab: torch.Tensor, in_shift: Optional[torch.Tensor], in_scale: Optional[torch.Tensor],
                          out_scale: Optional[torch.Tensor], out_shift: Optional[torch.Tensor], plan: List[int], want_cond: bool
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The exact discrete adjoint (ff_mlp_ode_launch_pull_discrete): the transposed row program of the FORWARD rows ``etab``,
    run backwards over ``record`` [n_evals, B, D] (``mlp_ode_record`` of the same table, cond and maps).  Returns (cot_x
    [B, K, D], cot_cond [B, K, C] -- [B, K, 0] unless ``want_cond`` --, status [1]) with ``cot_x[b, k] = cotangents[b, k]^T
    d x_out[b] / d x[b]`` of the discrete solver map and ``cot_cond[b, k]`` likewise for ``cond[b]``."""
    if not record.is_cuda:
        raise RuntimeError("flowfusion_amd::mlp_ode_pull_discrete needs tensors on the GPU (there is no CPU path)")
    dev = record.device
    p = _plan_from_words(plan)
    n = int(etab.shape[0])
    if record.dim() != 3 or record.shape[0] != n or record.shape[2] != p.dim:
        raise RuntimeError(f"record has shape {tuple(record.shape)}, expected [{n}, B, {p.dim}]")
    B, D = int(record.shape[1]), int(record.shape[2])
    if cotangents.dim() != 3 or cotangents.shape[0] != B or cotangents.shape[2] != D or cotangents.shape[1] < 1:
        raise RuntimeError(f"cotangents has shape {tuple(cotangents.shape)}, expected [{B}, K >= 1, {D}]")
    K = int(cotangents.shape[1])
    C = int(p.cond_dim) if want_cond else 0
    if want_cond and p.cond_dim == 0:
        raise RuntimeError("want_cond on a plan without conditional inputs")
    gx = torch.empty(B, K, D, dtype=torch.float32, device=dev)
    gc = torch.empty(B, K, C, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if B == 0:
        return gx, gc, status
    if cond is not None and tuple(cond.shape) != (B, p.cond_dim):
        raise RuntimeError(f"cond has shape {tuple(cond.shape)}, expected {(B, p.cond_dim)}")
    if etab.shape[1] != 32 + row_width(p):
        raise RuntimeError("evaluation table width does not match the plan")
    _launch_ode(p, dev, {"cond": cond, "wpack": wpack, "etab": etab,
                         "in_shift": in_shift, "in_scale": in_scale, "out_scale": out_scale, "out_shift": out_shift},
                discrete=(record, cotangents, gx, gc if want_cond else None), status=status.data_ptr(), batch=B,
                n_evals=n, mode=MODE_HUTCH, tangent_count=K, stage_slots=_slots_hint(plan))
    return gx, gc, status


@mlp_ode_pull_discrete.register_fake
def _(record, cond, cotangents, wpack, etab, in_shift, in_scale, out_scale, out_shift, plan, want_cond):
    B, K = record.shape[1], cotangents.shape[1]
    C = _plan_from_words(plan).cond_dim if want_cond else 0
    return (record.new_empty(B, K, record.shape[2]), record.new_empty(B, K, C),
            torch.empty(1, dtype=torch.int32, device=record.device))


@torch.library.custom_op("flowfusion_amd::mlp_ode_logp_grad", mutates_args=())
def mlp_ode_logp_grad(record: torch.Tensor, cond: Optional[torch.Tensor], probes: torch.Tensor, weight: Optional[torch.Tensor],
                      cotangent: torch.Tensor, wpack: torch.Tensor, etab: torch.Tensor, in_shift: Optional[torch.Tensor],
                      in_scale: Optional[torch.Tensor], out_scale: Optional[torch.Tensor], out_shift: Optional[torch.Tensor],
                      plan: List[int], want_cond: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The gradient of a fixed-grid Hutchinson log-density (ff_mlp_ode_launch_logp_grad): the transposed row program of the
    FORWARD rows ``etab`` with the divergence integral in it, run backwards over ``record`` [n_evals, B, D] (``mlp_ode_record``
    of the same table, cond and maps).  ``probes`` [B, D]: each row's probe; ``weight`` [B] or None (= 1): the cotangent of its
    divergence integral; ``cotangent`` [B, D]: that of its final state.  Returns (grad_x [B, D], grad_cond [B, C] -- [B, 0]
    unless ``want_cond`` --, status [1])."""
    if not record.is_cuda:
        raise RuntimeError("flowfusion_amd::mlp_ode_logp_grad needs tensors on the GPU (there is no CPU path)")
    dev = record.device
    p = _plan_from_words(plan)
    n = int(etab.shape[0])
    if record.dim() != 3 or record.shape[0] != n or record.shape[2] != p.dim:
        raise RuntimeError(f"record has shape {tuple(record.shape)}, expected [{n}, B, {p.dim}]")
    B, D = int(record.shape[1]), int(record.shape[2])
    for name, t in (("probes", probes), ("cotangent", cotangent)):
        if tuple(t.shape) != (B, D):
            raise RuntimeError(f"{name} has shape {tuple(t.shape)}, expected {(B, D)}")
    if weight is not None and tuple(weight.shape) != (B,):
        raise RuntimeError(f"weight has shape {tuple(weight.shape)}, expected {(B,)}")
    C = int(p.cond_dim) if want_cond else 0
    if want_cond and p.cond_dim == 0:
        raise RuntimeError("want_cond on a plan without conditional inputs")
    gx = torch.empty(B, D, dtype=torch.float32, device=dev)
    gc = torch.empty(B, C, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if B == 0:
        return gx, gc, status
    if cond is not None and tuple(cond.shape) != (B, p.cond_dim):
        raise RuntimeError(f"cond has shape {tuple(cond.shape)}, expected {(B, p.cond_dim)}")
    if etab.shape[1] != 32 + row_width(p):
        raise RuntimeError("evaluation table width does not match the plan")
    _launch_ode(p, dev, {"cond": cond, "wpack": wpack, "etab": etab,
                         "in_shift": in_shift, "in_scale": in_scale, "out_scale": out_scale, "out_shift": out_shift},
                logp_grad=(record, probes, weight, cotangent, gx, gc if want_cond else None), status=status.data_ptr(), batch=B,
                n_evals=n, mode=MODE_HUTCH, tangent_count=1, stage_slots=_slots_hint(plan))
    return gx, gc, status


@mlp_ode_logp_grad.register_fake
def _(record, cond, probes, weight, cotangent, wpack, etab, in_shift, in_scale, out_scale, out_shift, plan, want_cond):
    B = record.shape[1]
    C = _plan_from_words(plan).cond_dim if want_cond else 0
    return (record.new_empty(B, record.shape[2]), record.new_empty(B, C), torch.empty(1, dtype=torch.int32, device=record.device))


@torch.library.custom_op("flowfusion_amd::mlp_ode_step", mutates_args=())
def mlp_ode_step(x: torch.Tensor, cond: Optional[torch.Tensor], probe: Optional[torch.Tensor],
                 k1: Optional[torch.Tensor], kl1: Optional[torch.Tensor], dlogp0: Optional[torch.Tensor],
                 wpack: torch.Tensor, etab: torch.Tensor, plan: List[int], mode: int, n_aux: int,
                 tangent_first: int = 0, tangent_count: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """One attempt of an embedded Runge-Kutta step (adaptive solvers): the evaluation rows of `etab`
    fill the stage slots (slot 0 preloaded from `k1`/`kl1`), and `n_aux` linear combinations of the
    slots, described by the two trailing rows of `etab`, are returned: (aux [n_aux, B, D],
    aux_lp [n_aux, B])."""
    if not x.is_cuda:
        raise RuntimeError("flowfusion_amd::mlp_ode_step needs tensors on the GPU (there is no CPU path)")
    dev = x.device
    p = _plan_from_words(plan)
    B, D = x.shape
    aux = torch.empty(n_aux, B, D, dtype=torch.float32, device=dev)
    aux_lp = torch.zeros(n_aux, B if mode != MODE_STATE else 0, dtype=torch.float32, device=dev)
    if B == 0:
        return aux, aux_lp
    scratch = torch.empty_like(x)
    dl = torch.empty(B if mode != MODE_STATE else 0, dtype=torch.float32, device=dev)
    n_evals = etab.shape[0] - 2
    if etab.shape[1] != 32 + row_width(p) or n_evals < 0:
        raise RuntimeError("evaluation table does not match the plan")
    _chk_probe(probe, B, D, mode, tangent_count)
    _launch_ode(p, dev, {"x_in": x, "cond": cond, "probe": probe, "wpack": wpack, "etab": etab,
                         "k1_in": k1, "kl1_in": kl1, "dlogp_in": dlogp0},
                x_out=scratch.data_ptr(), dlogp_out=dl.data_ptr() if mode != MODE_STATE else 0,
                batch=B, n_evals=n_evals, mode=mode, tangent_first=tangent_first, tangent_count=tangent_count,
                aux_out=_row_ptrs(aux), aux_lp_out=_row_ptrs(aux_lp), n_aux=n_aux, stage_slots=_slots_hint(plan))
    return aux, aux_lp


@mlp_ode_step.register_fake
def _(x, cond, probe, k1, kl1, dlogp0, wpack, etab, plan, mode, n_aux, tangent_first=0, tangent_count=0):
    B = x.shape[0]
    return (x.new_empty(n_aux, B, x.shape[1]), x.new_empty(n_aux, B if mode != MODE_STATE else 0))


@torch.library.custom_op("flowfusion_amd::mlp_rhs_jac", mutates_args=("jac",))
def mlp_rhs_jac(x: torch.Tensor, cond: Optional[torch.Tensor], wpack: torch.Tensor, etab: torch.Tensor,
                plan: List[int], tangent_first: int, tangent_count: int, jac: torch.Tensor) -> torch.Tensor:
    """One right-hand-side evaluation with its Jacobian (ff_ode_args.jac_out): `etab` is one evaluation row
    followed by the two auxiliary rows; returns rhs [B, D] and fills rows [tangent_first, +count) of
    ``jac[b, j, i] = d rhs_i / d y_j``."""
    if not x.is_cuda:
        raise RuntimeError("flowfusion_amd::mlp_rhs_jac needs tensors on the GPU (there is no CPU path)")
    dev = x.device
    p = _plan_from_words(plan)
    B, D = x.shape
    rhs = torch.empty_like(x)
    if B == 0:
        return rhs
    if tuple(jac.shape) != (B, D, D) or etab.shape[0] != 3 or etab.shape[1] != 32 + row_width(p):
        raise RuntimeError("mlp_rhs_jac: jac must be [B, D, D] and etab one evaluation row + two auxiliary rows")
    scratch = torch.empty_like(x)
    dl = torch.empty(B, dtype=torch.float32, device=dev)
    _launch_ode(p, dev, {"x_in": x, "cond": cond, "wpack": wpack, "etab": etab, "jac_out": jac},
                x_out=scratch.data_ptr(), dlogp_out=dl.data_ptr(), batch=B, n_evals=1, mode=MODE_EXACT,
                tangent_first=tangent_first, tangent_count=tangent_count, aux_out=_AuxPtrs(rhs.data_ptr()), n_aux=1)
    return rhs


@mlp_rhs_jac.register_fake
def _(x, cond, wpack, etab, plan, tangent_first, tangent_count, jac):
    return torch.empty_like(x)


@torch.library.custom_op("flowfusion_amd::mlp_ode_jacobians", mutates_args=("jac",))
def mlp_ode_jacobians(x: torch.Tensor, cond: Optional[torch.Tensor], wpack: torch.Tensor, etab: torch.Tensor,
                      plan: List[int], tangent_first: int, tangent_count: int, jac: torch.Tensor) -> torch.Tensor:
    """Integrate a whole fixed-grid table in exact mode and record the Jacobian of EVERY evaluation row
    (ff_ode_args.jac_all): fills rows [tangent_first, +count) of ``jac[e, b, j, i] = d rhs_i / d y_j`` and returns the
    final state [B, D].  The state does not depend on the divergence, so the estimators that need per-evaluation
    Jacobians (Hutch++, XTrace) can run after the fact, for all rows at once."""
    if not x.is_cuda:
        raise RuntimeError("flowfusion_amd::mlp_ode_jacobians needs tensors on the GPU (there is no CPU path)")
    dev = x.device
    p = _plan_from_words(plan)
    B, D = x.shape
    x_out = torch.empty_like(x)
    if B == 0:
        return x_out
    n_evals = etab.shape[0]
    if tuple(jac.shape) != (n_evals, B, D, D) or etab.shape[1] != 32 + row_width(p):
        raise RuntimeError("mlp_ode_jacobians: jac must be [n_evals, B, D, D] and etab must match the plan")
    dl = torch.empty(B, dtype=torch.float32, device=dev)
    _launch_ode(p, dev, {"x_in": x, "cond": cond, "wpack": wpack, "etab": etab, "jac_out": jac},
                x_out=x_out.data_ptr(), dlogp_out=dl.data_ptr(), batch=B, n_evals=n_evals, mode=MODE_EXACT,
                tangent_first=tangent_first, tangent_count=tangent_count, jac_all=1)
    return x_out


@mlp_ode_jacobians.register_fake
def _(x, cond, wpack, etab, plan, tangent_first, tangent_count, jac):
    return torch.empty_like(x)
