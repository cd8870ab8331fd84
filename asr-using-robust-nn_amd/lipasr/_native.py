"""ctypes binding of liblipasr.so (include/lipasr.h).

The product has no CPU fallback: if the shared library is missing, importing this module raises.
Device memory, streams and process groups come from PyTorch (plumbing); every arithmetic step on
the hot path goes through the C ABI below.
"""
from __future__ import annotations

import ctypes as C
import os

# PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).  It must be
# in the process BEFORE liblipasr.so is opened so that liblipasr's DT_NEEDED libamdhip64.so.7 resolves to
# that same copy: two HIP runtimes in one process cannot both own the device ("no ROCm-capable device").
import torch  # noqa: F401  (plumbing: device memory, streams, process groups)

from . import knobs

_HERE = os.path.dirname(os.path.abspath(__file__))
# LIPASR_LIBRARY: another build of the same library (A/B timing of kernel changes); never a different backend
LIB_PATH = knobs.get("LIPASR_LIBRARY") or os.path.join(_HERE, "liblipasr.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build it with `python asr-using-robust-nn_amd/build.py` "
        "(or __graft_entry__.build()).  lipasr has no CPU fallback."
    )

lib = C.CDLL(LIB_PATH)

OK, EINVAL, ENOMEM, EHIP, EUNSUPPORTED, ESTATE = 0, -1, -2, -3, -4, -5
MAX_LAYERS = 16
SEG_W, SEG_B, SEG_GAMMA, SEG_BETA, SEG_MMEAN, SEG_MVAR = range(6)

c_f = C.c_void_p  # device float*
c_h = C.c_void_p
c_s = C.c_void_p
i32 = C.c_int
f32 = C.c_float
u64 = C.c_uint64
sz = C.c_size_t
PI = C.POINTER(C.c_int)
PV = C.POINTER(C.c_void_p)


class DropoutCfg(C.Structure):
    _fields_ = [("mode", C.c_int), ("seed", C.c_uint64), ("step_dev", C.c_void_p), ("masks", PV)]


# name -> (restype, argtypes); mirrors include/lipasr.h line by line
PROTOTYPES = {
    "lipasr_version": (i32, []),
    "lipasr_last_error": (C.c_char_p, []),
    "lipasr_create": (i32, [i32, C.POINTER(c_h)]),
    "lipasr_destroy": (i32, [c_h]),
    "lipasr_timer_create": (i32, [c_h, PI]),
    "lipasr_timer_start": (i32, [c_h, i32, c_s]),
    "lipasr_timer_stop": (i32, [c_h, i32, c_s]),
    "lipasr_timer_elapsed_ms": (i32, [c_h, i32, C.POINTER(f32)]),
    "lipasr_graph_begin": (i32, [c_h, c_s]),
    "lipasr_graph_end": (i32, [c_h, c_s, PI]),
    "lipasr_graph_launch": (i32, [c_h, i32, c_s]),
    "lipasr_stream_create_masked": (i32, [c_h, C.POINTER(C.c_uint32), i32, C.POINTER(c_s)]),
    "lipasr_stream_destroy": (i32, [c_h, c_s]),
    "lipasr_graph_destroy": (i32, [c_h, i32]),
    "lipasr_sigma_max": (i32, [c_h, c_f, i32, i32, c_f, i32, i32, i32, c_f, c_s]),
    "lipasr_project_per_layer": (i32, [c_h, PV, PI, PI, i32, f32, c_f, i32, i32, c_f, c_s]),
    "lipasr_project_product": (i32, [c_h, PV, PI, PI, i32, f32, PI, i32, c_f, c_s]),
    "lipasr_product_norm": (i32, [c_h, PV, PI, PI, i32, c_f, c_s]),
    "lipasr_frobenius_project": (i32, [c_h, c_f, sz, f32, c_s]),
    "lipasr_bn_correction": (i32, [c_h, c_f, c_f, i32, c_f, c_s]),
    "lipasr_sv_clip": (i32, [c_h, c_f, i32, i32, f32, c_f, c_f, c_s]),
    "lipasr_sign_step": (i32, [c_h, c_f, c_f, c_f, sz, f32, f32, c_s]),
    "lipasr_lp_step": (i32, [c_h, c_f, c_f, c_f, i32, i32, f32, f32, f32, c_s]),
    "lipasr_lp_ball_init": (i32, [c_h, c_f, c_f, i32, i32, f32, f32, u64, c_f, i32, c_s]),
    "lipasr_scaler_fit": (i32, [c_h, c_f, i32, i32, c_f, c_f, c_s]),
    "lipasr_scaler_apply": (i32, [c_h, c_f, i32, i32, c_f, c_f, c_f, c_s]),
    "lipasr_gemm_f32": (i32, [c_h, i32, i32, i32, i32, i32, c_f, i32, c_f, i32, c_f, i32, c_s]),
    "lipasr_gemm_f16x2": (i32, [c_h, i32, i32, i32, i32, i32, c_f, i32, c_f, i32, c_f, i32, f32, f32, c_s]),
    "lipasr_mlp_create": (i32, [c_h, i32, PI, PI, C.POINTER(f32), PI, i32, C.POINTER(c_h)]),
    "lipasr_mlp_destroy": (i32, [c_h]),
    "lipasr_mlp_sizes": (i32, [c_h, C.POINTER(sz), C.POINTER(sz)]),
    "lipasr_mlp_segment": (i32, [c_h, i32, i32, C.POINTER(sz), C.POINTER(sz)]),
    "lipasr_mlp_train_fwd_bwd": (i32, [c_h, c_f, c_f, c_f, c_f, i32, f32, C.POINTER(DropoutCfg), c_f, c_f, c_f, c_f, c_s]),
    "lipasr_mlp_train_fwd_bwd_head": (i32, [c_h, c_f, c_f, c_f, c_f, i32, f32, C.POINTER(DropoutCfg), c_f, c_f, c_f, c_f, c_s]),
    "lipasr_mlp_train_dw0": (i32, [c_h, c_f, i32, c_f, c_s]),
    "lipasr_mlp_train_fwd": (i32, [c_h, c_f, c_f, c_f, i32, C.POINTER(DropoutCfg), c_f, c_s]),
    "lipasr_mlp_train_bwd": (i32, [c_h, c_f, c_f, c_f, i32, f32, C.POINTER(DropoutCfg), c_f, c_s]),
    "lipasr_mlp_grad_split": (i32, [c_h, C.POINTER(sz)]),
    "lipasr_mlp_train_segments": (i32, [c_h, PI]),
    "lipasr_mlp_train_segment_exchange": (i32, [c_h, i32, i32, C.POINTER(sz)]),
    "lipasr_mlp_part_floats": (i32, [c_h, C.POINTER(sz)]),
    "lipasr_mlp_train_segment": (i32, [c_h, i32, c_f, c_f, c_f, c_f, i32, f32, C.POINTER(DropoutCfg), c_f, c_f, c_f, c_f, c_f, i32, f32, c_s]),
    "lipasr_mlp_adam_nonneg": (i32, [c_h, c_f, c_f, c_f, c_f, c_f, f32, f32, f32, f32, f32, c_s]),
    "lipasr_mlp_project_product": (i32, [c_h, c_f, f32, PI, i32, c_f, c_s]),
    "lipasr_mlp_adam_project_product": (i32, [c_h, c_f, c_f, c_f, c_f, c_f, f32, f32, f32, f32, f32, f32, PI, i32, c_f, c_s]),
    "lipasr_mlp_adam_project_product_signal": (i32, [c_h, c_f, c_f, c_f, c_f, c_f, f32, f32, f32, f32, f32, f32, PI, i32, c_f, C.c_void_p, i32, c_s]),
    "lipasr_mlp_project_per_layer": (i32, [c_h, c_f, f32, c_f, i32, i32, c_f, c_s]),
    "lipasr_mlp_product_norm": (i32, [c_h, c_f, c_f, c_s]),
    "lipasr_mlp_predict": (i32, [c_h, c_f, c_f, c_f, i32, c_f, c_f, c_s]),
    "lipasr_mlp_input_grad": (i32, [c_h, c_f, c_f, c_f, c_f, i32, c_f, c_s]),
    "lipasr_mlp_set_compute": (i32, [c_h, i32]),
    "lipasr_mlp_set_gemm_tiles": (i32, [c_h, i32]),
    "lipasr_mlp_set_fuse_bn": (i32, [c_h, i32]),
    "lipasr_mlp_set_cu_budget": (i32, [c_h, i32]),
    "lipasr_mlp_exchange_errors": (i32, [c_h, C.POINTER(C.c_int)]),
    "lipasr_mlp_output_vjp": (i32, [c_h, c_f, c_f, c_f, c_f, i32, i32, c_f, c_f, c_s]),
    "lipasr_mlp_jacobian": (i32, [c_h, c_f, c_f, c_f, i32, i32, c_f, c_f, C.c_long, C.c_long, c_s]),
    "lipasr_jacobian_sigma": (i32, [c_h, c_f, i32, i32, i32, C.c_long, C.c_long, c_f, c_f, c_f, c_s]),
    "lipasr_deepfool_step": (i32, [c_h, c_f, C.c_long, C.c_long, c_f, c_f, c_f, i32, i32, i32, f32, f32, f32, f32, c_f, c_f, c_f, c_f, c_s]),
    "lipasr_smooth_expand": (i32, [c_h, c_f, c_f, i32, i32, i32, C.c_uint32, C.c_uint32, f32, u64, f32, f32, c_f, c_s]),
    "lipasr_smooth_vote": (i32, [c_h, c_f, i32, i32, i32, c_f, c_s]),
    "lipasr_smooth_loss": (i32, [c_h, c_f, c_f, i32, i32, i32, f32, f32, f32, f32, f32, c_f, c_f, c_f, c_f, c_s]),
    "lipasr_smooth_loss_host": (i32, [c_f, c_f, i32, i32, i32, f32, f32, f32, f32, f32, c_f, c_f, c_f, c_f]),
    "lipasr_smooth_probit_host": (i32, [c_f, i32, c_f]),
    "lipasr_debug_smooth_loss_launches": (i32, [i32]),
    "lipasr_smooth_noise_host": (i32, [u64, C.c_uint32, C.c_uint32, i32, C.POINTER(f32)]),
    "lipasr_genetic_breed": (i32, [c_h, c_f, c_f, c_f, c_f, i32, i32, i32, C.c_uint32, C.c_uint32, u64, C.c_uint32, f32, f32, f32, f32, c_f, c_s]),
    "lipasr_genetic_breed_host": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, C.c_uint32, C.c_uint32, u64, C.c_uint32, f32, f32, f32, f32, c_f]),
    "lipasr_genetic_select": (i32, [c_h, c_f, c_f, i32, i32, i32, i32, f32, C.c_uint32, C.c_uint32, u64, c_f, c_f, c_f, c_f, c_s]),
    "lipasr_apgd_loss": (i32, [c_h, c_f, c_f, i32, i32, i32, i32, c_f, c_f, c_f, c_s]),
    "lipasr_apgd_step": (i32, [c_h, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, f32, f32,
                               f32, f32, f32, f32, f32, i32, i32, c_s]),
    "lipasr_debug_apgd_path": (i32, [i32, i32]),
    "lipasr_square_init": (i32, [c_h, c_f, c_f, i32, i32, i32, C.c_uint32, C.c_uint32, u64, f32, f32, f32, c_f, c_f, c_f, c_s]),
    "lipasr_square_step": (i32, [c_h, c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, C.c_uint32, i32, C.c_uint32, C.c_uint32, C.c_uint32,
                                 i32, u64, f32, f32, f32, c_f, c_f, c_f, c_f, c_f, c_s]),
    "lipasr_square_init_host": (i32, [c_f, c_f, i32, i32, i32, C.c_uint32, C.c_uint32, u64, f32, f32, f32, c_f, c_f, c_f]),
    "lipasr_square_step_host": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, C.c_uint32, i32, C.c_uint32, C.c_uint32, C.c_uint32,
                                      i32, u64, f32, f32, f32, c_f, c_f, c_f, c_f, c_f]),
    "lipasr_hsj_expand": (i32, [c_h, c_f, c_f, c_f, i32, i32, i32, C.c_uint32, C.c_uint32, C.c_uint32, u64, f32, f32, f32, c_f, c_s]),
    "lipasr_hsj_accumulate": (i32, [c_h, c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, c_f, c_f, c_s]),
    "lipasr_hsj_direction": (i32, [c_h, c_f, c_f, c_f, i32, i32, f32, c_f, c_s]),
    "lipasr_hsj_search": (i32, [c_h, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, C.c_uint32, C.c_uint32, u64, f32,
                                f32, i32, f32, f32, c_f, c_f, c_f, c_f, c_f, c_f, c_s]),
    "lipasr_hsj_expand_host": (i32, [c_f, c_f, c_f, i32, i32, i32, C.c_uint32, C.c_uint32, C.c_uint32, u64, f32, f32, f32, c_f]),
    "lipasr_hsj_accumulate_host": (i32, [c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, c_f, c_f]),
    "lipasr_hsj_direction_host": (i32, [c_f, c_f, c_f, i32, i32, f32, c_f]),
    "lipasr_hsj_search_host": (i32, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, C.c_uint32, C.c_uint32, u64, f32, f32,
                                     i32, f32, f32, c_f, c_f, c_f, c_f, c_f, c_f]),
    "lipasr_debug_hsj_path": (i32, [i32, i32]),
    "lipasr_room_apply": (i32, [c_f, c_f, c_f, i32, i32, i32, i32, c_f, c_s]),
    "lipasr_room_vjp": (i32, [c_f, c_f, c_f, i32, i32, i32, i32, f32, c_f, c_s]),
    "lipasr_room_apply_host": (i32, [c_f, c_f, c_f, i32, i32, i32, i32, c_f]),
    "lipasr_room_vjp_host": (i32, [c_f, c_f, c_f, i32, i32, i32, i32, f32, c_f]),
    "lipasr_universal_shifts": (i32, [c_h, i32, i32, C.c_uint32, C.c_uint32, u64, c_f, c_s]),
    "lipasr_universal_apply": (i32, [c_h, c_f, c_f, c_f, c_f, i32, i32, i32, f32, f32, c_f, c_s]),
    "lipasr_universal_reduce": (i32, [c_h, c_f, c_f, c_f, i32, i32, i32, c_f, c_s]),
    "lipasr_universal_step": (i32, [c_h, c_f, c_f, i32, i32, f32, f32, f32, c_s]),
    "lipasr_universal_shifts_host": (i32, [i32, i32, C.c_uint32, C.c_uint32, u64, c_f]),
    "lipasr_universal_apply_host": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, f32, f32, c_f]),
    "lipasr_universal_reduce_host": (i32, [c_f, c_f, c_f, i32, i32, i32, c_f]),
    "lipasr_universal_step_host": (i32, [c_f, c_f, i32, i32, f32, f32, f32]),
    "lipasr_mlp_bounds_workspace": (i32, [c_h, i32, C.POINTER(sz)]),
    "lipasr_mlp_bounds": (i32, [c_h, c_f, c_f, c_f, c_f, f32, f32, f32, c_f, i32, c_f, sz, c_f, c_f, c_f, c_f, c_f, c_s]),
    "lipasr_mlp_bounds_workspace_host": (i32, [i32, PI, i32, C.POINTER(sz)]),
    "lipasr_mlp_bounds_host": (i32, [i32, PI, PI, c_f, c_f, c_f, c_f, f32, f32, f32, c_f, i32, c_f, sz, c_f, c_f, c_f, c_f, c_f]),
    "lipasr_debug_bounds_launches": (C.c_long, [i32]),
    "lipasr_mlp_bounds_grad_workspace": (i32, [c_h, i32, C.POINTER(sz)]),
    "lipasr_mlp_bounds_grad": (i32, [c_h, c_f, c_f, c_f, c_f, c_f, c_f, i32, c_f, sz, f32, f32, c_f, c_f, c_s]),
    "lipasr_mlp_bounds_grad_workspace_host": (i32, [i32, PI, i32, C.POINTER(sz)]),
    "lipasr_mlp_bounds_grad_host": (i32, [i32, PI, PI, c_f, c_f, c_f, c_f, c_f, c_f, i32, c_f, sz, f32, f32, c_f, c_f]),
    "lipasr_debug_bounds_grad_launches": (C.c_long, [i32]),
    "lipasr_mlp_bounds_crown_grad_workspace": (i32, [c_h, i32, C.POINTER(sz)]),
    "lipasr_mlp_bounds_crown_grad": (i32, [c_h, c_f, c_f, c_f, c_f, c_f, c_f, c_f, i32, f32, c_f, sz, f32, f32, c_f, c_f, c_s]),
    "lipasr_mlp_bounds_crown_grad_workspace_host": (i32, [i32, PI, i32, C.POINTER(sz)]),
    "lipasr_mlp_bounds_crown_grad_host": (i32, [i32, PI, PI, c_f, c_f, c_f, c_f, c_f, c_f, c_f, i32, f32, c_f, sz, f32, f32, c_f, c_f]),
    "lipasr_debug_bounds_crown_grad_launches": (C.c_long, [i32]),
    "lipasr_warp_table_host": (i32, [c_f, c_f]),
    "lipasr_warp_apply": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, c_f, c_s]),
    "lipasr_warp_param_vjp": (i32, [c_f, c_f, c_f, c_f, c_f, i32, i32, i32, c_f, c_s]),
    "lipasr_warp_apply_host": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, c_f]),
    "lipasr_warp_param_vjp_host": (i32, [c_f, c_f, c_f, c_f, c_f, i32, i32, i32, c_f]),
    "lipasr_debug_warp_launches": (C.c_long, [i32]),
    "lipasr_defence_apply": (i32, [c_f, c_f, PI, PI, PV, i32, i32, i32, c_f, c_s]),
    "lipasr_defence_vjp": (i32, [c_f, c_f, c_f, PI, PI, PV, i32, i32, i32, c_f, c_s]),
    "lipasr_defence_apply_host": (i32, [c_f, c_f, PI, PI, PV, i32, i32, i32, c_f]),
    "lipasr_defence_vjp_host": (i32, [c_f, c_f, c_f, PI, PI, PV, i32, i32, i32, c_f]),
    "lipasr_debug_defence_launches": (C.c_long, [i32]),
    "lipasr_mlp_attack_step": (i32, [c_h, c_f, c_f, c_f, c_f, c_f, i32, f32, f32, c_s]),
    "lipasr_mlp_attack_step_lp": (i32, [c_h, c_f, c_f, c_f, c_f, c_f, i32, f32, f32, f32, c_s]),
    "lipasr_mlp_own_labels": (i32, [c_h, c_f, c_f, c_f, i32, c_f, c_s]),
    "lipasr_mfcc_plan": (i32, [c_h, i32, i32, i32]),
    "lipasr_mfcc_plan_ex": (i32, [c_h, i32, i32, i32, i32, i32]),
    "lipasr_mfcc_dims": (i32, [c_h, PI, PI]),
    "lipasr_mfcc_f32": (i32, [c_h, c_f, i32, i32, c_f, c_f, c_f, c_s]),
    "lipasr_resample_f32": (i32, [c_h, c_f, i32, c_f, c_s]),
    "lipasr_mfcc_from_22k": (i32, [c_h, c_f, i32, i32, i32, c_f, c_f, c_f, c_s]),
    "lipasr_mfcc_i16": (i32, [c_h, c_f, c_f, i32, i32, c_f, c_f, c_f, c_s]),
    "lipasr_mfcc_create": (i32, [c_h, i32, i32, i32, i32, i32, C.POINTER(c_h)]),
    "lipasr_mfcc_destroy": (i32, [c_h]),
    "lipasr_mfcc_plan_dims": (i32, [c_h, PI, PI, PI]),
    "lipasr_mfcc_extract": (i32, [c_h, c_f, i32, c_f, i32, i32, c_f, c_f, c_f, c_s]),
    "lipasr_mfcc_plan_resample": (i32, [c_h, c_f, i32, c_f, c_s]),
    "lipasr_mfcc_plan_from_22k": (i32, [c_h, c_f, i32, i32, i32, c_f, c_f, c_f, c_s]),
    "lipasr_mfcc_plan_vjp": (i32, [c_h, c_f, i32, i32, i32, c_f, c_f, c_f, i32, c_s]),
    "lipasr_mfcc_plan_resample_vjp": (i32, [c_h, c_f, i32, c_f, c_s]),
    "lipasr_mfcc_plan_vjp_short": (i32, [c_h, c_f, i32, i32, i32, c_f, c_f, c_f, i32, c_s]),
    "lipasr_mfcc_plan_vjp_ragged": (i32, [c_h, c_f, i32, c_f, i32, i32, i32, c_f, c_f, c_f, i32, c_s]),
    "lipasr_mfcc_plan_resample_ragged": (i32, [c_h, c_f, i32, c_f, i32, c_f, c_s]),
    "lipasr_mfcc_plan_from_22k_ragged": (i32, [c_h, c_f, c_f, i32, i32, c_f, c_f, c_f, c_s]),
    "lipasr_mfcc_plan_profile_begin": (i32, [c_h, i32]),
    "lipasr_mfcc_plan_profile_end": (i32, [c_h, C.POINTER(f32), PI]),
    "lipasr_mfcc_plan_set": (i32, [c_h, i32, i32]),
    "lipasr_mfcc_profile_begin": (i32, [c_h, i32]),
    "lipasr_mfcc_profile_end": (i32, [c_h, C.POINTER(f32), PI]),
    "lipasr_dolphin_create": (i32, [c_h, i32, i32, i32, C.c_double, C.c_double, C.POINTER(c_h)]),
    "lipasr_dolphin_destroy": (i32, [c_h]),
    "lipasr_dolphin_bandpass": (i32, [c_h, c_f, c_f, i32, c_f, c_s]),
    "lipasr_dolphin_generate": (i32, [c_h, c_f, c_f, i32, c_f, c_f, c_s]),
    "lipasr_dolphin_record": (i32, [c_h, c_f, c_f, i32, f32, f32, c_f, c_s]),
    "lipasr_dolphin_generate_recorded": (i32, [c_h, c_f, c_f, i32, f32, f32, c_f, c_s]),
    "lipasr_dolphin_table": (i32, [i32, i32, C.POINTER(C.c_double), i32]),
    "lipasr_psy_create": (i32, [c_h, i32, i32, i32, i32, C.POINTER(c_h)]),
    "lipasr_psy_destroy": (i32, [c_h]),
    "lipasr_psy_psd": (i32, [c_h, c_f, i32, i32, c_f, c_f, c_s]),
    "lipasr_psy_threshold": (i32, [c_h, c_f, i32, i32, c_f, c_f, c_s]),
    "lipasr_psy_prepare": (i32, [c_h, c_f, i32, i32, c_f, c_f, c_s]),
    "lipasr_psy_loss_grad": (i32, [c_h, c_f, i32, i32, c_f, c_f, c_f, c_f, c_s]),
    "lipasr_psy_step": (i32, [c_h, c_f, c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, f32, i32, f32, f32, c_s]),
    "lipasr_psy_table": (i32, [i32, i32, C.POINTER(C.c_double), i32]),
    "lipasr_add_noise_f32": (i32, [c_h, c_f, i32, i32, i32, f32, f32, u64, c_s]),
    "lipasr_debug_set": (i32, [c_h, i32, i32]),
    "lipasr_debug_gemm_mode": (i32, [i32]),
    "lipasr_debug_launch_count": (C.c_long, [i32]),
    "lipasr_debug_gemm_launches": (C.c_long, [i32, i32, i32, i32, i32, i32]),
    "lipasr_debug_group_launches": (C.c_long, [i32, i32, i32]),
    "lipasr_debug_k3_launches": (C.c_long, [i32]),
    "lipasr_debug_k1_launches": (C.c_long, [i32]),
    "lipasr_debug_mfcc_stage": (i32, [c_h, i32, i32, c_f, c_s]),
    "lipasr_debug_k1_vjp_launches": (C.c_long, [i32]),
    "lipasr_debug_mfcc_vjp_stage": (i32, [c_h, i32, i32, c_f, c_s]),
    "lipasr_debug_mfcc_stage_put": (i32, [c_h, i32, i32, c_f, c_s]),
    "lipasr_debug_k2_launches": (C.c_long, [i32]),
    "lipasr_debug_mlp_stage": (i32, [c_h, i32, i32, i32, c_f, c_s]),
    "lipasr_debug_gemm": (i32, [c_h, i32, i32, i32, i32, i32, i32, c_f, i32, c_f, i32, c_f, i32, f32, f32, c_s]),
    "lipasr_flag_signal": (i32, [c_h, C.c_void_p, i32, c_s]),
    "lipasr_flag_wait": (i32, [c_h, C.c_void_p, i32, i32, C.c_void_p, c_s]),
    "lipasr_debug_chain_head": (i32, [i32]),
    "lipasr_debug_table": (i32, [i32, i32, C.POINTER(f32), i32]),
}

# entry points an older build named by LIPASR_LIBRARY (the parent commit's, for A/B timing) does not have yet: name -> the
# lipasr_version() that added it.  Callers ask has() and otherwise make the calls the entry point stands for.
SINCE = {"lipasr_mlp_adam_project_product_signal": 560, "lipasr_dolphin_create": 570, "lipasr_dolphin_destroy": 570,
         "lipasr_dolphin_bandpass": 570, "lipasr_dolphin_generate": 570, "lipasr_dolphin_record": 570,
         "lipasr_dolphin_generate_recorded": 570, "lipasr_dolphin_table": 570, "lipasr_mlp_jacobian": 580,
         "lipasr_jacobian_sigma": 580, "lipasr_psy_create": 590, "lipasr_psy_destroy": 590, "lipasr_psy_psd": 590,
         "lipasr_psy_threshold": 590, "lipasr_psy_prepare": 590, "lipasr_psy_loss_grad": 590, "lipasr_psy_step": 590,
         "lipasr_psy_table": 590, "lipasr_deepfool_step": 600, "lipasr_smooth_expand": 610,
         "lipasr_smooth_vote": 610, "lipasr_smooth_noise_host": 610, "lipasr_genetic_breed": 620,
         "lipasr_genetic_breed_host": 620, "lipasr_genetic_select": 620, "lipasr_debug_k3_launches": 630,
         "lipasr_debug_k1_launches": 640, "lipasr_debug_mfcc_stage": 640, "lipasr_apgd_loss": 650, "lipasr_apgd_step": 650,
         "lipasr_debug_apgd_path": 650, "lipasr_square_init": 660, "lipasr_square_step": 660, "lipasr_square_init_host": 660,
         "lipasr_square_step_host": 660, "lipasr_hsj_expand": 670, "lipasr_hsj_accumulate": 670, "lipasr_hsj_direction": 670,
         "lipasr_hsj_search": 670, "lipasr_hsj_expand_host": 670, "lipasr_hsj_accumulate_host": 670, "lipasr_hsj_direction_host": 670,
         "lipasr_hsj_search_host": 670, "lipasr_debug_hsj_path": 670, "lipasr_room_apply": 680, "lipasr_room_vjp": 680,
         "lipasr_room_apply_host": 680, "lipasr_room_vjp_host": 680, "lipasr_debug_k1_vjp_launches": 690,
         "lipasr_debug_mfcc_vjp_stage": 690, "lipasr_debug_mfcc_stage_put": 690, "lipasr_universal_shifts": 700,
         "lipasr_universal_apply": 700, "lipasr_universal_reduce": 700, "lipasr_universal_step": 700,
         "lipasr_universal_shifts_host": 700, "lipasr_universal_apply_host": 700, "lipasr_universal_reduce_host": 700,
         "lipasr_universal_step_host": 700, "lipasr_mlp_bounds_workspace": 710, "lipasr_mlp_bounds": 710,
         "lipasr_mlp_bounds_workspace_host": 710, "lipasr_mlp_bounds_host": 710, "lipasr_debug_bounds_launches": 710, "lipasr_warp_table_host": 720,
         "lipasr_warp_apply": 720, "lipasr_warp_param_vjp": 720, "lipasr_warp_apply_host": 720, "lipasr_warp_param_vjp_host": 720,
         "lipasr_debug_warp_launches": 720, "lipasr_debug_k2_launches": 730, "lipasr_debug_mlp_stage": 730, "lipasr_defence_apply": 740,
         "lipasr_defence_vjp": 740, "lipasr_defence_apply_host": 740, "lipasr_defence_vjp_host": 740, "lipasr_debug_defence_launches": 740,
         "lipasr_mlp_bounds_grad_workspace": 750, "lipasr_mlp_bounds_grad": 750, "lipasr_mlp_bounds_grad_workspace_host": 750,
         "lipasr_mlp_bounds_grad_host": 750, "lipasr_debug_bounds_grad_launches": 750,
         "lipasr_mlp_bounds_crown_grad_workspace": 760, "lipasr_mlp_bounds_crown_grad": 760,
         "lipasr_mlp_bounds_crown_grad_workspace_host": 760, "lipasr_mlp_bounds_crown_grad_host": 760,
         "lipasr_debug_bounds_crown_grad_launches": 760, "lipasr_mlp_train_fwd": 770, "lipasr_mlp_train_bwd": 770,
         "lipasr_smooth_loss": 770, "lipasr_smooth_loss_host": 770, "lipasr_smooth_probit_host": 770,
         "lipasr_debug_smooth_loss_launches": 770}
lib.lipasr_version.restype = i32
_VERSION = lib.lipasr_version()


def has(name) -> bool:
    return _VERSION >= SINCE.get(name, 0)


for _name, (_res, _args) in PROTOTYPES.items():
    if not has(_name):
        continue
    _fn = getattr(lib, _name)  # AttributeError here = header and library out of sync
    _fn.restype = _res
    _fn.argtypes = _args


if knobs.get("LIPASR_CHAIN_HEAD") is not None:  # A/B timing knob (lipasr_debug_chain_head): same product bit for bit
    lib.lipasr_debug_chain_head(knobs.get("LIPASR_CHAIN_HEAD"))
if knobs.get("LIPASR_GEMM_MODE") is not None:  # A/B timing knob (lipasr_debug_gemm_mode): never a different backend
    lib.lipasr_debug_gemm_mode(knobs.get("LIPASR_GEMM_MODE"))


def last_error() -> str:
    return (lib.lipasr_last_error() or b"").decode("utf-8", "replace")


class LipasrError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"liblipasr error {code}: {msg}")
        self.code = code


def check(rc: int) -> int:
    """Raise for a negative return code: ValueError for LIPASR_EINVAL, LipasrError otherwise."""
    if rc >= 0:
        return rc
    msg = last_error()
    if rc == EINVAL:
        raise ValueError(f"liblipasr: {msg}")
    raise LipasrError(rc, msg)


def int_array(values):
    arr = (C.c_int * max(1, len(values)))(*[int(v) for v in values])
    return arr


def float_array(values):
    return (C.c_float * max(1, len(values)))(*[float(v) for v in values])


def ptr_array(ptrs):
    return (C.c_void_p * max(1, len(ptrs)))(*[C.c_void_p(int(p) if p else None) for p in ptrs])


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_handles = {}
# Objects that own native resources (pipelines: graphs + masked streams; models: classifier plans; extractors: MFCC
# plans).  shutdown() closes them newest-first and then destroys the handles, so that no HIP object of ours is left
# for the runtime's static destructors ("exit-time SIGSEGV").  Weak references: the registry never keeps
# an object alive.
_owners = []


def register_owner(obj):
    """obj.close() must be idempotent and must not raise once the handle is gone."""
    import weakref

    _owners.append(weakref.ref(obj))
    if len(_owners) > 256:
        _owners[:] = [r for r in _owners if r() is not None]


# Native destroy calls free device memory (hipFree synchronises), which is illegal while THIS thread captures a HIP graph:
# it invalidates the capture ("operation failed due to a previous error during capture").  Python finalisers run whenever
# the garbage collector decides -- also in the middle of TrainPipeline._capture -- so every destroy goes through
# destroy_or_defer(): during a capture it is parked and run right after the capture ends.
_capture_depth = 0
_deferred = []


def capture_enter():
    global _capture_depth
    _capture_depth += 1


def capture_exit():
    global _capture_depth
    _capture_depth = max(0, _capture_depth - 1)
    if _capture_depth == 0:
        pending, _deferred[:] = list(_deferred), []
        for fn, args in pending:
            fn(*args)


def destroy_or_defer(fn, *args):
    if _capture_depth > 0:
        _deferred.append((fn, args))
    else:
        fn(*args)


class Handle:
    """One lipasr handle per (process, device)."""

    def __init__(self, device: int):
        self.device = device
        h = c_h()
        check(lib.lipasr_create(device, C.byref(h)))
        self.h = h

    @property
    def alive(self):
        return bool(self.h)

    def close(self):
        """Closes every live owner made on this handle first (pipelines, models, extractors, newest first): lipasr_destroy frees
        their native plans, and an owner that still held a plan pointer would turn its next call into a use-after-free instead
        of an error.  Closed owners raise on use."""
        if self.h:
            for ref in reversed(list(_owners)):
                obj = ref()
                if obj is not None and (getattr(obj, "h", None) is self or getattr(obj, "_h", None) is self):
                    try:
                        obj.close()
                    except Exception:
                        pass
            lib.lipasr_destroy(self.h)
            self.h = None


def get_handle(device=None) -> Handle:
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("lipasr needs an MI355X (gfx950) GPU: torch.cuda.is_available() is False and there is no CPU path")
    if device is None:
        device = torch.cuda.current_device()
    h = _handles.get(device)
    if h is None or not h.alive:
        h = _handles[device] = Handle(device)
    return h


def shutdown():
    """Deterministic teardown: pipelines / models / extractors (newest first), then the handles -- graphs, CU-masked
    streams, plans, events, scratch -- all while the HIP runtime is still up.  Registered with atexit AFTER torch was
    imported, so it runs BEFORE torch's and the runtime's own exit handlers; safe to call more than once."""
    global _capture_depth
    _capture_depth = 0
    pending, _deferred[:] = list(_deferred), []
    for fn, args in pending:
        try:
            fn(*args)
        except Exception:
            pass
    owners, _owners[:] = list(_owners), []
    for ref in reversed(owners):
        obj = ref()
        if obj is not None:
            try:
                obj.close()
            except Exception:
                pass
    for h in list(_handles.values()):
        try:
            h.close()
        except Exception:
            pass
    _handles.clear()


import atexit  # noqa: E402

atexit.register(shutdown)


def dolphin_table(which: int, sr_in: int = 16000):
    """Host-only fp64 tables of the DolphinAttack chain (0 SOS[10][6], 1 h_up, 2 h_dn, 3 M^64 [10][4]) as numpy float64."""
    import numpy as np

    n = check(lib.lipasr_dolphin_table(which, sr_in, None, 0))
    out = np.zeros(n, dtype=np.float64)
    check(lib.lipasr_dolphin_table(which, sr_in, out.ctypes.data_as(C.POINTER(C.c_double)), n))
    return out


def psy_table(which: int, sample_rate: int = 16000):
    """Host-only fp64 tables of the psychoacoustic masker (0 f, 1 bark, 2 ATH in dB, 3 shift; [1025] each) as numpy float64."""
    import numpy as np

    n = check(lib.lipasr_psy_table(which, sample_rate, None, 0))
    out = np.zeros(n, dtype=np.float64)
    check(lib.lipasr_psy_table(which, sample_rate, out.ctypes.data_as(C.POINTER(C.c_double)), n))
    return out


def smooth_noise(seed: int, clip: int, draw: int, n: int):
    """Host-only: the n standard-normal draws lipasr_smooth_expand adds to clip `clip`, draw `draw` (numpy float32)."""
    import numpy as np

    out = np.zeros(max(int(n), 1), dtype=np.float32)
    check(lib.lipasr_smooth_noise_host(int(seed), int(clip), int(draw), int(n), out.ctypes.data_as(C.POINTER(f32))))
    return out[:int(n)]


SMOOTH_LOSS_KERNELS = ("loss", "expand")  # ids of lipasr_debug_smooth_loss_launches


def smooth_probit(q):
    """Host-only: Phi^-1 of every entry of ``q`` as lipasr_smooth_loss computes it (numpy float64)."""
    import numpy as np

    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    out = np.zeros(max(q.size, 1), dtype=np.float64)
    check(lib.lipasr_smooth_probit_host(q.ctypes.data_as(C.c_void_p), int(q.size), out.ctypes.data_as(C.c_void_p)))
    return out[:q.size]


def smooth_loss_host(logits, label, draws, sigma, lam, gamma, beta, scale):
    """Host-only: lipasr_smooth_loss_host on NumPy arrays (logits float32 [clips * draws, classes], label int32 [clips]) -> the dict
    of float32 arrays dz [clips * draws, classes], loss, correct and radius [clips] that lipasr_smooth_loss writes on the device."""
    import numpy as np

    logits = np.ascontiguousarray(logits, dtype=np.float32)
    label = np.ascontiguousarray(label, dtype=np.int32).reshape(-1)
    rows, classes = logits.shape
    clips, draws = label.size, int(draws)
    if rows != clips * draws:
        raise ValueError(f"{rows} rows of logits are not {clips} clips x {draws} draws")
    out = {"dz": np.zeros((rows, classes), dtype=np.float32)}
    out.update({k: np.zeros(max(clips, 1), dtype=np.float32) for k in ("loss", "correct", "radius")})
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    check(lib.lipasr_smooth_loss_host(vp(logits), vp(label), clips, draws, classes, float(sigma), float(lam), float(gamma), float(beta),
                                      float(scale), vp(out["dz"]), vp(out["loss"]), vp(out["correct"]), vp(out["radius"])))
    return {k: (v if k == "dz" else v[:clips]) for k, v in out.items()}


def genetic_breed_host(x0, pop, generation, seed, mutate_thresh, step, eps, *, pop_in=None, parents=None, n_valid=None, clip0=0,
                       clip_lo=-float("inf"), clip_hi=float("inf"), out=None):
    """Host-only: lipasr_genetic_breed_host on NumPy arrays (x0 float32 [B, n], pop_in float32 [B, pop, n] and parents int32
    [B, pop, 2] or neither, n_valid int32 [B] or None) -> float32 [B, pop, n]: the bits lipasr_genetic_breed writes on the device."""
    import numpy as np

    x0 = np.ascontiguousarray(x0, dtype=np.float32)
    b, n = x0.shape
    pop = int(pop)
    keep = [x0]

    def arr(a, dtype, shape):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.shape != shape:
            raise ValueError(f"expected shape {shape}, got {a.shape}")
        keep.append(a)
        return C.c_void_p(a.ctypes.data)

    if out is None:
        out = np.zeros((b, max(pop, 0), n), dtype=np.float32)
    elif out.dtype != np.float32 or out.shape != (b, pop, n) or not out.flags.c_contiguous:
        raise ValueError(f"out must be a contiguous float32 array ({b}, {pop}, {n})")
    check(lib.lipasr_genetic_breed_host(C.c_void_p(x0.ctypes.data), arr(n_valid, np.int32, (b,)), arr(pop_in, np.float32, (b, pop, n)),
                                        arr(parents, np.int32, (b, pop, 2)), b, pop, n, int(clip0), int(generation), int(seed),
                                        int(mutate_thresh), float(step), float(eps), float(clip_lo), float(clip_hi),
                                        C.c_void_p(out.ctypes.data)))
    return out


SQUARE_LAST = 1


def _host_array(a, dtype, shape, what):
    import numpy as np

    if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == tuple(shape) and a.flags.c_contiguous and a.flags.writeable):
        raise ValueError(f"{what} must be a contiguous writeable {np.dtype(dtype).name} array {tuple(shape)}")
    return C.c_void_p(a.ctypes.data)


def square_init_host(x0, height, width, restart, seed, eps, *, n_valid=None, clip0=0, clip_lo=-float("inf"), clip_hi=float("inf"),
                     x_best=None, x_cand=None, win=None):
    """Host-only: lipasr_square_init_host on NumPy arrays (x0 float32 [B, height * width], n_valid int32 [B] or None)
    -> (x_best, x_cand float32 [B, n], win int32 [B, 4]): the bits lipasr_square_init writes on the device."""
    import numpy as np

    x0 = np.ascontiguousarray(x0, dtype=np.float32)
    b, n = x0.shape
    height, width = int(height), int(width)
    if height * width != n:
        raise ValueError(f"{height} x {width} is not the row length {n}")
    nv = None if n_valid is None else np.ascontiguousarray(n_valid, dtype=np.int32).reshape(b)
    x_best = np.zeros((b, n), dtype=np.float32) if x_best is None else x_best
    x_cand = np.zeros((b, n), dtype=np.float32) if x_cand is None else x_cand
    win = np.zeros((b, 4), dtype=np.int32) if win is None else win
    check(lib.lipasr_square_init_host(C.c_void_p(x0.ctypes.data), None if nv is None else C.c_void_p(nv.ctypes.data), b, height, width,
                                      int(clip0), int(restart), int(seed) & 0xFFFFFFFFFFFFFFFF, float(eps), float(clip_lo),
                                      float(clip_hi), _host_array(x_best, np.float32, (b, n), "x_best"),
                                      _host_array(x_cand, np.float32, (b, n), "x_cand"), _host_array(win, np.int32, (b, 4), "win")))
    return x_best, x_cand, win


def square_step_host(logits, labels, x0, height, width, win_h, win_w, p_q, restart, it, seed, eps, *, x_best, x_cand, loss_best, done,
                     win, n_valid=None, targeted=False, last=False, clip0=0, clip_lo=-float("inf"), clip_hi=float("inf")):
    """Host-only: lipasr_square_step_host on NumPy arrays, in place on x_best, x_cand float32 [B, n], loss_best float32 [B], done
    int32 [B] and win int32 [B, 4]; logits float32 [B, classes], labels int32 [B]: the bits lipasr_square_step writes."""
    import numpy as np

    x0 = np.ascontiguousarray(x0, dtype=np.float32)
    b, n = x0.shape
    height, width = int(height), int(width)
    if height * width != n:
        raise ValueError(f"{height} x {width} is not the row length {n}")
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    if logits.ndim != 2 or logits.shape[0] != b:
        raise ValueError(f"logits must be [{b}, classes], got {logits.shape}")
    labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(b)
    nv = None if n_valid is None else np.ascontiguousarray(n_valid, dtype=np.int32).reshape(b)
    check(lib.lipasr_square_step_host(C.c_void_p(logits.ctypes.data), C.c_void_p(labels.ctypes.data), C.c_void_p(x0.ctypes.data),
                                      None if nv is None else C.c_void_p(nv.ctypes.data), b, logits.shape[1], height, width, int(win_h),
                                      int(win_w), int(p_q), 1 if targeted else 0, int(clip0), int(restart), int(it),
                                      SQUARE_LAST if last else 0, int(seed) & 0xFFFFFFFFFFFFFFFF, float(eps), float(clip_lo),
                                      float(clip_hi), _host_array(x_best, np.float32, (b, n), "x_best"),
                                      _host_array(x_cand, np.float32, (b, n), "x_cand"),
                                      _host_array(loss_best, np.float32, (b,), "loss_best"), _host_array(done, np.int32, (b,), "done"),
                                      _host_array(win, np.int32, (b, 4), "win")))


HSJ_START, HSJ_HALVE, HSJ_BISECT = 0, 1, 2
HSJ_FIRST, HSJ_LAST = 1, 2
# columns of lipasr_hsj_search's fstate and istate
HSJ_F = {"lo": 0, "hi": 1, "mid": 2, "thresh": 3, "eps": 4, "dist": 5, "dist_best": 6, "dist_far": 7}
HSJ_I = {"active": 0, "found": 1, "ok": 2, "moved": 3, "halvings": 4, "queries": 5}


def _host_in(a, dtype, shape, what):
    import numpy as np

    a = np.ascontiguousarray(a, dtype=dtype)
    if a.shape != tuple(shape):
        raise ValueError(f"{what} must be {tuple(shape)}, got {a.shape}")
    return a


def _norm_f(norm):
    return float("inf") if norm in ("inf", float("inf")) else float(norm)


def hsj_expand_host(x, delta, draws, it, seed, norm, *, n_valid=None, clip0=0, draw0=0, clip_lo=-float("inf"), clip_hi=float("inf"),
                    out=None):
    """Host-only: lipasr_hsj_expand_host on NumPy arrays (x float32 [B, n], delta float32 [B]) -> float32 [B * draws, n]."""
    import numpy as np

    x = np.ascontiguousarray(x, dtype=np.float32)
    b, n = x.shape
    delta = _host_in(delta, np.float32, (b,), "delta")
    nv = None if n_valid is None else _host_in(n_valid, np.int32, (b,), "n_valid")
    out = np.zeros((b * int(draws), n), dtype=np.float32) if out is None else out
    check(lib.lipasr_hsj_expand_host(C.c_void_p(x.ctypes.data), C.c_void_p(delta.ctypes.data), None if nv is None else C.c_void_p(nv.ctypes.data),
                                     b, n, int(draws), int(clip0), int(it), int(draw0), int(seed) & 0xFFFFFFFFFFFFFFFF, _norm_f(norm),
                                     float(clip_lo), float(clip_hi), _host_array(out, np.float32, (b * int(draws), n), "out")))
    return out


def hsj_accumulate_host(logits, labels, p, x, *, sums, counts, n_valid=None, targeted=False):
    """Host-only: lipasr_hsj_accumulate_host, in place on sums float64 [B, 2, n] and counts int32 [B, 2]."""
    import numpy as np

    x = np.ascontiguousarray(x, dtype=np.float32)
    b, n = x.shape
    p = np.ascontiguousarray(p, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != n or (b and p.shape[0] % b):
        raise ValueError(f"p must be [{b} * draws, {n}], got {p.shape}")
    draws = p.shape[0] // b if b else 0
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    if logits.ndim != 2 or logits.shape[0] != p.shape[0]:
        raise ValueError(f"logits must be [{p.shape[0]}, classes], got {logits.shape}")
    labels = _host_in(labels, np.int32, (b,), "labels")
    nv = None if n_valid is None else _host_in(n_valid, np.int32, (b,), "n_valid")
    check(lib.lipasr_hsj_accumulate_host(C.c_void_p(logits.ctypes.data), C.c_void_p(labels.ctypes.data), C.c_void_p(p.ctypes.data),
                                         C.c_void_p(x.ctypes.data), None if nv is None else C.c_void_p(nv.ctypes.data), b, logits.shape[1], n,
                                         draws, 1 if targeted else 0, _host_array(sums, np.float64, (b, 2, n), "sums"),
                                         _host_array(counts, np.int32, (b, 2), "counts")))


def hsj_direction_host(sums, counts, norm, *, n_valid=None, u=None):
    """Host-only: lipasr_hsj_direction_host (sums float64 [B, 2, n], counts int32 [B, 2]) -> u float32 [B, n]."""
    import numpy as np

    sums = np.ascontiguousarray(sums, dtype=np.float64)
    b, _, n = sums.shape
    counts = _host_in(counts, np.int32, (b, 2), "counts")
    nv = None if n_valid is None else _host_in(n_valid, np.int32, (b,), "n_valid")
    u = np.zeros((b, n), dtype=np.float32) if u is None else u
    check(lib.lipasr_hsj_direction_host(C.c_void_p(sums.ctypes.data), C.c_void_p(counts.ctypes.data),
                                        None if nv is None else C.c_void_p(nv.ctypes.data), b, n, _norm_f(norm),
                                        _host_array(u, np.float32, (b, n), "u")))
    return u


def hsj_search_host(logits, labels, x0, mode, flags, seed, norm, *, x_cand, x_far, x_adv, x_best, fstate, istate, start_lo, start_hi,
                    theta, u=None, n_valid=None, targeted=False, clip0=0, draw=0, step_scale=1.0, max_halvings=25,
                    clip_lo=-float("inf"), clip_hi=float("inf"), classes=None):
    """Host-only: lipasr_hsj_search_host on NumPy arrays, in place on x_cand, x_far, x_adv, x_best float32 [B, n], fstate float32
    [B, 8] and istate int32 [B, 8]; logits float32 [B, classes] or None (under HSJ_FIRST, then ``classes`` says how many)."""
    import numpy as np

    x0 = np.ascontiguousarray(x0, dtype=np.float32)
    b, n = x0.shape
    if logits is not None:
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        if logits.ndim != 2 or logits.shape[0] != b:
            raise ValueError(f"logits must be [{b}, classes], got {logits.shape}")
        classes = logits.shape[1]
    labels = _host_in(labels, np.int32, (b,), "labels")
    nv = None if n_valid is None else _host_in(n_valid, np.int32, (b,), "n_valid")
    sl, sh, th = (_host_in(a, np.float32, (b,), w) for a, w in ((start_lo, "start_lo"), (start_hi, "start_hi"), (theta, "theta")))
    uu = None if u is None else _host_in(u, np.float32, (b, n), "u")
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    check(lib.lipasr_hsj_search_host(vp(logits), vp(labels), vp(x0), vp(nv), vp(uu), vp(sl), vp(sh), vp(th), b, int(classes or 1), n, int(mode),
                                     int(flags), 1 if targeted else 0, int(clip0), int(draw), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                     _norm_f(norm), float(step_scale), int(max_halvings), float(clip_lo), float(clip_hi),
                                     _host_array(x_cand, np.float32, (b, n), "x_cand"), _host_array(x_far, np.float32, (b, n), "x_far"),
                                     _host_array(x_adv, np.float32, (b, n), "x_adv"), _host_array(x_best, np.float32, (b, n), "x_best"),
                                     _host_array(fstate, np.float32, (b, 8), "fstate"), _host_array(istate, np.int32, (b, 8), "istate")))


def room_apply_host(x, rirs, *, n_valid=None, out=None):
    """Host-only: lipasr_room_apply_host on NumPy arrays (x float32 [B, n], rirs float32 [R, taps]) -> float32 [B * R, n]."""
    import numpy as np

    x = np.ascontiguousarray(x, dtype=np.float32)
    rirs = np.ascontiguousarray(rirs, dtype=np.float32)
    if x.ndim != 2 or rirs.ndim != 2:
        raise ValueError("x must be [B, n] and rirs [R, taps]")
    (b, n), (r, taps) = x.shape, rirs.shape
    nv = None if n_valid is None else _host_in(n_valid, np.int32, (b,), "n_valid")
    out = np.zeros((b * r, n), dtype=np.float32) if out is None else out
    check(lib.lipasr_room_apply_host(C.c_void_p(x.ctypes.data), None if nv is None else C.c_void_p(nv.ctypes.data),
                                     C.c_void_p(rirs.ctypes.data), taps, r, b, n, _host_array(out, np.float32, (b * r, n), "out")))
    return out


def room_vjp_host(g, rirs, *, n_valid=None, scale=1.0, out=None):
    """Host-only: lipasr_room_vjp_host on NumPy arrays (g float32 [B * R, n], rirs float32 [R, taps]) -> float32 [B, n]."""
    import numpy as np

    g = np.ascontiguousarray(g, dtype=np.float32)
    rirs = np.ascontiguousarray(rirs, dtype=np.float32)
    if g.ndim != 2 or rirs.ndim != 2 or rirs.shape[0] == 0 or g.shape[0] % rirs.shape[0]:
        raise ValueError("g must be [B * R, n] and rirs [R, taps]")
    (rows, n), (r, taps) = g.shape, rirs.shape
    b = rows // r
    nv = None if n_valid is None else _host_in(n_valid, np.int32, (b,), "n_valid")
    out = np.zeros((b, n), dtype=np.float32) if out is None else out
    check(lib.lipasr_room_vjp_host(C.c_void_p(g.ctypes.data), None if nv is None else C.c_void_p(nv.ctypes.data),
                                   C.c_void_p(rirs.ctypes.data), taps, r, b, n, float(scale), _host_array(out, np.float32, (b, n), "out")))
    return out


WARP_Z, WARP_P = 16, 512  # zero crossings per wing and table steps per crossing of the time-warp table


def warp_table_host():
    """Host-only: lipasr_warp_table_host -> (win, delta), float32 [WARP_Z * WARP_P + 1] each."""
    import numpy as np

    win, delta = (np.zeros(WARP_Z * WARP_P + 1, dtype=np.float32) for _ in range(2))
    check(lib.lipasr_warp_table_host(C.c_void_p(win.ctypes.data), C.c_void_p(delta.ctypes.data)))
    return win, delta


def _warp_host_args(x, params, K, n_valid, table):
    import numpy as np

    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("x must be [B, n]")
    b, n = x.shape
    params = _host_in(params, np.float32, (b * int(K), 3), "params")
    nv = None if n_valid is None else _host_in(n_valid, np.int32, (b,), "n_valid")
    if table is None:
        table = np.stack(warp_table_host(), axis=1)
    table = _host_in(table, np.float32, (WARP_Z * WARP_P + 1, 2), "table")
    return x, params, nv, table, b, n


def warp_apply_host(x, params, K, *, n_valid=None, table=None, out=None):
    """Host-only: lipasr_warp_apply_host on NumPy arrays (x float32 [B, n], params float32 [B * K, 3]) -> float32 [B * K, n]."""
    import numpy as np

    x, params, nv, table, b, n = _warp_host_args(x, params, K, n_valid, table)
    out = np.zeros((b * int(K), n), dtype=np.float32) if out is None else out
    check(lib.lipasr_warp_apply_host(_vp(x), None if nv is None else _vp(nv), _vp(params), _vp(table), b, int(K), n,
                                     _host_array(out, np.float32, (b * int(K), n), "out")))
    return out


def warp_param_vjp_host(x, g, params, K, *, n_valid=None, table=None):
    """Host-only: lipasr_warp_param_vjp_host on NumPy arrays (g float32 [B * K, n]) -> float64 [B * K, 3]."""
    import numpy as np

    x, params, nv, table, b, n = _warp_host_args(x, params, K, n_valid, table)
    g = _host_in(g, np.float32, (b * int(K), n), "g")
    gp = np.zeros((b * int(K), 3), dtype=np.float64)
    check(lib.lipasr_warp_param_vjp_host(_vp(x), _vp(g), None if nv is None else _vp(nv), _vp(params), _vp(table), b, int(K), n, _vp(gp)))
    return gp


DEFENCE_MEDIAN, DEFENCE_FIR, DEFENCE_QUANTIZE = 0, 1, 2  # LIPASR_DEFENCE_*
DEFENCE_MAX_STAGES, DEFENCE_MAX_HALO = 4, 256


def defence_chain(stages, taps_ptrs):
    """The three host arrays of a defence chain (include/lipasr.h, lipasr_defence_apply) from ``stages``, a list of (kind, arg)
    with kind one of DEFENCE_*, and ``taps_ptrs``, one address (or None) per stage: (kinds, args, taps, count)."""
    return (int_array([k for k, _ in stages]), int_array([a for _, a in stages]), ptr_array(taps_ptrs), len(stages))


def _defence_host_args(x, stages, n_valid):
    import numpy as np

    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("x must be [B, n]")
    b, n = x.shape
    nv = None if n_valid is None else _host_in(n_valid, np.int32, (b,), "n_valid")
    keep = [None if t is None else np.ascontiguousarray(t, dtype=np.float32).reshape(-1) for _, _, t in stages]
    chain = defence_chain([(k, int(a)) for k, a, _ in stages], [None if t is None else t.ctypes.data for t in keep])
    return x, nv, keep, chain, b, n


def defence_apply_host(x, stages, *, n_valid=None, out=None):
    """Host-only: lipasr_defence_apply_host on NumPy arrays.  x float32 [B, n]; ``stages``: a list of (kind, arg, taps) with kind
    one of DEFENCE_*, arg the width, tap count or bits and taps a float32 array for a FIR stage (None otherwise) -> float32 [B, n]."""
    import numpy as np

    x, nv, keep, (kinds, args, taps, count), b, n = _defence_host_args(x, stages, n_valid)
    out = np.zeros((b, n), dtype=np.float32) if out is None else out
    check(lib.lipasr_defence_apply_host(_vp(x), _vp(nv), kinds, args, taps, count, b, n, _host_array(out, np.float32, (b, n), "out")))
    return out


def defence_vjp_host(x, g, stages, *, n_valid=None, out=None):
    """Host-only: lipasr_defence_vjp_host on NumPy arrays (x and the cotangent g float32 [B, n]) -> float32 [B, n]."""
    import numpy as np

    x, nv, keep, (kinds, args, taps, count), b, n = _defence_host_args(x, stages, n_valid)
    g = _host_in(g, np.float32, (b, n), "g")
    out = np.zeros((b, n), dtype=np.float32) if out is None else out
    check(lib.lipasr_defence_vjp_host(_vp(x), _vp(g), _vp(nv), kinds, args, taps, count, b, n, _host_array(out, np.float32, (b, n), "out")))
    return out


UNIVERSAL_GROUP = 64  # LIPASR_UNIVERSAL_GROUP: the rows one slab of lipasr_universal_reduce's sums holds


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def universal_shifts_host(batch, P, it, seed, *, clip0=0, out=None):
    """Host-only: lipasr_universal_shifts_host -> int32 [batch], the shifts of rows clip0 .. clip0 + batch - 1 at iteration ``it``."""
    import numpy as np

    batch = int(batch)
    out = np.zeros(max(batch, 0), dtype=np.int32) if out is None else out
    check(lib.lipasr_universal_shifts_host(batch, int(P), int(clip0), int(it), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                           _host_array(out, np.int32, (max(batch, 0),), "out")))
    return out


def universal_apply_host(x, noise, *, offs=None, n_valid=None, clip_lo=-float("inf"), clip_hi=float("inf"), out=None):
    """Host-only: lipasr_universal_apply_host on NumPy arrays (x float32 [B, n], noise float32 [P]) -> float32 [B, n]."""
    import numpy as np

    x = np.ascontiguousarray(x, dtype=np.float32)
    b, n = x.shape
    noise = np.ascontiguousarray(noise, dtype=np.float32).reshape(-1)
    of = None if offs is None else _host_in(offs, np.int32, (b,), "offs")
    nv = None if n_valid is None else _host_in(n_valid, np.int32, (b,), "n_valid")
    out = np.zeros((b, n), dtype=np.float32) if out is None else out
    check(lib.lipasr_universal_apply_host(_vp(x), _vp(noise), _vp(of), _vp(nv), b, n, noise.shape[0], float(clip_lo), float(clip_hi),
                                          _host_array(out, np.float32, (b, n), "out")))
    return out


def universal_reduce_host(g, P, *, offs=None, n_valid=None, sums=None):
    """Host-only: lipasr_universal_reduce_host on NumPy arrays (g float32 [B, n]) -> float64 [ceil(B / 64), P]."""
    import numpy as np

    g = np.ascontiguousarray(g, dtype=np.float32)
    b, n = g.shape
    P = int(P)
    groups = (b + UNIVERSAL_GROUP - 1) // UNIVERSAL_GROUP
    of = None if offs is None else _host_in(offs, np.int32, (b,), "offs")
    nv = None if n_valid is None else _host_in(n_valid, np.int32, (b,), "n_valid")
    sums = np.zeros((groups, max(P, 0)), dtype=np.float64) if sums is None else sums
    check(lib.lipasr_universal_reduce_host(_vp(g), _vp(of), _vp(nv), b, n, P, _host_array(sums, np.float64, (groups, max(P, 0)), "sums")))
    return sums


def universal_step_host(noise, sums, norm, alpha, eps):
    """Host-only: lipasr_universal_step_host, in place on noise float32 [P]; sums float64 [groups, P]."""
    import numpy as np

    sums = np.ascontiguousarray(sums, dtype=np.float64)
    groups, P = sums.shape
    check(lib.lipasr_universal_step_host(_host_array(noise, np.float32, (P,), "noise"), _vp(sums), groups, P, _norm_f(norm), float(alpha),
                                         float(eps)))
    return noise


def debug_table(which: int, sr_in: int = 16000):
    """Host-only constant tables as the kernels read them (numpy float32)."""
    import numpy as np

    n = check(lib.lipasr_debug_table(which, sr_in, None, 0))
    out = np.zeros(n, dtype=np.float32)
    check(lib.lipasr_debug_table(which, sr_in, out.ctypes.data_as(C.POINTER(C.c_float)), n))
    return out


BOUNDS_KERNELS = ("prep", "layer", "head", "back", "tail")  # ids of lipasr_debug_bounds_launches


def bounds_layout(widths, bn=None):
    """Offsets (in floats) of lipasr_mlp_create's flat layout for a model given by its widths: per layer a dict with W, b and (BatchNorm)
    gamma, beta in params and mean, var in bnstate; then (n_params, n_state)."""
    a4 = lambda v: (v + 3) & ~3
    po = so = 0
    out = []
    L = len(widths) - 1
    for l in range(L):
        ni, no = int(widths[l]), int(widths[l + 1])
        d = {"W": po}
        po = a4(po + ni * no)
        d["b"] = po
        po = a4(po + no)
        if bn is not None and l + 1 < L and bn[l]:
            d["gamma"] = po
            po = a4(po + no)
            d["beta"] = po
            po = a4(po + no)
            d["mean"] = so
            so = a4(so + no)
            d["var"] = so
            so = a4(so + no)
        out.append(d)
    return out, po, so


def bounds_family_floats(widths, batch):
    """Floats of layer_lo (or layer_hi) of lipasr_mlp_bounds: the input box and (z_l, h_l) of every hidden layer, [batch][n] each."""
    return int(batch) * (int(widths[0]) + 2 * sum(int(n) for n in widths[1:-1]))


def bounds_split_layers(flat, widths, batch):
    """layer_lo or layer_hi of lipasr_mlp_bounds as (input box [B, n_0], [(z_l, h_l) for the hidden layers])."""
    b, o = int(batch), 0
    box = flat[o:o + b * widths[0]].reshape(b, widths[0])
    o += b * widths[0]
    layers = []
    for n in widths[1:-1]:
        z = flat[o:o + b * n].reshape(b, n)
        o += b * n
        h = flat[o:o + b * n].reshape(b, n)
        o += b * n
        layers.append((z, h))
    return box, layers


def mlp_bounds_host(widths, bn, params, bnstate, x, eps, norm, y, *, clip_lo=-float("inf"), clip_hi=float("inf"), crown=True,
                    ws_offset=0):
    """Host-only: lipasr_mlp_bounds_host on NumPy arrays -> dict(margin_ibp, margin_crown, slack [B, C]; lo, hi: the flat layer
    boxes).  ws_offset: floats the workspace starts past a 16-byte boundary."""
    import numpy as np

    widths = [int(w) for w in widths]
    L = len(widths) - 1
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.shape[0]
    params = np.ascontiguousarray(params, dtype=np.float32)
    bnstate = None if bnstate is None else np.ascontiguousarray(bnstate, dtype=np.float32)
    eps = _host_in(eps, np.float32, (b,), "eps")
    y = _host_in(y, np.int32, (b,), "y")
    wa, ba = int_array(widths), (None if bn is None else int_array(bn))
    need = sz()
    check(lib.lipasr_mlp_bounds_workspace_host(L, wa, b, C.byref(need)))
    ws = np.zeros(need.value + 8, dtype=np.float32)
    skip = (-(ws.ctypes.data // 4)) % 4 + int(ws_offset)
    wsv = ws[skip:skip + need.value]
    fam = bounds_family_floats(widths, b)
    c = widths[-1]
    out = {"margin_ibp": np.zeros((b, c), np.float32), "margin_crown": np.zeros((b, c), np.float32) if crown else None,
           "slack": np.zeros((b, c), np.float32) if crown else None, "lo": np.zeros(fam, np.float32), "hi": np.zeros(fam, np.float32)}
    check(lib.lipasr_mlp_bounds_host(L, wa, ba, _vp(params), _vp(bnstate), _vp(x), _vp(eps), _norm_f(norm), float(clip_lo), float(clip_hi),
                                     _vp(y), b, _vp(wsv), need.value, _vp(out["margin_ibp"]), _vp(out["margin_crown"]), _vp(out["slack"]),
                                     _vp(out["lo"]), _vp(out["hi"])))
    return out


BOUNDS_GRAD_KERNELS = ("head", "wgrad", "back", "colsum")  # ids of lipasr_debug_bounds_grad_launches


def bounds_grad_launches(n_layers):
    """Launches of one lipasr_mlp_bounds_grad call per id of BOUNDS_GRAD_KERNELS, for a model of n_layers Dense layers."""
    h = int(n_layers) - 1
    return {"head": 2, "wgrad": h, "back": max(h - 1, 0), "colsum": h}


def mlp_bounds_grad_host(widths, bn, params, bnstate, margin_ibp, lo, hi, y, *, scale_old=0.0, scale_new=1.0, grads=None, ws_offset=0):
    """Host-only: lipasr_mlp_bounds_grad_host on NumPy arrays (margin_ibp, lo, hi as mlp_bounds_host returned them) ->
    dict(grads [n_params], loss_rows [B]).  grads: the buffer that scale_old applies to (default zeros); it is not changed.
    ws_offset: floats the workspace starts past a 16-byte boundary."""
    import numpy as np

    widths = [int(w) for w in widths]
    L = len(widths) - 1
    margin_ibp = np.ascontiguousarray(margin_ibp, dtype=np.float32)
    b = margin_ibp.shape[0]
    params = np.ascontiguousarray(params, dtype=np.float32)
    bnstate = None if bnstate is None else np.ascontiguousarray(bnstate, dtype=np.float32)
    fam = bounds_family_floats(widths, b)
    lo = _host_in(lo, np.float32, (fam,), "lo")
    hi = _host_in(hi, np.float32, (fam,), "hi")
    y = _host_in(y, np.int32, (b,), "y")
    wa, ba = int_array(widths), (None if bn is None else int_array(bn))
    need = sz()
    check(lib.lipasr_mlp_bounds_grad_workspace_host(L, wa, b, C.byref(need)))
    ws = np.zeros(need.value + 8, dtype=np.float32)
    skip = (-(ws.ctypes.data // 4)) % 4 + int(ws_offset)
    wsv = ws[skip:skip + need.value]
    out = {"grads": np.zeros(params.size, np.float32) if grads is None else np.array(grads, dtype=np.float32, copy=True),
           "loss_rows": np.zeros(b, np.float32)}
    check(lib.lipasr_mlp_bounds_grad_host(L, wa, ba, _vp(params), _vp(bnstate), _vp(margin_ibp), _vp(lo), _vp(hi), _vp(y), b, _vp(wsv),
                                          need.value, float(scale_old), float(scale_new), _vp(out["grads"]), _vp(out["loss_rows"])))
    return out


# ids of lipasr_debug_bounds_crown_grad_launches
BOUNDS_CROWN_GRAD_KERNELS = ("soft", "relax", "product", "adjoint", "wgrad", "wreduce", "colsum", "finish", "head")


def bounds_crown_grad_launches(n_layers):
    """Launches of one lipasr_mlp_bounds_crown_grad call at beta > 0 per id of BOUNDS_CROWN_GRAD_KERNELS, for a model of n_layers
    Dense layers; the sweep of lipasr_mlp_bounds_grad that follows counts under bounds_grad_launches(n_layers)."""
    h = int(n_layers) - 1
    return {"soft": 1, "relax": max(h, 1), "product": h, "adjoint": h, "wgrad": h, "wreduce": h, "colsum": h, "finish": h, "head": 1}


def mlp_bounds_crown_grad_host(widths, bn, params, bnstate, margin_ibp, margin_crown, lo, hi, y, beta, *, scale_old=0.0, scale_new=1.0,
                               grads=None, ws_offset=0):
    """Host-only: lipasr_mlp_bounds_crown_grad_host on NumPy arrays (margin_ibp, margin_crown, lo, hi as mlp_bounds_host returned
    them) -> dict(grads [n_params], loss_rows [B]).  grads: the buffer that scale_old applies to (default zeros); it is not
    changed.  ws_offset: floats the workspace starts past a 16-byte boundary."""
    import numpy as np

    widths = [int(w) for w in widths]
    L = len(widths) - 1
    margin_ibp = np.ascontiguousarray(margin_ibp, dtype=np.float32)
    b = margin_ibp.shape[0]
    margin_crown = _host_in(margin_crown, np.float32, (b, widths[-1]), "margin_crown")
    params = np.ascontiguousarray(params, dtype=np.float32)
    bnstate = None if bnstate is None else np.ascontiguousarray(bnstate, dtype=np.float32)
    fam = bounds_family_floats(widths, b)
    lo = _host_in(lo, np.float32, (fam,), "lo")
    hi = _host_in(hi, np.float32, (fam,), "hi")
    y = _host_in(y, np.int32, (b,), "y")
    wa, ba = int_array(widths), (None if bn is None else int_array(bn))
    need = sz()
    check(lib.lipasr_mlp_bounds_crown_grad_workspace_host(L, wa, b, C.byref(need)))
    ws = np.zeros(need.value + 8, dtype=np.float32)
    skip = (-(ws.ctypes.data // 4)) % 4 + int(ws_offset)
    wsv = ws[skip:skip + need.value]
    out = {"grads": np.zeros(params.size, np.float32) if grads is None else np.array(grads, dtype=np.float32, copy=True),
           "loss_rows": np.zeros(b, np.float32)}
    check(lib.lipasr_mlp_bounds_crown_grad_host(L, wa, ba, _vp(params), _vp(bnstate), _vp(margin_ibp), _vp(margin_crown), _vp(lo), _vp(hi),
                                                _vp(y), b, float(beta), _vp(wsv), need.value, float(scale_old), float(scale_new),
                                                _vp(out["grads"]), _vp(out["loss_rows"])))
    return out
