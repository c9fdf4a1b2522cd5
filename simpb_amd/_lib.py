"""ctypes binding of include/simpb_hip.h. The library is mandatory: there is no CPU or PyTorch
fallback behind these entry points, and a missing .so is an error, not a silent downgrade."""
import ctypes
import os

from .build import LIB

_lib = None

_P = ctypes.c_void_p
_I = ctypes.c_int
_F = ctypes.c_float
_LL = ctypes.c_longlong


class WorldTables(ctypes.Structure):
    """simpb_world_tables of include/simpb_hip.h, passed by value."""
    _fields_ = [("class_range", _F * 32), ("attr_moving", ctypes.c_ubyte * 32), ("attr_still", ctypes.c_ubyte * 32),
                ("threshold", _F), ("has_threshold", _I), ("num_output", _I)]


class RigCamera(ctypes.Structure):
    """simpb_rig_camera of include/simpb_hip.h: one camera of a rig (simpb_preprocess_rig_nhwc4_f16 takes a host array of them)."""
    _fields_ = ([(n, _I) for n in ("format", "src_height", "src_width", "src_row0", "src_rows", "taps_x", "taps_y", "flip")] +
                [(n, _LL) for n in ("pitch", "chroma_pitch", "chroma_offset")] +
                [(n, _I) for n in ("kx_offset", "x_offset", "ky_offset", "y_offset", "mid_row", "yoff", "iy", "irv", "igu", "igv", "ibu")] +
                [("chroma2_offset", _LL)])


class HealthParams(ctypes.Structure):
    """simpb_health_params of include/simpb_hip.h, passed by value."""
    _fields_ = [("dark_below", ctypes.c_double), ("bright_above", ctypes.c_double), ("flat_below", ctypes.c_double),
                ("mean", ctypes.c_double * 3), ("std", ctypes.c_double * 3),
                ("check_dark", _I), ("check_bright", _I), ("check_flat", _I), ("check_frozen", _I), ("frozen_after", _I), ("act", _I)]


SIGNATURES = {
    "simpb_abi_version": ([], _I),
    "simpb_last_error": ([], ctypes.c_char_p),
    "simpb_timing_enable": ([_I], _I),
    "simpb_timing_read": ([_I, _P, _I], _I),
    "simpb_timing_reset": ([], None),
    "simpb_deformable_aggregation_forward": ([_P] * 6 + [_I] * 8 + [_P], _I),
    "simpb_dfa_fused_forward": ([_P, _P, _I] + [_P] * 11 + [_I] * 9 + [_P], _I),
    "simpb_dfa_fused_forward_cams": ([_P, _P, _I] + [_P] * 11 + [_I] * 9 + [_P, _P], _I),
    "simpb_dfa_fused_forward_rig": ([_P, _P, _I] + [_P] * 11 + [_I] * 9 + [_P, _P], _I),
    "simpb_deformable_aggregation_backward": ([_P] * 9 + [_I] * 8 + [_P], _I),
    "simpb_ms_deform_attn_grouped_forward": ([_P] * 7 + [_I] * 8 + [_P], _I),
    "simpb_msda_linear_forward": ([_P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _P, _P] + [_I] * 8 + [_P], _I),
    "simpb_ms_deform_attn_grouped_backward": ([_P] * 10 + [_I] * 8 + [_P], _I),
    "simpb_linear_f32": ([_P] * 4 + [_I] * 4 + [_P], _I),
    "simpb_linear_f16x3": ([_P] * 5 + [_I] * 3 + [_P], _I),
    "simpb_gemm_f32": ([_P, _P], _I),
    "simpb_layernorm_f32": ([_P, _I, _P, _I, _I, _P, _I, _I, _P, _P, _I, _P, _P], _I),
    "simpb_bias_act_nhwc_f16": ([_P, _P, _P, ctypes.c_longlong, _I, _I, _P], _I),
    "simpb_bias_relu_maxpool_nhwc_f16": ([_P, _P, _P, _I, _I, _I, _I, _P], _I),
    "simpb_conv1x1_nhwc_f16": ([_P] * 5 + [_I] * 8 + [_P, _I, _P], _I),
    "simpb_conv3x3_nhwc_f16": ([_P, _P, _P, _I, _I, _P, _P, _P] + [_I] * 8 + [_P], _I),
    "simpb_conv3x3_choose_variant": ([_LL, _I, _I], _I),
    "simpb_conv3x3_group_tokens_f16": ([_I, _P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _P], _I),
    "simpb_conv3x3_choose_resident": ([_LL, _I, _I, _I, _I, _I], _I),
    "simpb_conv3x3_group_choose_resident": ([_I, _I, _P, _P, _I, _I], _I),
    "simpb_conv3x3_group_tokens_forms_f16": ([_I, _P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _P, _P], _I),
    "simpb_stem_conv7x7_pool_f16": ([_P] * 4 + [_I] * 4 + [_P], _I),
    # the same four with a trailing live-image table (NULL: the entry point without the suffix)
    "simpb_stem_conv7x7_pool_f16_live": ([_P] * 4 + [_I] * 4 + [_P, _P], _I),
    "simpb_conv1x1_nhwc_f16_live": ([_P] * 5 + [_I] * 8 + [_P, _I, _P, _P], _I),
    "simpb_conv3x3_nhwc_f16_live": ([_P, _P, _P, _I, _I, _P, _P, _P] + [_I] * 8 + [_P, _P], _I),
    "simpb_conv3x3_group_tokens_forms_f16_live": ([_I, _P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _P, _P, _P], _I),
    "simpb_image_to_nhwc4_f16": ([_P, _P] + [ctypes.c_longlong] * 4 + [_I] * 4 + [_P], _I),
    "simpb_preprocess_u8_nhwc4_f16": ([_P] * 10 + [_I] * 11 + [_P], _I),
    "simpb_preprocess_yuv420sp_nhwc4_f16": ([_P] * 10 + [_I] * 18 + [_P], _I),
    "simpb_preprocess_surface_nhwc4_f16": ([_P] * 11 + [_I] * 12 + [_LL] * 4 + [_I] * 6 + [_P], _I),
    "simpb_preprocess_planes_nhwc4_f16": ([_P] * 11 + [_I] * 12 + [_LL] * 5 + [_I] * 6 + [_P], _I),
    "simpb_preprocess_mid_pitch": ([_I], _I),
    "simpb_preprocess_rig_nhwc4_f16": ([_P] * 10 + [ctypes.POINTER(RigCamera)] + [_I] * 10 + [_P], _I),
    # the two above with a camera roll: + host int32 [cams][6] (and, uniform, the number of rows)
    "simpb_preprocess_roll_nhwc4_f16": ([_P] * 11 + [_I] * 12 + [_LL] * 5 + [_I] * 6 + [ctypes.POINTER(_I), _I, _P], _I),
    "simpb_preprocess_rig_roll_nhwc4_f16": ([_P] * 10 + [ctypes.POINTER(RigCamera)] + [_I] * 10 + [ctypes.POINTER(_I), _P], _I),
    "simpb_linear_f16in_split": ([_P] * 5 + [_I] * 3 + [_P], _I),
    "simpb_format_tokens": ([_P, _P, _P, _P, _I, _I, _I, _I, _P], _I),
    "simpb_attention_f32": ([_P] * 6 + [_I] * 9 + [_F, _P], _I),
    "simpb_attention_f32_split": ([_P] * 6 + [_I] * 9 + [_F, _P], _I),
    "simpb_attention_split_halfs": ([_P] * 6 + [_I] * 9 + [_P], _I),
    "simpb_attention_select": ([_I] + [_P] * 7 + [_I] * 12 + [_F, _P], _I),
    "simpb_mlp_chain_forward": ([_P, _P], _I),
    "simpb_bank_get": ([_P] * 6 + [_I] * 2 + [_F] * 2 + [_P], _I),
    "simpb_bank_get_restart": ([_P] * 6 + [_I] * 2 + [_F] * 2 + [_P, _P], _I),
    "simpb_bank_update": ([_P] * 10 + [_I] * 5 + [_P], _I),
    "simpb_bank_update_rank": ([_P, _P] + [_I] * 4 + [_P], _I),
    "simpb_bank_update_merge": ([_P] * 13 + [_I, _P] + [_I] * 5 + [_P], _I),
    "simpb_bank_update_merge_active": ([_P] * 13 + [_I, _P] + [_I] * 5 + [_P, _P], _I),
    "simpb_bank_cache": ([_P] * 10 + [_I] * 6 + [_F, _I, _F, _P, _I, _P, _P], _I),
    "simpb_bank_cache_streams": ([_P] * 10 + [_I] * 6 + [_F, _I, _F, _P, _I, _P, _P, _P], _I),
    "simpb_bank_cache_streams_active": ([_P] * 10 + [_I] * 6 + [_F, _I, _F, _P, _I, _P, _P, _P, _P], _I),
    "simpb_bank_cache_streams_restart": ([_P] * 10 + [_I] * 6 + [_F, _I, _F, _P, _I, _P, _P, _P, _P, _P], _I),
    "simpb_bank_export_stream": ([_P] * 5 + [_I] * 6 + [_P], _I),
    "simpb_bank_import_stream": ([_P] * 6 + [_I] * 6 + [_P], _I),
    "simpb_decode3d_record": ([_P] * 6 + [_I] * 4 + [_P], _I),
    "simpb_decode2d_record": ([_P] * 6 + [_I] * 4 + [_F] * 4 + [_P], _I),
    "simpb_record2d_compact": ([_P, _LL, _P, _LL, _I, _I, _I, _P], _I),
    "simpb_decode2d_record_ragged": ([_P] * 7 + [_I] * 5 + [_F] * 4 + [_P], _I),
    "simpb_decode2d_record_cams": ([_P] * 6 + [_I] * 4 + [_P, _I, _P], _I),
    "simpb_decode2d_record_ragged_cams": ([_P] * 7 + [_I] * 5 + [_P, _P], _I),
    "simpb_world_record": ([_P] * 5 + [WorldTables, _I, _P], _I),
    "simpb_image_health_stats": ([_P, _P, _I, _I, _I, _P], _I),
    "simpb_image_health_partials_bytes": ([_I, _I, _I], _I),
    "simpb_camera_health_verdict": ([_P] * 6 + [HealthParams] + [_I] * 4 + [_P], _I),
    "simpb_topk_rows": ([_P, _P, _P, _I, _I, _I, _P], _I),
    "simpb_rowdot_sigmoid": ([_P, _P, _I, _P, _P, _I, _I, _P, _P], _I),
    "simpb_anchor_projection": ([_P] * 4 + [_I] * 2 + [_P], _I),
    "simpb_msda_prep": ([_P, _P, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P], _I),
    "simpb_dfa_points": ([_P] * 7 + [_I] * 5 + [_P], _I),
    "simpb_dfa_weights": ([_P] * 3 + [_I] * 6 + [_P], _I),
    "simpb_dfa_points_cams": ([_P] * 7 + [_I] * 5 + [_P, _P], _I),
    "simpb_dfa_weights_cams": ([_P] * 3 + [_I] * 6 + [_P, _P], _I),
    "simpb_alloc_project_cams": ([_P] * 5 + [_I] * 3 + [_F] * 5 + [_P, _P], _I),
    "simpb_alloc_project": ([_P] * 5 + [_I] * 3 + [_F] * 5 + [_P], _I),
    "simpb_alloc_compact": ([_P] * 3 + [_I] * 3 + [_P], _I),
    "simpb_alloc_group_start": ([_P] * 3 + [_I] * 3 + [_P], _I),
    "simpb_alloc_scatter": ([_P] * 12 + [_I] * 4 + [_F] * 2 + [_P], _I),
    "simpb_alloc_static": ([_P] * 15 + [_I] * 4 + [_F] * 5 + [_P], _I),
    "simpb_alloc_ragged": ([_P] * 15 + [_I] * 4 + [_F] * 5 + [_P], _I),
    "simpb_alloc_ragged_active": ([_P] * 15 + [_I] * 4 + [_F] * 5 + [_P, _P], _I),
    "simpb_alloc_static_cams": ([_P] * 15 + [_I] * 4 + [_F] * 5 + [_P, _P], _I),
    "simpb_alloc_ragged_cams": ([_P] * 15 + [_I] * 4 + [_F] * 5 + [_P, _P, _P], _I),
    "simpb_gather_rows": ([_P] * 3 + [_I] * 4 + [_P], _I),
    "simpb_aggregate_2d_to_3d": ([_P] * 8 + [_I] * 5 + [_P], _I),
    "simpb_aggregate_2d_to_3d_alpha": ([_P] * 9 + [_I, _I, _P, _P] + [_I] * 5 + [_P], _I),
}

ERRORS = {1: "SIMPB_EINVAL (bad pointer/size/layout)", 2: "SIMPB_ELAUNCH (kernel launch failed)"}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise RuntimeError(
                f"{LIB} is missing: build it with `python -m simpb_amd.build` (hipcc --offload-arch=gfx950). "
                "simpb_amd has no fallback path for its HIP kernels.")
        # torch first: it brings its own HIP runtime (libamdhip64), and the library must bind to
        # that one. Loaded the other way round the process ends up with two runtimes and the
        # kernels launch on one that never saw the device ("no ROCm-capable device is detected").
        import torch  # noqa: F401
        handle = ctypes.CDLL(LIB)
        for name, (argtypes, restype) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if include/simpb_hip.h and the .so disagree
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        detail = ""
        if status == 2:
            detail = " - " + (lib().simpb_last_error() or b"").decode()
        raise RuntimeError(f"{what} failed: {ERRORS.get(status, status)}{detail}")
