"""ctypes binding of ``include/vitpose_hip.h`` (libvitpose_hip.so).

This is the stub a maintainer of the reference would add next to
``easy_ViTPose/inference.py``.  There is deliberately no
fallback: if the shared object is missing or cannot be loaded, importing the
compute entry points raises ``HipExtensionMissing``.
"""
from __future__ import annotations

import ctypes as C
import os

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_lib', 'libvitpose_hip.so')

VP_OK, VP_ERR_INVALID, VP_ERR_HIP, VP_ERR_STATE, VP_ERR_MISSING_TENSOR, VP_ERR_SHAPE = range(6)
VP_DTYPE_F16, VP_DTYPE_BF16, VP_DTYPE_FP8 = 0, 1, 2
VP_INPUT_F32_NCHW, VP_INPUT_U8_NHWC = 0, 1
VP_PIX_RGB24, VP_PIX_BGR24, VP_PIX_NV12 = 0, 1, 2
VP_YUV_BT601, VP_YUV_BT709, VP_YUV_BT601_FULL = 0, 1, 2
VP_PROF_NAMES = ['gemm_proj', 'gemm_fc1', 'gemm_qkv', 'gemm_patch', 'gemm_deconv', 'gemm_final',
                 'attention', 'layernorm', 'im2col', 'decode', 'gemm_fc2']
VP_PROF_COUNT = len(VP_PROF_NAMES)
DTYPES = {'fp16': VP_DTYPE_F16, 'f16': VP_DTYPE_F16, 'bf16': VP_DTYPE_BF16, 'fp8': VP_DTYPE_FP8}

# every symbol include/vitpose_hip.h declares (tests check the .so exports all of them)
SYMBOLS = ['vp_abi_version', 'vp_create', 'vp_load_weights', 'vp_infer', 'vp_infer_device', 'vp_infer_device_stream', 'vp_host_alloc', 'vp_host_free',
           'vp_infer_submit', 'vp_infer_wait', 'vp_group_create', 'vp_group_size', 'vp_group_member', 'vp_group_load_weights', 'vp_group_infer',
           'vp_group_infer_allgather', 'vp_group_destroy', 'vp_group_last_error', 'vp_infer_frame', 'vp_infer_flip', 'vp_infer_heatmaps',
           'vp_infer_tokens', 'vp_decode_only', 'vp_stream', 'vp_synchronize', 'vp_set_profiling',
           'vp_reset_profile', 'vp_get_profile', 'vp_profile_kernel', 'vp_group_peer_access_missing', 'vp_destroy', 'vp_last_error',
           'vp_dbg_gemm', 'vp_dbg_attention', 'vp_dbg_layernorm', 'vp_dbg_deconv', 'vp_dbg_gemm_case', 'vp_dbg_crop_prep',
           'vp_dbg_group_plan', 'vp_dbg_group_trace', 'vp_dbg_gemm8_pick', 'vp_dbg_gemm2_pick', 'vp_dbg_splitk_pick', 'vp_dbg_run_batch', 'vp_dbg_fp8_gemm', 'vp_dbg_mx_gemm', 'vp_dbg_host_e4m3', 'vp_dbg_gemm_fp8_case', 'vp_dbg_gemm_fp8_case_raw', 'vp_dbg_gemm_fp8_pick', 'vp_dbg_qkvattn',
           'vp_expert_info', 'vp_set_expert', 'vp_infer_experts', 'vp_dbg_expert_tile', 'vp_infer_frames', 'vp_dbg_frame_plan',
           'vp_dbg_chunk_plan', 'vp_infer_boxes_stream', 'vp_dbg_box_geometry',
           'vp_set_flip_test', 'vp_clear_flip_test', 'vp_flip_test_enabled', 'vp_group_set_flip_test', 'vp_group_clear_flip_test',
           'vp_dbg_flip_partner', 'vp_dbg_flip_layout', 'vp_dbg_decode_flip',
           'vp_infer_experts_device_stream', 'vp_infer_frames_experts', 'vp_infer_boxes_experts_stream', 'vp_dbg_mix_plan', 'vp_dbg_decode_mix',
           'vp_set_flip_test_experts', 'vp_dbg_mix_plan_flip', 'vp_dbg_decode_flip_mix',
           'vp_infer_images', 'vp_infer_boxes_images_stream', 'vp_dbg_image_plan', 'vp_dbg_crop_prep_image',
           'vp_dbg_gemm_case_planes', 'vp_dbg_gemm_fp8_case_planes', 'vp_dbg_attention_case',
           'vp_pose_nms_stream', 'vp_pose_nms', 'vp_dbg_pose_nms_host', 'vp_dbg_pose_oks',
           'vp_dbg_ln_finalize', 'vp_dbg_gemm_case_lnpart', 'vp_dbg_qkvattn_ln', 'vp_dbg_ln_quant',
           'vp_infer_images_affine', 'vp_infer_boxes_affine_stream', 'vp_dbg_box_cs', 'vp_dbg_affine_plan', 'vp_dbg_crop_affine', 'vp_dbg_decode_affine',
           'vp_dbg_decode_affine_flip',
           'vp_draw_poses_stream', 'vp_draw_poses', 'vp_dbg_draw_host',
           'vp_draw_labels_stream', 'vp_draw_labels', 'vp_dbg_draw_labels_host', 'vp_dbg_label_text', 'vp_dbg_label_glyph',
           'vp_collect_bytes', 'vp_collect_stream', 'vp_collect', 'vp_dbg_collect_host',
           'vp_tracker_create', 'vp_tracker_destroy', 'vp_tracker_reset_stream', 'vp_tracker_update_stream', 'vp_tracker_update', 'vp_tracker_state_bytes',
           'vp_tracker_download_state', 'vp_dbg_track_host', 'vp_dbg_lsap', 'vp_tracker_update_counted_stream',
           'vp_detector_create', 'vp_detector_destroy', 'vp_detect_stream', 'vp_detect', 'vp_dbg_detect_host',
           'vp_letterbox_plan', 'vp_letterbox_stream', 'vp_letterbox', 'vp_dbg_letterbox_host',
           'vp_orient_plan', 'vp_orient_stream', 'vp_orient', 'vp_dbg_orient_host',
           'vp_smoother_create', 'vp_smoother_destroy', 'vp_smoother_reset_stream', 'vp_smooth_update_stream', 'vp_smooth_update', 'vp_smoother_state_bytes',
           'vp_smoother_download_state', 'vp_dbg_smooth_host',
           'vp_metrics_create', 'vp_metrics_destroy', 'vp_metrics_reset_stream', 'vp_metrics_update_stream', 'vp_metrics_update', 'vp_metrics_snapshot_stream',
           'vp_metrics_state_bytes', 'vp_metrics_download_state', 'vp_dbg_metrics_host',
           'vp_cocoeval_create', 'vp_cocoeval_destroy', 'vp_cocoeval_reset_stream', 'vp_cocoeval_update_stream', 'vp_cocoeval_update', 'vp_cocoeval_accumulate_stream',
           'vp_cocoeval_accumulate', 'vp_cocoeval_state_bytes', 'vp_cocoeval_result_bytes', 'vp_cocoeval_download_state', 'vp_dbg_cocoeval_update_host',
           'vp_dbg_cocoeval_accumulate_host',
           'vp_dbg_head_case', 'vp_dbg_im2col', 'vp_dbg_layernorm_planes',
           'vp_yolo_create', 'vp_yolo_destroy', 'vp_yolo_info', 'vp_yolo_forward_stream', 'vp_yolo_forward', 'vp_dbg_yolo_plan', 'vp_dbg_yolo_fold',
           'vp_dbg_yolo_decode_host', 'vp_dbg_yolo_activation', 'vp_dbg_yolo_conv_case',
           'vp_head_kind', 'vp_dbg_simple_head_pack', 'vp_dbg_simple_head_case']


class HipExtensionMissing(RuntimeError):
    pass


class VpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f'[vitpose_hip status {code}] {msg}')
        self.code = code
        self.msg = msg


class vp_config(C.Structure):
    _fields_ = [('embed_dim', C.c_int32), ('depth', C.c_int32), ('num_heads', C.c_int32),
                ('num_keypoints', C.c_int32), ('dtype', C.c_int32), ('device_id', C.c_int32),
                ('max_batch', C.c_int32)]


class vp_tensor_desc(C.Structure):
    _fields_ = [('name', C.c_char_p), ('data', C.POINTER(C.c_float)), ('numel', C.c_int64)]


class vp_frame(C.Structure):
    _fields_ = [('data', C.c_void_p), ('h', C.c_int32), ('w', C.c_int32)]


class vp_image(C.Structure):
    _fields_ = [('plane', C.c_void_p * 2), ('pitch', C.c_int64 * 2), ('h', C.c_int32), ('w', C.c_int32), ('format', C.c_int32), ('matrix', C.c_int32)]


class vp_pose_nms_cfg(C.Structure):
    _fields_ = [('oks_thr', C.c_float), ('vis_thr', C.c_float), ('use_vis_thr', C.c_int32), ('soft', C.c_int32), ('max_dets', C.c_int32),
                ('n_sigmas', C.c_int32), ('sigmas', C.c_void_p)]


class vp_draw_cfg(C.Structure):
    _fields_ = [('conf_thr', C.c_float), ('radius', C.c_int32), ('thickness', C.c_int32), ('n_limbs', C.c_int32), ('limbs', C.c_void_p),
                ('n_point_colors', C.c_int32), ('point_colors', C.c_void_p), ('n_limb_colors', C.c_int32), ('limb_colors', C.c_void_p)]


class vp_label_cfg(C.Structure):
    _fields_ = [('scale', C.c_int32), ('n_colors', C.c_int32), ('colors', C.c_void_p), ('auto_ink', C.c_int32), ('ink', C.c_uint8 * 3), ('show_score', C.c_int32)]


class vp_track_cfg(C.Structure):
    _fields_ = [('max_age', C.c_int32), ('min_hits', C.c_int32), ('iou_threshold', C.c_float), ('n_streams', C.c_int32)]


class vp_det_cfg(C.Structure):
    _fields_ = [('nc', C.c_int32), ('max_anchors', C.c_int32), ('max_images', C.c_int32), ('dtype', C.c_int32), ('layout', C.c_int32), ('conf_thr', C.c_float),
                ('iou_thr', C.c_float), ('extent', C.c_float), ('agnostic', C.c_int32), ('max_det', C.c_int32), ('class_mask', C.c_uint32 * 8)]


class vp_det_image(C.Structure):
    _fields_ = [('gain', C.c_float), ('pad_x', C.c_float), ('pad_y', C.c_float), ('frame_w', C.c_float), ('frame_h', C.c_float)]


class vp_letterbox_cfg(C.Structure):
    _fields_ = [('in_h', C.c_int32), ('in_w', C.c_int32), ('dtype', C.c_int32), ('layout', C.c_int32), ('order', C.c_int32), ('pad_value', C.c_int32),
                ('scaleup', C.c_int32)]


class vp_smooth_cfg(C.Structure):
    _fields_ = [('min_cutoff', C.c_double), ('beta', C.c_double), ('d_cutoff', C.c_double), ('max_age', C.c_int32), ('n_streams', C.c_int32),
                ('n_joints', C.c_int32), ('max_rows', C.c_int32), ('missing', C.c_int32)]


class vp_metrics_cfg(C.Structure):
    _fields_ = [('auc_norm', C.c_double), ('pck_thr', C.c_float * 8), ('vis_thr', C.c_float), ('n_joints', C.c_int32), ('n_pck', C.c_int32), ('auc_steps', C.c_int32),
                ('use_oks', C.c_int32), ('reserved', C.c_int32)]


class vp_cocoeval_cfg(C.Structure):
    _fields_ = [('n_joints', C.c_int32), ('max_records', C.c_int32), ('reserved', C.c_int32 * 2)]


class vp_yolo_cfg(C.Structure):
    _fields_ = [('in_h', C.c_int32), ('in_w', C.c_int32), ('max_images', C.c_int32), ('input_layout', C.c_int32), ('head_dtype', C.c_int32), ('head_layout', C.c_int32),
                ('reserved', C.c_int32 * 2)]


class vp_yolo_tensor(C.Structure):
    _fields_ = [('name', C.c_char_p), ('data', C.POINTER(C.c_float)), ('numel', C.c_int64), ('ndim', C.c_int32), ('shape', C.c_int32 * 4), ('reserved', C.c_int32)]


class vp_yolo_launch(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('kind', 'layer', 'conv', 'k', 's', 'act', 'f32_out', 'h_in', 'w_in', 'h_out', 'w_out', 'c_in', 'c_out', 'in_buf', 'in_off',
                                         'in_stride', 'out_buf', 'out_off', 'out_stride', 'res_buf', 'res_off', 'res_stride')] + [('reserved', C.c_int32 * 2)]


class vp_yolo_buffer(C.Structure):
    _fields_ = [('h', C.c_int32), ('w', C.c_int32), ('c', C.c_int32), ('elem_bytes', C.c_int32)]


class vp_profile(C.Structure):
    _fields_ = [('ms', C.c_double * VP_PROF_COUNT), ('flops', C.c_double * VP_PROF_COUNT),
                ('bytes', C.c_double * VP_PROF_COUNT), ('launches', C.c_int64 * VP_PROF_COUNT)]


_lib = None


def load_library():
    """dlopen the in-tree HIP library (once).  Raises HipExtensionMissing loudly."""
    global _lib
    if _lib is not None:
        return _lib
    lib_path = os.environ.get('VP_HIP_LIB', LIB_PATH)   # kernel development only: A/B two builds on the same box
    if not os.path.exists(lib_path):
        raise HipExtensionMissing(
            f'{lib_path} not found. Build it with `python -m easy_vitpose_amd.build` '
            '(needs hipcc). There is no CPU fallback for the ViTPose path.')
    try:
        lib = C.CDLL(lib_path)
    except OSError as e:  # e.g. libamdhip64 missing
        raise HipExtensionMissing(f'cannot load {lib_path}: {e}') from e
    H = C.c_void_p
    lib.vp_abi_version.restype = C.c_int
    lib.vp_create.argtypes = [C.POINTER(H), C.POINTER(vp_config)]
    lib.vp_load_weights.argtypes = [H, C.POINTER(vp_tensor_desc), C.c_int32]
    lib.vp_infer.argtypes = [H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.vp_infer_device.argtypes = [H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
    lib.vp_infer_device_stream.argtypes = [H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp_host_alloc.argtypes = [C.c_size_t]
    lib.vp_host_alloc.restype = C.c_void_p
    lib.vp_host_free.argtypes = [C.c_void_p]
    lib.vp_host_free.restype = None
    lib.vp_infer_submit.argtypes = [H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    lib.vp_infer_wait.argtypes = [H, C.c_int32]
    lib.vp_group_create.argtypes = [C.POINTER(H), C.POINTER(vp_config), C.POINTER(C.c_int32), C.c_int32]
    lib.vp_group_size.argtypes = [H]
    lib.vp_group_member.argtypes = [H, C.c_int32]
    lib.vp_group_member.restype = C.c_void_p
    lib.vp_group_load_weights.argtypes = [H, C.POINTER(vp_tensor_desc), C.c_int32]
    lib.vp_group_infer.argtypes = [H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.vp_group_infer_allgather.argtypes = [H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]
    lib.vp_group_destroy.argtypes = [H]
    lib.vp_group_last_error.argtypes = [H]
    lib.vp_group_last_error.restype = C.c_char_p
    lib.vp_infer_frame.argtypes = [H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.vp_infer_frames.argtypes = [H, C.POINTER(vp_frame), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.vp_dbg_frame_plan.argtypes = [C.POINTER(vp_frame), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.vp_infer_boxes_stream.argtypes = [H, C.POINTER(vp_frame), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp_dbg_box_geometry.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.vp_dbg_crop_prep.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.vp_infer_heatmaps.argtypes = [H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.vp_infer_tokens.argtypes = [H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.vp_decode_only.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.vp_stream.argtypes = [H]
    lib.vp_stream.restype = C.c_void_p
    lib.vp_synchronize.argtypes = [H]
    lib.vp_set_profiling.argtypes = [H, C.c_int32]
    lib.vp_reset_profile.argtypes = [H]
    lib.vp_get_profile.argtypes = [H, C.POINTER(vp_profile)]
    lib.vp_destroy.argtypes = [H]
    lib.vp_last_error.argtypes = [H]
    lib.vp_last_error.restype = C.c_char_p
    lib.vp_dbg_gemm.argtypes = [C.c_int32] * 6 + [C.c_void_p] * 5
    lib.vp_dbg_attention.argtypes = [C.c_int32] * 5 + [C.c_void_p] * 2
    lib.vp_dbg_attention_case.argtypes = [C.c_int32] * 6 + [C.c_void_p] * 3
    lib.vp_dbg_layernorm.argtypes = [C.c_int32] * 4 + [C.c_void_p] * 5
    lib.vp_dbg_deconv.argtypes = [C.c_int32] * 6 + [C.c_void_p, C.POINTER(vp_tensor_desc), C.c_int32, C.c_void_p]
    lib.vp_infer_flip.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                  C.c_void_p, C.c_void_p]
    lib.vp_dbg_gemm_case.argtypes = [C.c_int32] * 9 + [C.c_void_p] * 8
    if hasattr(lib, 'vp_dbg_gemm8_timeline'):   # the measurement build (include/vitpose_hip_tools.h; tools/ point VP_HIP_LIB at it)
        lib.vp_dbg_gemm8_timeline.argtypes = [C.c_int32] * 9 + [C.POINTER(C.c_uint64), C.c_int32]
        lib.vp_dbg_gemm_timeline.argtypes = [C.c_int32] * 6 + [C.POINTER(C.c_uint64), C.c_int32]
        lib.vp_dbg_gemm8_timeline.restype = lib.vp_dbg_gemm_timeline.restype = C.c_int
        lib.vp_dbg_gemm_bench.argtypes = [C.c_int32] * 9 + [C.POINTER(C.c_float)]
        lib.vp_dbg_gemm_bench2.argtypes = [C.c_int32] * 10 + [C.POINTER(C.c_float)]
        lib.vp_dbg_gemm_compare.argtypes = [C.c_int32] * 13 + [C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        lib.vp_dbg_peak.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_double)]
        for n_ in ('vp_dbg_gemm_bench', 'vp_dbg_gemm_bench2', 'vp_dbg_gemm_compare', 'vp_dbg_peak'):
            getattr(lib, n_).restype = C.c_int
    lib.vp_profile_kernel.argtypes = [H, C.c_int32, C.c_char_p, C.c_int32]
    lib.vp_group_peer_access_missing.argtypes = [H]
    lib.vp_dbg_group_plan.argtypes = [C.c_int32] * 3 + [C.c_void_p, C.c_void_p, C.c_int32]
    lib.vp_dbg_gemm8_pick.argtypes = [C.c_int32] * 4 + [C.c_void_p]
    lib.vp_dbg_gemm2_pick.argtypes = [C.c_int32] * 4 + [C.c_void_p]
    lib.vp_dbg_splitk_pick.argtypes = [C.c_int32] * 3 + [C.c_void_p]
    lib.vp_dbg_run_batch.argtypes = [C.c_int32] * 3
    lib.vp_dbg_group_trace.argtypes = [C.c_int32] * 3 + [C.c_void_p, C.c_int32]
    lib.vp_dbg_fp8_gemm.argtypes = [C.c_int32] * 4 + [C.c_void_p] * 7
    lib.vp_dbg_mx_gemm.argtypes = [C.c_int32] * 4 + [C.c_void_p] * 7
    lib.vp_dbg_host_e4m3.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.vp_dbg_gemm_fp8_case.argtypes = [C.c_int32] * 5 + [C.c_void_p] * 8
    lib.vp_dbg_gemm_fp8_case_raw.argtypes = [C.c_int32] * 5 + [C.c_void_p] * 8 + [C.c_int32] + [C.c_void_p] * 3
    lib.vp_dbg_gemm_fp8_pick.argtypes = [C.c_int32] * 3 + [C.c_void_p] * 2
    lib.vp_dbg_gemm_case_planes.argtypes = [C.c_int32] * 9 + [C.c_void_p] * 6 + [C.c_int32] + [C.c_void_p] * 3
    lib.vp_dbg_gemm_fp8_case_planes.argtypes = [C.c_int32] * 4 + [C.c_void_p] * 5 + [C.c_int32] + [C.c_void_p] * 5
    lib.vp_expert_info.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp_set_expert.argtypes = [H, C.c_int32]
    lib.vp_infer_experts.argtypes = [H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp_dbg_expert_tile.argtypes = [C.c_int32] * 4 + [C.c_void_p, C.c_int32]
    lib.vp_infer_experts_device_stream.argtypes = [H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp_infer_frames_experts.argtypes = [H, C.POINTER(vp_frame), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.vp_infer_boxes_experts_stream.argtypes = [H, C.POINTER(vp_frame), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp_dbg_mix_plan.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6
    lib.vp_dbg_decode_mix.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp_dbg_chunk_plan.argtypes = [C.POINTER(vp_config), C.c_int32, C.c_void_p, C.c_int32]
    lib.vp_dbg_qkvattn.argtypes = [C.c_int32] * 5 + [C.c_void_p] * 4
    lib.vp_dbg_qkvattn_ln.argtypes = [C.c_int32] * 5 + [C.c_void_p] * 6
    lib.vp_dbg_ln_finalize.argtypes = [C.c_int32] * 4 + [C.c_void_p] * 2
    lib.vp_dbg_gemm_case_lnpart.argtypes = [C.c_int32] * 9 + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 2
    lib.vp_dbg_ln_quant.argtypes = [C.c_int32] * 5 + [C.c_void_p] * 4
    lib.vp_head_kind.argtypes = [H]
    lib.vp_dbg_simple_head_pack.argtypes = [C.c_int32] * 3 + [C.c_void_p] * 3
    lib.vp_dbg_simple_head_case.argtypes = [C.c_int32] * 4 + [C.c_void_p] * 3 + [C.c_int32, C.c_void_p, C.c_void_p]
    lib.vp_dbg_head_case.argtypes = [C.c_int32] * 9 + [C.c_void_p, C.POINTER(vp_tensor_desc), C.c_int32, C.c_int32] + [C.c_void_p] * 6
    lib.vp_dbg_im2col.argtypes = [C.c_int32] * 6 + [C.c_void_p] * 3
    lib.vp_dbg_layernorm_planes.argtypes = [C.c_int32] * 5 + [C.c_void_p] * 6
    lib.vp_set_flip_test.argtypes = [H, C.c_void_p, C.c_int32, C.c_int32]
    lib.vp_clear_flip_test.argtypes = [H]
    lib.vp_flip_test_enabled.argtypes = [H]
    lib.vp_group_set_flip_test.argtypes = [H, C.c_void_p, C.c_int32, C.c_int32]
    lib.vp_group_clear_flip_test.argtypes = [H]
    lib.vp_set_flip_test_experts.argtypes = [H, C.c_void_p, C.c_void_p, C.c_int32]
    lib.vp_dbg_mix_plan_flip.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6
    lib.vp_dbg_decode_flip_mix.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.vp_infer_images.argtypes = [H, C.POINTER(vp_image), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.vp_infer_boxes_images_stream.argtypes = [H, C.POINTER(vp_image), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp_dbg_image_plan.argtypes = [C.POINTER(vp_image), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.vp_dbg_crop_prep_image.argtypes = [C.c_int32, C.POINTER(vp_image), C.c_void_p, C.c_int32, C.c_void_p]
    lib.vp_dbg_flip_partner.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.vp_dbg_flip_layout.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.vp_dbg_decode_flip.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    nms_host = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(vp_pose_nms_cfg), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp_pose_nms_stream.argtypes = [H] + nms_host + [C.c_void_p]
    lib.vp_pose_nms.argtypes = [H] + nms_host
    lib.vp_dbg_pose_nms_host.argtypes = nms_host
    lib.vp_dbg_pose_oks.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(vp_pose_nms_cfg), C.c_void_p]
    lib.vp_infer_images_affine.argtypes = [H, C.POINTER(vp_image), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.vp_infer_boxes_affine_stream.argtypes = [H, C.POINTER(vp_image), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp_dbg_box_cs.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]
    lib.vp_dbg_affine_plan.argtypes = [C.POINTER(vp_image), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.vp_dbg_crop_affine.argtypes = [C.c_int32, C.POINTER(vp_image), C.c_void_p, C.c_int32, C.c_void_p]
    lib.vp_dbg_decode_affine.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.vp_dbg_decode_affine_flip.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    draw_host = [C.POINTER(vp_image), C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                 C.POINTER(vp_draw_cfg)]
    lib.vp_draw_poses_stream.argtypes = [H] + draw_host + [C.c_void_p]
    lib.vp_draw_poses.argtypes = [H] + draw_host
    lib.vp_dbg_draw_host.argtypes = draw_host
    label_host = [C.POINTER(vp_image), C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                  C.POINTER(vp_label_cfg)]
    lib.vp_draw_labels_stream.argtypes = [H] + label_host + [C.c_void_p]
    lib.vp_draw_labels.argtypes = [H] + label_host
    lib.vp_dbg_draw_labels_host.argtypes = label_host
    lib.vp_dbg_label_text.argtypes = [C.c_int32, C.c_int32, C.c_float, C.c_char_p]
    lib.vp_dbg_label_glyph.argtypes = [C.c_int32]
    collect_host = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.vp_collect_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.vp_collect_stream.argtypes = [H] + collect_host + [C.c_void_p]
    lib.vp_collect.argtypes = [H] + collect_host
    lib.vp_dbg_collect_host.argtypes = collect_host
    trk_io = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.vp_tracker_create.argtypes = [H, C.POINTER(vp_track_cfg), C.POINTER(C.c_void_p)]
    lib.vp_tracker_destroy.argtypes = [C.c_void_p]
    lib.vp_tracker_reset_stream.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.vp_tracker_update_stream.argtypes = [C.c_void_p] + trk_io + [C.c_void_p]
    lib.vp_tracker_update.argtypes = [C.c_void_p] + trk_io
    lib.vp_tracker_state_bytes.argtypes = [C.c_int32, C.POINTER(C.c_int64)]
    lib.vp_tracker_download_state.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp_dbg_track_host.argtypes = [C.c_void_p, C.POINTER(vp_track_cfg)] + trk_io
    lib.vp_dbg_lsap.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p]
    lib.vp_tracker_update_counted_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    det_io = [C.c_void_p, C.c_int32, C.POINTER(vp_det_image), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.vp_detector_create.argtypes = [H, C.POINTER(vp_det_cfg), C.POINTER(C.c_void_p)]
    lib.vp_detector_destroy.argtypes = [C.c_void_p]
    lib.vp_detect_stream.argtypes = [C.c_void_p] + det_io + [C.c_void_p]
    lib.vp_detect.argtypes = [C.c_void_p] + det_io
    lib.vp_dbg_detect_host.argtypes = [C.POINTER(vp_det_cfg)] + det_io
    lb_io = [C.POINTER(vp_letterbox_cfg), C.POINTER(vp_image), C.c_int32]
    lb_tabs = [C.POINTER(vp_det_image), C.c_void_p]
    lib.vp_letterbox_plan.argtypes = lb_io + lb_tabs
    lib.vp_letterbox_stream.argtypes = [H] + lb_io + [C.c_void_p] + lb_tabs + [C.c_void_p]
    lib.vp_letterbox.argtypes = [H] + lb_io + [C.c_void_p] + lb_tabs
    lib.vp_dbg_letterbox_host.argtypes = lb_io + [C.c_void_p] + lb_tabs
    orient_io = [C.POINTER(vp_image), C.c_void_p, C.POINTER(vp_image), C.c_int32]
    lib.vp_orient_plan.argtypes = [C.POINTER(vp_image), C.c_void_p, C.c_int32, C.POINTER(vp_image), C.c_void_p]
    lib.vp_orient_stream.argtypes = [H] + orient_io + [C.c_void_p]
    lib.vp_orient.argtypes = [H] + orient_io
    lib.vp_dbg_orient_host.argtypes = orient_io
    smooth_io = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp_smoother_create.argtypes = [H, C.POINTER(vp_smooth_cfg), C.POINTER(C.c_void_p)]
    lib.vp_smoother_destroy.argtypes = [C.c_void_p]
    lib.vp_smoother_reset_stream.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.vp_smooth_update_stream.argtypes = [C.c_void_p] + smooth_io + [C.c_void_p]
    lib.vp_smooth_update.argtypes = [C.c_void_p] + smooth_io
    lib.vp_smoother_state_bytes.argtypes = [C.POINTER(vp_smooth_cfg), C.POINTER(C.c_int64)]
    lib.vp_smoother_download_state.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp_dbg_smooth_host.argtypes = [C.c_void_p, C.POINTER(vp_smooth_cfg)] + smooth_io
    metrics_io = [C.c_void_p] * 6 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.vp_metrics_create.argtypes = [H, C.POINTER(vp_metrics_cfg), C.c_void_p, C.POINTER(C.c_void_p)]
    lib.vp_metrics_destroy.argtypes = [C.c_void_p]
    lib.vp_metrics_reset_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp_metrics_update_stream.argtypes = [C.c_void_p] + metrics_io + [C.c_void_p]
    lib.vp_metrics_update.argtypes = [C.c_void_p] + metrics_io
    lib.vp_metrics_snapshot_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp_metrics_state_bytes.argtypes = [C.POINTER(vp_metrics_cfg), C.POINTER(C.c_int64)]
    lib.vp_metrics_download_state.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp_dbg_metrics_host.argtypes = [C.c_void_p, C.POINTER(vp_metrics_cfg), C.c_void_p] + metrics_io
    coco_io = [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 5 + [C.c_int32, C.c_int32, C.c_void_p]
    lib.vp_cocoeval_create.argtypes = [H, C.POINTER(vp_cocoeval_cfg), C.c_void_p, C.POINTER(C.c_void_p)]
    lib.vp_cocoeval_destroy.argtypes = [C.c_void_p]
    lib.vp_cocoeval_reset_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp_cocoeval_update_stream.argtypes = [C.c_void_p] + coco_io + [C.c_void_p]
    lib.vp_cocoeval_update.argtypes = [C.c_void_p] + coco_io
    lib.vp_cocoeval_accumulate_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp_cocoeval_accumulate.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp_cocoeval_state_bytes.argtypes = [C.POINTER(vp_cocoeval_cfg), C.POINTER(C.c_int64)]
    lib.vp_cocoeval_result_bytes.argtypes = [C.POINTER(C.c_int64)]
    lib.vp_cocoeval_download_state.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp_dbg_cocoeval_update_host.argtypes = [C.c_void_p, C.POINTER(vp_cocoeval_cfg), C.c_void_p] + coco_io
    lib.vp_dbg_cocoeval_accumulate_host.argtypes = [C.c_void_p, C.POINTER(vp_cocoeval_cfg), C.c_void_p]
    yolo_ck = [C.POINTER(vp_yolo_cfg), C.POINTER(vp_yolo_tensor), C.c_int32]
    lib.vp_yolo_create.argtypes = [H] + yolo_ck + [C.POINTER(C.c_void_p)]
    lib.vp_yolo_destroy.argtypes = [C.c_void_p]
    lib.vp_yolo_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    lib.vp_yolo_forward_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.vp_yolo_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.vp_dbg_yolo_plan.argtypes = yolo_ck + [C.POINTER(vp_yolo_launch), C.c_int32, C.POINTER(vp_yolo_buffer), C.c_int32, C.c_void_p]
    lib.vp_dbg_yolo_fold.argtypes = yolo_ck + [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp_dbg_yolo_decode_host.argtypes = [C.c_int32] * 4 + [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.vp_dbg_yolo_activation.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.vp_dbg_yolo_conv_case.argtypes = [H, C.POINTER(vp_yolo_launch), C.c_int32] + [C.c_void_p] * 5
    for name in SYMBOLS:
        if name not in ('vp_stream', 'vp_last_error', 'vp_host_alloc', 'vp_host_free', 'vp_group_member', 'vp_group_last_error'):
            getattr(lib, name).restype = C.c_int
    lib.vp_dbg_label_glyph.restype = C.c_uint64
    lib.vp_collect_bytes.restype = C.c_int64
    _lib = lib
    return lib


def last_error(handle=None) -> str:
    lib = load_library()
    s = lib.vp_last_error(handle)
    return s.decode('utf-8', 'replace') if s else ''


def check(code: int, handle=None):
    if code != VP_OK:
        raise VpError(code, last_error(handle))
