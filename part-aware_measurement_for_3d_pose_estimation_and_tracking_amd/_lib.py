"""ctypes binding of csrc/libpam_hip.so (the C ABI declared in include/pam.h).

There is deliberately no CPU fallback: if the library is missing or does not load, importing the product path
raises with the build command.  Build with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C <package>/csrc``."""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PAM_LIB') or os.path.join(_HERE, 'csrc', 'libpam_hip.so')     # PAM_LIB: another build of the same library (tools/ab_build.sh)

PAM_J = 17
PAM_MAX_TAPS = 16
PAM_EXP_TABLE = 64


class PamParams(C.Structure):
    _fields_ = [
        ('conf_threshold', C.c_double), ('epi_threshold', C.c_double), ('init_threshold', C.c_double),
        ('joint_threshold', C.c_double), ('alpha2d', C.c_double), ('lambda_a', C.c_double), ('lambda_t', C.c_double),
        ('n_init', C.c_int32), ('max_age', C.c_int32), ('count_gate', C.c_int32), ('n_taps_body', C.c_int32),
        ('n_taps_arm', C.c_int32), ('reserved', C.c_int32),
        ('taps_body', C.c_double * PAM_MAX_TAPS), ('taps_arm', C.c_double * PAM_MAX_TAPS),
        ('exp_lambda_a', C.c_double * PAM_EXP_TABLE), ('w_lambda_t', C.c_double * 4),
    ]


class PamOneEuro(C.Structure):
    _fields_ = [('freq', C.c_double), ('mincutoff', C.c_double), ('beta', C.c_double), ('dcutoff', C.c_double)]


class PamOutLayout(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        'n_views', 'max_dets', 'max_tracks', 'n_scenes', 'int_words', 'dbl_words', 'hdr_words', 'trk_words',
        'off_order', 'off_matched', 'off_time2d', 'off_nviews', 'dbl_hdr_words', 'dbl_trk_words')]


class PamJpegInfo(C.Structure):
    """What pam_jpeg_probe reads from a file's header (include/pam.h)."""
    _fields_ = [('width', C.c_int32), ('height', C.c_int32), ('n_comp', C.c_int32), ('unsupported', C.c_int32),
                ('h_samp', C.c_int32 * 3), ('v_samp', C.c_int32 * 3), ('mcu_w', C.c_int32), ('mcu_h', C.c_int32),
                ('blocks_w', C.c_int32 * 3), ('blocks_h', C.c_int32 * 3), ('restart_interval', C.c_int32), ('reserved', C.c_int32),
                ('coef_offset', C.c_int64 * 3), ('coef_words', C.c_int64), ('quant', (C.c_uint16 * 64) * 3)]


class PamJpegImage(C.Structure):
    """One image of a pam_jpeg_reconstruct call: four device pointers and what fixes the layout."""
    _fields_ = [('dev_coef', C.c_void_p), ('dev_quant', C.c_void_p), ('dev_planes', C.c_void_p), ('dev_out', C.c_void_p),
                ('width', C.c_int32), ('height', C.c_int32), ('n_comp', C.c_int32), ('h_samp', C.c_int32), ('v_samp', C.c_int32),
                ('reserved', C.c_int32)]


class PamJpegFwdImage(C.Structure):
    """One image of a pam_jpeg_forward call: the BGR frame, the three quantisation tables, the coefficient buffer it fills."""
    _fields_ = [('dev_bgr', C.c_void_p), ('dev_quant', C.c_void_p), ('dev_coef', C.c_void_p),
                ('width', C.c_int32), ('height', C.c_int32), ('h_samp', C.c_int32), ('v_samp', C.c_int32)]


class PamJpegEncodeParams(C.Structure):
    """What pam_jpeg_encode needs besides the coefficients; quality 0 = the tables in ``quant`` (luma, chroma; natural order)."""
    _fields_ = [('width', C.c_int32), ('height', C.c_int32), ('h_samp', C.c_int32), ('v_samp', C.c_int32),
                ('quality', C.c_int32), ('reserved', C.c_int32), ('quant', (C.c_uint16 * 64) * 2)]


class PamOverlayPrim(C.Structure):
    """One capsule of the overlay table, coordinates and half-width in 1/8 pixel (a joint's disc has a == b)."""
    _fields_ = [('ax', C.c_int32), ('ay', C.c_int32), ('bx', C.c_int32), ('by', C.c_int32), ('hw', C.c_int32), ('bgr', C.c_uint32),
                ('reserved', C.c_int32 * 2)]


class PamOverlayView(C.Structure):
    """One view of a pam_overlay_draw call: its frame and its range of the primitive table."""
    _fields_ = [('dev_bgr', C.c_void_p), ('width', C.c_int32), ('height', C.c_int32), ('prim_first', C.c_int32), ('prim_count', C.c_int32)]


class PamOverlayTrackView(C.Structure):
    """One view of a pam_overlay_tracks call: a camera of the handle (or -1 and a row of the extra matrices) and the size of its frame."""
    _fields_ = [('camera', C.c_int32), ('extra', C.c_int32), ('width', C.c_int32), ('height', C.c_int32)]


# every symbol include/pam.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_I = C.c_int
_SIGS = {
    'pam_create': (_I, [C.POINTER(_P), _I, _I, _I, _I, _I, _I, C.POINTER(PamParams)]),
    'pam_destroy': (_I, [_P]),
    'pam_last_error': (C.c_char_p, [_P]),
    'pam_version': (C.c_char_p, []),
    'pam_set_cameras': (_I, [_P, _P, _P, _P, _P]),
    'pam_reset': (_I, [_P]),
    'pam_out_layout': (_I, [_P, C.POINTER(PamOutLayout)]),
    'pam_frame_plan': (_I, [_P, _P, _P, _P]),
    'pam_frame': (_I, [_P, _I, _P, _P, _P, _P]),
    'pam_frame_dev': (_I, [_P, _P, _I, _P, _P]),
    'pam_frame_dev_views': (_I, [_P, _P, _I, _P, _P]),
    'pam_fetch': (_I, [_P, _P, _P, _P]),
    'pam_sync': (_I, [_P, _P]),
    'pam_op_project': (_I, [_P, _I, _I, _P, _P]),
    'pam_op_track_affinity': (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
    'pam_op_lsap': (_I, [_P, _I, _I, _P, _P, _P, _P]),
    'pam_op_epi_dist': (_I, [_P, _I, _P, _P, _P]),
    'pam_op_epi_pair': (_I, [_P, _I, _P, _I, _P, _P]),
    'pam_op_epi_dist_init': (_I, [_P, _I, _P, _P, _P]),
    'pam_op_greedy': (_I, [_P, _I, _I, _P, _P, _P, _P, _P]),
    'pam_op_dlt': (_I, [_P, _I, _P, _P, _P, _P, _P, _P]),
    'pam_op_dlt_paths': (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _P, _P]),
    'pam_op_smooth': (_I, [_P, _I, _P, _P, _P]),
    'pam_op_velocity': (_I, [_P, _I, _P, _P]),
    'pam_op_hyp_cost': (_I, [_P, _I, _P, _P, _I, _P, _P, _P]),
    'pam_preprocess_crops': (_I, [_P, _I, _P, _I, _I, _P, _P, _I, _I, _I, _P]),
    'pam_preprocess_crops_ex': (_I, [_P, _I, _I, _P, _I, _I, _P, _P, _I, _I, _I, _P, _I]),
    'pam_preprocess_crops_flip': (_I, [_P, _I, _I, _P, _I, _I, _P, _P, _I, _I, _I, _P, _I]),
    'pam_preprocess_crops_affine': (_I, [_P, _I, _I, _I, _P, _I, _I, _P, _P, C.c_float, _I, _I, _I, _P, _I, _P]),
    'pam_preprocess_crops_udp': (_I, [_P, _I, _I, _I, _P, _I, _I, _P, _P, C.c_float, _I, _I, _I, _P, _I, _P]),
    'pam_box_cs': (_I, [_P, _I, _P, _I, _I, C.c_float, _P]),
    'pam_box_cs_host': (_I, [_I, _P, _I, _I, C.c_float, _P]),
    'pam_decode_heatmaps': (_I, [_P, _I, _P, _I, _I, _I, _P, _P, _P, _I, _P, _P]),
    'pam_clock_probe': (_I, [_P, _P, _I]),
    'pam_conv2d_nhwc_bf16': (_I, [_P, _P, _P, _P, _P, _P, _P] + [_I] * 11),
    'pam_conv2d_nhwc_bf16_ex': (_I, [_P, _P, _P, _P, _P, _P, _P] + [_I] * 13),
    'pam_conv3x3_slab': (_I, [_I, _I, _I, _I]),
    'pam_conv3x3_layout': (_I, [_I, _I, _I, _I]),
    'pam_conv_last_kernel': (_I, []),
    'pam_conv_last_form': (_I, []),
    'pam_conv_plan': (_I, [_I] * 18 + [_P, _P]),
    'pam_conv3x3_layout_ex': (_I, [_I, _I, _I, _I, _I]),
    'pam_conv3x3_layout_gen': (_I, [_I, _I, _I, _I]),
    'pam_conv3x3_layout_small': (_I, [_I, _I, _I, _I]),
    'pam_conv_debug_stamps': (_I, [_P]),
    'pam_upsample_add_nhwc_bf16': (_I, [_P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I]),
    'pam_upsample_add_nhwc_bf16_ex': (_I, [_P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I]),
    'pam_basic_block2_tile': (_I, [_I, _I, _I, _I, _P]),
    'pam_basic_block2_nhwc_bf16': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I]),
    'pam_pointwise64_relu_nhwc_bf16': (_I, [_P, _P, _P, _P, _P, C.c_longlong]),
    'pam_pointwise64_act_nhwc_bf16': (_I, [_P, _P, _P, _P, _P, C.c_longlong, _I]),
    'pam_stem_fused_nhwc_bf16': (_I, [_P] * 10 + [_I, _I, _I]),
    'pam_bottleneck_fused_nhwc_bf16': (_I, [_P] * 12 + [_I, _I, _I]),
    'pam_resnet_stem_nhwc_bf16': (_I, [_P] * 5 + [_I, _I, _I]),
    'pam_deconv4x4s2_nhwc_bf16': (_I, [_P] * 5 + [_I] * 6),
    'pam_vit_linear_bf16': (_I, [_P] * 6 + [_I] * 4),
    'pam_vit_patch_embed_bf16': (_I, [_P] * 5 + [_I] * 4),
    'pam_vit_layernorm_bf16': (_I, [_P] * 5 + [_I, _I, C.c_float]),
    'pam_vit_attention_bf16': (_I, [_P] * 3 + [_I] * 3),
    'pam_bottleneck_tail_nhwc_bf16': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_longlong, _I]),
    'pam_conv3x3s2_c48_tile': (_I, [_I, _I, _I, _I, _P]),
    'pam_conv3x3s2_c48_nhwc_bf16': (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _I] + [_I] * 9),
    'pam_conv3x3s2_slab': (_I, [_I, _I, _I, _I]),
    'pam_conv3x3s2_nhwc_bf16': (_I, [_P, _P, _I, _P, _P, _P] + [_I] * 7),
    'pam_fuse_sum_nhwc_bf16': (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P] + [_I] * 8),
    'pam_fuse_sum_plan': (_I, [_I] * 6 + [_P, _P] + [_I] * 4 + [_P]),
    'pam_flag_signal': (_I, [_P, _P]),
    'pam_flag_signal_mask': (_I, [_P, _P, C.c_uint32]),
    'pam_flag_gate': (_I, [_P, _P, _I, _P, _P, _I, _P, _P]),
    'pam_set_input_guard': (_I, [_P, _P]),
    'pam_track_boxes': (_I, [_P, _P, _I, _I, _I, _I, C.c_float, C.c_float, C.c_float, _I, _I, _P, _P, _P, _P]),
    'pam_crop_table': (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    'pam_pose_nms': (_I, [_P, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P, C.c_longlong, C.c_longlong, _P, _P, C.c_double, C.c_double, _P, _P, _P]),
    'pam_undistort_keypoints': (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P]),
    'pam_set_lens': (_I, [_P, _P]),
    'pam_set_one_euro': (_I, [_P, C.POINTER(PamOneEuro)]),
    'pam_one_euro': (_I, [_P, _P, _I, _P, _P]),
    'pam_op_one_euro': (_I, [_P, _I, _I, _P, _P, C.POINTER(PamOneEuro), _P]),
    'pam_comm_unique_id': (_I, [_P]),
    'pam_comm_init': (_I, [C.POINTER(_P), _I, _I, _P, _I]),
    'pam_comm_destroy': (_I, [_P]),
    'pam_comm_last_error': (C.c_char_p, []),
    'pam_allgather_keypoints': (_I, [_P, _P, _P, _P, _I, _P]),
    'pam_head_decode_scratch_bytes': (C.c_longlong, [_I, _I, _I]),
    'pam_head_decode': (_I, [_P, _I, _I, _I, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    'pam_head_decode_soft_scratch_bytes': (C.c_longlong, [_I, _I, _I]),
    'pam_head_decode_soft': (_I, [_P, _I, _I, _I, _P, _I, _P, _P, _I, C.c_float, _P, _P, _P, _P, _I, _P, _P, _P]),
    'pam_head_decode_flip_scratch_bytes': (C.c_longlong, [_I, _I, _I]),
    'pam_head_decode_flip': (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _P, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    'pam_head_decode_dark_scratch_bytes': (C.c_longlong, [_I, _I, _I]),
    'pam_head_decode_dark': (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    'pam_head_decode_udp_scratch_bytes': (C.c_longlong, [_I, _I, _I]),
    'pam_head_decode_udp': (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    'pam_head_heatmaps': (_I, [_P, _I, _P, _I, _P, _P, _I, _P]),
    'pam_resize_frames': (_I, [_P, _I, _P, _I, _I, _I, _I, _P]),
    'pam_upsample_concat_nhwc_bf16': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I]),
    'pam_yolo_detect': (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, C.c_float, C.c_float, _I, _I, _I, _P, _P]),
    'pam_yolo_detect_ws': (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, C.c_float, C.c_float, _I, _I, _I, _P, _P, _P, C.c_longlong]),
    'pam_yolo_detect_workspace_bytes': (C.c_longlong, [_I, _P, _P]),
    'pam_yolo_detect_heads': (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, C.c_float, C.c_float, _I, _I, _I, _P, _P]),
    'pam_yolo_detect_heads_ws': (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, C.c_float, C.c_float, _I, _I, _I, _P, _P, _P, C.c_longlong]),
    'pam_yolo_detect_heads_workspace_bytes': (C.c_longlong, [_I, _I, _P, _P]),
    'pam_yolo_detect_heads_sxy': (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, C.c_float, C.c_float, _I, _I, _I, _P, _P]),
    'pam_yolo_detect_heads_sxy_ws': (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, C.c_float, C.c_float, _I, _I, _I, _P, _P, _P, C.c_longlong]),
    'pam_route_concat_nhwc_bf16': (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I]),
    'pam_maxpool_nhwc_bf16': (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I]),
    'pam_spp_concat_nhwc_bf16': (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I]),
    'pam_spp_concat_slab_nhwc_bf16': (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I]),
    'pam_jpeg_probe': (_I, [_P, C.c_size_t, C.POINTER(PamJpegInfo)]),
    'pam_jpeg_entropy': (_I, [_P, C.c_size_t, C.POINTER(PamJpegInfo), _P, C.c_size_t]),
    'pam_jpeg_reconstruct': (_I, [_P, _I, C.POINTER(PamJpegImage)]),
    'pam_jpeg_forward': (_I, [_P, _I, C.POINTER(PamJpegFwdImage)]),
    'pam_jpeg_quality_tables': (_I, [_I, _P]),
    'pam_jpeg_encode_bound': (_I, [_I, _I, _I, _I, C.POINTER(C.c_size_t)]),
    'pam_jpeg_encode': (_I, [_P, C.c_size_t, C.POINTER(PamJpegEncodeParams), _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    'pam_overlay_draw': (_I, [_P, _I, C.POINTER(PamOverlayView), _P, _I]),
    'pam_overlay_draw_counted': (_I, [_P, _I, C.POINTER(PamOverlayView), _P, _I, _P]),
    'pam_overlay_tracks': (_I, [_P, _P, _I, _I, C.POINTER(PamOverlayTrackView), _P, _I, _P, _P, _I, _I, _P, _P]),
}
EXPORTS = tuple(_SIGS)
YOLO_MAX_CAND = 1024        # PAM_YOLO_MAX_CAND in include/pam.h
SPP_MAX_HW = 32             # PAM_SPP_MAX_HW in include/pam.h

# the box rule of pam_track_boxes as the Python layers default it: synth.to_dump_results' growth, the pad that the oracle-tracker
# measurement needed, the reference's 2D age filter (time_interval <= 3)
TRACK_BOX_RULE = dict(grow=1.25, pad_px=8.0, min_size_px=8.0, max_gap=3)
CROP_CUT_VIEW, CROP_CUT_CAP = 1, 2         # pam_crop_table's info[2]
POSE_NMS_MAX = 32                          # rows per view pam_pose_nms takes (one bit each)
# pam_pose_nms' per-joint constants: (2 sigma_j)^2 of the COCO keypoint sigmas, by the expression of the official oks_nms (the kernel
# gets these 17 doubles, whatever produced them: a caller with other joints passes its own)
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
OKS_VARS = (COCO_SIGMAS * 2) ** 2
LENS_WORDS = 10                            # doubles of a camera's row in a lens table: fx, fy, cx, cy, skew, k1, k2, p1, p2, k3
LENS_ITERS, LENS_TOL = 8, 1e-9             # Newton steps of the inverse and its residual bound, normalised units (include/pam.h)
# the One-Euro filter on the tracks' 3D output (pam_set_one_euro): the values IterTrack.__init__ gives its 3D filters
# (IterativeTracker.py:225-237); freq is the frame rate, the time of frame f is f / freq
ONE_EURO_3D = dict(freq=25, mincutoff=0.8, beta=0.4, dcutoff=0.4)
JPEG_MAX_IMAGES = 32                       # images of one pam_jpeg_reconstruct / pam_jpeg_forward call (PAM_MAX_VIEWS)
OVERLAY_MAX_VIEWS = 32                     # views of one pam_overlay_draw call (PAM_MAX_VIEWS)
OVERLAY_TRACK_ROWS = 36                    # rows of one track in one view of pam_overlay_tracks' table (PAM_OVERLAY_TRACK_ROWS)
# PamJpegInfo.unsupported: why pam_jpeg_probe leaves a file to another decoder (PAM_JPEG_U_* in include/pam.h)
JPEG_UNSUPPORTED = {1: 'not a JPEG', 2: 'progressive', 3: 'arithmetic coding', 4: 'SOF1 / lossless / differential frame',
                    5: 'sample precision other than 8 bits', 6: '16-bit quantisation table', 7: 'neither one nor three components',
                    8: 'three components that are not YCbCr', 9: 'sampling other than 4:4:4, 4:2:2, 4:2:0', 10: 'not one interleaved scan',
                    11: 'zero height / DNL'}


def one_euro_config(cfg):
    """None / False -> None; True -> ONE_EURO_3D; a dict (keys freq, mincutoff, beta, dcutoff in either letter case, missing ones from
    ONE_EURO_3D) or a PamOneEuro -> a PamOneEuro.  ValueError for an unknown key and for what pam_set_one_euro refuses."""
    if cfg is None or cfg is False:
        return None
    if isinstance(cfg, PamOneEuro):
        cfg = dict(freq=cfg.freq, mincutoff=cfg.mincutoff, beta=cfg.beta, dcutoff=cfg.dcutoff)
    v = dict(ONE_EURO_3D)
    if cfg is not True:
        for k, x in dict(cfg).items():
            if str(k).lower() not in v:
                raise ValueError('one_euro: unknown key %r (freq, mincutoff, beta, dcutoff)' % (k,))
            v[str(k).lower()] = x
    v = {k: float(x) for k, x in v.items()}
    if not all(math.isfinite(x) for x in v.values()) or v['freq'] <= 0 or v['mincutoff'] <= 0 or v['dcutoff'] <= 0:
        raise ValueError('one_euro: values must be finite, freq, mincutoff and dcutoff > 0 (got %r)' % (v,))
    return PamOneEuro(v['freq'], v['mincutoff'], v['beta'], v['dcutoff'])


def lens_table(K, dist, always=False):
    """K (C, 3, 3) upper-triangular, dist (C, 5) (k1, k2, p1, p2, k3) or None -> the (C, 10) float64 table of pam_undistort_keypoints /
    pam_set_lens, or None when there is nothing to undo (dist None or all zero; always=True: the table of pin-holes then)."""
    if dist is None and always:
        dist = np.zeros((len(K), 5))
    if dist is None:
        return None
    K, dist = np.asarray(K, dtype=np.float64), np.asarray(dist, dtype=np.float64)
    if dist.ndim != 2 or dist.shape != (len(K), 5):
        raise ValueError('distCoef must be (%d, 5): k1, k2, p1, p2, k3 per camera (got %s)' % (len(K), dist.shape))
    if not np.any(dist) and not always:
        return None
    K = K / K[:, 2:3, 2:3]
    return np.ascontiguousarray(np.concatenate([np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 0, 1]], axis=1), dist], axis=1))


def check_lens(lens, n_cameras):
    """A caller's lens table as a contiguous (n_cameras, 10) float64 array; None when it is None or holds no non-zero coefficient."""
    if lens is None:
        return None
    lens = np.ascontiguousarray(lens, dtype=np.float64)
    if lens.shape != (n_cameras, LENS_WORDS) or not np.all(np.isfinite(lens)):
        raise ValueError('lens table must be (%d, %d) finite doubles (got %s)' % (n_cameras, LENS_WORDS, lens.shape))
    if not np.any(lens[:, 5:]):
        return None
    if np.any(lens[:, :2] == 0):
        raise ValueError('lens table: zero focal length')
    return lens

_lib = None


def load():
    """Load libpam_hip.so and declare signatures.  Raises RuntimeError (loudly) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError('HIP extension missing: %s not built. Run `make -C %s` (needs hipcc, --offload-arch=gfx950). '
                           'There is no CPU fallback.' % (LIB_PATH, os.path.join(_HERE, 'csrc')))
    # One HIP runtime per process: libtorch_hip NEEDs "libamdhip64.so" (its bundled copy, SONAME libamdhip64.so.7) while
    # this library NEEDs "libamdhip64.so.7".  With torch loaded first the loader satisfies ours from torch's copy by
    # SONAME; the other way round it maps /opt/rocm's AND torch's, and the second runtime to initialise finds no device.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib



_live_graphs = None


def new_graph():
    """A torch.cuda.CUDAGraph that is NOT destroyed while the interpreter shuts down (every graph the package captures is one).

    Destroying a captured multi-stream graph on ROCm 7.2 corrupts the runtime's heap now and then (tools/graph_destroy_stress.py: 3 of
    4 processes that capture 160 forwards and destroy 120 of them die of 'double free or corruption' / SIGSEGV inside a LATER
    synchronize or allocation, 0 of 5 when nothing is destroyed).  The package therefore never drops a capture while its network lives
    (one capture per crop-count bucket and replay slot, all of a slot in ONE memory pool), and at interpreter exit every graph still
    alive gets one reference that is never returned, so torch's destructor (hipGraphExecDestroy / hipGraphDestroy) does not run in the
    teardown either and a finished run cannot turn into a non-zero exit code.  Graphs do die with their network when a process drops one
    mid-run (the test-suite does); making them immortal outright was tried and is worse: with every capture of every earlier network
    still alive, a replay in tests/test_gpu_image.py segfaults inside hipGraphLaunch (3 of 3 full-suite runs)."""
    global _live_graphs
    import torch
    if _live_graphs is None:
        import atexit
        import weakref
        _live_graphs = weakref.WeakSet()

        def _keep():
            for g in list(_live_graphs):
                C.pythonapi.Py_IncRef(C.py_object(g))
        atexit.register(_keep)

    graph = torch.cuda.CUDAGraph()
    _live_graphs.add(graph)
    return graph


class PamError(RuntimeError):
    pass


# status bits of the frame record (include/pam.h, PamOutLayout.hdr_words)
ST_TRACK_OVERFLOW, ST_HYP_OVERFLOW, ST_LSAP_INFEASIBLE, ST_NDET_CLAMPED, ST_INPUT_VOID = 1, 2, 4, 8, 16


class FrameVoid(PamError):
    """The frame step skipped frames because the producer of their keypoints declared them void (a device-side gate of the captured
    HRNet forward timed out; pam_set_input_guard): the tracker state is that of the last applied frame.  ``first`` = the first skipped
    frame -- re-submit from there (the pose network orders its branch streams by stream events by now)."""

    def __init__(self, first, last):
        PamError.__init__(self, 'frames %d..%d were not applied: their keypoints were void (gate time-out); re-submit from frame %d' % (first, last, first))
        self.first, self.last = int(first), int(last)


def gaussian_taps(sigma, truncate=4.0):
    """One-sided taps of scipy.ndimage.gaussian_filter1d's kernel (w[0] = centre), built the way SciPy builds it
    so the device convolves with identical constants (IterativeTracker.py:381-382 call sites)."""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return phi[r:].copy()


def make_params(matcher, conf_threshold):
    """PamParams from the reference's PERSON_MATCHERS.ITERATIVE config block (attribute or key access)."""
    g = (lambda k: matcher[k]) if isinstance(matcher, dict) else (lambda k: getattr(matcher, k))
    p = PamParams()
    p.conf_threshold = float(conf_threshold)
    p.epi_threshold = float(g('EPI_THRESHOLD'))
    p.init_threshold = float(g('INIT_THRESHOLD'))
    p.joint_threshold = float(g('JOINT_THRESHOLD'))
    p.alpha2d = float(g('ALPHA2D'))
    p.lambda_a = float(g('LAMBDA_A'))
    p.lambda_t = float(g('LAMBDA_T'))
    p.n_init = int(g('N_INIT'))
    p.max_age = int(g('MAX_AGE'))
    p.count_gate = 10
    tb, ta = gaussian_taps(g('SIGMA')), gaussian_taps(g('ARM_SIGMA'))
    if len(tb) > PAM_MAX_TAPS or len(ta) > PAM_MAX_TAPS:
        raise ValueError('SIGMA too large for %d taps' % PAM_MAX_TAPS)
    p.n_taps_body, p.n_taps_arm = len(tb), len(ta)
    for i, w in enumerate(tb):
        p.taps_body[i] = w
    for i, w in enumerate(ta):
        p.taps_arm[i] = w
    e = np.exp(g('LAMBDA_A') * np.arange(PAM_EXP_TABLE))          # np.exp, as IterativeTracker.py:148
    for i in range(PAM_EXP_TABLE):
        p.exp_lambda_a[i] = e[i]
    for t in range(4):
        p.w_lambda_t[t] = math.exp(-g('LAMBDA_T') * t)             # math.exp, as construction.py:96
    return p


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Handle(object):
    """Owns one PamHandle (one GPU, device-resident tracker state for n_scenes scenes)."""

    def __init__(self, n_views, params, max_dets=16, max_tracks=32, max_hyps=0, n_scenes=1, device=0):
        self.lib = load()
        self._h = C.c_void_p()
        self.params = params
        rc = self.lib.pam_create(C.byref(self._h), device, n_views, max_dets, max_tracks, max_hyps, n_scenes,
                                 C.byref(params))
        if rc != 0:
            raise PamError('pam_create failed (%d): %s' % (rc, self.lib.pam_last_error(None).decode()))
        self.layout = PamOutLayout()
        self._chk(self.lib.pam_out_layout(self._h, C.byref(self.layout)))
        self.C, self.max_dets, self.max_tracks, self.n_scenes, self.device = n_views, max_dets, max_tracks, n_scenes, device
        self.one_euro_cfg = None
        self.out_i = np.zeros((n_scenes, self.layout.int_words), dtype=np.int32)
        self.out_d = np.zeros((n_scenes, self.layout.dbl_words), dtype=np.float64)

    def _chk(self, rc):
        if rc != 0:
            raise PamError('libpam_hip error %d: %s' % (rc, self.lib.pam_last_error(self._h).decode()))

    def close(self):
        if self._h:
            self.lib.pam_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def raw(self):
        return self._h

    def set_cameras(self, P, F, RK_INV, position):
        P = np.ascontiguousarray(P, dtype=np.float32); F = np.ascontiguousarray(F, dtype=np.float32)
        RK = np.ascontiguousarray(RK_INV, dtype=np.float32); pos = np.ascontiguousarray(position, dtype=np.float64)
        assert P.shape == (self.C, 3, 4) and F.shape == (self.C, self.C, 3, 3) and RK.shape == (self.C, 3, 3)
        self._chk(self.lib.pam_set_cameras(self._h, _ptr(P), _ptr(F), _ptr(RK), _ptr(pos)))

    def reset(self):
        self._chk(self.lib.pam_reset(self._h))

    def plan(self):
        """How the frame step runs on this handle: dict(block=threads per workgroup, launches=kernel launches per frame,
        hot_in_lds=whether the hot scratch and integer state live in LDS during the frame) (pam_frame_plan)."""
        v = [C.c_int32() for _ in range(3)]
        self._chk(self.lib.pam_frame_plan(self._h, *[C.byref(x) for x in v]))
        return dict(block=v[0].value, launches=v[1].value, hot_in_lds=v[2].value)

    def frame(self, frame_id, n_det, det):
        """n_det (S,C) int32, det (S,C,max_dets,17,3) float64 (y,x,score) host arrays -> (out_i, out_d)."""
        n_det = np.ascontiguousarray(n_det, dtype=np.int32).reshape(self.n_scenes, self.C)
        det = np.ascontiguousarray(det, dtype=np.float64).reshape(self.n_scenes, self.C, self.max_dets, PAM_J, 3)
        self._chk(self.lib.pam_frame(self._h, int(frame_id), _ptr(n_det), _ptr(det), _ptr(self.out_i), _ptr(self.out_d)))
        return self.out_i, self.out_d

    def frame_dev(self, stream, frame_id, dev_n_det_ptr, dev_det_ptr):
        self._chk(self.lib.pam_frame_dev(self._h, C.c_void_p(stream), int(frame_id), C.c_void_p(dev_n_det_ptr),
                                         C.c_void_p(dev_det_ptr)))

    def frame_dev_views(self, stream, frame_id, dev_records_ptr, dev_view_row_ptr):
        """The frame on the all-gathered per-view records (ViewGather.recv), read in place through the row map."""
        self._chk(self.lib.pam_frame_dev_views(self._h, C.c_void_p(stream), int(frame_id), C.c_void_p(dev_records_ptr),
                                               C.c_void_p(dev_view_row_ptr)))

    def set_input_guard(self, dev_word_ptr):
        """While the device int32 at dev_word_ptr is non-zero the frame step skips its frame (record status ``ST_INPUT_VOID``, state
        untouched): the word is raised by the producer of the keypoints (HRNetPose.void_word).  None / 0 removes the guard."""
        self._chk(self.lib.pam_set_input_guard(self._h, C.c_void_p(dev_word_ptr or None)))

    def set_lens(self, lens):
        """lens: (C, 10) host table (lens_table) or None.  While one is set, track_boxes draws its boxes in the RAW image: every joint's
        projection goes through its camera's forward model before the min / max (pam_set_lens).  None or all-zero coefficients remove it."""
        lens = check_lens(lens, self.C)
        self._chk(self.lib.pam_set_lens(self._h, _ptr(lens)))

    def set_one_euro(self, cfg):
        """cfg: what one_euro_config takes (None: off, the state is freed).  Setting it (again) starts every filter over; so does reset()
        while one is set (pam_set_one_euro)."""
        c = one_euro_config(cfg)
        self._chk(self.lib.pam_set_one_euro(self._h, C.byref(c) if c is not None else None))
        self.one_euro_cfg = c

    def one_euro_buffers(self, pinned=False):
        """(pose, meta) for one_euro: (n_scenes, max_tracks, 17, 3) float64 and (n_scenes, 2 + 3 * max_tracks) int32 torch tensors, on the
        handle's device or (pinned=True) in pinned host memory."""
        import torch
        kw = dict(device='cuda:%d' % self.device) if not pinned else {}
        pose = torch.zeros((self.n_scenes, self.max_tracks, PAM_J, 3), dtype=torch.float64, **kw)
        meta = torch.zeros((self.n_scenes, 2 + 3 * self.max_tracks), dtype=torch.int32, **kw)
        return (pose.pin_memory(), meta.pin_memory()) if pinned else (pose, meta)

    def one_euro(self, stream, frame_id, pose, meta):
        """The tracks' newest 3D poses through their One-Euro filters, behind whatever is queued on ``stream`` (pam_one_euro; the rules:
        include/pam.h).  pose / meta: the device tensors of one_euro_buffers.  Reads the tracker state, never writes it."""
        assert pose.is_contiguous() and meta.is_contiguous() and pose.numel() == self.n_scenes * self.max_tracks * PAM_J * 3
        assert meta.numel() == self.n_scenes * (2 + 3 * self.max_tracks) and str(pose.dtype) == 'torch.float64' and str(meta.dtype) == 'torch.int32'
        self._chk(self.lib.pam_one_euro(self._h, C.c_void_p(stream), int(frame_id), C.c_void_p(pose.data_ptr()), C.c_void_p(meta.data_ptr())))

    @staticmethod
    def decode_one_euro(pose, meta, scene=0):
        """host copies of one_euro's buffers (shaped as one_euro_buffers gives them) -> dict(n_tracks, n_fresh, ids, fresh, samples (n_tracks,), pose (n_tracks, 17, 3)), rows in
        the record's order."""
        m, p = np.asarray(meta)[scene], np.asarray(pose)[scene]
        n = int(m[0])
        rows = m[2:2 + 3 * n].reshape(n, 3)
        return dict(n_tracks=n, n_fresh=int(m[1]), ids=rows[:, 0].copy(), fresh=rows[:, 1].astype(bool), samples=rows[:, 2].copy(),
                    pose=p[:n].copy())

    def track_box_buffers(self, max_det=None):
        """(boxes, count, ids, info) for track_boxes: zeroed (C, max_det, 5) float32, (2C,) int32, (C, max_det) int32 and (2,) int32
        tensors on the handle's device; max_det: rows per view, the handle's max_dets by default."""
        import torch
        dev, md = 'cuda:%d' % self.device, int(self.max_dets if max_det is None else max_det)
        return (torch.zeros((self.C, md, 5), dtype=torch.float32, device=dev), torch.zeros(2 * self.C, dtype=torch.int32, device=dev),
                torch.zeros((self.C, md), dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev))

    def track_boxes(self, stream, frame_id, frame_w, frame_h, boxes, count, ids=None, info=None, scene=0, **rule):
        """Person boxes of ``frame_id`` from the tracker state behind whatever is queued on ``stream`` (pam_track_boxes).  boxes
        (C, max_det, 5) float32, count (2C,) int32, ids (C, max_det) int32 or None, info (2,) int32: contiguous device tensors
        (track_box_buffers), written in the detector's layout (``YOLOv3.detect_dev``).  rule: grow, pad_px, min_size_px, max_gap; a
        key that is not given has TRACK_BOX_RULE's value."""
        if set(rule) - set(TRACK_BOX_RULE):
            raise TypeError('track_boxes: unknown rule key(s) %s (%s)' % (sorted(set(rule) - set(TRACK_BOX_RULE)), ', '.join(TRACK_BOX_RULE)))
        rule = dict(TRACK_BOX_RULE, **rule)
        max_det = int(boxes.shape[1])
        assert tuple(boxes.shape) == (self.C, max_det, 5) and boxes.is_contiguous() and count.numel() == 2 * self.C and info.numel() >= 2
        assert ids is None or (ids.numel() == self.C * max_det and ids.is_contiguous())
        self._chk(self.lib.pam_track_boxes(self._h, C.c_void_p(stream), int(scene), int(frame_id), int(frame_w), int(frame_h),
                                           float(rule['grow']), float(rule['pad_px']), float(rule['min_size_px']), int(rule['max_gap']),
                                           max_det, C.c_void_p(boxes.data_ptr()),
                                           C.c_void_p(count.data_ptr()), C.c_void_p(ids.data_ptr()) if ids is not None else None,
                                           C.c_void_p(info.data_ptr())))

    def overlay_tracks(self, stream, views, palette, prims, count, extra_P=None, pose=None, emitted_only=True, scene=0):
        """The overlay's primitive table from the tracker state behind whatever is queued on ``stream`` (pam_overlay_tracks; the rules:
        include/pam.h).  views: a PamOverlayTrackView array; palette: 25 words B | G << 8 | R << 16 (8 limb, 17 joint colours);
        prims (len(views), cap, 8) int32 and count (len(views),) int32: contiguous device tensors, every row of which is written;
        extra_P: (n_extra, 3, 4) float32 device tensor for the views with camera -1; pose: one_euro's device pose buffer (the rows of
        ``scene`` are taken), None = the tracks' newest raw poses.  Reads the tracker state, never writes it."""
        n = len(views)
        assert prims.dim() == 3 and prims.shape[0] == n and prims.shape[2] == 8 and prims.is_contiguous() and str(prims.dtype) == 'torch.int32'
        assert count.numel() == n and count.is_contiguous() and str(count.dtype) == 'torch.int32'
        assert extra_P is None or (extra_P.is_contiguous() and str(extra_P.dtype) == 'torch.float32' and extra_P.numel() % 12 == 0)
        pal = (C.c_uint32 * 25)(*[int(c) for c in palette])
        pose_ptr = None
        if pose is not None:
            assert pose.is_contiguous() and str(pose.dtype) == 'torch.float64' and pose.numel() == self.n_scenes * self.max_tracks * PAM_J * 3
            pose_ptr = C.c_void_p(pose.data_ptr() + 8 * int(scene) * self.max_tracks * PAM_J * 3)
        self._chk(self.lib.pam_overlay_tracks(self._h, C.c_void_p(stream), int(scene), n, views,
                                              C.c_void_p(extra_P.data_ptr()) if extra_P is not None else None,
                                              extra_P.numel() // 12 if extra_P is not None else 0, pose_ptr, pal, int(bool(emitted_only)),
                                              int(prims.shape[1]), C.c_void_p(prims.data_ptr()), C.c_void_p(count.data_ptr())))

    def pinned_record(self):
        """(keep, out_i, out_d): ONE pinned host buffer laid out like the device record (int32 section padded to 8 bytes, float64 section
        behind it) and NumPy views of its two sections -- ``fetch`` into them is a single device -> host copy."""
        import torch
        L = self.layout
        ib = (4 * self.n_scenes * L.int_words + 7) & ~7
        buf = torch.zeros(ib + 8 * self.n_scenes * L.dbl_words, dtype=torch.uint8).pin_memory()
        a = buf.numpy()
        oi = a[:4 * self.n_scenes * L.int_words].view(np.int32).reshape(self.n_scenes, L.int_words)
        od = a[ib:].view(np.float64).reshape(self.n_scenes, L.dbl_words)
        return buf, oi, od

    def fetch(self, stream, out_i=None, out_d=None):
        out_i = self.out_i if out_i is None else out_i
        out_d = self.out_d if out_d is None else out_d
        self._chk(self.lib.pam_fetch(self._h, C.c_void_p(stream), _ptr(out_i), _ptr(out_d)))
        return out_i, out_d

    def sync(self, stream=0):
        self._chk(self.lib.pam_sync(self._h, C.c_void_p(stream)))

    # ---- decoding of the output record -----------------------------------------------------------------------------
    def decode(self, scene=0, out_i=None, out_d=None):
        """-> list of per-track dicts in the reference's self.tracks order."""
        L = self.layout
        oi = (self.out_i if out_i is None else out_i)[scene]
        od = (self.out_d if out_d is None else out_d)[scene]
        n = int(oi[0])
        tracks = []
        for i in range(n):
            b = oi[L.hdr_words + i * L.trk_words: L.hdr_words + (i + 1) * L.trk_words]
            dd = od[L.dbl_hdr_words + i * L.dbl_trk_words: L.dbl_hdr_words + (i + 1) * L.dbl_trk_words]
            nv2 = int(b[6])
            tracks.append(dict(
                track_id=int(b[0]), state=int(b[1]), hits=int(b[2]), age=int(b[3]), time_since_update=int(b[4]),
                emitted=bool(b[5]), order=[int(c) for c in b[L.off_order:L.off_order + nv2]], V=int(b[7]),
                nhist=int(b[8]), last_time=int(b[9]),
                matched_det=b[L.off_matched:L.off_matched + self.C].copy(),
                time2d=b[L.off_time2d:L.off_time2d + self.C].copy(),
                nviews=b[L.off_nviews:L.off_nviews + PAM_J].copy(),
                pose3d=dd[:PAM_J * 3].reshape(PAM_J, 3).copy(), velocity=dd[PAM_J * 3:].reshape(PAM_J, 3).copy()))
        # status word: bits 0-15 = this frame's bits, bits 16-31 = OR of every frame's bits since create / reset (include/pam.h)
        w = int(oi[1]) & 0xffffffff
        return dict(n_tracks=n, status=w & 0xffff, status_sticky=(w >> 16) & 0xffff, frame_id=int(oi[2]), n_hyp=int(oi[3]),
                    first_void=int(oi[3]) if (w & ST_INPUT_VOID) else None,
                    clocks=od[:4].copy(), clocks_all=od[:L.dbl_hdr_words].copy(), tracks=tracks)

    # ---- per-operator entry points (parity tests) -------------------------------------------------------------------
    def op_project(self, cid, poses3d):
        p = np.ascontiguousarray(poses3d, dtype=np.float64).reshape(-1, PAM_J, 3)
        out = np.zeros((len(p), PAM_J, 2))
        self._chk(self.lib.pam_op_project(self._h, cid, len(p), _ptr(p), _ptr(out)))
        return out

    def op_track_affinity(self, cid, tracks_pose, dt, dets):
        tp = np.ascontiguousarray(tracks_pose, dtype=np.float64); dd = np.ascontiguousarray(dets, dtype=np.float64)
        t = np.ascontiguousarray(dt, dtype=np.int32)
        out = np.zeros((len(tp), len(dd)))
        self._chk(self.lib.pam_op_track_affinity(self._h, cid, len(tp), len(dd), _ptr(tp), _ptr(t), _ptr(dd), _ptr(out)))
        return out

    def op_lsap(self, cost):
        c = np.ascontiguousarray(cost, dtype=np.float64)
        nr, nc = c.shape
        N = max(nr, nc, 1)
        rows = np.zeros(N, dtype=np.int32); cols = np.zeros(N, dtype=np.int32); n = C.c_int32(0)
        self._chk(self.lib.pam_op_lsap(self._h, nr, nc, _ptr(c), _ptr(rows), _ptr(cols), C.byref(n)))
        return rows[:n.value].copy(), cols[:n.value].copy()

    def op_epi_dist(self, cids, pose_mat):
        c = np.ascontiguousarray(cids, dtype=np.int32); pm = np.ascontiguousarray(pose_mat, dtype=np.float64)
        V = len(c); out = np.zeros((V, V, PAM_J))
        self._chk(self.lib.pam_op_epi_dist(self._h, V, _ptr(c), _ptr(pm), _ptr(out)))
        return out

    def op_epi_pair(self, c1, p1, c2, p2):
        a = np.ascontiguousarray(p1, dtype=np.float64); b = np.ascontiguousarray(p2, dtype=np.float64)
        out = np.zeros((PAM_J, 2))
        self._chk(self.lib.pam_op_epi_pair(self._h, int(c1), _ptr(a), int(c2), _ptr(b), _ptr(out)))
        return out

    def op_epi_dist_init(self, cids, pose_mat):
        c = np.ascontiguousarray(cids, dtype=np.int32); pm = np.ascontiguousarray(pose_mat, dtype=np.float64)
        V = len(c); out = np.zeros((V, V, PAM_J), dtype=np.float32)
        self._chk(self.lib.pam_op_epi_dist_init(self._h, V, _ptr(c), _ptr(pm), _ptr(out)))
        return out

    def op_greedy(self, mode, cids, aff, pose_j=None, next_pose_j=None):
        c = np.ascontiguousarray(cids, dtype=np.int32)
        V = len(c)
        if mode == 'update':
            a = np.ascontiguousarray(aff, dtype=np.float64)
            pj = np.ascontiguousarray(pose_j, dtype=np.float64).reshape(V, 3)
            nj = np.ascontiguousarray(next_pose_j, dtype=np.float64).reshape(3)
        else:
            a = np.ascontiguousarray(aff, dtype=np.float32); pj = nj = None
        k = C.c_uint32(0)
        self._chk(self.lib.pam_op_greedy(self._h, 0 if mode == 'update' else 1, V, _ptr(c), _ptr(a), _ptr(pj), _ptr(nj),
                                         C.byref(k)))
        return k.value

    def op_dlt(self, cids, Ts, pose_mat, keep_masks, next_pose):
        c = np.ascontiguousarray(cids, dtype=np.int32); t = np.ascontiguousarray(Ts, dtype=np.int32)
        pm = np.ascontiguousarray(pose_mat, dtype=np.float64); k = np.ascontiguousarray(keep_masks, dtype=np.uint32)
        nx = np.ascontiguousarray(next_pose, dtype=np.float64); out = np.zeros((PAM_J, 3))
        self._chk(self.lib.pam_op_dlt(self._h, len(c), _ptr(c), _ptr(t), _ptr(pm), _ptr(k), _ptr(nx), _ptr(out)))
        return out

    def op_dlt_paths(self, cids, Ts, pose_mat, keep_masks, next_pose, nsplit=1, solver=0):
        """op_dlt with the solver's paths selectable (nsplit 1 / 4: unsplit or the four-way fold / pack / merge of the wide rigs; solver 0 /
        1: inverse iteration with the Jacobi fall-back, or Jacobi alone) -> (out (17, 3), path (17,) int32: 0 copied, 1 inverse iteration,
        2 Jacobi)."""
        c = np.ascontiguousarray(cids, dtype=np.int32); t = np.ascontiguousarray(Ts, dtype=np.int32)
        pm = np.ascontiguousarray(pose_mat, dtype=np.float64); k = np.ascontiguousarray(keep_masks, dtype=np.uint32)
        nx = np.ascontiguousarray(next_pose, dtype=np.float64); out = np.zeros((PAM_J, 3)); path = np.full(PAM_J, -1, dtype=np.int32)
        assert len(t) == len(c) and pm.shape == (len(c), PAM_J, 3) and k.shape == (PAM_J,) and nx.shape == (PAM_J, 3)
        self._chk(self.lib.pam_op_dlt_paths(self._h, len(c), _ptr(c), _ptr(t), _ptr(pm), _ptr(k), _ptr(nx), int(nsplit), int(solver),
                                            _ptr(out), _ptr(path)))
        return out, path

    def op_smooth(self, hist, raw):
        hs = np.ascontiguousarray(hist, dtype=np.float64).reshape(-1, PAM_J, 3)
        L = len(hs)
        if L == 0:
            hs = np.zeros((1, PAM_J, 3))
        r = np.ascontiguousarray(raw, dtype=np.float64); out = np.zeros((PAM_J, 3))
        self._chk(self.lib.pam_op_smooth(self._h, L, _ptr(hs), _ptr(r), _ptr(out)))
        return out

    def op_one_euro(self, t, x, cfg=True):
        """t (n,) time stamps, x (n, K) samples -> (n, K): every column through a new One-Euro filter of configuration cfg
        (one_euro_config), by the device function k_one_euro runs."""
        tt = np.ascontiguousarray(t, dtype=np.float64); xx = np.ascontiguousarray(x, dtype=np.float64)
        assert xx.ndim == 2 and tt.shape == (xx.shape[0],)
        out = np.zeros_like(xx)
        c = one_euro_config(cfg)
        self._chk(self.lib.pam_op_one_euro(self._h, xx.shape[0], xx.shape[1], _ptr(tt), _ptr(xx), C.byref(c), _ptr(out)))
        return out

    def op_velocity(self, hist):
        hs = np.ascontiguousarray(hist, dtype=np.float64).reshape(-1, PAM_J, 3)
        out = np.zeros((PAM_J, 3), dtype=np.float32)
        self._chk(self.lib.pam_op_velocity(self._h, len(hs), _ptr(hs), _ptr(out)))
        return out

    def op_hyp_cost(self, cids, poses, o_cid, o_pose):
        c = np.ascontiguousarray(cids, dtype=np.int32); ps = np.ascontiguousarray(poses, dtype=np.float64)
        po = np.ascontiguousarray(o_pose, dtype=np.float64)
        cost = C.c_double(0); veto = C.c_int32(0)
        self._chk(self.lib.pam_op_hyp_cost(self._h, len(c), _ptr(c), _ptr(ps), int(o_cid), _ptr(po), C.byref(cost), C.byref(veto)))
        return cost.value, bool(veto.value)


def crop_table(stream, boxes, count, frame_w, frame_h, max_dets, view_of, slot_of, xywh, n_det, info, views=None):
    """Detector-layout box lists -> crop table (pam_crop_table).  boxes (V, max_det_in, 5) float32 and count (>= V,) int32 as
    ``YOLOv3.detect_dev`` / ``Handle.track_boxes`` leave them; views: int32 device tensor of the images to take, in order (None = the
    first ``n_det.numel()``); view_of / slot_of (cap,) int32, xywh (cap, 4) float32, n_det (n_views,) int32, info (4,) int32 are written.
    All contiguous device tensors; asynchronous on ``stream``."""
    cap, n_views = int(view_of.numel()), int(n_det.numel())
    assert boxes.dim() == 3 and boxes.shape[2] == 5 and boxes.is_contiguous() and xywh.numel() == 4 * cap and slot_of.numel() == cap
    assert info.numel() >= 4 and (views is None or views.numel() == n_views) and (views is not None or n_views <= boxes.shape[0])
    rc = load().pam_crop_table(C.c_void_p(stream), n_views, C.c_void_p(views.data_ptr()) if views is not None else None,
                               C.c_void_p(boxes.data_ptr()), C.c_void_p(count.data_ptr()), int(boxes.shape[1]), int(frame_w), int(frame_h),
                               int(max_dets), cap, C.c_void_p(view_of.data_ptr()), C.c_void_p(slot_of.data_ptr()),
                               C.c_void_p(xywh.data_ptr()), C.c_void_p(n_det.data_ptr()), C.c_void_p(info.data_ptr()))
    if rc != 0:
        raise PamError('pam_crop_table failed (%d)' % rc)


# HRNetPose(box_transform=): the raw box stretched to the input, the checkpoints' own transform, or its UDP form (align-corners grids)
BOX_TRANSFORMS = ('stretch', 'affine', 'udp')
BOX_SCALE = 1.25                           # _box2cs's enlargement


def check_box_transform(box_transform, box_scale=BOX_SCALE):
    """(box_transform, box_scale) as HRNetPose takes them -> (name, float scale); anything but 'stretch' / 'affine' / 'udp', or a scale that is
    not > 0, is a ValueError.  None stands for the default of either (a YAML without the optional keys)."""
    name = 'stretch' if box_transform is None else box_transform
    if name not in BOX_TRANSFORMS:
        raise ValueError("box_transform must be 'stretch', 'affine' or 'udp' (got %r)" % (box_transform,))
    scale = BOX_SCALE if box_scale is None else float(box_scale)
    if not scale > 0.0:
        raise ValueError('box_scale must be > 0 (got %r)' % (box_scale,))
    return name, scale


def box_cs(boxes, out_w, out_h, scale=BOX_SCALE):
    """The effective boxes of person boxes (n, 4) xywh for a network input of out_w x out_h on the host (pam_box_cs_host; the
    transform: include/pam.h) -> (n, 4) float32, bit for bit what pam_box_cs and the affine crop launch leave on the device."""
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
    out = np.empty_like(b)
    rc = load().pam_box_cs_host(len(b), _ptr(b), int(out_w), int(out_h), float(scale), _ptr(out))
    if rc != 0:
        raise PamError('pam_box_cs_host failed (%d)' % rc)
    return out


def box_cs_dev(stream, boxes, out_w, out_h, scale, eff):
    """pam_box_cs: boxes (n, 4) float32 device rows -> eff (n, 4) float32, the whole table in one launch on ``stream``."""
    n = int(boxes.numel()) // 4
    assert eff.numel() >= 4 * n and boxes.is_contiguous() and eff.is_contiguous()
    rc = load().pam_box_cs(C.c_void_p(stream), n, C.c_void_p(boxes.data_ptr()), int(out_w), int(out_h), float(scale),
                           C.c_void_p(eff.data_ptr()))
    if rc != 0:
        raise PamError('pam_box_cs failed (%d)' % rc)


def pose_nms(stream, det, n_det_in, view_of, slot_of, xywh, n_det_out, keep_from, pose_score, max_dets=None, score=None,
             score_strides=(0, 0), views=None, oks_thre=0.9, in_vis_thre=0.2, oks_vars=None):
    """Rescoring + greedy OKS-NMS of every view's decoded poses, in place (pam_pose_nms; the rule: include/pam.h).  det (V, det_slots,
    17, 3) float64 rows (y, x, score), the first max_dets (None: det_slots; at most 32) rows of a view are its slots; n_det_in (V,) int32;
    view_of / slot_of (n_rows,) int32 and xywh (n_rows, 4) float32: the crop rows that produced det; score: float32 device tensor or
    data pointer of the box scores, read at [g * score_strides[0] + slot * score_strides[1]] with g = views[v] (views: int32 device
    tensor) or v -- None = 1.0; oks_vars: 17 doubles (None: OKS_VARS).  Written: n_det_out (V,) int32 (not n_det_in), keep_from (V,
    max_dets) int32, pose_score (V, max_dets) float64.  All contiguous device tensors; asynchronous on ``stream``."""
    V, det_slots = int(det.shape[0]), int(det.shape[1])
    max_dets = det_slots if max_dets is None else int(max_dets)
    if max_dets > POSE_NMS_MAX:
        raise ValueError('pose_nms: %d slots per view, at most %d' % (max_dets, POSE_NMS_MAX))
    n_rows = int(view_of.numel())
    assert det.is_contiguous() and tuple(det.shape[2:]) == (PAM_J, 3) and n_det_in.numel() >= V and n_det_out.numel() >= V
    assert slot_of.numel() == n_rows and xywh.numel() == 4 * n_rows and keep_from.numel() >= V * max_dets and pose_score.numel() >= V * max_dets
    assert views is None or views.numel() >= V
    vs = np.ascontiguousarray(OKS_VARS if oks_vars is None else oks_vars, dtype=np.float64)
    assert vs.shape == (PAM_J,)
    sp = None if score is None else C.c_void_p(score if isinstance(score, int) else score.data_ptr())
    rc = load().pam_pose_nms(C.c_void_p(stream), V, max_dets, det_slots, C.c_void_p(det.data_ptr()), C.c_void_p(n_det_in.data_ptr()), n_rows,
                             C.c_void_p(view_of.data_ptr()), C.c_void_p(slot_of.data_ptr()), C.c_void_p(xywh.data_ptr()), sp,
                             int(score_strides[0]), int(score_strides[1]), C.c_void_p(views.data_ptr()) if views is not None else None,
                             _ptr(vs), float(oks_thre), float(in_vis_thre), C.c_void_p(n_det_out.data_ptr()),
                             C.c_void_p(keep_from.data_ptr()), C.c_void_p(pose_score.data_ptr()))
    if rc != 0:
        raise PamError('pam_pose_nms failed (%d)' % rc)


def undistort_keypoints(stream, det, n_det, lens, info, max_dets=None, views=None):
    """Lens distortion out of every view's decoded poses, in place (pam_undistort_keypoints; the model: include/pam.h).  det (V, det_slots,
    17, 3) float64 rows (y, x, score), the first max_dets (None: det_slots; at most 32) rows of a view are its slots; n_det (V,) int32;
    lens (G, 10) float64 device table, read at row views[v] (views: int32 device tensor) or v; info (2,) int32 is written: [0] points left
    as they were because they could not be inverted, [1] points below the counts.  All contiguous device tensors; asynchronous on
    ``stream``."""
    V, det_slots = int(det.shape[0]), int(det.shape[1])
    max_dets = det_slots if max_dets is None else int(max_dets)
    if max_dets > POSE_NMS_MAX:
        raise ValueError('undistort_keypoints: %d slots per view, at most %d' % (max_dets, POSE_NMS_MAX))
    assert det.is_contiguous() and tuple(det.shape[2:]) == (PAM_J, 3) and str(det.dtype) == 'torch.float64' and n_det.numel() >= V
    assert lens.is_contiguous() and str(lens.dtype) == 'torch.float64' and lens.dim() == 2 and lens.shape[1] == LENS_WORDS and info.numel() >= 2
    assert (views is None and lens.shape[0] >= V) or (views is not None and views.numel() >= V)
    rc = load().pam_undistort_keypoints(C.c_void_p(stream), V, max_dets, det_slots, C.c_void_p(det.data_ptr()), C.c_void_p(n_det.data_ptr()),
                                        C.c_void_p(views.data_ptr()) if views is not None else None, C.c_void_p(lens.data_ptr()),
                                        C.c_void_p(info.data_ptr()))
    if rc != 0:
        raise PamError('pam_undistort_keypoints failed (%d)' % rc)
