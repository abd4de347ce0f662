"""ctypes binding of libstereotrack_hip.so (the C ABI declared in include/stereotrack.h).

The HIP library is the ONLY compute path of this package: if it is missing, loading raises —
there is no CPU fallback.  `import torch` happens first so that the library resolves
libamdhip64.so.7 to the HIP runtime PyTorch already loaded (one runtime, shared device pointers
and streams).
"""
import ctypes as C
import os

import torch  # noqa: F401  (must be loaded before the HIP library, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libstereotrack_hip.so')

ST_OK = 0
_ERR_NAMES = {-1: 'ST_ERR_INVALID', -2: 'ST_ERR_HIP', -3: 'ST_ERR_STATE', -4: 'ST_ERR_WORKSPACE',
              -5: 'ST_ERR_NOTFOUND'}


class StError(RuntimeError):
    """A libstereotrack_hip call returned a non-zero status."""


class StConvDesc(C.Structure):
    _fields_ = [
        ('in_dev', C.c_void_p),
        ('N', C.c_int), ('Hi', C.c_int), ('Wi', C.c_int), ('Cin', C.c_int), ('in_ld', C.c_int), ('in_off', C.c_int),
        ('wgt_dev', C.c_void_p), ('bias_dev', C.c_void_p),
        ('Cout', C.c_int), ('KH', C.c_int), ('KW', C.c_int), ('stride', C.c_int), ('pad', C.c_int),
        ('out1_dev', C.c_void_p), ('out1_ld', C.c_int), ('out1_off', C.c_int), ('split', C.c_int),
        ('out2_dev', C.c_void_p), ('out2_ld', C.c_int), ('out2_off', C.c_int),
        ('up_dev', C.c_void_p), ('up_ld', C.c_int), ('up_off', C.c_int),
        ('res_dev', C.c_void_p), ('res_ld', C.c_int), ('res_off', C.c_int),
        ('post_scale', C.c_float), ('act', C.c_int), ('wgt_wino_dev', C.c_void_p),
    ]


class StDetectorConfig(C.Structure):
    _fields_ = [
        ('struct_size', C.c_int), ('widen_factor', C.c_float), ('deepen_factor', C.c_float),
        ('num_classes', C.c_int), ('batch', C.c_int), ('height', C.c_int), ('width', C.c_int),
        ('bn_eps', C.c_double), ('with_right_branch', C.c_int), ('disp_planes_identical', C.c_int),
        ('rgb_only', C.c_int), ('out_fd', C.c_int),
    ]


class StDispHeadConfig(C.Structure):
    _fields_ = [('struct_size', C.c_int), ('batch', C.c_int), ('p3_height', C.c_int), ('p3_width', C.c_int),
                ('in_channels', C.c_int), ('channels', C.c_int), ('bn_eps', C.c_double)]


class StTrackerConfig(C.Structure):
    _fields_ = [
        ('struct_size', C.c_int), ('obj_score_thr', C.c_float), ('init_track_thr', C.c_float),
        ('weight_iou_with_det_scores', C.c_int), ('match_iou_thr', C.c_float), ('num_tentatives', C.c_int),
        ('vel_consist_weight', C.c_float), ('vel_delta_t', C.c_int), ('num_frames_retain', C.c_int),
    ]


TRACKER_OPTIONS = tuple(name for name, _ in StTrackerConfig._fields_[1:])


def tracker_config(obj_score_thr, init_track_thr, weight_iou_with_det_scores, match_iou_thr, num_tentatives,
                   vel_consist_weight, vel_delta_t, num_frames_retain):
    """StTrackerConfig of the tracker options, under their names in OCSORTTracker_Disparity's constructor."""
    return StTrackerConfig(C.sizeof(StTrackerConfig), float(obj_score_thr), float(init_track_thr),
                           int(bool(weight_iou_with_det_scores)), float(match_iou_thr), int(num_tentatives),
                           float(vel_consist_weight), int(vel_delta_t), int(num_frames_retain))


TRACK_WINDOW = 8      # ST_TRACK_WINDOW


class StTrackState(C.Structure):
    """Everything a track knows (include/stereotrack.h section 8), the same layout from the host tracker
    (st_tracker_get_states) and from the device tracker (st_batched_tracker_get_states)."""
    _fields_ = [
        ('struct_size', C.c_int), ('tentative', C.c_int), ('tracked', C.c_int), ('last_frame', C.c_int),
        ('n_fed', C.c_int), ('win_len', C.c_int), ('trailing_none', C.c_int), ('vel_placeholder', C.c_int),
        ('id', C.c_int64), ('n_obs', C.c_int64),
        ('mean', C.c_double * 8), ('cov', (C.c_double * 8) * 8),
        ('saved_mean', C.c_double * 8), ('saved_cov', (C.c_double * 8) * 8),
        ('win', (C.c_float * 4) * TRACK_WINDOW), ('win_valid', C.c_int * TRACK_WINDOW),
        ('last_valid', C.c_float * 4), ('vel', C.c_float * 2),
    ]


TRACK_STATE_FIELDS = tuple(name for name, _ in StTrackState._fields_[1:])


def track_state_dicts(buf, n):
    """The first n StTrackState of a ctypes array -> [{field: int / bool / numpy array (a copy)}], the format of
    OCSORTTracker_Disparity.track_states() and BatchedGpuTracker.track_states()."""
    import numpy as np
    out = []
    for i in range(n):
        s, d = buf[i], {}
        for name in TRACK_STATE_FIELDS:
            v = getattr(s, name)
            if isinstance(v, C.Array):
                v = np.ctypeslib.as_array(v).copy()
            elif name in ('tentative', 'tracked', 'vel_placeholder'):
                v = bool(v)
            else:
                v = int(v)
            d[name] = v
        out.append(d)
    return out


class StCmcParams(C.Structure):
    _fields_ = [('struct_size', C.c_int), ('step', C.c_int), ('winsize', C.c_int), ('ransac_thr', C.c_float),
                ('min_inlier_ratio', C.c_float)]


class StEccParams(C.Structure):
    _fields_ = [('struct_size', C.c_int), ('warp_mode', C.c_int), ('num_iters', C.c_int), ('stop_eps', C.c_float),
                ('gauss_filt_size', C.c_int), ('downscale', C.c_int)]


class StSgbmParams(C.Structure):
    _fields_ = [('struct_size', C.c_int), ('num_disparities', C.c_int), ('block_size', C.c_int), ('P1', C.c_int),
                ('P2', C.c_int), ('disp12_max_diff', C.c_int), ('uniqueness_ratio', C.c_int),
                ('speckle_window_size', C.c_int), ('speckle_range', C.c_int), ('pre_filter_cap', C.c_int),
                ('color', C.c_int)]


class StCocoArgs(C.Structure):
    _fields_ = [('struct_size', C.c_int), ('num_images', C.c_int), ('num_cats', C.c_int), ('num_dets', C.c_int),
                ('num_gts', C.c_int), ('T', C.c_int), ('A', C.c_int), ('M', C.c_int), ('R', C.c_int)] + \
        [(n, C.c_void_p) for n in ('det_boxes', 'det_scores', 'det_labels', 'det_img', 'gt_boxes', 'gt_area', 'gt_crowd',
                                   'gt_cat', 'gt_img', 'gt_img_host', 'gt_cat_host', 'iou_thrs', 'area_rng', 'rec_thrs',
                                   'max_dets', 'ws')] + [('ws_bytes', C.c_size_t)] + \
        [(n, C.c_void_p) for n in ('det_rank', 'det_matched', 'det_ignored', 'npig', 'precision', 'recall', 'scores',
                                   'status')]


class StMotArgs(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('struct_size', 'num_seqs', 'num_frames', 'num_gt', 'num_pred', 'num_alphas',
                                       'max_frame_objects', 'flags')] + \
        [(n, C.c_longlong) for n in ('num_pairs', 'num_cells', 'num_gids', 'num_tids')] + [('iou_thr', C.c_double)] + \
        [(n, C.c_void_p) for n in ('gt_rows', 'pred_rows', 'seq_frame_off', 'frame_seq', 'frame_no', 'frame_gt_off',
                                   'frame_pred_off', 'frame_pair_off', 'seq_ng', 'seq_nt', 'seq_gid_off', 'seq_tid_off',
                                   'seq_mat_off', 'alphas', 'ws')] + [('ws_bytes', C.c_size_t)] + \
        [(n, C.c_void_p) for n in ('gt_count', 'tr_count', 'id_potential', 'hota_potential', 'gt_frames', 'gt_matched',
                                   'gt_frag', 'clear_counts', 'motp_sum', 'hota_counts', 'hota_sums', 'status')]


class StMotKittiArgs(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('struct_size', 'num_frames', 'num_classes', 'num_gt', 'num_pred', 'num_ignore',
                                       'max_frame_objects')] + [('num_ws_cells', C.c_longlong)] + \
        [(n, C.c_double) for n in ('max_occlusion', 'max_truncation', 'min_height', 'match_thr', 'ignore_thr')] + \
        [(n, C.c_void_p) for n in ('gt_rows', 'pred_rows', 'ignore_rows', 'frame_gt_off', 'frame_pred_off',
                                   'frame_ignore_off', 'frame_ws_off', 'class_table', 'ws')] + [('ws_bytes', C.c_size_t)] + \
        [(n, C.c_void_p) for n in ('gt_keep', 'pred_keep', 'status')]


class StMotChallengeArgs(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('struct_size', 'num_frames', 'num_gt', 'num_pred', 'max_frame_objects', 'do_preproc',
                                       'num_distractors')] + [('distractors', C.c_int * 8), ('num_ws_cells', C.c_longlong)] + \
        [(n, C.c_void_p) for n in ('gt_rows', 'pred_rows', 'frame_gt_off', 'frame_pred_off', 'frame_ws_off', 'ws')] + \
        [('ws_bytes', C.c_size_t)] + [(n, C.c_void_p) for n in ('gt_keep', 'pred_keep', 'status')]


class StStereoEvalArgs(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('struct_size', 'N', 'H', 'W', 'gt_kind', 'num_bins', 'num_thresholds',
                                       'max_boxes')] + \
        [(n, C.c_size_t) for n in ('pred_img_pitch', 'gt_img_pitch', 'workspace_bytes')] + \
        [('bf', C.c_float), ('depth_edges', C.c_float * 9), ('bad_thresholds', C.c_float * 6)]


class StTrackletArgs(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('struct_size', 'num_rows', 'num_out_rows', 'num_tracks', 'first', 'count',
                                       'num_groups', 'max_rows')] + \
        [(n, C.c_void_p) for n in ('rows', 'row_out_off', 'row_gap', 'trk_out_off', 'trk_order', 'trk_len_scale', 'ws')] + \
        [('ws_bytes', C.c_size_t), ('out_rows', C.c_void_p), ('status', C.c_void_p), ('phase_ticks', C.c_void_p)]


class StAflinkArgs(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('struct_size', 'num_sets', 'num_tracks', 'num_rows', 'capacity', 'first', 'count',
                                       'chunk')] + \
        [(n, C.c_double) for n in ('t_lo', 't_hi', 'spatial_thr')] + \
        [(n, C.c_void_p) for n in ('feat', 'trk_off', 'trk_set', 'set_off', 'ws_off', 'ws_x', 'header', 'cand', 'conf',
                                   'logits')]


class StStreamTick(C.Structure):
    _fields_ = [('struct_size', C.c_int), ('streams', C.c_int), ('chunk', C.c_int), ('num_chunks', C.c_int),
                ('max_dets', C.c_int), ('det_rows', C.c_int), ('stream_of_slot', C.c_void_p), ('frame_ids', C.c_void_p)]


class StHeadPredLevel(C.Structure):
    _fields_ = [('cls_dev', C.c_void_p), ('cls_ld', C.c_int), ('cls_off', C.c_int),
                ('reg_dev', C.c_void_p), ('reg_ld', C.c_int), ('reg_off', C.c_int),
                ('wgt_cls_dev', C.c_void_p), ('bias_cls_dev', C.c_void_p),
                ('wgt_reg_dev', C.c_void_p), ('bias_reg_dev', C.c_void_p),
                ('out_dev', C.c_void_p), ('M', C.c_int)]


class StDecodeDesc(C.Structure):
    _fields_ = [
        ('struct_size', C.c_int), ('batch', C.c_int), ('num_levels', C.c_int),
        ('level_h', C.c_int * 4), ('level_w', C.c_int * 4), ('level_stride', C.c_int * 4),
        ('level_offset', C.c_size_t * 4),
        ('score_thr', C.c_float), ('iou_thr', C.c_float), ('max_det', C.c_int),
        ('scale_x', C.c_float), ('scale_y', C.c_float), ('pad_left', C.c_float), ('pad_top', C.c_float),
        ('ori_w', C.c_float), ('ori_h', C.c_float), ('nms_mask_rows', C.c_int), ('num_classes', C.c_int),
        ('single_label', C.c_int),
    ]


_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_PROTOS = {
    'st_version': (C.c_int, []),
    'st_head_row_floats': (_i, [_i]),
    'st_png_unfilter': (_i, [_vp, _i, _i, _i, _vp]),
    'st_stem_focus_conv_u8': (_i, [_vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _i, _vp, _i, _i, _i, _vp]),
    'st_detector_forward_raw': (_i, [_vp, _vp, _i, _i, _f, _vp, _vp, _sz, _vp, _vp]),
    'st_detector_forward_phase0_raw': (_i, [_vp, _vp, _vp, _i, _i, _f, _vp, _sz, _vp]),
    'st_pack_raw_frames': (_i, [_vp, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    'st_resize_planes': (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _vp]),
    'st_rectify_remap': (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'st_detector_set_split': (_i, [_vp, _i]),
    'st_split_instances_available': (_i, []),
    'st_volume_agg3d': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _f, _i, _vp]),
    'st_last_error': (C.c_char_p, []),
    'st_conv2d_nhwc': (_i, [C.POINTER(StConvDesc), _vp]),
    'st_conv2d_nhwc_variant': (_i, [C.POINTER(StConvDesc), _vp, _i]),
    'st_conv3x3_wino_group': (_i, [C.POINTER(StConvDesc), _i, _vp]),
    'st_head_pred': (_i, [C.POINTER(StHeadPredLevel), _i, _i, _vp]),
    'st_detector_op_owner': (_i, [_vp, _i, _vp, _vp]),
    'st_conv1x1_chain': (_i, [C.POINTER(StConvDesc), C.POINTER(StConvDesc), _vp]),
    'st_front_frag_floats': (_sz, [_i, _i]),
    'st_front_pack_frags': (_i, [_vp, _i, _i, _vp]),
    'st_conv3x3s2_csp_front': (_i, [C.POINTER(StConvDesc), C.POINTER(StConvDesc), C.POINTER(StConvDesc), _vp, _vp, _vp]),
    'st_csp_tail_frag_floats': (_sz, []),
    'st_csp_tail_pack_frags': (_i, [_vp, _vp]),
    'st_conv3x3_csp_tail': (_i, [C.POINTER(StConvDesc), C.POINTER(StConvDesc), _vp, _vp]),
    'st_conv_packed_floats': (_sz, [_i, _i, _i, _i]),
    'st_wino_packed_floats': (_sz, [_i, _i]),
    'st_wino_pack_weights': (_i, [_vp, _i, _i, _vp]),
    'st_conv_pack_weights': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_double, _i, _i, _i, _i, _vp, _vp]),
    'st_focus_pack': (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    'st_stem_packed_floats': (_sz, [_i]),
    'st_stem_pack_weights': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_double, _i, _i, _vp, _vp]),
    'st_stem_focus_conv': (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i, _i, _i, _vp]),
    'st_pack_raw_inputs': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp]),
    'st_spp_pool': (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    'st_detector_create': (_i, [C.POINTER(StDetectorConfig), C.POINTER(_vp)]),
    'st_detector_destroy': (_i, [_vp]),
    'st_detector_num_params': (_i, [_vp]),
    'st_detector_param_info': (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(C.c_int64), C.POINTER(_i)]),
    'st_detector_set_param': (_i, [_vp, C.c_char_p, _vp, C.c_int64]),
    'st_detector_finalize': (_i, [_vp]),
    'st_detector_workspace_bytes': (_sz, [_vp]),
    'st_detector_head_floats': (_sz, [_vp]),
    'st_detector_num_levels': (_i, [_vp]),
    'st_detector_level_info': (_i, [_vp, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_sz)]),
    'st_detector_forward': (_i, [_vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    'st_detector_forward_phase': (_i, [_vp, _i, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    'st_detector_macs': (C.c_double, [_vp]),
    'st_detector_set_timing': (_i, [_vp, _i]),
    'st_detector_num_ops': (_i, [_vp]),
    'st_detector_op_times': (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    'st_detector_autotune': (_i, [_vp, _vp, _sz, _vp, _vp, _i]),
    'st_conv_variant_name': (C.c_char_p, [_i]),
    'st_conv_variant_signature': (C.c_char_p, [_i]),
    'st_detector_get_tuning': (_i, [_vp, _vp, _i]),
    'st_detector_set_tuning': (_i, [_vp, _vp, _i]),
    'st_detector_op_desc': (_i, [_vp, _i, C.c_char_p, _i]),
    'st_detector_tap': (_i, [_vp, C.c_char_p, _vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i),
                             C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    'st_decode_nms_workspace_bytes': (_sz, [C.POINTER(StDecodeDesc)]),
    'st_lapjv_extended': (_i, [_vp, _i, _i, C.c_double, _vp, _vp]),
    'st_tracker_create': (_i, [C.POINTER(StTrackerConfig), C.POINTER(_vp)]),
    'st_tracker_destroy': (_i, [_vp]),
    'st_tracker_reset': (_i, [_vp]),
    'st_tracker_track': (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, C.POINTER(_i)]),
    'st_tracker_track_records': (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp]),
    'st_tracker_cmc_needed': (_i, [_vp, _i, _i]),
    'st_tracker_track_cmc': (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i, C.POINTER(_i)]),
    'st_tracker_track_records_cmc': (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, C.POINTER(_i), _vp, _vp, _i, _vp,
                                          C.POINTER(_i)]),
    'st_cmc_num_levels': (_i, [_vp]),
    'st_cmc_workspace_bytes': (_sz, [_i]),
    'st_cmc_front_u8': (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    'st_cmc_front_f32': (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    'st_cmc_flow': (_i, [_vp, _vp, _i, _i, _vp, _sz, _vp, _vp, _vp]),
    'st_cmc_estimate': (_i, [_vp, _vp, _i, _i, _i, C.POINTER(StCmcParams), _vp, _sz, _vp, _vp, _vp, _vp]),
    'st_cmc_mesh_fit': (_i, [_vp, _i, _i, _i, C.POINTER(StCmcParams), _vp, _sz, _vp, _vp, _vp, _vp]),
    'st_cmc_fit': (_i, [_vp, _i, _i, C.c_float, C.c_float, _vp, _sz, _vp, _vp, _vp]),
    'st_cmc_ecc_plane_size': (_i, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    'st_cmc_ecc_workspace_bytes': (_sz, [_i, _i, _i]),
    'st_cmc_ecc_front_u8': (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    'st_cmc_ecc_front_f32': (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    'st_cmc_ecc_prepare': (_i, [_vp, _vp, _i, _i, _i, C.POINTER(StEccParams), _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    'st_cmc_ecc_step': (_i, [_vp, _vp, _i, _i, _i, C.POINTER(StEccParams), _vp, _vp, _sz, _vp, _vp]),
    'st_cmc_ecc_estimate': (_i, [_vp, _vp, _i, _i, _i, C.POINTER(StEccParams), _vp, _sz, _vp, _vp, _vp]),
    'st_sgbm_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'st_sgbm_u8': (_i, [_vp, _vp, _i, _i, _i, _i, _i, C.POINTER(StSgbmParams), _vp, _sz, _vp, _i, _i, _vp, _vp]),
    'st_sgbm_f32': (_i, [_vp, _vp, _i, _i, _i, _i, _i, C.POINTER(StSgbmParams), _vp, _sz, _vp, _vp, _vp]),
    'st_sgbm_match_f32': (_i, [_vp, _vp, _i, _i, _i, _i, _i, C.POINTER(StSgbmParams), _vp, _sz, _vp, _vp, _vp]),
    'st_sgbm_median': (_i, [_vp, _i, _i, _i, _vp, _vp]),
    'st_sgbm_speckle': (_i, [_vp, _i, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _i, _i, _vp, _vp]),
    'st_tracker_num_tracks': (_i, [_vp]),
    'st_tracker_next_id': (C.c_longlong, [_vp]),
    'st_tracker_get_track': (_i, [_vp, _i, _vp, _vp, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    'st_tracker_get_states': (_i, [_vp, _vp, _i, _i, C.POINTER(_i), C.POINTER(C.c_longlong)]),
    'st_batched_tracker_get_states': (_i, [_vp, _vp, _i, _vp, _i, _i, C.POINTER(_i), C.POINTER(C.c_longlong),
                                           C.POINTER(_i), _vp]),
    'st_batched_tracker_create': (_i, [C.POINTER(StTrackerConfig), _i, _i, _i, C.POINTER(_vp)]),
    'st_batched_tracker_create_multi': (_i, [C.POINTER(StTrackerConfig), _i, _i, _i, C.POINTER(_vp)]),
    'st_batched_tracker_run': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'st_batched_tracker_destroy': (_i, [_vp]),
    'st_batched_tracker_state_bytes': (_sz, [_vp]),
    'st_batched_tracker_scratch_bytes': (_sz, [_vp]),
    'st_batched_tracker_step': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'st_decode_nms': (_i, [C.POINTER(StDecodeDesc), _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    'st_costvolume_softargmin': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp]),
    'st_softargmin': (_i, [_vp, _i, _i, _i, _i, _f, _vp, _vp]),
    'st_disp_upsample_pack': (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    'st_softargmin_right': (_i, [_vp, _i, _i, _i, _i, _f, _vp, _vp]),
    'st_lr_check_pack': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp]),
    'st_feat_upsample': (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    'st_costvolume_agg3d_supported': (_i, [_i, _i]),
    'st_costvolume_agg3d': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _f, _i, _vp, _vp]),
    'st_costvolume_agg3d_softargmin': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _f, _i, _f, _vp, _vp]),
    'st_box_depth_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'st_pack_records': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    'st_box_depth': (_i, [_vp, _sz, _i, _i, _i, _vp, _vp, _i, _f, _f, _vp, _sz, _vp, _vp, _vp, _vp]),
    'st_coco_max_gt': (_i, []),
    'st_coco_workspace_bytes': (_sz, [C.POINTER(StCocoArgs)]),
    'st_coco_prepare': (_i, [C.POINTER(StCocoArgs), _vp]),
    'st_coco_match': (_i, [C.POINTER(StCocoArgs), _vp]),
    'st_coco_accumulate': (_i, [C.POINTER(StCocoArgs), _vp]),
    'st_mot_max_objects': (_i, []),
    'st_mot_max_alphas': (_i, []),
    'st_mot_workspace_bytes': (_sz, [C.POINTER(StMotArgs)]),
    'st_mot_workspace_sim_offset': (_sz, [C.POINTER(StMotArgs)]),
    'st_mot_similarity': (_i, [C.POINTER(StMotArgs), _vp]),
    'st_mot_walk': (_i, [C.POINTER(StMotArgs), _vp]),
    'st_mot_hota_match': (_i, [C.POINTER(StMotArgs), _vp]),
    'st_mot_hota_accumulate': (_i, [C.POINTER(StMotArgs), _vp]),
    'st_mot_kitti_workspace_bytes': (_sz, [C.POINTER(StMotKittiArgs)]),
    'st_mot_kitti_preprocess': (_i, [C.POINTER(StMotKittiArgs), _vp]),
    'st_mot_file_round': (_i, [_vp, _vp, C.c_longlong, _i, C.POINTER(C.c_int), _vp, _vp]),
    'st_mot_challenge_workspace_bytes': (_sz, [C.POINTER(StMotChallengeArgs)]),
    'st_mot_challenge_preprocess': (_i, [C.POINTER(StMotChallengeArgs), _vp]),
    'st_stereo_eval_workspace_bytes': (_sz, [C.POINTER(StStereoEvalArgs)]),
    'st_stereo_eval': (_i, [C.POINTER(StStereoEvalArgs), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'st_tracklet_max_rows': (_i, []),
    'st_tracklet_gsi_workspace_bytes': (_sz, [C.POINTER(StTrackletArgs)]),
    'st_tracklet_interpolate': (_i, [C.POINTER(StTrackletArgs), _vp]),
    'st_tracklet_gsi': (_i, [C.POINTER(StTrackletArgs), _vp]),
    'st_aflink_group_pairs': (_i, []),
    'st_aflink_packed_floats': (_sz, []),
    'st_aflink_max_candidates': (_i, []),
    'st_aflink_weights_create': (_i, [_vp, _sz, C.POINTER(_vp)]),
    'st_aflink_weights_destroy': (_i, [_vp]),
    'st_aflink_gate': (_i, [C.POINTER(StAflinkArgs), _vp]),
    'st_aflink_transform': (_i, [C.POINTER(StAflinkArgs), _vp]),
    'st_aflink_score': (_i, [C.POINTER(StAflinkArgs), _vp, _vp]),
    'st_aflink_run': (_i, [C.POINTER(StAflinkArgs), _vp, _vp]),
    'st_box_depth_method': (_i, [_vp, _sz, _i, _i, _i, _vp, _vp, _i, _f, _f, _vp, _sz, _vp, _vp, _vp, _vp, _i]),
    'st_stream_record_bytes': (_sz, [_i, _i, _i]),
    'st_stream_gather': (_i, [C.POINTER(StStreamTick), _vp, _vp, _vp, _vp, _vp, _vp]),
    'st_stream_unscale': (_i, [C.POINTER(StStreamTick), _vp, _vp, _vp, _vp, _vp]),
    'st_disp_head_create': (_i, [C.POINTER(StDispHeadConfig), C.POINTER(_vp)]),
    'st_disp_head_destroy': (_i, [_vp]),
    'st_disp_head_num_params': (_i, [_vp]),
    'st_disp_head_param_info': (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(C.c_int64), C.POINTER(_i)]),
    'st_disp_head_set_param': (_i, [_vp, C.c_char_p, _vp, C.c_int64]),
    'st_disp_head_finalize': (_i, [_vp]),
    'st_disp_head_workspace_bytes': (_sz, [_vp]),
    'st_disp_head_forward': (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _sz, _vp, _vp]),
    'st_disp_head_tap': (_i, [_vp, C.c_char_p, _vp, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i),
                              C.POINTER(_i), C.POINTER(_i)]),
    'st_disp_head_resize': (_i, [_vp, _i, _i, _i, _vp, _i, _i, _vp]),
    'st_disp_fuse': (_i, [_vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    'st_disp_head_set_timing': (_i, [_vp, _i]),
    'st_disp_head_num_launches': (_i, []),
    'st_disp_head_launch_name': (C.c_char_p, [_i]),
    'st_disp_head_launch_times': (_i, [_vp, _i, _vp]),
    'st_stream_record': (_i, [C.POINTER(StStreamTick), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}

_lib = None


def load():
    """Load (once) and return the ctypes handle; raises if the HIP library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get('ST_LIBRARY') or LIB_PATH   # ST_LIBRARY: tools/ load the -DST_ABLATION build
    if not os.path.exists(path):
        raise RuntimeError(
            f'{path} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            f'(or `make -C stereotracking_amd/csrc`).  stereotracking_amd has no CPU fallback.')
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)  # AttributeError = the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=''):
    if rc != ST_OK:
        msg = load().st_last_error()
        raise StError(f'{what or "libstereotrack_hip"}: {_ERR_NAMES.get(rc, rc)}: '
                      f'{msg.decode() if msg else ""}')


def ptr(t):
    """Device/host pointer of a contiguous float32/int tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError('tensor must be contiguous')
    return C.c_void_p(t.data_ptr())


def current_stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
