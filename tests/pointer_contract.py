"""The pointer contract of the C ABI, one row per (export, device-pointer argument) - test infrastructure, a helper
module like stream_schedule.py (DESIGN.md "Pointer contract").

include/stereotrack.h and include/stereotrack_jpeg.h take raw pointers and raw `ld` / `off` integers.  What an entry
point does with a pointer that is aligned to its element but not to 16 bytes is one of three things, read off its
launcher (the file and the clause are named in every row):

  dispatch  the launcher (or the kernel, per address) takes a scalar path: same results, bit for bit
  required  refused with ST_ERR_INVALID, by name, in front of the first launch, memset or copy
  free      every kernel makes element-sized accesses through it; any alignment of the element type works.  For a
            `void*` workspace the element is the widest field it holds (8 bytes: fp64 sums, 64-bit keys)

ROWS[export][argument] = (class, align, fields, where):
  align   the smallest alignment in bytes the entry accepts for the pointer (`required`: below it the call is refused;
          `dispatch` / `free`: the element size)
  fields  the `ld` / `off` integers that belong to the pointer and fall under the same rule (multiples of 4 floats
          for the 16-byte path), () where it has none
  where   file:clause the class was read from
An argument `d.in_dev` is field in_dev of the struct the parameter `d` points to; `args.*` is every pointer field of
the struct that HOST does not name; `frames_host[]` is every device pointer the host array `frames_host` holds.

HOST[export] = the pointer parameters (and struct fields) that are host memory or opaque handles: out of scope, listed
by name so that the completeness check of tests/test_cpu_pointer_contract.py sees every pointer of the two headers.

Every `dispatch` and `required` row is executed - by tests/test_pointer_contract_gpu.py (CASES), or on host memory by
tests/test_cpu_pointer_contract.py (HOST_CASES) - or is named in NOT_RUN with the reason; the CPU test holds the three to
the table, so a new row of either class without a test fails there."""
import os
import re

import stream_schedule as ss

HEADERS = (ss.HEADER, os.path.join(ss.ROOT, 'include', 'stereotrack_jpeg.h'))

D, R, F = 'dispatch', 'required', 'free'

# ---- the conv descriptor: the same struct under six entry points ------------------------------------------------------
# st_conv2d_nhwc and the tile instances 0..21 of st_conv2d_nhwc_variant (conv_igemm.hip conv2d_launch): the operands are
# staged in 16-byte buffer loads, the epilogue stores element by element.
_TILE = {
    'in_dev': (R, 16, ('in_ld', 'in_off', 'Cin'), 'conv_igemm.hip: conv2d_launch, "Cin/in_ld/in_off" + "in_dev and wgt_dev"'),
    'wgt_dev': (R, 16, (), 'conv_igemm.hip: conv2d_launch, "in_dev and wgt_dev"'),
    'bias_dev': (F, 4, (), 'conv_igemm.hip: conv_epilogue reads p.bias[j]'),
    'out1_dev': (F, 4, ('out1_ld', 'out1_off', 'split'), 'conv_igemm.hip: conv_epilogue stores o1[...] = v'),
    'out2_dev': (F, 4, ('out2_ld', 'out2_off'), 'conv_igemm.hip: conv_epilogue, as out1'),
    'up_dev': (F, 4, ('up_ld', 'up_off'), 'conv_igemm.hip: conv_epilogue, the four upsampled stores'),
    'res_dev': (F, 4, ('res_ld', 'res_off'), 'conv_igemm.hip: conv_epilogue reads rs[...]'),
    'wgt_wino_dev': (F, 4, (), 'conv_igemm.hip: not read by the tile instances'),
}


def _desc(param, table):
    return {f'{param}.{k}': v for k, v in table.items()}


def _all16(param, fields, where, also_free=()):
    out = {f'{param}.{k}': (R, 16, (), where) for k in fields}
    out.update({f'{param}.{k}': (F, 4, (), where + ' (not read)') for k in also_free})
    return out


ROWS = {
    # ---- 1. convolutions -------------------------------------------------------------------------------------------
    'st_conv2d_nhwc': _desc('d', _TILE),
    # tile instances as st_conv2d_nhwc; what a forced special instance (41 .. 46) does with each base pointer is the
    # BASES table of tests/test_pointer_contract_gpu.py, executed there against the *_applicable functions
    'st_conv2d_nhwc_variant': _desc('d', _TILE),
    'st_conv3x3_wino_group': dict(
        _all16('descs', ('in_dev', 'out1_dev', 'wgt_wino_dev', 'bias_dev'),
               'wino_conv.hip: wino_group_applicable -> wino_conv_applicable',
               also_free=('wgt_dev', 'out2_dev', 'up_dev', 'res_dev'))),      # a residual of any alignment is refused
    'st_conv1x1_chain': dict(
        {'a.in_dev': (R, 16, ('in_ld', 'in_off'), 'pointwise_conv.hip: pw_conv_applicable / pointwise_resident.hip: pwr_conv_applicable'),
         'a.wgt_dev': (R, 16, (), 'pointwise_conv.hip: pw_conv_applicable / pointwise_resident.hip: pwr_conv_applicable'),
         'a.bias_dev': (F, 4, (), 'pointwise_conv.hip: bl[tid] = p.bias[tid]'),
         'a.out1_dev': (D, 4, ('out1_ld', 'out1_off', 'split'), 'pointwise_conv.hip: pw_conv_launch `vec` (Cin 32 / 64; the resident pair 128 / 256 -> 64 | 64 refuses: pwr_conv_applicable)'),
         'a.out2_dev': (D, 4, ('out2_ld', 'out2_off'), 'pointwise_conv.hip: pw_conv_launch `vec`'),
         'a.res_dev': (F, 4, (), 'pointwise_conv.hip: pw_chain_applicable refuses a residual on `a`'),
         'a.up_dev': (F, 4, (), 'pointwise_conv.hip: pw_conv_applicable refuses an upsample store'),
         'a.wgt_wino_dev': (F, 4, (), 'pointwise_conv.hip: not read'),
         'b.in_dev': (R, 16, (), 'pointwise_conv.hip: pw_chain_applicable runs pw_conv_applicable on `b` too (the field is otherwise ignored)'),
         'b.wgt_dev': (R, 16, (), 'pointwise_conv.hip: pw_chain_applicable -> pw_conv_applicable(b)'),
         'b.bias_dev': (F, 4, (), 'pointwise_conv.hip: bl2[tid] = p.bias2[tid]'),
         'b.out1_dev': (D, 4, ('out1_ld', 'out1_off'), 'pointwise_conv.hip: pw_conv_launch `vec`, chain clause'),
         'b.out2_dev': (F, 4, (), 'pointwise_conv.hip: pw_chain_applicable refuses a split on `b`'),
         'b.up_dev': (F, 4, (), 'pointwise_conv.hip: pw_chain_applicable refuses it'),
         'b.res_dev': (F, 4, (), 'pointwise_conv.hip: pw_chain_applicable refuses it'),
         'b.wgt_wino_dev': (F, 4, (), 'pointwise_conv.hip: not read')}),
    'st_conv3x3s2_csp_front': dict(
        {'a.in_dev': (R, 16, ('in_ld', 'in_off'), 'front_fused.hip: front_fused_applicable'),
         'a.wgt_dev': (R, 16, (), 'front_fused.hip: front_fused_applicable'),
         'a.bias_dev': (F, 4, (), 'front_fused.hip: bias[tid] = p.bias_a[tid]'),
         'ms.bias_dev': (F, 4, (), 'front_fused.hip: staged element by element'),
         'c1.bias_dev': (F, 4, (), 'front_fused.hip: staged element by element'),
         'ms.out1_dev': (R, 16, ('out1_ld', 'out1_off'), 'front_fused.hip: front_fused_applicable'),
         'ms.out2_dev': (R, 16, ('out2_ld', 'out2_off'), 'front_fused.hip: front_fused_applicable'),
         'c1.out1_dev': (R, 16, ('out1_ld', 'out1_off'), 'front_fused.hip: front_fused_applicable'),
         'frag_ms_dev': (R, 16, (), 'front_fused.hip: front_fused_launch, "fragment weights must be 16-byte aligned"'),
         'frag_c1_dev': (R, 16, (), 'front_fused.hip: front_fused_launch, "fragment weights must be 16-byte aligned"')},
        **{f'{p}.{k}': (F, 4, (), 'front_fused.hip: not read') for p, ks in (
            ('a', ('out1_dev', 'out2_dev', 'up_dev', 'res_dev', 'wgt_wino_dev')),
            ('ms', ('in_dev', 'wgt_dev', 'up_dev', 'res_dev', 'wgt_wino_dev')),
            ('c1', ('in_dev', 'wgt_dev', 'out2_dev', 'up_dev', 'res_dev', 'wgt_wino_dev'))) for k in ks}),
    'st_conv3x3_csp_tail': dict(
        {'frag_fin_dev': (R, 16, (), 'wino_csp_tail.hip: csp_tail_launch, first clause')},
        **_all16('conv2', ('in_dev', 'res_dev', 'bias_dev', 'wgt_wino_dev', 'out1_dev'),
                 'wino_csp_tail.hip: csp_tail_applicable `al` (out1_dev == fin.in_dev)', also_free=('wgt_dev', 'out2_dev', 'up_dev')),
        **_all16('fin', ('in_dev', 'out1_dev', 'res_dev', 'bias_dev'), 'wino_csp_tail.hip: csp_tail_applicable `al`',
                 also_free=('wgt_dev', 'out2_dev', 'up_dev', 'wgt_wino_dev'))),
    # ---- 2. input packing ------------------------------------------------------------------------------------------
    'st_focus_pack': {
        'img_nchw_dev': (R, 8, (), 'pack_pool.hip: focus_pack_launch, "8-byte and the output 16-byte"'),
        'out_nhwc_dev': (R, 16, (), 'pack_pool.hip: focus_pack_launch')},
    'st_stem_focus_conv': {
        'img_nchw_dev': (R, 16, (), 'stem_focus_conv.hip: stem_focus_conv_launch, "input must be 16-byte aligned"'),
        'wgt_dev': (F, 4, (), 'stem_focus_conv.hip: wl[idx] = p.wgt[idx]'),
        'bias_dev': (R, 16, (), 'stem_focus_conv.hip: stem_focus_conv_launch, "bias must be 16-byte aligned"'),
        'out_nhwc_dev': (D, 4, ('out_ld', 'out_off', 'Cout'), 'stem_focus_conv.hip: stem_focus_conv_launch `vec`')},
    'st_stem_focus_conv_u8': {
        'frames_u8_dev_ptrs_host[]': (R, 4, (), 'stem_focus_conv.hip: stem_focus_conv_launch, "raw frame %d null or not 4-byte aligned"'),
        'wgt_dev': (F, 4, (), 'stem_focus_conv.hip: as st_stem_focus_conv'),
        'bias_dev': (R, 16, (), 'stem_focus_conv.hip: as st_stem_focus_conv'),
        'out_dev': (D, 4, ('out_ld', 'out_off', 'Cout'), 'stem_focus_conv.hip: stem_focus_conv_launch `vec`')},
    'st_pack_raw_inputs': {
        'img_u8_dev': (D, 1, (), 'pack_pool.hip: st_pack_raw_inputs `al(img_u8_dev, 4)`'),
        'disp_u16_dev': (D, 2, (), 'pack_pool.hip: `al(disp_u16_dev, 8)`'),
        'img_out_dev': (D, 4, (), 'pack_pool.hip: `al(img_out_dev, 16)`'),
        'disp_postp_out_dev': (D, 4, (), 'pack_pool.hip: `al(disp_postp_out_dev, 16)`'),
        'disp_mask_out_dev': (D, 4, (), 'pack_pool.hip: `al(disp_mask_out_dev, 16)`')},
    'st_pack_raw_frames': {'img_out_dev': (R, 16, (), 'pack_pool.hip: st_pack_raw_frames, second clause'),
                           'frames_u8_dev_ptrs_host[]': (R, 4, (), 'pack_pool.hip: st_pack_raw_frames, "frame %d null or not 4-byte aligned"')},
    'st_resize_planes': {'in_dev': (F, 1, (), 'pack_pool.hip: resize_*_kernel index element by element'),
                         'out_dev': (F, 1, (), 'pack_pool.hip: as in_dev')},
    'st_rectify_remap': {
        'src_dev_ptrs_host[]': (R, 1, (), 'rectify.hip: st_rectify_remap, "frame %d not aligned to its element size" (1, 2 or 4 bytes)'),
        'dst_dev_ptrs_host[]': (D, 1, (), 'rectify.hip: as dst_block_dev, per address; the element size is required'),
        'maps_dev': (R, 8, (), 'rectify.hip: st_rectify_remap, "maps must be 8-byte aligned"'),
        'dst_block_dev': (D, 1, (), 'rectify.hip: rectify_bilinear_u8_kernel, per address `(dst & 3) == 0`; the element size is required')},
    'st_spp_pool': {'x_dev': (R, 16, ('x_ld', 'x_off', 'C'), 'pack_pool.hip: spp_pool_launch'),
                    'out_dev': (R, 16, ('out_ld', 'out_off'), 'pack_pool.hip: spp_pool_launch')},
    # ---- 3. detector -----------------------------------------------------------------------------------------------
    **{name: {a: (R, 16, (), 'detector.cpp: run_ops, first clause') for a in args} for name, args in (
        ('st_detector_forward', ('img_dev', 'disp_dev', 'workspace_dev', 'head_out_dev')),
        ('st_detector_forward_phase', ('img_dev', 'disp_dev', 'right_dev', 'workspace_dev', 'head_out_dev')),
        ('st_detector_forward_phase0_raw', ('workspace_dev',)),
        ('st_detector_forward_raw', ('disp_dev', 'workspace_dev', 'head_out_dev')),
        ('st_detector_autotune', ('workspace_dev', 'head_out_dev')))},
    'st_detector_tap': {'workspace_dev': (F, 1, (), 'detector.cpp: pointer arithmetic only, never dereferenced')},
    'st_head_pred': dict(
        {f'levels.{k}': (R, 16, f, 'head_pred.hip: head_pred_launch, per level') for k, f in (
            ('cls_dev', ('cls_ld', 'cls_off')), ('reg_dev', ('reg_ld', 'reg_off')), ('out_dev', ()))},
        **{f'levels.{k}': (F, 4, (), 'head_pred.hip: staged into LDS element by element') for k in (
            'wgt_cls_dev', 'bias_cls_dev', 'wgt_reg_dev', 'bias_reg_dev')}),
    # ---- 4. decode + NMS -------------------------------------------------------------------------------------------
    'st_decode_nms': {
        'head_out_dev': (R, 16, ('level_offset',), 'decode_nms.hip: st_decode_nms, "head_out_dev" (1..3 classes; wider heads read element by element)'),
        'workspace_dev': (R, 16, (), 'decode_nms.hip: st_decode_nms, "workspace_dev and out_boxes_dev"'),
        'out_boxes_dev': (R, 16, (), 'decode_nms.hip: st_decode_nms, "workspace_dev and out_boxes_dev"'),
        'out_scores_dev': (F, 4, (), 'decode_nms.hip: nms_reduce_kernel'),
        'out_labels_dev': (F, 8, (), 'decode_nms.hip: nms_reduce_kernel'),
        'out_prior_idx_dev': (F, 4, (), 'decode_nms.hip: nms_reduce_kernel'),
        'out_count_dev': (F, 4, (), 'decode_nms.hip: nms_reduce_kernel')},
    # ---- 5. stereo module ------------------------------------------------------------------------------------------
    'st_costvolume_softargmin': {
        'featL_dev': (R, 16, ('C', 'feat_ld'), 'costvolume.hip: st_costvolume_softargmin, "featL_dev and featR_dev"'),
        'featR_dev': (R, 16, ('C', 'feat_ld'), 'costvolume.hip: st_costvolume_softargmin, "featL_dev and featR_dev"'),
        'out_cost_dev': (D, 4, (), 'costvolume.hip: `dgt <= 32 && (out_cost_dev == nullptr || aligned)` -> tiled, else generic'),
        'out_disp_dev': (F, 4, (), 'costvolume.hip: one float per pixel')},
    'st_volume_agg3d': {'vol_in_dev': (R, 16, ('D',), 'agg3d.hip: st_volume_agg3d, "volumes must be 16-byte aligned"'),
                        'vol_out_dev': (R, 16, ('D',), 'agg3d.hip: st_volume_agg3d')},
    'st_costvolume_agg3d': {'featL_dev': (R, 16, ('feat_ld',), 'agg3d.hip: cva_launch, "buffers must be 16-byte aligned"'),
                            'featR_dev': (R, 16, ('feat_ld',), 'agg3d.hip: cva_launch'),
                            'vol_out_dev': (R, 16, ('D',), 'agg3d.hip: cva_launch')},
    'st_costvolume_agg3d_softargmin': {'featL_dev': (R, 16, ('feat_ld',), 'agg3d.hip: cva_launch'),
                                       'featR_dev': (R, 16, ('feat_ld',), 'agg3d.hip: cva_launch'),
                                       'disp_out_dev': (F, 4, (), 'agg3d.hip: one float per pixel')},
    'st_softargmin': {'cost_dev': (D, 4, ('D',), 'costvolume.hip: st_softargmin, both `(cost_dev & 15) == 0` clauses'),
                      'out_disp_dev': (F, 4, (), 'costvolume.hip: one float per pixel')},
    'st_disp_upsample_pack': {'disp_lr_dev': (F, 4, (), 'costvolume.hip: bilinear gathers, element by element'),
                              'disp_postp_dev': (D, 4, ('W',), 'costvolume.hip: st_disp_upsample_pack `W % 4 == 0 && aligned`')},
    'st_softargmin_right': {'vol_dev': (D, 4, ('D',), 'lr_check.hip: st_softargmin_right `D % 4 == 0 && aligned`'),
                            'out_disp_right_dev': (F, 4, (), 'lr_check.hip: one float per pixel')},
    'st_lr_check_pack': {'disp_left_dev': (F, 4, (), 'lr_check.hip: gathers, element by element'),
                         'disp_right_dev': (F, 4, (), 'lr_check.hip: gathers, element by element'),
                         'disp_postp_dev': (D, 4, ('W',), 'lr_check.hip: st_lr_check_pack `align`'),
                         'disp_mask_dev': (D, 4, ('W',), 'lr_check.hip: st_lr_check_pack `align`')},
    'st_feat_upsample': {'feat_dev': (R, 16, ('C', 'feat_ld'), 'costvolume.hip: st_feat_upsample, third clause'),
                         'out_dev': (R, 16, (), 'costvolume.hip: st_feat_upsample, third clause')},
    # ---- 6. per-box depth, records ---------------------------------------------------------------------------------
    **{name: {'disp_dev': (F, 4, (), 'box_depth.hip: window reads element by element'),
              'boxes_dev': (R, 16, (), 'box_depth.hip: box_depth_launch, "boxes_dev and out_scaled_boxes_dev"'),
              'counts_dev': (F, 4, (), 'box_depth.hip'),
              'workspace_dev': (F, 1, (), 'box_depth.hip: unused (st_box_depth_workspace_bytes() == 0)'),
              'out_depth_dev': (F, 4, (), 'box_depth.hip'), 'out_scale_dev': (F, 4, (), 'box_depth.hip'),
              'out_scaled_boxes_dev': (R, 16, (), 'box_depth.hip: box_depth_launch')}
       for name in ('st_box_depth', 'st_box_depth_method')},
    'st_pack_records': dict(
        {'boxes_dev': (R, 16, (), 'box_depth.hip: st_pack_records, "boxes_dev and scaled_boxes_dev"'),
         'scaled_boxes_dev': (R, 16, (), 'box_depth.hip: st_pack_records'),
         'labels_dev': (F, 8, (), 'box_depth.hip: pack_records_kernel')},
        **{k: (F, 4, (), 'box_depth.hip: pack_records_kernel, element by element') for k in (
            'scores_dev', 'depth_dev', 'scales_dev', 'prior_idx_dev', 'counts_dev', 'out_records_dev')}),
    # ---- 9. batched association (batched_assoc.hip: no access wider than its element) ------------------------------
    **{name: dict({k: (F, 4, (), 'batched_assoc.hip: element by element') for k in (
        'frame_ids_dev', 'dets_dev', 'counts_dev', 'out_rows_dev', 'out_counts_dev', 'status_dev') + extra},
        out_ids_dev=(F, 8, (), 'batched_assoc.hip'), state_dev=(F, 8, (), 'batched_assoc.hip: fp64 Kalman state'),
        scratch_dev=(F, 8, (), 'batched_assoc.hip: fp64 scratch'))
       for name, extra in (('st_batched_tracker_step', ()), ('st_batched_tracker_run', ('video_of_dev',)))},
    'st_batched_tracker_get_states': {'state_dev': (F, 8, (), 'batched_assoc.hip: copied to the host as bytes')},
    # ---- 10. camera-motion compensation ----------------------------------------------------------------------------
    'st_cmc_front_u8': {'planes_dev': (F, 4, (), 'cmc_flow.hip: element by element'),
                        'frames_u8_dev_ptrs_host[]': (F, 1, (), 'cmc_flow.hip: bytes')},
    'st_cmc_front_f32': {'batch_dev': (F, 4, (), 'cmc_flow.hip'), 'planes_dev': (F, 4, (), 'cmc_flow.hip')},
    'st_cmc_flow': {'prev_planes_dev': (F, 4, (), 'cmc_flow.hip'), 'curr_planes_dev': (F, 4, (), 'cmc_flow.hip'),
                    'ws': (F, 4, (), 'cmc_flow.hip: the Farneback buffers are fp32; the 64-bit keys belong to the fit'),
                    'flow_out_dev': (F, 4, (), 'cmc_flow.hip'), 'levels_out_dev': (F, 4, (), 'cmc_flow.hip')},
    'st_cmc_estimate': {'prev_planes_dev': (F, 4, (), 'cmc_flow.hip'), 'curr_planes_dev': (F, 4, (), 'cmc_flow.hip'),
                        'ws': (R, 8, (), 'cmc_flow.hip: require_estimate_args, "workspace must be 8-byte aligned" (64-bit atomicMax keys)'),
                        'warps_out_dev': (F, 4, (), 'cmc_flow.hip'), 'mesh_out_dev': (F, 4, (), 'cmc_flow.hip'),
                        'inliers_out_dev': (F, 1, (), 'cmc_flow.hip')},
    'st_cmc_mesh_fit': {'flow_dev': (F, 4, (), 'cmc_flow.hip'),
                        'ws': (R, 8, (), 'cmc_flow.hip: require_estimate_args'),
                        'warps_out_dev': (F, 4, (), 'cmc_flow.hip'), 'mesh_out_dev': (F, 4, (), 'cmc_flow.hip'),
                        'inliers_out_dev': (F, 1, (), 'cmc_flow.hip')},
    'st_cmc_fit': {'points_dev': (F, 4, (), 'cmc_flow.hip'),
                   'ws': (R, 8, (), 'cmc_flow.hip: st_cmc_fit, "workspace must be 8-byte aligned"'),
                   'warps_out_dev': (F, 4, (), 'cmc_flow.hip'), 'inliers_out_dev': (F, 1, (), 'cmc_flow.hip')},
    # ---- 11. SGBM --------------------------------------------------------------------------------------------------
    **{name: dict({k: (F, 4, (), 'sgbm.hip: element by element') for k in keys},
                  ws=(R, 8, (), 'sgbm.hip: check_params, "workspace must be 8-byte aligned" (D > 64: 8-byte volume words)'))
       for name, keys in (('st_sgbm_u8', ('disp_postp_dev', 'status_dev', 'left_ptrs_host[]', 'right_ptrs_host[]')),
                          ('st_sgbm_f32', ('left_dev', 'right_dev', 'disp_postp_dev', 'status_dev')))},
    'st_sgbm_match_f32': {'left_dev': (F, 4, (), 'sgbm.hip'), 'right_dev': (F, 4, (), 'sgbm.hip'),
                          'ws': (R, 8, (), 'sgbm.hip: check_params'),
                          'cost_out_dev': (F, 2, (), 'sgbm.hip'), 'disp_out_dev': (F, 2, (), 'sgbm.hip')},
    'st_sgbm_median': {'in_dev': (F, 2, (), 'sgbm.hip'), 'out_dev': (F, 2, (), 'sgbm.hip')},
    'st_sgbm_speckle': {'in_dev': (F, 2, (), 'sgbm.hip'), 'ws': (F, 4, (), 'sgbm.hip: int32 labels'),
                        'out_dev': (F, 2, (), 'sgbm.hip'), 'disp_postp_dev': (F, 4, (), 'sgbm.hip'),
                        'status_dev': (F, 4, (), 'sgbm.hip')},
    # ---- 12 .. 19: the evaluators and post-processors (no access wider than its element in their files) -------------
    **{name: {'args.*': (F, 8, (), f'{src}: element by element; fp64 / 64-bit fields at their own 8 bytes')}
       for src, names in (
           ('coco_eval.hip', ('st_coco_workspace_bytes', 'st_coco_prepare', 'st_coco_match', 'st_coco_accumulate')),
           ('mot_eval.hip', ('st_mot_workspace_bytes', 'st_mot_workspace_sim_offset', 'st_mot_similarity', 'st_mot_walk',
                             'st_mot_hota_match', 'st_mot_hota_accumulate', 'st_mot_kitti_workspace_bytes',
                             'st_mot_kitti_preprocess', 'st_mot_challenge_workspace_bytes', 'st_mot_challenge_preprocess')),
           ('tracklet_post.hip', ('st_tracklet_gsi_workspace_bytes', 'st_tracklet_interpolate', 'st_tracklet_gsi')),
           ('aflink.hip', ('st_aflink_gate', 'st_aflink_transform', 'st_aflink_score', 'st_aflink_run')))
       for name in names},
    'st_mot_file_round': {'rows_dev': (F, 8, (), 'mot_eval.hip'), 'out_dev': (F, 8, (), 'mot_eval.hip'),
                          'status_dev': (F, 4, (), 'mot_eval.hip')},
    # ---- 13. multi-stream tick (stream_track.hip: no access wider than its element) --------------------------------
    'st_stream_gather': {'dets_dev': (F, 4, (), 'stream_track.hip'), 'counts_dev': (F, 4, (), 'stream_track.hip'),
                         'frame_ids_dev': (F, 4, (), 'stream_track.hip'),
                         'record_dev': (F, 8, (), 'stream_track.hip: the record starts with its int64 ids')},
    'st_stream_unscale': {k: (F, 4, (), 'stream_track.hip') for k in ('rows_dev', 'out_counts_dev', 'boxes_dev', 'box_counts_dev')},
    'st_stream_record': dict({k: (F, 4, (), 'stream_track.hip') for k in (
        'rows_dev', 'out_counts_dev', 'status_dev', 'counts_dev', 'boxes_dev')},
        ids_dev=(F, 8, (), 'stream_track.hip'), record_dev=(F, 8, (), 'stream_track.hip')),
    # ---- 20. ECC ---------------------------------------------------------------------------------------------------
    'st_cmc_ecc_front_u8': {'planes_dev': (F, 4, (), 'cmc_ecc.hip'),
                            'frames_u8_dev_ptrs_host[]': (F, 1, (), 'cmc_ecc.hip: bytes')},
    'st_cmc_ecc_front_f32': {'batch_dev': (F, 4, (), 'cmc_ecc.hip'), 'planes_dev': (F, 4, (), 'cmc_ecc.hip')},
    **{name: dict({'prev_planes_dev': (F, 4, (), 'cmc_ecc.hip'), 'curr_planes_dev': (F, 4, (), 'cmc_ecc.hip'),
                   'ws': (R, 16, (), 'cmc_ecc.hip: require_args, "workspace must be 16-byte aligned" (float4 gradients)')},
                  **{k: (F, a, (), 'cmc_ecc.hip') for k, a in outs})
       for name, outs in (
           ('st_cmc_ecc_prepare', (('tmpl_out_dev', 4), ('input_out_dev', 4), ('gx_out_dev', 4), ('gy_out_dev', 4))),
           ('st_cmc_ecc_step', (('warps_in_dev', 8), ('step_out_dev', 8))),
           ('st_cmc_ecc_estimate', (('warps_out_dev', 4), ('iters_out_dev', 4))))},
    # ---- 22. stereo metric -----------------------------------------------------------------------------------------
    'st_stereo_eval': dict(
        {'pred_dev': (D, 4, ('W', 'pred_img_pitch'), 'stereo_eval.hip: st_stereo_eval `vec`'),
         'gt_dev': (D, 4, ('W', 'gt_img_pitch'), 'stereo_eval.hip: st_stereo_eval `vec`'),
         'workspace_dev': (R, 8, (), 'stereo_eval.hip: "workspace must be 8-byte aligned"'),
         'counts_dev': (F, 8, (), 'stereo_eval.hip'), 'sums_dev': (F, 8, (), 'stereo_eval.hip'),
         'hist_dev': (F, 8, (), 'stereo_eval.hip')},
        **{k: (F, 4, (), 'stereo_eval.hip: element by element') for k in ('extent_dev', 'boxes_dev', 'box_counts_dev')}),
    # ---- 23. disparity-completion head -----------------------------------------------------------------------------
    'st_disp_head_forward': {
        'p3_dev': (R, 16, ('p3_ld', 'p3_off'), 'disp_head.hip: st_disp_head_forward, "strides and offsets ... 16-byte aligned"'),
        'df_dev': (R, 16, ('df_ld', 'df_off'), 'disp_head.hip: st_disp_head_forward'),
        'workspace_dev': (R, 16, (), 'disp_head.hip: st_disp_head_forward'),
        'pred_out_dev': (F, 4, (), 'disp_head.hip: elu_reg_relu_kernel pred2[p] = y')},
    'st_disp_head_tap': {'workspace_dev': (F, 1, (), 'disp_head.hip: pointer arithmetic only')},
    'st_disp_head_resize': {'pred_dev': (F, 4, (), 'disp_head.hip: bilinear_kernel'), 'out_dev': (F, 4, (), 'disp_head.hip: bilinear_kernel')},
    'st_disp_fuse': {'dense_dev': (F, 4, (), 'disp_head.hip: disp_fuse_kernel, eight scalar taps'),
                     'disp_dev': (D, 4, (), 'disp_head.hip: disp_fuse_kernel, per address `(dn + o) & 15`'),
                     'out_dev': (D, 4, (), 'disp_head.hip: disp_fuse_kernel, per address `(on + o) & 15`'),
                     'filled_dev': (F, 4, (), 'disp_head.hip: one integer atomic per workgroup')},
    # ---- JPEG ------------------------------------------------------------------------------------------------------
    'st_jpeg_reconstruct': {
        'coef_dev': (R, 16, (), 'jpeg_decode.hip: st_jpeg_reconstruct, "coef_dev, quant_dev and work_dev"'),
        'quant_dev': (R, 16, (), 'jpeg_decode.hip: st_jpeg_reconstruct'),
        'work_dev': (R, 16, (), 'jpeg_decode.hip: st_jpeg_reconstruct'),
        'out_dev': (D, 1, ('image_stride', 'plane_stride', 'row_stride'), 'jpeg_decode.hip: colour kernel, per address `(op & 3) == 0`')},
    'st_jpeg_entropy_decode_dev': {
        'blob_dev': (R, 16, (), 'jpeg_entropy.hip: st_jpeg_entropy_decode_dev, "blob_dev and work_dev"'),
        'work_dev': (R, 16, (), 'jpeg_entropy.hip: st_jpeg_entropy_decode_dev'),
        'coef_dev': (R, 2, (), 'jpeg_entropy.hip: "the outputs to their element size"'),
        'quant_dev': (R, 2, (), 'jpeg_entropy.hip: "the outputs to their element size"'),
        'status_dev': (R, 4, (), 'jpeg_entropy.hip: "the outputs to their element size"')},
}

# ---- out of scope: host memory and opaque handles, by name ------------------------------------------------------------
_DESC_HOST = 'the descriptor struct itself is host memory'
HOST = {
    'st_conv2d_nhwc': ('d',), 'st_conv2d_nhwc_variant': ('d',), 'st_conv3x3_wino_group': ('descs',),
    'st_conv1x1_chain': ('a', 'b'), 'st_conv3x3s2_csp_front': ('a', 'ms', 'c1'), 'st_conv3x3_csp_tail': ('conv2', 'fin'),
    'st_wino_pack_weights': ('packed_wgt_host', 'out_host'), 'st_front_pack_frags': ('packed_wgt_host', 'out_host'),
    'st_csp_tail_pack_frags': ('packed_wgt_host', 'out_host'),
    'st_conv_pack_weights': ('w', 'conv_bias', 'bn_gamma', 'bn_beta', 'bn_mean', 'bn_var', 'wgt_out', 'bias_out'),
    'st_stem_pack_weights': ('w', 'conv_bias', 'bn_gamma', 'bn_beta', 'bn_mean', 'bn_var', 'wgt_out', 'bias_out'),
    # host arrays of device frame pointers: the arrays are host memory, the frames they hold are the `name[]` rows of ROWS
    'st_stem_focus_conv_u8': ('frames_u8_dev_ptrs_host',), 'st_pack_raw_frames': ('frames_u8_dev_ptrs_host',),
    'st_rectify_remap': ('src_dev_ptrs_host', 'map_index_host', 'dst_dev_ptrs_host'),
    'st_detector_create': ('cfg', 'out'), 'st_detector_destroy': ('det',), 'st_detector_num_params': ('det',),
    'st_detector_param_info': ('det', 'name', 'shape', 'ndim'), 'st_detector_set_param': ('det', 'name', 'host'),
    'st_detector_finalize': ('det',), 'st_detector_workspace_bytes': ('det',), 'st_detector_head_floats': ('det',),
    'st_detector_num_levels': ('det',), 'st_detector_level_info': ('det', 'h', 'w', 'stride', 'float_offset'),
    'st_detector_forward': ('det',), 'st_detector_macs': ('det',), 'st_detector_forward_phase': ('det',),
    'st_detector_forward_phase0_raw': ('det', 'left_frames_host', 'right_frames_host'),
    'st_detector_forward_raw': ('det', 'img_frames_host'), 'st_detector_set_timing': ('det',),
    'st_detector_num_ops': ('det',), 'st_detector_op_times': ('det', 'ms', 'kind', 'variant', 'macs', 'phase'),
    'st_detector_op_desc': ('det', 'buf'), 'st_detector_op_owner': ('det', 'owner', 'variant'),
    'st_detector_set_split': ('det',), 'st_detector_autotune': ('det',), 'st_detector_get_tuning': ('det', 'variants'),
    'st_detector_set_tuning': ('det', 'variants'),
    'st_detector_tap': ('det', 'name', 'ptr_dev', 'N', 'C', 'H', 'W', 'ld'),
    'st_head_pred': ('levels',), 'st_decode_nms_workspace_bytes': ('d',), 'st_decode_nms': ('d',),
    'st_volume_agg3d': ('weight27_host',), 'st_costvolume_agg3d': ('weight27_host',),
    'st_costvolume_agg3d_softargmin': ('weight27_host',),
    'st_lapjv_extended': ('cost', 'x_out', 'y_out'),
    'st_tracker_create': ('cfg', 'out'), 'st_tracker_destroy': ('t',), 'st_tracker_reset': ('t',),
    'st_tracker_track': ('t', 'dets', 'out_rows', 'out_ids', 'out_n'),
    'st_tracker_track_records': ('t', 'frame_ids', 'records', 'out_rows', 'out_ids', 'out_counts'),
    'st_tracker_num_tracks': ('t',), 'st_tracker_next_id': ('t',),
    'st_tracker_get_track': ('t', 'id', 'mean8', 'cov64', 'tentative', 'tracked', 'last_frame'),
    'st_tracker_get_states': ('t', 'out', 'out_n', 'next_id'),
    'st_batched_tracker_create': ('cfg', 'out'), 'st_batched_tracker_destroy': ('t',),
    'st_batched_tracker_state_bytes': ('t',), 'st_batched_tracker_scratch_bytes': ('t',),
    'st_batched_tracker_step': ('t',), 'st_batched_tracker_run': ('t',),
    'st_batched_tracker_get_states': ('t', 'out_host', 'n_tracks', 'next_id', 'status'),
    'st_batched_tracker_create_multi': ('cfgs', 'out'),
    'st_cmc_num_levels': ('sides',), 'st_cmc_front_u8': ('frames_u8_dev_ptrs_host',),
    'st_cmc_estimate': ('params',), 'st_cmc_mesh_fit': ('params',),
    'st_tracker_cmc_needed': ('t',), 'st_tracker_track_cmc': ('t', 'dets', 'warp', 'out_rows', 'out_ids', 'out_n'),
    'st_tracker_track_records_cmc': ('t', 'frame_ids', 'records', 'warps', 'warp_src', 'cmc_prev', 'out_rows',
                                     'out_ids', 'out_counts', 'stop_at'),
    'st_sgbm_u8': ('left_ptrs_host', 'right_ptrs_host', 'params'), 'st_sgbm_f32': ('params',),
    'st_sgbm_match_f32': ('params',),
    'st_coco_workspace_bytes': ('args', 'args.gt_img_host', 'args.gt_cat_host', 'args.max_dets'),
    'st_coco_prepare': ('args', 'args.gt_img_host', 'args.gt_cat_host', 'args.max_dets'),
    'st_coco_match': ('args', 'args.gt_img_host', 'args.gt_cat_host', 'args.max_dets'),
    'st_coco_accumulate': ('args', 'args.gt_img_host', 'args.gt_cat_host', 'args.max_dets'),
    'st_stream_gather': ('tick', 'tick.stream_of_slot', 'tick.frame_ids', 'chunk_records'),
    'st_stream_unscale': ('tick', 'tick.stream_of_slot', 'tick.frame_ids'),
    'st_stream_record': ('tick', 'tick.stream_of_slot', 'tick.frame_ids', 'chunk_depth', 'chunk_gt_depth'),
    **{n: ('args',) for n in ('st_mot_workspace_bytes', 'st_mot_workspace_sim_offset', 'st_mot_similarity', 'st_mot_walk',
                              'st_mot_hota_match', 'st_mot_hota_accumulate', 'st_mot_kitti_workspace_bytes', 'st_mot_kitti_preprocess', 'st_tracklet_gsi_workspace_bytes',
                              'st_tracklet_interpolate', 'st_tracklet_gsi', 'st_aflink_gate', 'st_aflink_transform',
                              'st_mot_challenge_workspace_bytes', 'st_mot_challenge_preprocess')},
    'st_aflink_weights_create': ('packed_host', 'handle'), 'st_aflink_weights_destroy': ('handle',),
    'st_aflink_score': ('args', 'weights'), 'st_aflink_run': ('args', 'weights'),
    'st_cmc_ecc_plane_size': ('plane_h', 'plane_w'), 'st_cmc_ecc_front_u8': ('frames_u8_dev_ptrs_host',),
    'st_cmc_ecc_prepare': ('params',), 'st_cmc_ecc_step': ('params',), 'st_cmc_ecc_estimate': ('params',),
    'st_mot_file_round': ('col_modes',),
    'st_stereo_eval_workspace_bytes': ('args',), 'st_stereo_eval': ('args',),
    'st_disp_head_create': ('cfg', 'out'), 'st_disp_head_destroy': ('head',), 'st_disp_head_num_params': ('head',),
    'st_disp_head_param_info': ('head', 'name', 'shape', 'ndim'), 'st_disp_head_set_param': ('head', 'name', 'host'),
    'st_disp_head_finalize': ('head',), 'st_disp_head_workspace_bytes': ('head',), 'st_disp_head_forward': ('head',),
    'st_disp_head_tap': ('head', 'name', 'ptr_dev', 'N', 'C', 'H', 'W', 'ld'),
    'st_disp_head_set_timing': ('head',), 'st_disp_head_launch_times': ('head', 'ms'),
    'st_png_unfilter': ('filtered', 'out'),
    'st_jpeg_info': ('data', 'info'), 'st_jpeg_entropy_decode': ('data', 'coef_out', 'quant_out'),
    'st_jpeg_reconstruct_host': ('coef', 'quant', 'info', 'out'), 'st_jpeg_work_bytes': ('info',),
    'st_jpeg_reconstruct': ('info',), 'st_jpeg_entropy_prepare': ('data', 'desc'),
    'st_jpeg_entropy_work_bytes': ('info',), 'st_jpeg_entropy_decode_dev': ('blob_host', 'info', 'tuning'),
}

# ---- the rows tests/test_pointer_contract_gpu.py executes --------------------------------------------------------------
# (export, argument): what the GPU file does with it.  Every key is a `dispatch` or `required` row above; a `dispatch`
# row of the stereo, pack, lr-check, eval, stem, rectify and conv families without a case here fails the CPU test.
CASES = {
    ('st_softargmin', 'cost_dev'): 'dispatch: D = 16 (register), 20 (LDS), 112 (two-lane register) at (1, 3, 37)',
    ('st_costvolume_softargmin', 'out_cost_dev'): 'dispatch: (1, 3, 70), C = 8, D = 16, with and without out_disp_dev',
    ('st_disp_upsample_pack', 'disp_postp_dev'): 'dispatch: (Hf, Wf, s) = (6, 10, 4)',
    ('st_softargmin_right', 'vol_dev'): 'dispatch: D = 16, (H, W) = (3, 33)',
    ('st_lr_check_pack', 'disp_postp_dev'): 'dispatch: (Hl, Wl, s) = (6, 10, 4)',
    ('st_lr_check_pack', 'disp_mask_dev'): 'dispatch: (Hl, Wl, s) = (6, 10, 4)',
    ('st_stereo_eval', 'pred_dev'): 'dispatch: N = 2, H = 9, W = 16',
    ('st_stereo_eval', 'gt_dev'): 'dispatch: N = 2, H = 9, W = 16',
    ('st_stem_focus_conv', 'out_nhwc_dev'): 'dispatch: N = 1, H = 16, W = 24, Cout = 32; +4 bytes and out_off = 1',
    ('st_rectify_remap', 'dst_block_dev'): 'dispatch: u8, (h, w) = (5, 8), +1 .. +3 bytes',
    ('st_costvolume_softargmin', 'featL_dev'): 'required',
    ('st_costvolume_softargmin', 'featR_dev'): 'required',
    ('st_decode_nms', 'head_out_dev'): 'required',
    ('st_decode_nms', 'workspace_dev'): 'required',
    ('st_decode_nms', 'out_boxes_dev'): 'required',
    ('st_box_depth', 'boxes_dev'): 'required',
    ('st_box_depth', 'out_scaled_boxes_dev'): 'required',
    ('st_box_depth_method', 'boxes_dev'): 'required',
    ('st_box_depth_method', 'out_scaled_boxes_dev'): 'required',
    ('st_pack_records', 'boxes_dev'): 'required',
    ('st_pack_records', 'scaled_boxes_dev'): 'required',
    ('st_feat_upsample', 'feat_dev'): 'required',
    ('st_feat_upsample', 'out_dev'): 'required',
    ('st_volume_agg3d', 'vol_in_dev'): 'required',
    ('st_volume_agg3d', 'vol_out_dev'): 'required',
    ('st_focus_pack', 'img_nchw_dev'): 'required',
    ('st_focus_pack', 'out_nhwc_dev'): 'required',
    ('st_spp_pool', 'x_dev'): 'required',
    ('st_spp_pool', 'out_dev'): 'required',
    ('st_stem_focus_conv', 'img_nchw_dev'): 'required',
    ('st_stem_focus_conv', 'bias_dev'): 'required',
    ('st_conv2d_nhwc', 'd.in_dev'): 'required; conv cases: every tile and instance',
    ('st_conv2d_nhwc', 'd.wgt_dev'): 'required',
    ('st_conv2d_nhwc_variant', 'd.in_dev'): 'required; conv cases',
    ('st_conv2d_nhwc_variant', 'd.wgt_dev'): 'required; conv cases',
    ('st_conv1x1_chain', 'a.in_dev'): 'required; conv cases',
    ('st_conv1x1_chain', 'a.wgt_dev'): 'required; conv cases, streaming and resident pair',
    ('st_conv1x1_chain', 'b.in_dev'): 'required; conv cases',
    ('st_conv1x1_chain', 'b.wgt_dev'): 'required; conv cases, streaming and resident pair',
    ('st_pack_raw_inputs', 'img_u8_dev'): 'dispatch: (N, h, w, H, W) = (2, 5, 8, 6, 12), +1 .. +3 bytes',
    ('st_pack_raw_inputs', 'disp_u16_dev'): 'dispatch: +2, +4, +6 bytes',
    ('st_pack_raw_inputs', 'img_out_dev'): 'dispatch',
    ('st_pack_raw_inputs', 'disp_postp_out_dev'): 'dispatch',
    ('st_pack_raw_inputs', 'disp_mask_out_dev'): 'dispatch',
    ('st_stem_focus_conv_u8', 'out_dev'): 'dispatch: as st_stem_focus_conv, from one 12 x 24 raw frame',
    ('st_disp_fuse', 'disp_dev'): 'dispatch: N = 2, (H, W) = (6, 16), mode 2',
    ('st_disp_fuse', 'out_dev'): 'dispatch: N = 2, (H, W) = (6, 16), mode 2',
    ('st_jpeg_reconstruct', 'out_dev'): 'dispatch: two 24 x 40 4:2:0 images, +1 .. +3 bytes',
    **{('st_conv3x3s2_csp_front', a): 'required: an aligned launch, then this pointer at +4 bytes'
       for a in ('a.in_dev', 'a.wgt_dev', 'ms.out1_dev', 'ms.out2_dev', 'c1.out1_dev', 'frag_ms_dev', 'frag_c1_dev')},
    **{('st_conv3x3_csp_tail', a): 'required: an aligned launch, then this pointer at +4 bytes'
       for a in ('conv2.in_dev', 'conv2.res_dev', 'conv2.bias_dev', 'conv2.wgt_wino_dev', 'conv2.out1_dev', 'fin.in_dev',
                 'fin.out1_dev', 'fin.res_dev', 'fin.bias_dev', 'frag_fin_dev')},
    **{('st_conv3x3_wino_group', a): 'required: an aligned launch, then this pointer of the second layer at +4 bytes'
       for a in ('descs.in_dev', 'descs.out1_dev', 'descs.wgt_wino_dev', 'descs.bias_dev')},
    **{('st_head_pred', a): 'required: an aligned launch, then this pointer of level 1 at +4 bytes'
       for a in ('levels.cls_dev', 'levels.reg_dev', 'levels.out_dev')},
    **{('st_detector_forward', a): 'required: a forward that runs, then this pointer at +4 bytes'
       for a in ('img_dev', 'disp_dev', 'workspace_dev', 'head_out_dev')},
    **{('st_detector_forward_phase', a): 'required: both phases run, then this pointer at +4 bytes'
       for a in ('img_dev', 'disp_dev', 'right_dev', 'workspace_dev', 'head_out_dev')},
    ('st_conv1x1_chain', 'a.out1_dev'): 'dispatch; conv cases',
    ('st_conv1x1_chain', 'a.out2_dev'): 'dispatch; conv cases',
    ('st_conv1x1_chain', 'b.out1_dev'): 'dispatch; conv cases',
}
# `required` rows test_cpu_pointer_contract.py makes on host memory (no device needed: the refusal precedes every launch)
HOST_CASES = (
    ('st_cmc_estimate', 'ws'), ('st_cmc_mesh_fit', 'ws'), ('st_cmc_fit', 'ws'),
    ('st_cmc_ecc_prepare', 'ws'), ('st_cmc_ecc_step', 'ws'), ('st_cmc_ecc_estimate', 'ws'),
    ('st_pack_raw_frames', 'img_out_dev'), ('st_pack_raw_frames', 'frames_u8_dev_ptrs_host[]'),
    ('st_stem_focus_conv_u8', 'bias_dev'), ('st_stem_focus_conv_u8', 'frames_u8_dev_ptrs_host[]'),
    ('st_rectify_remap', 'maps_dev'), ('st_rectify_remap', 'src_dev_ptrs_host[]'),
    ('st_costvolume_agg3d', 'featL_dev'), ('st_costvolume_agg3d', 'featR_dev'), ('st_costvolume_agg3d', 'vol_out_dev'),
    ('st_costvolume_agg3d_softargmin', 'featL_dev'), ('st_costvolume_agg3d_softargmin', 'featR_dev'),
    ('st_stereo_eval', 'workspace_dev'),
    ('st_jpeg_reconstruct', 'coef_dev'), ('st_jpeg_reconstruct', 'quant_dev'), ('st_jpeg_reconstruct', 'work_dev'),
)

# `dispatch` / `required` rows no test executes, each with its reason; everything else must be in CASES or HOST_CASES
NOT_RUN = {
    **{(e, a): 'reaches run_ops\' first statement like st_detector_forward / _phase, which the GPU file runs; needs raw '
               'frame chunks / a timing loop around the same check'
       for e, args in (('st_detector_forward_phase0_raw', ('workspace_dev',)),
                       ('st_detector_forward_raw', ('disp_dev', 'workspace_dev', 'head_out_dev')),
                       ('st_detector_autotune', ('workspace_dev', 'head_out_dev'))) for a in args},
    **{('st_disp_head_forward', a): 'refusal predates the contract table; needs a finalized StDispHead (open)'
       for a in ('p3_dev', 'df_dev', 'workspace_dev')},
    **{(e, 'ws'): 'refusal predates the contract table (D > 64 only); needs a full StSgbmParams (open)'
       for e in ('st_sgbm_u8', 'st_sgbm_f32', 'st_sgbm_match_f32')},
    **{('st_jpeg_entropy_decode_dev', a): 'refusal predates the contract table; needs a prepared descriptor blob (open)'
       for a in ('blob_dev', 'work_dev', 'coef_dev', 'quant_dev', 'status_dev')},
    ('st_rectify_remap', 'dst_dev_ptrs_host[]'): 'the same kernel line as dst_block_dev, which the GPU file runs at +1 .. +3',
}


# ---- the headers -------------------------------------------------------------------------------------------------------
def declarations(headers=HEADERS):
    """{export: [(type text, parameter name)]} of the pointer parameters of every declaration of the headers."""
    out = {}
    for h in headers:
        with open(h) as f:
            text = f.read()
        for name, params in ss._declarations(text):
            ptrs = []
            for p in params:
                if '*' not in p and '[' not in p:       # `T name[3]` is a pointer parameter too
                    continue
                m = re.match(r'^(.*?)(\w+)\s*(\[\d*\])?$', p.strip(), flags=re.S)
                ptrs.append((re.sub(r'\s+', ' ', m.group(1)).strip() + ('*' if m.group(3) else ''), m.group(2)))
            out[name] = ptrs
    return out


def structs(headers=HEADERS):
    """{struct name: [pointer field names]} of every `typedef struct` of the headers."""
    out = {}
    for h in headers:
        with open(h) as f:
            text = re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)
        for m in re.finditer(r'typedef struct (\w+)\s*\{(.*?)\}\s*(\w+)\s*;', text, flags=re.S):
            fields = []
            for piece in m.group(2).split(';'):
                if '*' in piece:
                    fields.append(re.search(r'(\w+)\s*(\[\d*\])?\s*$', piece.strip()).group(1))
            out[m.group(3)] = fields
    return out


def pointers(headers=HEADERS):
    """Every pointer the headers publish as (export, argument): the pointer parameters, and `param.field` for the
    pointer fields of a struct a parameter points to (opaque structs have no definition and no fields)."""
    st = structs(headers)
    out = []
    for name, ptrs in declarations(headers).items():
        for typ, arg in ptrs:
            out.append((name, arg))
            base = re.sub(r'\bconst\b|\*|\s', '', typ)
            for field in st.get(base, ()):
                out.append((name, f'{arg}.{field}'))
    return out


def lookup(export, arg):
    """The row of (export, argument): ROWS, through `param.*`, or None."""
    rows = ROWS.get(export, {})
    if arg in rows:
        return rows[arg]
    if '.' in arg and arg.split('.')[0] + '.*' in rows:
        return rows[arg.split('.')[0] + '.*']
    return None


def missing_and_stale(headers=HEADERS, rows=None, host=None):
    """(pointers of the headers with neither a row nor a HOST entry, rows / HOST entries that name nothing)."""
    rows = ROWS if rows is None else rows
    host = HOST if host is None else host
    published = pointers(headers)
    missing = []
    for export, arg in published:
        in_rows = arg in rows.get(export, {}) or ('.' in arg and arg.split('.')[0] + '.*' in rows.get(export, {}))
        if not in_rows and arg not in host.get(export, ()):
            missing.append((export, arg))
    known = set(published)
    params = {(e, a.split('.')[0]) for e, a in published}
    stale = [(e, a) for e, r in rows.items() for a in r
             if ((e, a.split('.')[0]) not in params if a.endswith('.*') else
                 (e, a[:-2]) not in known if a.endswith('[]') else (e, a) not in known)]
    stale += [(e, a) for e, names in host.items() for a in names if (e, a) not in known]
    return missing, stale
