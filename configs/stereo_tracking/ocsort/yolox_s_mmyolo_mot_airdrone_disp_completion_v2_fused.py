# The disparity-completion config (yolox_s_mmyolo_mot_airdrone_disp_completion_v2.py) with the head's output in use: the
# per-box depths - the detections' depths and scales the tracker associates on, and the tracks' `depth` column - are read
# from `disp_depth`, the input disparity with its invalid pixels (<= 0) filled from DispHeadV2's prediction, instead of
# from `disp_postp` with its holes.  Every sample's metainfo also gets `disp_filled` and
# `disp_fill_ratio`.  No trained completion weights exist: the accuracy of the filled depths is unmeasured.
_base_ = ['./yolox_s_mmyolo_mot_airdrone_disp_completion_v2.py']

model = dict(depth_source='fused')
