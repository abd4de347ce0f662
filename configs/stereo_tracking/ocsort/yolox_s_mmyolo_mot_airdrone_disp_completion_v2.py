# Two-branch (RGB + disparity) YOLOX-s with the disparity-completion head + depth-guided OC-SORT on AirDrone, inference.
# The shipped disparity config (yolox_s_mmyolo_mot_airdrone_disp.py) with the model family of the reference's
# mmtrack/models/multi_task/yolox_disp_completion_v2.py, dense_head/disp_head_v2.py and mot/ocsort_disp_completion_v2.py:
# the backbone also returns the disparity branch's stage-1 features (out_fd=True), DispHeadV2 turns them and the stride-8
# neck level into a dense disparity map, and every returned sample carries it as `dense_depth_map`.
# The reference publishes no config and no weights for this family: the model dict below follows the constructors'
# signatures, and the head's accuracy on trained weights is unmeasured.
_base_ = ['../../_base_/default_runtime.py', '../../_base_/yolox_s_8x8_mmyolo.py']

data_root = 'data/AirSim_drone/'
DEPTH_RANGE = 80
img_scale = (720, 1280)
num_classes = 1
classes = ['drone']

model = dict(
    type='OCSORT_Disp_Completion_V2',
    data_preprocessor=dict(type='TrackDataPreprocessor_Disparity_V1', pad_size_divisor=32, batch_augments=[]),
    detector=dict(
        type='mmtrack.YOLOX_DISP_Completion_V2',
        backbone=dict(type='mmtrack.YOLOXCSPDarknet_Disparity_V1_MMYOLO', input_channels=3, out_fd=True),
        bbox_head=dict(head_module=dict(num_classes=num_classes)),
        disparity_head=dict(type='DispHeadV2', in_channels=128, channels=256, in_index=0),
        test_cfg=dict(score_thr=0.01, nms=dict(type='nms', iou_threshold=0.5))),
    motion=dict(type='KalmanFilter'),
    tracker=dict(
        type='OCSORTTracker_Disparity',
        obj_score_thr=0.3,
        init_track_thr=0.7,
        weight_iou_with_det_scores=False,
        match_iou_thr=0.1,
        num_tentatives=3,
        vel_consist_weight=0.2,
        vel_delta_t=3,
        num_frames_retain=30))

# test-time input contract: as yolox_s_mmyolo_mot_airdrone_disp.py (img, disp_postp, disp_mask); `disp_mask` is accepted
# and, as in the reference's predict path, not read.
