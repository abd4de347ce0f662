# yolox_s_mmyolo_mot_airdrone_disp_eval.py plus the MOTDroneMetrics block that the reference's config of that name
# carries commented out (yolox_s_mmyolo_mot_airdrone_disp.py:222-230), with its postprocess_tracklet_cfg line switched on
# and the Gaussian-smoothed interpolation enabled.  METRICS.build(cfg.test_evaluator[1]) gives
# stereotracking_amd.metrics.MOTDroneMetrics; its InterpolateTracklets entry inherits the metric's backend.
_base_ = ['./yolox_s_mmyolo_mot_airdrone_disp_eval.py']

data_root = 'data/AirSim_drone/'
DEPTH_RANGE = 80

val_evaluator = [
    dict(type='mmdet.CocoMetric',
         ann_file=data_root + f'annotations/val_cocoformat_{DEPTH_RANGE}.json',
         metric='bbox',
         format_only=False),
    dict(type='mmtrack.MOTDroneMetrics',
         metric=['HOTA', 'CLEAR', 'Identity'],
         depth_thr=DEPTH_RANGE,
         ignore_depth=False,
         postprocess_tracklet_cfg=[
             dict(type='InterpolateTracklets', min_num_frames=5, max_num_frames=20, use_gsi=True)
         ]),
]
test_evaluator = val_evaluator
