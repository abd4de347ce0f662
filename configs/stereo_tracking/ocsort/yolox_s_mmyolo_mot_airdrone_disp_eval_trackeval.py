# yolox_s_mmyolo_mot_airdrone_disp_eval.py plus the MOTDroneMetrics block that the reference's config of that name
# carries commented out (yolox_s_mmyolo_mot_airdrone_disp.py:222-230), scoring what the reference's TrackEval run scores:
# protocol='trackeval' = the values of the written MOTChallenge files ('%d' ground truth, '%.3f' predictions) after
# MotChallenge2DBox's preprocessing for `benchmark` (the reference's default, MOT17).  METRICS.build(cfg.test_evaluator[1])
# gives stereotracking_amd.metrics.MOTDroneMetrics.
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
         benchmark='MOT17',
         protocol='trackeval'),
]
test_evaluator = val_evaluator
