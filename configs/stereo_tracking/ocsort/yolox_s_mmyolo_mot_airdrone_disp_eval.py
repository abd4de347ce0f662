# yolox_s_mmyolo_mot_airdrone_disp.py plus the evaluator section: the one evaluator the reference's config of that
# name switches on is COCO bbox mAP / AR of the detector's boxes against the validation split's COCO-format
# annotations (same type string and keyword names as there; MOTDroneMetrics is commented out in that file).
# METRICS.build(cfg.test_evaluator[0]) gives stereotracking_amd.coco_metric.CocoMetric (device evaluation).
_base_ = ['./yolox_s_mmyolo_mot_airdrone_disp.py']

data_root = 'data/AirSim_drone/'
DEPTH_RANGE = 80

val_evaluator = [
    dict(type='mmdet.CocoMetric',
         ann_file=data_root + f'annotations/val_cocoformat_{DEPTH_RANGE}.json',
         metric='bbox',
         format_only=False),
]
test_evaluator = val_evaluator
