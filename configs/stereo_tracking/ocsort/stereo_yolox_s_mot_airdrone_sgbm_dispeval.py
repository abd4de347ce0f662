# stereo_yolox_s_mot_airdrone_sgbm.py with the dense stereo evaluator on: every chunk's SGBM disparity is scored against
# the dataset's depth maps (`depth_postp`, LoadDepthFromFile) in one st_stereo_eval launch on the device, with the
# frames' ground-truth boxes as the object region; every sample's metainfo then carries `stereo_stats` and StereoMetric
# (METRICS.build(cfg.test_evaluator[2])) turns them into stereo/EPE, stereo/bad_3, stereo/D1, stereo/density, ... per
# video and combined, per depth range (stereo/EPE@20-40) and for the object region (stereo/obj/EPE).
_base_ = ['./stereo_yolox_s_mot_airdrone_sgbm.py']

data_root = 'data/AirSim_drone/'
DEPTH_RANGE = 80

model = dict(
    stereo_eval=dict(
        depth_edges=(0, 20, 40, DEPTH_RANGE),
        bad_thresholds=(0.5, 1, 2, 3),
        boxes='gt'))

val_evaluator = [
    dict(type='mmdet.CocoMetric',
         ann_file=data_root + f'annotations/val_cocoformat_{DEPTH_RANGE}.json',
         metric='bbox',
         format_only=False),
    dict(type='mmtrack.MOTDroneMetrics',
         metric=['HOTA', 'CLEAR', 'Identity'],
         depth_thr=DEPTH_RANGE,
         ignore_depth=False),
    dict(type='mmtrack.StereoMetric', invalid='skip'),
]
test_evaluator = val_evaluator
