# Same tracker + detector as the _disp config, but the disparity is COMPUTED on the GPU from the left/right pair by
# the StereoSGBM module: OpenCV's StereoSGBM (mode SGBM_3WAY) restated in HIP with the fixed configuration that made the
# AirDrone disparity PNGs the detector was trained on (reference reproducibility.md section 3).  The right image
# replaces disp_postp in the inputs; the detector is the unchanged two-branch (image + disparity) model.
_base_ = ['./yolox_s_mmyolo_mot_airdrone_disp.py']

model = dict(
    stereo=dict(
        type='StereoSGBM',
        min_disparity=0,
        num_disparities=48,
        block_size=3,
        P1=96,
        P2=384,
        disp12_max_diff=0,
        uniqueness_ratio=10,
        speckle_window_size=400,
        speckle_range=10,
        pre_filter_cap=63,
        mode='SGBM_3WAY'))
