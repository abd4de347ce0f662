# The _sgbm config with 192 disparity levels (3 levels per lane of a wave in csrc/sgbm.hip) for rigs whose near objects
# pass 64 px of disparity: KITTI Tracking at 1600 x 576 (reference reproducibility.md section 1, "Depth source: Stereo
# images"; 0.54 m baseline, about 930 px of focal length) sees nothing nearer than about 7.8 m at 64 levels and about
# 2.6 m at 192 - the range the StereoCostVolume front end (max_disp 192) is sized for.  Everything else is inherited.
_base_ = ['./stereo_yolox_s_mot_airdrone_sgbm.py']

model = dict(stereo=dict(num_disparities=192))
