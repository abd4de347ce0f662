# The StereoCostVolume configuration with the module's LEFT-RIGHT CHECK switched on (stereotracking_amd/stereo.py,
# DESIGN.md "Left-right check of the stereo module"): half-occluded pixels, pixels whose match lies left of the right
# image's border and pixels whose left and right disparities disagree become 0 = invalid in disp_postp, so they drop
# out of the per-box depth statistics (extract_depth keeps 0 < depth < 150) as they do with the SGBM configurations.
_base_ = ['./stereo_yolox_s_mot_airdrone_costvolume.py']

model = dict(
    stereo=dict(
        lr_check=True,
        lr_max_diff=4.0))    # image pixels: one level of the 1/4-resolution volume
