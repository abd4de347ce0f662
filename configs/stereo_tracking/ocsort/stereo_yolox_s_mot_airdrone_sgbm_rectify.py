# The SGBM stereo-input config for a PHYSICAL rig: the left / right frames arrive raw (lens distortion, cameras slightly
# rotated against each other) and are undistorted + rectified on the device (StereoRectify, one launch per chunk) before
# the stem and StereoSGBM read them.  Results are in rectified-left pixel coordinates (StereoRectify.to_raw_boxes maps
# boxes back).  The calibration below is an EXAMPLE of a 1280 x 720 rig with a 0.25 m baseline: K / D from the
# cameras' intrinsic calibration, R / P the rectifying rotation and new projection of each camera
# (cv2.stereoRectify's R1, P1 / R2, P2, or stereotracking_amd.rectify.stereo_rectify from the extrinsics - this one:
# om = (0.004, -0.011, 0.006), T = (-0.25, 0.0012, -0.0021), new_focal = 640).  Replace it with the rig's own, or
# point `calibration='rig.json'` at a file with the same keys.
_base_ = ['./stereo_yolox_s_mot_airdrone_sgbm.py']

model = dict(
    baseline='calibration',          # -P_right[0, 3] / P_right[0, 0]
    focal_length='calibration',      # P_left[0, 0]
    rectify=dict(
        type='StereoRectify',
        size=(720, 1280),
        border=0,
        left=dict(
            K=[[642.1, 0.0, 637.2], [0.0, 641.7, 361.8], [0.0, 0.0, 1.0]],
            D=[-0.052, 0.021, 0.0006, -0.0004, -0.004],
            R=[[0.9999385097, -0.0107878752, -0.0025687803],
               [0.0107826492, 0.9999397853, -0.0020396455],
               [0.0025906291, 0.0020118218, 0.9999946206]],
            P=[[640.0, 0.0, 639.5, 0.0], [0.0, 640.0, 359.5, 0.0], [0.0, 0.0, 1.0, 0.0]]),
        right=dict(
            K=[[641.3, 0.0, 641.9], [0.0, 641.0, 357.4], [0.0, 0.0, 1.0]],
            D=[-0.049, 0.018, -0.0003, 0.0007, -0.003],
            R=[[0.9999532033, -0.0047997754, 0.0083996069],
               [0.0047827497, 0.9999864698, 0.0020458756],
               [-0.008409313, -0.0020056066, 0.9999626298]],
            P=[[640.0, 0.0, 639.5, -160.0074878248], [0.0, 640.0, 359.5, 0.0], [0.0, 0.0, 1.0, 0.0]])))
