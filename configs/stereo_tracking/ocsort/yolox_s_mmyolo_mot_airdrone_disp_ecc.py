# The _disp config with ECC camera-motion compensation in the tracker: the 2 x 3 background warp between consecutive
# frames is estimated on the device (cv2.findTransformECC restated, csrc/cmc_ecc.hip) and applied to the confirmed
# tracks' Kalman states right after the predict.  Options: cmc=dict(method='ecc', ecc=dict(warp_mode='MOTION_EUCLIDEAN',
# num_iters=50, stop_eps=1e-3, gauss_filt_size=1, downscale=2)) (DESIGN.md "ECC camera-motion compensation").
_base_ = ['./yolox_s_mmyolo_mot_airdrone_disp.py']

model = dict(tracker=dict(cmc=dict(method='ecc')))
