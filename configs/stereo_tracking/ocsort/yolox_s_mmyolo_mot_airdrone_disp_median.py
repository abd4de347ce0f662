# The _disp config with the per-box depth taken as the median of the box's valid depths (scale max(min(d^2/400, 3), 1)):
# the `median` row of the reference's depth-extraction comparison (mmtrack/models/mot/depth_extraction_comparison.py),
# which the reference selects by decorating extract_depth.  depth_extraction applies to the detections, the track boxes
# and the gt depth alike.  The choices are 'reference' (the default extract_depth), 'truncated_mean', 'mean', 'median'
# and 'center' (DESIGN.md section 11).
_base_ = ['./yolox_s_mmyolo_mot_airdrone_disp.py']

model = dict(depth_extraction='median')
