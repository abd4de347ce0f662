# yolox_s_mmyolo_mot_airdrone_disp.py with the visualisation hook turned on: every test iteration's frames are painted
# with their tracks (score > score_thr) on the device and written as JPEG to <work_dir>/<timestamp>/vis (test_out_dir as
# given when the loop has no runner).  The model, test_step and test_steps are the parent config's, untouched: the hook
# sits outside the model, where the reference's sits (mmtrack/engine/hooks/visualization_hook.py:107-147).
_base_ = ['./yolox_s_mmyolo_mot_airdrone_disp.py']

default_hooks = dict(visualization=dict(draw=True, interval=1, score_thr=0.3, test_out_dir='vis'))
visualizer = dict(line_width=3, alpha=0.8, quality=90, subsampling='420')
