# Runtime defaults for the inference entry points of this repo (no training hooks: out of scope).
default_scope = 'mmtrack'
env_cfg = dict(dist_cfg=dict(backend='nccl'))  # 'nccl' is RCCL on ROCm
log_level = 'INFO'
load_from = None

# the reference's visualisation entries (its configs/_base_/default_runtime.py:3-22): the hook is built but draws
# nothing until a config turns it on (yolox_s_mmyolo_mot_airdrone_disp_vis.py); vis_backends is accepted and ignored
default_hooks = dict(visualization=dict(type='TrackVisualizationHook', draw=False))
vis_backends = [dict(type='LocalVisBackend')]
visualizer = dict(type='TrackLocalVisualizer', vis_backends=vis_backends, name='visualizer')
