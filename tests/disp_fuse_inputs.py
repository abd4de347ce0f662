"""The scenario of the depth_source tests (a helper module, not a test file): seeded frames with ground-truth boxes, zero
rectangles punched into the disparity over those boxes, a ground-truth depth map, and conditioned head weights.

  frame size     64 x 96 (a multiple of 32: padded size = img_shape), the tiny model of tests/test_disp_head_gpu.py
  gt boxes       GT_PER_FRAME seeded boxes of 10..22 px per frame, inside the frame
  holes          disp_postp = 0 (all three planes) on the central half of every even gt box and on all of every odd one.
                 Centre on a hole, valid rim: `center` returns 0.25 * 640 / 1e-6 = 1.6e8 m; a box that is all hole has no
                 valid pixel and every estimator returns -1
  head weights   tests/disp_head_ref.random_state_dict with the regression conv scaled by 0.05 and its bias at 8: the
                 prediction is 8 px +- a little everywhere (about 20 m), so a filled depth is finite and far below 150 m

tests/test_cpu_disp_fuse.py asserts from numpy alone that the holes do cover the boxes and that 10 % .. 90 % of the
extent is invalid - a scenario that cannot tell 'fused' from 'input' fails there, without a GPU."""
import os

import numpy as np
import torch

import disp_head_ref as ref
from stereotracking_amd.synthetic import synthetic_batch, synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_V2 = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone_disp_completion_v2.py')
CFG_FUSED = CFG_V2.replace('_v2.py', '_v2_fused.py')
ORI = (64, 96)
MAX_DISP = 32
GT_PER_FRAME = 4
HEAD_CHANNELS = 32
SEEDS_SHELL = (70, 71, 72)                  # the ragged 3-frame call (dense_batch 2)
SEEDS_LONG = tuple(range(100, 120))         # 20 frames at dense_batch 8: chunks of 8 + 8 + 4
# three streams of ragged length; a frame shown again keeps its tracks matched
SEEDS_STREAMS = ((200, 200, 201, 200), (210, 210), (220, 220, 221))


_WEIGHTS = {}


def gt_boxes(seed):
    """(GT_PER_FRAME, 4) float32 xyxy boxes of one frame, integer corners, inside ORI."""
    rng = np.random.RandomState(9000 + int(seed))
    wh = rng.randint(10, 23, size=(GT_PER_FRAME, 2))
    x1 = rng.randint(2, ORI[1] - 2 - wh[:, 0])
    y1 = rng.randint(2, ORI[0] - 2 - wh[:, 1])
    return np.stack([x1, y1, x1 + wh[:, 0], y1 + wh[:, 1]], axis=1).astype(np.float32)


def punch(disp, boxes):
    """A copy of disp (3, H, W) with zero rectangles over the box centres: the central half of every even box (the
    centre pixel is a hole, the rim keeps its disparity), all of every odd box."""
    out = disp.copy()
    for k, (x1, y1, x2, y2) in enumerate(boxes.astype(int)):
        if k % 2 == 0:
            qx, qy = (x2 - x1) // 4, (y2 - y1) // 4
            x1, y1, x2, y2 = x1 + qx, y1 + qy, x2 - qx, y2 - qy
        out[:, y1:y2, x1:x2] = 0.0
    return out


def box_classes(disp_plane, boxes):
    """Per box: (its centre pixel is invalid, it holds at least one valid pixel) as two bool arrays."""
    b = boxes.astype(int)
    cx, cy = (b[:, 0] + b[:, 2]) // 2, (b[:, 1] + b[:, 3]) // 2
    centre_invalid = ~(disp_plane[cy, cx] > 0)
    any_valid = np.array([bool((disp_plane[y1:y2, x1:x2] > 0).any()) for x1, y1, x2, y2 in b])
    return centre_invalid, any_valid


def frames(seeds, holes=True, all_valid=False):
    """-> dict(img uint8 (N,3,H,W), disp (N,3,H,W) fp32, depth (N,1,H,W) fp32 metres, boxes [(K,4)]), numpy.  holes: the
    gt boxes punched out; all_valid: every disparity >= 1 px instead (the synthetic map has its own invalid band)."""
    b = synthetic_batch(list(seeds), ORI[0], ORI[1], MAX_DISP)
    disp = b['disp_postp'].numpy().copy()
    truth = np.maximum(disp[:, :1], 1.0)                       # the scene's disparity without invalid pixels
    boxes = [gt_boxes(s) for s in seeds]
    if all_valid:
        disp = np.repeat(truth, 3, axis=1)
    elif holes:
        disp = np.stack([punch(d, bx) for d, bx in zip(disp, boxes)])
    return dict(img=b['img'].numpy().astype(np.uint8), disp=np.ascontiguousarray(disp, dtype=np.float32),
                depth=(0.25 * 640 / truth).astype(np.float32), boxes=boxes)


def invalid_fraction(disp_plane):
    """Share of the (H, W) extent the loader's rule calls invalid: not > 0."""
    return float((~(disp_plane > 0)).mean())


def head_weights():
    sd = ref.random_state_dict(128, HEAD_CHANNELS, seed=31)
    sd['reg.conv.weight'] = sd['reg.conv.weight'] * 0.05
    sd['reg.conv.bias'] = torch.tensor([8.0])
    return sd


def build(cfg_path=CFG_V2, **options):
    """The tiny V2 shell of tests/test_disp_head_gpu.py's shell test (heuristic launch plan, seeded weights, thresholds
    that let random weights start tracks) with `options` on top of the config's model dict."""
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    cfg = Config.fromfile(cfg_path)
    cfg.model.tracker['init_track_thr'] = 0.03
    cfg.model.tracker['obj_score_thr'] = 0.02
    cfg.model.detector.disparity_head['channels'] = HEAD_CHANNELS
    model = MODELS.build(dict(cfg.model, **dict(dict(autotune=False, dense_batch=2), **options)))
    if 'sd' not in _WEIGHTS:      # computed once and shared: read-only
        sd = synthetic_state_dict(list(model.detector._table), seed=5, prior_prob=0.2, logit_std=2.5)
        sd.update({'disp_head.' + k: v for k, v in head_weights().items()})
        _WEIGHTS['sd'] = sd
    sd = _WEIGHTS['sd']
    missing = model.detector.load_state_dict(sd, strict=False)
    assert not [k for k in missing.missing_keys if not k.endswith('num_batches_tracked')]
    return model


def data(fr, device, first_frame_id=0, with_depth=False, stream=None):
    """test_step input of the frames `fr` (frames()): lists of per-frame device tensors + samples with gt boxes."""
    from stereotracking_amd.structures import InstanceData, TrackDataSample
    n = len(fr['img'])
    inputs = dict(img=[torch.from_numpy(fr['img'][t:t + 1]).to(device) for t in range(n)],
                  disp_postp=[torch.from_numpy(fr['disp'][t:t + 1]).to(device) for t in range(n)])
    if with_depth:
        inputs['depth_postp'] = [torch.from_numpy(fr['depth'][t:t + 1]).to(device) for t in range(n)]
    samples = []
    for t in range(n):
        meta = dict(frame_id=first_frame_id + t, ori_shape=ORI, img_shape=ORI, scale_factor=(1.0, 1.0))
        if stream is not None:
            meta['stream'] = stream
        s = TrackDataSample(meta)
        s.gt_instances = InstanceData(bboxes=torch.from_numpy(fr['boxes'][t]))
        samples.append(s)
    return dict(inputs=inputs, data_samples=samples)
