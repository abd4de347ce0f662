"""MOT model shell + data preprocessor, registered under the reference's type strings.

  TrackDataPreprocessor_Disparity_V1   mmtrack/models/data_preprocessors/data_preprocessor_disparity_v1.py:19-84
                                       (+ data_preprocessor.py:95-158, utils/misc.py:13-64 stack_batch)
  OCSORT_Disparity                     mmtrack/models/mot/ocsort_disparity.py:16-220 (+ ocsort.py:13-114,
                                       base.py:12-145)
  OCSORT_Disp_Completion_V2            mmtrack/models/mot/ocsort_disp_completion_v2.py (the shell of the
                                       disparity-completion detector: `dense_depth_map` on every sample)

The dense work (detector, decode+NMS, per-box depth) is enqueued on the GPU through the C ABI; the
association step runs on the CPU (stereotracking_amd/trackers.py), as north_star prescribes.
Relaxation of the reference: `predict` accepts N >= 1 frames of ONE video in frame
order — the dense path runs batched, the tracker consumes the frames sequentially.
Per-box depth: OCSORT_Disparity(depth_extraction=...) picks the estimator of every depth call, 'reference' (the
reference's default extract_depth) or one of its depth-extraction comparison, 'truncated_mean', 'mean', 'median' or
'center' (DESIGN.md §11).
"""
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import check, current_stream, ptr
from . import records, shell_inputs
from .pipeline import InflightPipelines, depth_method_code, depth_source_code, launch_box_depth
from .registry import MODELS, TASK_UTILS
from .shell_inputs import RawFrames
from .structures import InstanceData, TrackDataSample
from .trackers import OCSORTTracker_Disparity  # noqa: F401  (registers the tracker)
from .motion import KalmanFilter  # noqa: F401  (registers the motion model)
from . import detectors  # noqa: F401  (registers detector / backbone / neck / head)
from . import stereo as _stereo  # noqa: F401  (registers StereoCostVolume)
from . import sgbm as _sgbm  # noqa: F401  (registers StereoSGBM)
from . import rectify as _rectify  # noqa: F401  (registers StereoRectify)
from . import coco_metric as _coco_metric  # noqa: F401  (registers CocoMetric in METRICS)
from . import kitti_metrics as _kitti_metrics  # noqa: F401  (registers MOTKittiMetrics in METRICS)
from . import tracklets as _tracklets  # noqa: F401  (registers InterpolateTracklets in TASK_UTILS)
from . import camera_motion as _camera_motion  # noqa: F401  (registers CameraMotionCompensation in TASK_UTILS)
from . import stereo_eval as _stereo_eval  # noqa: F401  (registers StereoMetric in METRICS)


def stack_batch(tensors, pad_size_divisor=0, pad_value=0):
    """Right/bottom pad (T,C,H,W) tensors to a common, divisible size and stack -> (N,T,C,H,W)
    (reference mmtrack/utils/misc.py:13-64)."""
    assert isinstance(tensors, list) and tensors and all(t.ndim == 4 for t in tensors)
    H = max(t.shape[-2] for t in tensors)
    W = max(t.shape[-1] for t in tensors)
    if pad_size_divisor > 1:
        H = (H + pad_size_divisor - 1) // pad_size_divisor * pad_size_divisor
        W = (W + pad_size_divisor - 1) // pad_size_divisor * pad_size_divisor
    out = []
    for t in tensors:
        ph, pw = H - t.shape[-2], W - t.shape[-1]
        out.append(F.pad(t, [0, pw, 0, ph], value=pad_value) if (ph or pw) else t)
    return torch.stack(out, dim=0)


@MODELS.register_module(name=['TrackDataPreprocessor_Disparity_V1'])
class TrackDataPreprocessor_Disparity_V1(nn.Module):
    """H2D copy, .float(), optional BGR<->RGB / mean-std, pad to `pad_size_divisor`, stack every key of
    `inputs` to (N,T,C,H,W).  The shipped stereo config sets only pad_size_divisor=32."""

    def __init__(self, mean=None, std=None, pad_size_divisor=1, pad_value=0, pad_mask=False, mask_pad_value=0,
                 bgr_to_rgb=False, rgb_to_bgr=False, batch_augments=None, non_blocking=False, device=None):
        super().__init__()
        assert not (bgr_to_rgb and rgb_to_bgr)
        self.channel_conversion = bgr_to_rgb or rgb_to_bgr
        self._enable_normalize = mean is not None
        if self._enable_normalize:
            self.register_buffer('mean', torch.tensor(mean, dtype=torch.float32).view(1, -1, 1, 1), False)
            self.register_buffer('std', torch.tensor(std, dtype=torch.float32).view(1, -1, 1, 1), False)
        self.pad_size_divisor, self.pad_value = pad_size_divisor, pad_value
        self.non_blocking = non_blocking
        self._device = torch.device(device) if device is not None else None

    @property
    def device(self):
        if self._device is not None:
            return self._device
        return torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')

    def forward(self, data, training=False, lazy_raw=False):
        """lazy_raw (used by OCSORT_Disparity.test_step): keys whose frames are equal-sized uint8 (1,3,h,w) CUDA
        tensors, with no normalisation / channel swap configured, come back as RawFrames (converted chunk by chunk
        inside the pipelined dense path) instead of one (N,1,3,H,W) fp32 tensor; the metainfo is set as usual."""
        inputs, samples = data['inputs'], data.get('data_samples')
        dev = self.device
        out = {}
        for key, imgs in inputs.items():
            imgs = [im.to(dev, non_blocking=self.non_blocking) for im in imgs]
            pad_shapes = [tuple(im.shape[-2:]) for im in imgs]
            plain = not (self.channel_conversion and imgs[0].size(1) == 3) and not self._enable_normalize
            if (lazy_raw and plain and imgs[0].is_cuda and len(set(pad_shapes)) == 1 and
                    all(im.dtype == torch.uint8 and tuple(im.shape[:2]) == (1, 3) for im in imgs)):
                d = self.pad_size_divisor
                h, w = pad_shapes[0]
                H, W = ((h + d - 1) // d * d, (w + d - 1) // d * d) if d > 1 else (h, w)
                out[key] = RawFrames(imgs, (H, W), self.pad_value)
                if samples is not None:
                    prefix = key[:-3]
                    for sm, ps in zip(samples, pad_shapes):
                        sm.set_metainfo({f'{prefix}batch_input_shape': (H, W), f'{prefix}pad_shape': ps})
                continue
            if plain and len({tuple(im.shape[:2]) for im in imgs}) == 1:
                # cast + pad + stack as ONE pass per frame: the (N,T,C,H,W) fp32 result is allocated once, filled with
                # the pad value, and every frame is converted straight into its slot (same values as
                # .float() -> F.pad -> torch.stack, reference utils/misc.py:13-64, without two extra full-size passes)
                d = self.pad_size_divisor
                H = max(s[0] for s in pad_shapes)
                W = max(s[1] for s in pad_shapes)
                if d > 1:
                    H, W = (H + d - 1) // d * d, (W + d - 1) // d * d
                T, Cc = imgs[0].shape[:2]
                if len(set(pad_shapes)) == 1 and len({im.dtype for im in imgs}) == 1:
                    # equal-sized frames (a video): one concatenation in the source dtype, one converting copy into
                    # the padded batch, and the pad value written to the pad strips only
                    h, w = pad_shapes[0]
                    batch = torch.empty((len(imgs), T, Cc, H, W), dtype=torch.float32, device=dev)
                    if imgs[0].dtype == torch.uint8 and imgs[0].is_cuda and T == 1 and Cc == 3:
                        # frames uploaded raw (uint8): cast + pad in ONE HIP pass (st_pack_raw_inputs)
                        raw = torch.cat(imgs, dim=0)
                        check(_lib.load().st_pack_raw_inputs(ptr(raw), None, len(imgs), h, w, H, W,
                                                             float(self.pad_value), ptr(batch), None, None,
                                                             current_stream()), 'st_pack_raw_inputs')
                    else:
                        batch[..., :h, :w].copy_(torch.stack(imgs, dim=0))
                        if h < H:
                            batch[..., h:, :] = float(self.pad_value)
                        if w < W:
                            batch[..., :h, w:] = float(self.pad_value)
                else:
                    batch = torch.full((len(imgs), T, Cc, H, W), float(self.pad_value), dtype=torch.float32, device=dev)
                    for i, im in enumerate(imgs):
                        batch[i, :, :, :im.shape[-2], :im.shape[-1]].copy_(im)
                out[key] = batch
            else:
                if self.channel_conversion and imgs[0].size(1) == 3:
                    imgs = [im[:, [2, 1, 0], ...] for im in imgs]
                imgs = [im.float() for im in imgs]
                if self._enable_normalize:
                    imgs = [(im - self.mean) / self.std for im in imgs]
                out[key] = stack_batch(imgs, self.pad_size_divisor, self.pad_value)
            if samples is not None:
                prefix = key[:-3]  # 'img' -> '', 'ref_img' -> 'ref_'
                shape = tuple(out[key].shape[-2:])
                for s, ps in zip(samples, pad_shapes):
                    s.set_metainfo({f'{prefix}batch_input_shape': shape, f'{prefix}pad_shape': ps})
        return dict(inputs=out, data_samples=samples)


def pack_raw_inputs(img_u8=None, disp_u16=None, pad_size_divisor=32, img_pad=114.0):
    """Device-side input pipeline for frames uploaded raw: uint8 (N,3,h,w) image and/or
    uint16 (N,h,w) disparity PNG codes, both CUDA tensors -> dict(img, disp_postp, disp_mask) fp32 padded to
    `pad_size_divisor`, exactly what LoadDisparityFromFile + Pad_Disparity + the preprocessor produce."""
    src = img_u8 if img_u8 is not None else disp_u16
    if src is None or not src.is_cuda:
        raise RuntimeError('pack_raw_inputs needs CUDA tensors (HIP path only)')
    N, h, w = src.shape[0], src.shape[-2], src.shape[-1]
    d = pad_size_divisor
    H, W = (h + d - 1) // d * d, (w + d - 1) // d * d
    dev = src.device
    out = {}
    if img_u8 is not None:
        assert img_u8.dtype == torch.uint8 and tuple(img_u8.shape) == (N, 3, h, w)
        img_u8 = img_u8.contiguous()
        out['img'] = torch.empty(N, 3, H, W, dtype=torch.float32, device=dev)
    if disp_u16 is not None:
        assert disp_u16.dtype in (torch.uint16, torch.int16) and tuple(disp_u16.shape) == (N, h, w)
        disp_u16 = disp_u16.contiguous()
        out['disp_postp'] = torch.empty(N, 3, H, W, dtype=torch.float32, device=dev)
        out['disp_mask'] = torch.empty(N, 1, H, W, dtype=torch.float32, device=dev)
    check(_lib.load().st_pack_raw_inputs(ptr(img_u8), ptr(disp_u16), N, h, w, H, W, float(img_pad), ptr(out.get('img')),
                                         ptr(out.get('disp_postp')), ptr(out.get('disp_mask')), current_stream()),
          'st_pack_raw_inputs')
    return out


CSV_HEADER = ['frame', 'id', 'label', 'tl_x', 'tl_y', 'br_x', 'br_y', 'depth', 'gt_depth', 'score']


def append_prediction_results(file_path, results):
    """The CSV side effect of the reference's predict (mmtrack/utils/collect_results.py:1-44: one row per track,
    `frame,id,label,tl_x,tl_y,br_x,br_y,depth,gt_depth,score`, header written when the file is empty), for EVERY
    sample of a batched call (the reference handles results[0] because it never batches)."""
    import csv
    import os
    if not file_path.endswith('.csv'):
        raise ValueError('The saving format is not supported.')
    with open(file_path, 'a') as f:
        writer = csv.writer(f)
        f.seek(0, os.SEEK_END)
        if f.tell() == 0:
            writer.writerow(CSV_HEADER)
        for sample in results:
            trk = sample.pred_track_instances
            frame_id = sample.metainfo.get('frame_id')
            boxes = trk.get('bboxes').cpu().numpy()
            ids = trk.get('instances_id').cpu().numpy()
            labels = trk.get('labels').cpu().numpy()
            scores = trk.get('scores').cpu().numpy()
            # plain floats, as the reference's d_values list yields them (a 0-d tensor would print as `tensor(10.)`)
            depth = _as_float_list(trk.get('depth'), len(ids))
            gt_depth = _as_float_list(trk.get('gt_depth'), len(ids))
            for iid, label, box, d, gd, sc in zip(ids, labels, boxes, depth, gt_depth, scores):
                writer.writerow([frame_id, iid, label, *box, d, gd, sc])


def _as_float_list(v, n):
    if v is None:
        return [float('nan')] * n
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    return [float(x) for x in np.asarray(v, dtype=np.float64).reshape(-1)]


def save_prediction_results(file_path):
    """Decorator form, as the reference applies it to OCSORT_Disparity.predict (collect_results.py:1-44): an existing
    file is deleted when the decorator is applied."""
    import os

    def decorator(predict_func):
        if os.path.exists(file_path):
            os.remove(file_path)

        def wrapper(*args, **kwargs):
            results = predict_func(*args, **kwargs)
            append_prediction_results(file_path, results)
            return results
        return wrapper
    return decorator


def scale_bbox(bboxes, scales):
    """Scale boxes about their centres (reference mmtrack/models/trackers/utils.py:58-73)."""
    cx, cy = (bboxes[:, 0] + bboxes[:, 2]) / 2, (bboxes[:, 1] + bboxes[:, 3]) / 2
    w, h = (bboxes[:, 2] - bboxes[:, 0]) * scales, (bboxes[:, 3] - bboxes[:, 1]) * scales
    return torch.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), dim=-1).reshape(-1, 4)


@MODELS.register_module(name=['OCSORT_Disparity'])
class OCSORT_Disparity(nn.Module):
    """MOT shell (reference mmtrack/models/mot/ocsort_disparity.py:16-220).  `predict` accepts N >= 1 frames of ONE
    video in frame order and drives the batched dense path (pipeline.InflightPipelines): the frames go through the
    HIP launch plan `dense_batch` at a time on `inflight` contexts / streams; per chunk there is ONE device->host
    copy of the fixed-size detection records and ONE batched st_box_depth launch for the tracks' depth column - no
    per-frame launches, no per-frame syncs.  The association step consumes the frames sequentially on the CPU while
    the GPU works on the following chunks.

    New (optional) constructor arguments next to the reference's: `stereo` (StereoCostVolume or StereoSGBM config; with
    StereoSGBM the mono detector runs on the SGBM disparity of the left / right frames), `dense_batch`,
    `inflight`, `max_det` (rows of the detection buffer: a capacity, overflow raises) and `results_device`
    ('cpu': results stay where the CPU tracker produced them - the consumers are the host-side evaluator / CSV
    writer; 'input': moved back to the device of the inputs like the reference's tensors) and `depth_extraction`
    (the per-box depth estimator of the detections, the track boxes and the gt depth alike: 'reference', or
    'truncated_mean' / 'mean' / 'median' / 'center', the alternatives the reference selects by decorating
    extract_depth, mmtrack/models/mot/depth_extraction_comparison.py), `stereo_eval` (None, or
    dict(depth_edges=..., bad_thresholds=..., boxes='gt' | None): every chunk's disparity is scored against the call's
    `depth_postp` maps in one st_stereo_eval launch beside the track-box depth, and every sample's metainfo gets
    `stereo_stats`, a one-frame stereo_eval.StereoStats) and `rectify` (a StereoRectify config for RAW,
    unrectified stereo pairs: each chunk's uint8 left / right frames are undistorted + rectified on the device in one
    launch before the stem and the stereo module read them; results are then in rectified-left coordinates, see
    StereoRectify.to_raw_boxes; baseline='calibration' / focal_length='calibration' take the rectifier's values).
    stereo_eval may also carry map='input' | 'depth': which map is scored, disp_postp (default) or the `disp_depth` of a
    `depth_source` other than 'input' (an option of the completion shell below)."""

    _has_disp_head = False      # OCSORT_Disp_Completion_V2: the pipeline runs DispHeadV2, depth_source may name its map

    def __init__(self, detector=None, tracker=None, motion=None, data_preprocessor=None, init_cfg=None,
                 baseline=0.25, focal_length=640, stereo=None, dense_batch=8, inflight=3, max_det=1000,
                 results_device='cpu', autotune=True, tuning_cache=None, results_csv=None, split_bf16=None,
                 queue_depth=1, depth_extraction='reference', rectify=None, stereo_eval=None, depth_source='input'):
        super().__init__()
        depth_method_code(depth_extraction)     # ValueError for an unknown estimator, before anything is built
        # depth_source: the map the per-box depths (detections, their scales, the tracks' `depth` column) are read from.
        # 'input' = disp_postp; 'completed' / 'fused' need the completion head (OCSORT_Disp_Completion_V2)
        if depth_source_code(depth_source) and not self._has_disp_head:
            raise ValueError(f'depth_source={depth_source!r} reads the disparity-completion head: it is an option of '
                             f'OCSORT_Disp_Completion_V2, {type(self).__name__} has no such head')
        self.depth_source = depth_source
        self.stereo_eval = self._stereo_eval_options(stereo_eval)      # None: the dense evaluator is off
        self.stereo_eval_map = stereo_eval.get('map', 'input') if self.stereo_eval is not None else 'input'
        if self.stereo_eval_map == 'depth' and depth_source == 'input':
            raise ValueError("stereo_eval: map='depth' scores disp_depth, the map of a depth_source other than 'input'")
        self.depth_extraction = depth_extraction
        self.data_preprocessor = MODELS.build(data_preprocessor) if data_preprocessor is not None else None
        self.detector = MODELS.build(detector) if detector is not None else None
        self.motion = TASK_UTILS.build(motion) if motion is not None else None
        self.tracker = MODELS.build(tracker) if tracker is not None else None
        # raw (distorted, unrectified) pairs: a StereoRectify config; each chunk's left / right frames are rectified on
        # the device in one launch (shell_inputs.chunk_inputs).  None: the inputs are rectified pairs, as ever
        if isinstance(rectify, (list, tuple)):
            raise NotImplementedError('rectify takes ONE StereoRectify calibration; a list of calibrations (one per '
                                      'stream) is not implemented')
        self.rectify = MODELS.build(rectify) if isinstance(rectify, dict) else rectify
        if self.rectify is not None:
            if not isinstance(self.rectify, _rectify.StereoRectify):
                raise TypeError('rectify must be a StereoRectify config or instance')
            if self.rectify.out_size != self.rectify.size:
                raise NotImplementedError(
                    f'rectify: out_size {self.rectify.out_size} != size {self.rectify.size} is not wired into the shell '
                    f'(ori_shape, the detector plan and the box rescale follow the raw frame size); st_rectify_remap '
                    f'itself supports it (StereoRectify.remap)')
            if getattr(self.tracker, 'with_cmc', False) or getattr(self.tracker, 'cmc_cfg', None) is not None:
                raise NotImplementedError('rectify with camera-motion compensation is not implemented: cmc estimates '
                                          'its warps on the raw left frames')
        for name, given in (('baseline', baseline), ('focal_length', focal_length)):
            if isinstance(given, str):
                if given != 'calibration' or self.rectify is None:
                    raise ValueError(f"{name}='calibration' takes the value from the `rectify` calibration; got "
                                     f"{name}={given!r} with rectify={'set' if self.rectify is not None else None}")
        if baseline == 'calibration':
            baseline = self.rectify.baseline
        if focal_length == 'calibration':
            focal_length = self.rectify.focal_length
        self.baseline, self.focal_length = baseline, focal_length
        if (stereo is not None and stereo.get('full_res') and 'feat_channels' not in stereo and self.detector is not None):
            # the full-resolution mode's reduce conv reads the detector's stage-1 features: make_divisible(128, widen)
            import math
            stereo = dict(stereo, feat_channels=int(math.ceil(128 * self.detector.widen_factor / 8) * 8))
        self.stereo = MODELS.build(stereo) if stereo is not None else None  # StereoCostVolume / StereoSGBM (new modules)
        if self.stereo is not None and self.detector is not None:
            self.detector.__dict__['stereo'] = self.stereo   # plain reference: registered once, under the shell
        self.dense_batch, self.inflight, self.max_det = int(dense_batch), int(inflight), int(max_det)
        # chunks queued per context: with 2 a context's next chunk is already in its stream when the host learns that the
        # current one finished (the device never waits for the host's refill); the per-context staging buffers and the
        # disparity ring have queue_depth + 1 slots: one being consumed by the host + queue_depth behind it
        self.queue_depth = max(1, int(queue_depth))
        self.raw_stem = True      # uint8 frames go to the stem kernels as they are (False: st_pack_raw_frames first)
        if results_device not in ('cpu', 'input'):
            raise ValueError("results_device must be 'cpu' or 'input'")
        self.results_device = results_device
        self.autotune, self.tuning_cache = bool(autotune), tuning_cache
        self.split_bf16 = split_bf16      # None: $ST_SPLIT_BF16; True: the autotuner may pick the split-operand conv instances
        # the reference decorates predict with save_prediction_results('results.csv') unconditionally
        # (ocsort_disparity.py:49); here the side effect is opt-in: results_csv='results.csv' reproduces it
        self.results_csv = results_csv
        if results_csv is not None:
            import os
            if os.path.exists(results_csv):
                os.remove(results_csv)
        self._pre_lazy = False
        if self.data_preprocessor is not None:
            import inspect
            fwd = getattr(self.data_preprocessor, 'forward', self.data_preprocessor)
            try:
                self._pre_lazy = 'lazy_raw' in inspect.signature(fwd).parameters
            except (TypeError, ValueError):
                self._pre_lazy = False
        self.lib = _lib.load()
        self._dense = {}          # (batch, ori_h, ori_w, stereo, depth_extraction) -> [InflightPipelines, weights version]
        self._staging = {}        # name -> pinned host buffer (grow-only): no pinned allocation on the per-chunk path
        self.timings = dict(frames=0, tracker_s=0.0, host_s=0.0, wait_s=0.0, pre_s=0.0, tail_s=0.0, submit_s=0.0, depth_s=0.0)   # cumulative host-side costs

    @staticmethod
    def _stereo_eval_options(cfg):
        if cfg is None:
            return None
        if not isinstance(cfg, dict):
            raise TypeError(f'stereo_eval must be None or a dict, got {type(cfg).__name__}')
        unknown = set(cfg) - {'depth_edges', 'bad_thresholds', 'boxes', 'map'}
        if unknown:
            raise ValueError(f'stereo_eval: unknown keys {sorted(unknown)} (depth_edges, bad_thresholds, boxes, map)')
        if cfg.get('boxes') not in ('gt', None):
            raise ValueError(f"stereo_eval: boxes must be 'gt' or None, got {cfg.get('boxes')!r}")
        if cfg.get('map', 'input') not in ('input', 'depth'):
            raise ValueError(f"stereo_eval: map must be 'input' or 'depth', got {cfg.get('map')!r}")
        edges, taus = _stereo_eval.check_options(cfg.get('depth_edges'), cfg.get('bad_thresholds'))
        return dict(depth_edges=edges, bad_thresholds=taus, boxes=cfg.get('boxes'))

    def _stereo_eval_launch(self, st, job, ci, s, e, B):
        """Under the side stream, beside the track-box depth launch: ONE st_stereo_eval call of the chunk's disparity
        against its depth maps; the accumulators start their way to a page-locked buffer that finalize() reads."""
        opt, samples, dev = self.stereo_eval, st['data_samples'], st['dev']
        disp = job['eval_disp']      # disp_postp, or (map='depth') the chunk's disp_depth: same slot, same guard
        H, W = int(disp.shape[-2]), int(disp.shape[-1])
        idx = list(range(s, e)) + [e - 1] * (B - (e - s))      # the padding frames repeat the last one (dropped later)
        ext = []
        for n in idx:
            shape = samples[n].metainfo.get('img_shape', (H, W))
            ext.append((min(int(shape[0]), H), min(int(shape[1]), W)))
        boxes = counts = None
        if opt['boxes'] == 'gt':
            rows = []
            for n in idx:
                gi = samples[n].get('gt_instances')
                rows.append(gi.bboxes.detach().float().cpu().reshape(-1, 4) if gi is not None and 'bboxes' in gi
                            else torch.zeros(0, 4))
            M = max(len(r) for r in rows)
            if M > 0:
                hb = torch.zeros(B, M, 4)
                for i, r in enumerate(rows):
                    hb[i, :len(r)] = r
                boxes = hb.to(dev)
                counts = torch.tensor([len(r) for r in rows], dtype=torch.int32).to(dev)
        out = _stereo_eval.launch_stereo_eval(
            disp, shell_inputs.padded(st['gt'], s, e, B), 'depth',
            _stereo_eval.bf_float32(self.baseline, self.focal_length),
            torch.tensor(ext, dtype=torch.int32).to(dev), boxes, counts, opt['depth_edges'], opt['bad_thresholds'],
            lib=self.lib)
        host = self._pinned(('stereo_stats', id(st['runner']), ci), out.shape, out.dtype)   # read at the end of the call
        host.copy_(out, non_blocking=True)
        return host

    # ---- reference plumbing (mot/base.py:68-113) -----------------------------------------------------
    def init_weights(self):
        if self.detector is not None:
            self.detector.init_weights()

    def test_step(self, data):
        t0 = time.perf_counter()
        data = shell_inputs.preprocess(self, data)
        self.timings['pre_s'] += time.perf_counter() - t0
        return self.forward(data['inputs'], data['data_samples'], mode='predict')

    def forward(self, inputs, data_samples=None, mode='predict', **kwargs):
        if mode == 'predict':
            return self.predict(inputs, data_samples, **kwargs)
        if mode == 'loss':
            raise NotImplementedError('training is out of scope of the HIP hot path (SURVEY.md §3.3)')
        raise NotImplementedError('tensor mode is not supported (reference mot/base.py:144-145)')

    # ---- the batched dense path behind the plugin surface ----------------------------------------------
    def _weights_version(self):
        return tuple(t._version for t in self.state_dict(keep_vars=True).values())

    def dense_runner(self, ori_hw, stereo, batch=None):
        """InflightPipelines context set for (batch, ori_hw, stereo), built from this model's config and
        loaded from its state_dict (reference keys `detector.*`, plus `stereo.agg.*` of the new module)."""
        det = self.detector
        cfg = det.test_cfg
        nms = cfg.get('nms', dict(type='nms', iou_threshold=0.65))
        if nms.get('type', 'nms') != 'nms':
            raise NotImplementedError(f"nms type {nms.get('type')} (only greedy 'nms')")
        if not cfg.get('yolox_style', False):
            raise NotImplementedError('the batched dense path implements the shipped yolox_style=True post-processing '
                                      '(no max_per_img cut); use detector.predict for other test_cfg')
        batch = int(batch or self.dense_batch)
        key = (batch, int(ori_hw[0]), int(ori_hw[1]), bool(stereo), self.depth_extraction)
        ent = self._dense.get(key)
        if ent is None:
            sm = self.stereo
            sgbm = sm if stereo and isinstance(sm, _sgbm.StereoSGBM) else None
            if sgbm is not None:    # SGBM disparity feeding the mono detector plan: no cost-volume attributes
                sm, stereo = None, False
            runner = InflightPipelines(
                max(1, self.inflight), batch, (key[1], key[2]), det.widen_factor, det.deepen_factor,
                det.num_classes, stereo=bool(stereo), max_disp=sm.max_disp if stereo else 192,
                feat_stride=sm.feat_stride if stereo else 4, temperature=sm.temperature if stereo else 32.0,
                score_thr=cfg.get('score_thr', 0.01), iou_thr=nms.get('iou_threshold', 0.65), max_det=self.max_det,
                baseline=self.baseline, focal_length=self.focal_length,
                pad_size_divisor=getattr(self.data_preprocessor, 'pad_size_divisor', 32) or 32,
                agg_layers=sm.agg_layers if stereo else 0, agg3d_layers=sm.agg3d_layers if stereo else 0,
                split_bf16=self.split_bf16, multi_label=getattr(det, 'multi_label', True),
                rgb_only=getattr(det, 'rgb_only', False),
                full_res=bool(getattr(sm, 'full_res', False)) if stereo else False,
                full_res_channels=(sm.reduce.out_channels if stereo and getattr(sm, 'full_res', False) else 8),
                sgbm=sgbm, depth_method=self.depth_extraction,
                lr_check=bool(getattr(sm, 'lr_check', False)) if stereo else False,
                lr_max_diff=getattr(sm, 'lr_max_diff', 1.0) if stereo else 1.0, **self._runner_extras())
            for p in runner.pipes:     # the track-box depth reads run k's disparity while later runs are in flight
                p.disp_buffers = self.queue_depth + 1
            ent = self._dense[key] = [runner, None]
        ver = self._weights_version()
        if ent[1] != ver:
            sd = {k[len('detector.'):]: v for k, v in self.state_dict().items() if k.startswith('detector.')}
            sd.update({k: v for k, v in self.state_dict().items() if k.startswith('stereo.')})
            ent[0].load_state_dict(sd, autotune=self.autotune, tuning_cache=self.tuning_cache)
            ent[1] = ver
        return ent[0]

    def _runner_extras(self):
        """Further StereoDensePipeline kwargs of a shell subclass (none here)."""
        return {}

    def _chunk_post(self, st, ci, pipe, out, s, e):
        """Under the context's stream, after chunk `ci` (frames [s, e) of call `st`) has been enqueued on `pipe`: a
        subclass's own per-chunk device work (none here)."""

    @staticmethod
    def _chunk_img_shape(st, s, e):
        """The img_shape (h, w) the frames [s, e) of call `st` share: as the reference's predict requires it; a sample
        without one is taken at its un-padded frame size."""
        metas = [st['data_samples'][n].metainfo for n in range(s, e)]
        shapes = {tuple(int(v) for v in (m.get('img_shape') or m['pad_shape'])[:2]) for m in metas}
        if len(shapes) != 1:
            raise NotImplementedError('dense_depth_map / depth_source over a chunk needs one img_shape')
        return shapes.pop()

    def _side_stream(self, dev):
        st = self._staging.get(('side_stream', dev))
        if st is None:
            st = self._staging[('side_stream', dev)] = torch.cuda.Stream(device=dev)
        return st

    def _pinned(self, name, shape, dtype=torch.float32):
        """View of a cached page-locked staging buffer.  Allocating pinned memory per chunk (hipHostMalloc) stalls the
        host until the device is idle, which serialises the in-flight contexts; these buffers are allocated once and
        grow only when a chunk needs more room."""
        n = 1
        for v in shape:
            n *= int(v)
        buf = self._staging.get(name)
        if buf is None or buf.dtype != dtype or buf.numel() < n:
            cap = max(256, 1 << max(n - 1, 1).bit_length())
            buf = self._staging[name] = torch.empty(cap, dtype=dtype, pin_memory=True)
        return buf[:n].view(*shape)

    # ---- per-box depth on the device (ocsort_disparity.py:113-175) -------------------------------------
    def bbox_postp_depth(self, pred_instances, disp, gt_depth=None):
        """disp: (1,3,H,W) disp_postp.  Returns (instances with scaled `bboxes`, `scales`, `depth`), depth dict.
        Single-frame form of the reference method (predict() uses the batched launch instead)."""
        boxes = pred_instances['bboxes'].float().contiguous()
        d_values, scales, scaled = self._box_depth(disp, boxes[None], None, self.baseline, self.focal_length)
        depth_values = dict(d_values=d_values[0])
        if gt_depth is not None:
            depth_values['gt_d_values'] = self._box_depth(gt_depth, boxes[None], None, -1.0, 1.0)[0][0]
        pred_instances['bboxes'] = scaled[0]
        pred_instances['scales'] = scales[0]
        pred_instances['depth'] = d_values[0]
        return pred_instances, depth_values

    def _box_depth(self, disp, boxes, counts, baseline, focal):
        """ONE st_box_depth launch for a whole batch: disp (N,C,H,W), boxes (N,M,4), counts (N,) int32 or None
        (= all M rows) -> depth (N,M), scales (N,M), scaled boxes (N,M,4).  The estimator is `depth_extraction`
        (st_box_depth_method for the alternatives)."""
        N, M = boxes.shape[0], boxes.shape[1]
        dev = boxes.device
        if M == 0:
            return torch.zeros(N, 0, device=dev), torch.zeros(N, 0, device=dev), torch.zeros(N, 0, 4, device=dev)
        out = (torch.empty(N, M, device=dev), torch.empty(N, M, device=dev),      # depth, scales, scaled boxes:
               torch.empty(N, M, 4, device=dev))                                   # st_box_depth defines every row
        _, Cc, H, W = disp.shape
        disp = disp.float().contiguous()
        if counts is None:
            counts = torch.full((N,), M, dtype=torch.int32, device=dev)
        boxes = boxes.float().contiguous()
        launch_box_depth(self.lib, disp, boxes, counts, baseline, focal, depth_method_code(self.depth_extraction), out,
                         Cc * H * W)
        return out

    # ---- predict (ocsort_disparity.py:50-111) ------------------------------------------------------------
    def predict(self, inputs, data_samples, **kwargs):
        """One call = begin (validate, split into dense_batch chunks) + finish (run, associate, complete the samples)."""
        return self.finish(self.begin(inputs, data_samples, **kwargs))

    def test_steps(self, data_iter):
        """The test loop over successive `test_step` inputs of one or more videos, with the contexts kept primed ACROSS
        calls: a generator that yields, per element of `data_iter`, exactly what `test_step(data)` returns (same values,
        same order - the association runs strictly in frame order), but call k+1's preprocessor and first chunks are
        submitted while call k drains, so the device never idles between calls (fill + drain cost 5 % at 64 frames per
        call).  Stands where mmengine's TestLoop calls `model.test_step(data_batch)` per batch
        (reference mot/base.py:68-113 is the per-call entry this keeps)."""
        prev = None
        for data in data_iter:
            t0 = time.perf_counter()
            data = shell_inputs.preprocess(self, data)
            self.timings['pre_s'] += time.perf_counter() - t0
            st = self.begin(data['inputs'], data['data_samples'])
            if prev is not None:
                yield self.finish(prev, lookahead=st)
            prev = st
        if prev is not None:
            yield self.finish(prev)

    def begin(self, inputs, data_samples, **kwargs):
        """Validate one call's inputs and plan its chunks; nothing is launched yet (finish() does, or the finish() of
        the call before this one when it is passed there as `lookahead`)."""
        img, second, gt, stereo, ori = shell_inputs.plan_inputs(self, inputs, data_samples, 'OCSORT_Disparity')
        N = len(img)
        B = min(self.dense_batch, N)      # a call with fewer frames than dense_batch gets a plan of its own size
        runner = self.dense_runner(ori, stereo, B)
        if self.stereo_eval is not None and gt is None:
            raise KeyError("stereo_eval is set: the inputs need 'depth_postp' (the ground-truth depth maps)")
        return dict(img=img, second=second, gt=gt, stereo=stereo, N=N, B=B, runner=runner, dev=img.device,
                    data_samples=data_samples, kwargs=kwargs, jobs={}, submitted=0,
                    chunks=[(s, min(s + B, N)) for s in range(0, N, B)])

    def _submit_next(self, st):
        """Enqueue call `st`'s next chunk on the runner's next context (round-robin)."""
        ts = time.perf_counter()
        runner, B, stereo = st['runner'], st['B'], st['stereo']
        ci = st['submitted']
        st['submitted'] += 1
        s, e = st['chunks'][ci]
        a, b = shell_inputs.chunk_inputs(self, st['img'], st['second'], stereo, s, e, B, runner)
        holder = {}
        from_head = self.depth_source != 'input'
        ext = None
        if from_head:      # where disp_filled counts: the frames' img_shape inside the padded input
            h, w = self._chunk_img_shape(st, s, e)
            ext = (min(h, runner.height), min(w, runner.width))
        # staging buffers of a context alternate: it is resubmitted before the chunk it just finished is consumed
        turns = self._staging.setdefault(('ctx_turns', id(runner)), [0] * len(runner))

        def post(out, ctx):   # under the context's stream: pack + start the ONE device->host copy of this chunk
            slot = turns[ctx] % (self.queue_depth + 1)
            turns[ctx] += 1
            rec = runner.pipes[ctx].pack_detections(out, scaled='both', n_real=e - s)
            host = self._pinned(('records', id(runner), ctx, slot), rec.shape, rec.dtype)
            host.copy_(rec, non_blocking=True)
            self._chunk_post(st, ci, runner.pipes[ctx], out, s, e)
            # the depth of the TRACK boxes is read from this chunk's disparity after the association, when the context
            # already runs its next chunk: the stereo module's output cycles through queue_depth + 1 buffers (disp_slot;
            # the read is ordered before the buffer's next rewrite by pipe.disp_guard), the mono input `b` is a
            # tensor of this chunk's own - no private copy either way.  With a depth_source other than 'input' the map
            # read there is the chunk's disp_depth, which lives in a slot of that ring in BOTH configurations
            holder.update(ctx=ctx, disp=out['disp_postp'], eval_disp=out['disp_postp'],
                          disp_slot=runner.pipes[ctx].disp_slot if stereo or from_head else None, host=host, slot=slot)
            if from_head:
                filled = self._pinned(('disp_filled', id(runner), ctx, slot), (B,), torch.int32)
                filled.copy_(out['disp_filled'], non_blocking=True)
                holder.update(disp=out['disp_depth'], filled=filled, ext=ext)
                if self.stereo_eval_map == 'depth':
                    holder['eval_disp'] = out['disp_depth']
            return out
        _, ev = runner.submit(a, right=b if stereo else None, disp_postp=None if stereo else b, post=post, ext=ext)
        cmc = self._cmc_submit(st, s, e) if getattr(self.tracker, 'with_cmc', False) else None
        self.timings['submit_s'] += time.perf_counter() - ts
        st['jobs'][ci] = dict(s=s, e=e, ev=ev, cmc=cmc, **holder)

    # ---- camera-motion compensation of the tracker (cmc=dict(method='glme_affine' | 'ecc')) -------------------------
    def _cmc_submit(self, st, s, e):
        """On a side stream, from the chunk's input already on the device: the grey planes of frames [s, e) and the
        SPECULATIVE warps of the consecutive pairs (n - 1, n) (the first frame's pair reaches back to the last frame of
        the chunk submitted before).  The warps travel to the host beside the chunk's records; the association uses
        one only when its pair is (previous CMC image, frame) - see _cmc_track_records."""
        from . import cmc
        est = self.tracker.cmc_estimator
        dev, img = st['dev'], st['img']
        metas = [st['data_samples'][n].metainfo for n in range(s, e)]
        shapes = {tuple(int(v) for v in m['img_shape'][:2]) for m in metas}
        if len(shapes) != 1:
            raise NotImplementedError('camera-motion compensation over a chunk needs one img_shape')
        hw = shapes.pop()
        fids = [int(m.get('frame_id', -1)) for m in metas]
        cs = self._staging.get(('cmc_stream', dev))
        if cs is None:
            cs = self._staging[('cmc_stream', dev)] = torch.cuda.Stream(device=dev)
        cs.wait_stream(torch.cuda.current_stream(dev))       # the chunk's input is written on the current stream
        tail = self._staging.get('cmc_tail')                  # (planes, index, frame id, img_shape) of the last chunk
        k = e - s
        with torch.cuda.stream(cs):
            planes = torch.empty(k + 1, *est.plane_shape(hw[0], hw[1]), dtype=est.plane_dtype, device=dev)
            est.front(img.frames[s:e] if isinstance(img, RawFrames) else img[s:e], hw[0], hw[1], out=planes[1:])
            if tail is not None and tail[3] == hw:
                planes[0].copy_(tail[0][tail[1]])
                src0 = tail[2]
            else:
                planes[0].copy_(planes[1])
                src0 = -2                                     # matches no frame: computed on demand if needed
            warps = est.estimate(planes[:-1], planes[1:], hw[0], hw[1])
            host = torch.empty(k, cmc.WARP_FLOATS, pin_memory=True)
            host.copy_(warps, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cs)
        self._staging['cmc_tail'] = (planes, k, fids[-1], hw)
        return dict(planes=planes, host=host, ev=ev, fids=fids, warp_src=[src0] + fids[:-1], hw=hw, stream=cs)

    def _cmc_plane(self, job, fid):
        """Grey plane (1, ph, pw) of frame `fid`: from the chunk, else the tracker's previous CMC image."""
        if fid in job['fids']:
            i = job['fids'].index(fid) + 1
            return job['planes'][i:i + 1]
        if self.tracker.prev_cmc_fid == fid and self.tracker.prev_cmc_img is not None:
            return self.tracker.prev_cmc_img
        raise RuntimeError(f'camera-motion compensation: no plane of frame {fid}')

    def _cmc_track_records(self, fids, chunk_np, job):
        """The chunk's association in native calls (st_tracker_track_records_cmc): a frame whose speculative pair is
        not (previous CMC image, frame) stops the call; that pair is estimated on demand and the call resumes there."""
        trk = self.tracker
        warps = job['host'].numpy().copy()
        src = np.asarray(job['warp_src'], np.int32)

        def on_demand(f, prev_fid):
            with torch.cuda.stream(job['stream']):     # the copy too: it must follow the estimate on the CMC stream
                w = trk.cmc_estimator.estimate(self._cmc_plane(job, prev_fid), job['planes'][f + 1:f + 2], job['hw'][0],
                                               job['hw'][1])
                return w[0].cpu().numpy()

        out = trk.track_records(fids, chunk_np, cmc=(warps, src, on_demand))
        prev = trk.prev_cmc_fid
        trk.prev_cmc_img = None if prev == -1 else self._cmc_plane(job, prev)
        return out

    def finish(self, st, lookahead=None):
        """Run call `st` to completion and return its samples.  `lookahead`: the begin() state of the NEXT call on the
        same runner - as this call's contexts free up they are refilled with that call's first chunks."""
        from .dist import DetectionOverflow
        runner, B, N, dev, gt = st['runner'], st['B'], st['N'], st['dev'], st['gt']
        data_samples, kwargs, chunks, jobs = st['data_samples'], st['kwargs'], st['chunks'], st['jobs']
        if lookahead is not None and (lookahead['runner'] is not runner or lookahead is st):
            lookahead = None
        t_host0 = time.perf_counter()

        def refill():       # one context is free: this call's next chunk, else the next call's
            if st['submitted'] < len(chunks):
                self._submit_next(st)
            elif lookahead is not None and lookahead['submitted'] < min(len(lookahead['chunks']), depth):
                self._submit_next(lookahead)

        depth = self.queue_depth * len(runner)      # chunks outstanding on the device (+ the one the host consumes)
        while st['submitted'] < min(len(chunks), depth):
            self._submit_next(st)
        outs, pending = [None] * N, []
        t_tail0 = time.perf_counter()
        def finalize(entry):   # depth of the unscaled track boxes has arrived: complete the chunk's samples
            s, e, tracks_of, dh, _ev2, _keep, sev = entry
            if sev is not None:    # the chunk's dense-evaluation accumulators: one StereoStats per REAL frame
                opt = self.stereo_eval
                cnt, sm, hs = _stereo_eval.unpack(sev, B, len(opt['depth_edges']) - 1, len(opt['bad_thresholds']))
                for i in range(e - s):
                    data_samples[s + i].set_metainfo(dict(stereo_stats=_stereo_eval.StereoStats(
                        cnt[i:i + 1].numpy().copy(), sm[i:i + 1].numpy().copy(), hs[i:i + 1].numpy().copy(),
                        opt['depth_edges'], opt['bad_thresholds'])))
            for i, tracks in enumerate(tracks_of):
                k = len(tracks)
                tracks['depth'] = dh[0, i, :k].clone()
                tracks['gt_depth'] = dh[-1, i, :k].clone()   # = depth when no gt depth map was given (:104)
                sample = data_samples[s + i]
                if self.results_device == 'input':
                    tracks = tracks.to(dev)
                    sample.pred_det_instances = sample.pred_det_instances.to(dev)
                sample.pred_track_instances = tracks
                outs[s + i] = sample

        for ci in range(len(chunks)):
            job = jobs.pop(ci)
            tw = time.perf_counter()
            job['ev'].synchronize()                       # the only wait of this chunk's forward pass
            self.timings['wait_s'] += time.perf_counter() - tw
            if ci == len(chunks) - 1:
                t_tail0 = time.perf_counter()
            refill()     # refill this context FIRST: the device keeps `inflight` chunks while the host associates this
            # one (its results live in buffers of their own)
            rec = job['host']
            s, e = job['s'], job['e']
            tracks_of = []
            t0 = time.perf_counter()
            if getattr(self.tracker, 'backend', None) == 'native' and not kwargs:
                # the whole chunk in ONE native call (st_tracker_track_records reads the page-locked record buffer the
                # D2H copy landed in: detections in, unscaled track rows out); per frame only views are taken
                fids = [int(data_samples[n].metainfo.get('frame_id', -1)) for n in range(s, e)]
                # (numpy copies: a torch CPU op above ~32 K elements wakes the whole intra-op thread pool - tens of
                # milliseconds on a 256-core host whose process owns a 16-core share - for a 400 KB memcpy)
                chunk_np = rec[:e - s].numpy().copy()  # the staging buffer is reused by a later chunk
                if job['cmc'] is not None:
                    job['cmc']['ev'].synchronize()     # the chunk's speculative warps (long done: ~0.2 ms of work)
                    trows, tids, tcnt = self._cmc_track_records(fids, chunk_np, job['cmc'])
                else:
                    trows, tids, tcnt = self.tracker.track_records(fids, chunk_np)
                det_labels = records.int_column(chunk_np[:, 1:], records.LABEL)
                det_prior = records.int_column(chunk_np[:, 1:], records.REC_PRIOR)
                trk_labels = records.int_column(trows, records.LABEL)
                counts_h = chunk_np[:, records.REC_HEADER, records.REC_COUNT].astype(np.int64).tolist()
                chunk, trows, tids = torch.from_numpy(chunk_np), torch.from_numpy(trows), torch.from_numpy(tids)
                for i, sample in enumerate(data_samples[s:e]):
                    k, m = counts_h[i], int(tcnt[i])
                    sample.pred_det_instances = records.detections(chunk[i, 1:1 + k], det_labels[i, :k], det_prior[i, :k])
                    # (:107-108); the track rows are already unscaled (:95-97)
                    tracks_of.append(records.tracks(trows[i, :m], trk_labels[i, :m], tids[i, :m], records.TRACK_ROW))
            else:
              cj = job['cmc']
              if cj is not None:
                  cj['ev'].synchronize()
              for n in range(s, e):
                r = rec[n - s]
                k, cap = int(r[records.REC_HEADER, records.REC_COUNT]), int(r[records.REC_HEADER, records.REC_CAP])
                if k > cap:
                    raise DetectionOverflow(f'frame {n}: {k} detections kept but the detection buffer has {cap} rows; '
                                            f'build the model with a larger max_det')
                rows = r[1:1 + k].clone()      # the staging buffer is reused by a later chunk
                sample = data_samples[n]
                # reference :82-86: the tracker consumes the depth-SCALED boxes + scales + depth
                labels = rows[:, records.LABEL].long()
                sample.pred_det_instances = InstanceData(bboxes=rows[:, records.REC_SCALED_BOX], scores=rows[:, records.SCORE],
                                                         labels=labels, scales=rows[:, records.REC_SCALE],
                                                         depth=rows[:, records.REC_DEPTH])
                cimg = None
                if cj is not None:
                    from .cmc import CmcFrame
                    i = n - s
                    cimg = CmcFrame(cj['planes'][i + 1:i + 2], cj['fids'][i], cj['host'][i].numpy(), cj['warp_src'][i])
                tracks = self.tracker.track(model=self, img=cimg, feats=None, data_sample=sample, **kwargs)
                tracks['bboxes'] = scale_bbox(tracks.bboxes, 1 / tracks.scales)      # unscale (:95-97)
                sample.pred_det_instances = InstanceData(bboxes=rows[:, records.BOX].clone(), scores=rows[:, records.SCORE].clone(),
                                                         labels=labels, prior_idx=rows[:, records.REC_PRIOR].long())   # (:107-108)
                tracks_of.append(tracks)
            self.timings['tracker_s'] += time.perf_counter() - t0
            # reference :99-104: depth (and gt depth) of the UNSCALED track boxes - ONE batched launch per chunk, on a
            # side stream (the chunk's forward pass has completed: `ev` above), reading the chunk's own disparity copy
            td = time.perf_counter()
            mt = max([len(t) for t in tracks_of] + [1])
            # the page-locked (ctx, slot) pair below was the SOURCE of an asynchronous host->device copy two rounds ago:
            # wait for that copy's event before the host overwrites the buffer (it has long completed in practice -
            # now it is ordered, not probable)
            slot_key = ('track_slot_event', id(runner), job['ctx'], job['slot'])
            prev_ev = self._staging.get(slot_key)
            if prev_ev is not None:
                prev_ev.synchronize()
            tb = self._pinned(('track_boxes', id(runner), job['ctx'], job['slot']), (B, mt, 4)).zero_()
            tc = self._pinned(('track_counts', id(runner), job['ctx'], job['slot']), (B,), torch.int32).zero_()
            for i, t in enumerate(tracks_of):
                tb[i, :len(t)] = t.bboxes
                tc[i] = len(t)
            stream = self._side_stream(dev)
            if 'filled' in job:      # depth_source: the chunk's head-filled pixel counts arrived with its records
                eh, ew = job['ext']
                for i, k in enumerate(job['filled'][:e - s].tolist()):
                    data_samples[s + i].set_metainfo(dict(disp_filled=int(k), disp_fill_ratio=k / float(eh * ew)))
            with torch.cuda.stream(stream):
                job['disp'].record_stream(stream)
                if job['eval_disp'] is not job['disp']:
                    job['eval_disp'].record_stream(stream)
                tbd, tcd = tb.to(dev, non_blocking=True), tc.to(dev, non_blocking=True)
                d = self._box_depth(job['disp'], tbd, tcd, self.baseline, self.focal_length)[0]
                cols = [d]
                if gt is not None:
                    cols.append(self._box_depth(shell_inputs.padded(gt, s, e, B), tbd, tcd, -1.0, 1.0)[0])
                dh = self._pinned(('track_depth', id(runner), ci), (len(cols), B, mt))   # read at the end of the call
                dh.copy_(torch.stack(cols), non_blocking=True)
                sev = self._stereo_eval_launch(st, job, ci, s, e, B) if self.stereo_eval is not None else None
                ev2 = torch.cuda.Event()
                ev2.record(stream)
                self._staging[slot_key] = ev2      # recorded after the copies that read tb / tc
                if job['disp_slot'] is not None:   # ... and after the last read of this disparity buffer
                    runner.pipes[job['ctx']].disp_guard[job['disp_slot']] = ev2
            pending.append((s, e, tracks_of, dh, ev2, (tbd, tcd), sev))
            self.timings['depth_s'] += time.perf_counter() - td
            while pending and pending[0][4].query():       # earlier chunks whose track depth has landed: complete
                finalize(pending.pop(0))                   # them now, while the device works on the next chunks
        for entry in pending:
            tw = time.perf_counter()
            entry[4].synchronize()
            self.timings['wait_s'] += time.perf_counter() - tw
            finalize(entry)
        self.timings['tail_s'] += time.perf_counter() - t_tail0
        self.timings['frames'] += N
        self.timings['host_s'] += time.perf_counter() - t_host0
        if self.results_csv is not None:
            append_prediction_results(self.results_csv, outs)
        return outs


@MODELS.register_module(name=['OCSORT_Disp_Completion_V2'])
class OCSORT_Disp_Completion_V2(OCSORT_Disparity):
    """The MOT shell of the disparity-completion family (reference mmtrack/models/mot/ocsort_disp_completion_v2.py): the
    detector is YOLOX_DISP_Completion_V2, and every returned sample also carries `dense_depth_map`, a (1, 1, h, w) fp32
    device tensor (h, w = img_shape): the head's completed disparity, resized as the reference's predict(rescale=True)
    does.  Same chunking, in-flight contexts and tracker as OCSORT_Disparity; the head runs on each context's stream
    right after the detector forward.  `disp_mask` may be among the inputs; as in the reference's predict path nothing
    reads it.  One deliberate difference: the reference's V2 shell hands the tracker boxes without depth, but the
    registered tracker (OCSORTTracker_Disparity) associates on depth, so this shell keeps OCSORT_Disparity's per-box
    depth from `disp_postp`.

    depth_source='input' | 'completed' | 'fused' (default 'input': everything as above).  Otherwise the per-box depths -
    the detections' depths and scales the tracker associates on, and the tracks' `depth` column - are read from
    `disp_depth`, the head's prediction at the padded input size ('fused': disp_postp wherever it is > 0, the head in its
    holes; one st_disp_fuse launch per chunk), and every sample's metainfo gets `disp_filled`, the pixels of its
    img_shape extent that came from the head, and `disp_fill_ratio` = disp_filled / (h * w).  `gt_depth` and
    `dense_depth_map` are unaffected.  stereo_eval=dict(..., map='depth') scores `disp_depth` instead of disp_postp."""

    _has_disp_head = True

    def __init__(self, detector=None, **kwargs):
        super().__init__(detector=detector, **kwargs)
        if not isinstance(self.detector, detectors.YOLOX_DISP_Completion_V2):
            raise TypeError('OCSORT_Disp_Completion_V2 needs a YOLOX_DISP_Completion_V2 detector')

    def _runner_extras(self):     # the checkpoint's `detector.disp_head.*` are the pipeline's `disp_head.*`
        extras = dict(disp_head=self.detector.head_config())
        if self.depth_source != 'input':
            extras['depth_source'] = self.depth_source
        return extras

    def _chunk_post(self, st, ci, pipe, out, s, e):
        # a tensor of the chunk's own: the context's buffers are overwritten by its next chunk
        st.setdefault('dense', {})[ci] = pipe.disp_head.resize(out['dense_disp'], self._chunk_img_shape(st, s, e))

    def finish(self, st, lookahead=None):
        outs = super().finish(st, lookahead)       # has waited for every chunk's event
        for ci, (s, e) in enumerate(st['chunks']):
            maps = st['dense'].pop(ci)
            maps.record_stream(torch.cuda.current_stream(maps.device))   # allocated on the context's stream, read on the caller's
            for i in range(e - s):
                outs[s + i].dense_depth_map = maps[i:i + 1]
        return outs


from . import multistream as _multistream  # noqa: E402,F401  (registers MultiStreamTracker; it wraps the shell above)
