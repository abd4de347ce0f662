"""Dense stereo evaluation: how good is a disparity map.

  stereo_error_stats   one st_stereo_eval launch over (N, C, H, W) prediction / ground-truth maps on the device ->
                       StereoStats: integer counters, fp64 sums and a 1/16 px error histogram per (frame, region, depth
                       bin) cell.  The per-pixel definitions are those of include/stereotrack.h section 22
                       (tests/stereo_eval_ref.py restates them in numpy).
  StereoStats          the accumulators; cells add, so frames merge into videos and videos into a dataset
                       (pixel-weighted, like TrackEval's COMBINED_SEQ); summary() turns a cell into EPE, bad-pixel rates,
                       KITTI's D1, density, error quantiles and the depth-error measures.
  StereoMetric         METRICS entry: collects the `stereo_stats` that OCSORT_Disparity(stereo_eval=...) leaves in every
                       sample's metainfo, gathers whole videos over the ranks, summarises per video and combined.

The accumulation is the HIP kernel's; there is no host fall-back (CPU tensors raise).
"""
import ctypes as C
import math
from collections import defaultdict

import numpy as np
import torch

from . import _lib
from ._lib import StStereoEvalArgs, check, current_stream
from .metrics import GatheredVideoMetric
from .registry import METRICS

HIST_BINS = 512            # ST_STEREO_EVAL_HIST_BINS: 1/16 px each, the last one holds everything >= 31.9375 px
NUM_SUMS = 5               # sum e, e^2, |dz| / gz, dz^2 / gz, dz^2
MAX_BINS, MAX_THRESHOLDS, MAX_BOXES = 8, 6, 256
DEFAULT_DEPTH_EDGES = (0, 20, 40, 80)
DEFAULT_BAD_THRESHOLDS = (0.5, 1, 2, 3)
GT_KINDS = {'depth': 0, 'disp': 1}
REGIONS = {'all': (0, 1), 'background': (0,), 'object': (1,)}


def check_options(depth_edges=None, bad_thresholds=None):
    """-> (edges, thresholds) as tuples of floats; ValueError for what st_stereo_eval would refuse."""
    edges = tuple(float(v) for v in (DEFAULT_DEPTH_EDGES if depth_edges is None else depth_edges))
    taus = tuple(float(v) for v in (DEFAULT_BAD_THRESHOLDS if bad_thresholds is None else bad_thresholds))
    if not 1 <= len(edges) - 1 <= MAX_BINS:
        raise ValueError(f'depth_edges: {len(edges) - 1} depth ranges, 1..{MAX_BINS} are supported')
    f32 = [float(np.float32(v)) for v in edges]
    if any(math.isnan(v) for v in f32) or any(a >= b for a, b in zip(f32[:-1], f32[1:])):
        raise ValueError(f'depth_edges must ascend strictly (as float32), got {edges}')
    if not 1 <= len(taus) <= MAX_THRESHOLDS:
        raise ValueError(f'bad_thresholds: {len(taus)} thresholds, 1..{MAX_THRESHOLDS} are supported')
    if any(math.isnan(v) for v in taus):
        raise ValueError('bad_thresholds: not a number')
    return edges, taus


def packed_sizes(N, K, T):
    """int64 elements of the three accumulator blocks of one launch, in their order inside the packed buffer."""
    return N * 2 * K * (T + 6), N * 2 * K * NUM_SUMS, N * 2 * K * HIST_BINS


def unpack(buf, N, K, T):
    """A packed int64 buffer (device or host tensor) -> counts (N, 2, K, T + 6) int64, sums (N, 2, K, 5) float64,
    hist (N, 2, K, 512) int64, views of it."""
    a, b, c = packed_sizes(N, K, T)
    return (buf[:a].view(N, 2, K, T + 6), buf[a:a + b].view(torch.float64).view(N, 2, K, NUM_SUMS),
            buf[a + b:a + b + c].view(N, 2, K, HIST_BINS))


def _plane0(t, name):
    """(N, C, H, W) / (N, H, W) fp32 CUDA map -> (tensor that owns the memory, N, H, W, image pitch in floats)."""
    if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
        raise RuntimeError(f'stereo_error_stats runs on the HIP path only: {name} must be a CUDA tensor')
    if t.dim() == 3:
        t = t[:, None]
    if t.dim() != 4:
        raise ValueError(f'{name} must be (N, C, H, W) or (N, H, W), got {tuple(t.shape)}')
    if t.dtype != torch.float32:
        t = t.float()
    N, _, H, W = t.shape
    if t.stride(3) != 1 or t.stride(2) != W or (N > 1 and t.stride(0) < H * W):
        t = t.contiguous()
    return t, N, H, W, (t.stride(0) if N > 1 else H * W)


def launch_stereo_eval(pred, gt, gt_kind, bf, extent, boxes, box_counts, edges, taus, lib=None):
    """ONE st_stereo_eval call on the current stream.  pred / gt: CUDA maps; extent: int32 (N, 2) CUDA tensor; boxes
    (N, M, 4) fp32 + box_counts (N,) int32 CUDA tensors or None; edges / taus from check_options.  -> the packed int64
    device buffer (unpack()).  No host wait."""
    lib = lib or _lib.load()
    if gt_kind not in GT_KINDS:
        raise ValueError(f"gt_kind must be 'depth' or 'disp', got {gt_kind!r}")
    pred, N, H, W, ppitch = _plane0(pred, 'pred')
    gt, Ng, Hg, Wg, gpitch = _plane0(gt, 'gt')
    if (Ng, Hg, Wg) != (N, H, W):
        raise ValueError(f'pred is {(N, H, W)} (N, H, W), gt is {(Ng, Hg, Wg)}')
    K, T = len(edges) - 1, len(taus)
    M = 0 if boxes is None else int(boxes.shape[1])
    if M > MAX_BOXES:
        raise ValueError(f'{M} box rows per frame, at most {MAX_BOXES} are supported')
    a = StStereoEvalArgs()
    a.struct_size = C.sizeof(StStereoEvalArgs)
    a.N, a.H, a.W, a.gt_kind, a.num_bins, a.num_thresholds, a.max_boxes = N, H, W, GT_KINDS[gt_kind], K, T, M
    a.pred_img_pitch, a.gt_img_pitch = ppitch, gpitch
    a.bf = float(bf)
    for k, v in enumerate(edges):
        a.depth_edges[k] = v
    for k, v in enumerate(taus):
        a.bad_thresholds[k] = v
    need = lib.st_stereo_eval_workspace_bytes(C.byref(a))
    if need == 0:
        check(-1, 'st_stereo_eval_workspace_bytes')
    a.workspace_bytes = need
    dev = pred.device
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)       # arbitrary contents: the call defines them
    out = torch.empty(sum(packed_sizes(N, K, T)), dtype=torch.int64, device=dev)
    counts, sums, hist = unpack(out, N, K, T)
    vp = C.c_void_p
    check(lib.st_stereo_eval(C.byref(a), vp(pred.data_ptr()), vp(gt.data_ptr()), vp(extent.data_ptr()),
                             vp(boxes.data_ptr()) if M else None, vp(box_counts.data_ptr()) if M else None,
                             vp(counts.data_ptr()), vp(sums.data_ptr()), vp(hist.data_ptr()), vp(ws.data_ptr()),
                             current_stream()), 'st_stereo_eval')
    return out


def bf_float32(baseline, focal_length):
    """bf of the definitions: the product in double, rounded once to float32."""
    return float(np.float32(float(baseline) * float(focal_length)))


def stereo_error_stats(pred, gt, gt_kind='depth', baseline=0.25, focal_length=640, extent=None, boxes=None,
                       box_counts=None, depth_edges=DEFAULT_DEPTH_EDGES, bad_thresholds=DEFAULT_BAD_THRESHOLDS):
    """Error of the disparity maps `pred` (N, C, H, W; plane 0, pixels, <= 0 / non-finite = no estimate) against `gt`
    (N, Cg, H, W; plane 0; metres for gt_kind='depth', pixels for 'disp'), both CUDA tensors, in one launch on the
    current stream.  extent (N, 2) = (h_n, w_n): the part of every frame that is not padding (default: all of it).
    boxes (N, M, 4) xyxy + box_counts (N,): the object region.  -> StereoStats of N frames."""
    edges, taus = check_options(depth_edges, bad_thresholds)
    for name, t in (('pred', pred), ('gt', gt)):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
            raise RuntimeError(f'stereo_error_stats runs on the HIP path only: {name} must be a CUDA tensor')
    dev = pred.device
    N, H, W = pred.shape[0], pred.shape[-2], pred.shape[-1]
    if extent is None:
        extent = [(H, W)] * N
    extent = torch.as_tensor(extent, dtype=torch.int32).reshape(N, 2).to(dev).contiguous()
    if boxes is not None:
        boxes = torch.as_tensor(boxes, dtype=torch.float32).to(dev).contiguous()
        if boxes.dim() != 3 or boxes.shape[0] != N or boxes.shape[2] != 4:
            raise ValueError(f'boxes must be (N, M, 4), got {tuple(boxes.shape)}')
    if boxes is not None and boxes.shape[1] > 0:
        if box_counts is None:
            box_counts = [boxes.shape[1]] * N
        box_counts = torch.as_tensor(box_counts, dtype=torch.int32).reshape(N).to(dev).contiguous()
    else:
        boxes = box_counts = None
    out = launch_stereo_eval(pred, gt, gt_kind, bf_float32(baseline, focal_length), extent, boxes, box_counts, edges,
                             taus)
    counts, sums, hist = unpack(out.cpu(), N, len(edges) - 1, len(taus))
    return StereoStats(counts.numpy(), sums.numpy(), hist.numpy(), edges, taus)


def _div(a, b):
    return float(a) / float(b) if b else float('nan')


def summarize_cell(counts, sums, hist, bad_thresholds, invalid='skip'):
    """One (already added) cell -> dict: counts (T + 6,), sums (5,), hist (512,).  An empty cell gives NaN."""
    if invalid not in ('skip', 'bad'):
        raise ValueError(f"invalid must be 'skip' or 'bad', got {invalid!r}")
    T = len(bad_thresholds)
    n_gt, n_both = int(counts[0]), int(counts[1])

    def rate(k):
        return _div(int(k), n_both) if invalid == 'skip' else _div(int(k) + n_gt - n_both, n_gt)
    out = dict(n_gt=n_gt, n_both=n_both, EPE=_div(sums[0], n_both), RMSE=math.sqrt(_div(sums[1], n_both)),
               density=_div(n_both, n_gt))
    for t, tau in enumerate(bad_thresholds):
        out['bad_%g' % tau] = rate(counts[2 + t])
    out['D1'] = rate(counts[2 + T])
    cum = np.cumsum(np.asarray(hist, np.int64))
    for name, q in (('A50', 0.5), ('A90', 0.9), ('A99', 0.99)):
        # (b + 1) / 16 px for the smallest bin b whose cumulative count reaches ceil(q * n_both)
        out[name] = (int(np.searchsorted(cum, math.ceil(q * n_both), side='left')) + 1) / 16.0 if n_both else float('nan')
    out['abs_rel'] = _div(sums[2], n_both)
    out['sq_rel'] = _div(sums[3], n_both)
    out['depth_rmse'] = math.sqrt(_div(sums[4], n_both))
    for k in range(3):
        out['delta%d' % (k + 1)] = _div(int(counts[3 + T + k]), n_both)
    return out


class StereoStats:
    """Accumulators of F frames: counts (F, 2, K, T + 6) int64, sums (F, 2, K, 5) float64, hist (F, 2, K, 512) int64,
    indexed (frame, region: 0 background / 1 object, depth bin)."""

    def __init__(self, counts, sums, hist, depth_edges=DEFAULT_DEPTH_EDGES, bad_thresholds=DEFAULT_BAD_THRESHOLDS):
        self.depth_edges, self.bad_thresholds = check_options(depth_edges, bad_thresholds)
        K, T = len(self.depth_edges) - 1, len(self.bad_thresholds)
        self.counts = np.ascontiguousarray(counts, dtype=np.int64)
        self.sums = np.ascontiguousarray(sums, dtype=np.float64)
        self.hist = np.ascontiguousarray(hist, dtype=np.int64)
        F = self.counts.shape[0] if self.counts.ndim == 4 else -1
        if (self.counts.shape != (F, 2, K, T + 6) or self.sums.shape != (F, 2, K, NUM_SUMS) or
                self.hist.shape != (F, 2, K, HIST_BINS)):
            raise ValueError(f'accumulator shapes {self.counts.shape}, {self.sums.shape}, {self.hist.shape} do not fit '
                             f'{K} depth ranges and {T} thresholds')

    def __len__(self):
        return self.counts.shape[0]

    def _like(self, counts, sums, hist):
        return StereoStats(counts, sums, hist, self.depth_edges, self.bad_thresholds)

    def __add__(self, other):
        """The frames of both (self's first)."""
        if not isinstance(other, StereoStats):
            return NotImplemented
        if (other.depth_edges, other.bad_thresholds) != (self.depth_edges, self.bad_thresholds):
            raise ValueError('StereoStats with different depth_edges / bad_thresholds do not merge')
        return self._like(np.concatenate([self.counts, other.counts]), np.concatenate([self.sums, other.sums]),
                          np.concatenate([self.hist, other.hist]))

    def __radd__(self, other):
        return self if other == 0 else NotImplemented      # sum(list_of_stats)

    def frames(self):
        return [self._like(self.counts[i:i + 1], self.sums[i:i + 1], self.hist[i:i + 1]) for i in range(len(self))]

    def total(self):
        """One entry: the sum over the frames."""
        return self._like(self.counts.sum(0, keepdims=True), self.sums.sum(0, keepdims=True),
                          self.hist.sum(0, keepdims=True))

    def select(self, region='all', bin=None):
        """(counts (T + 6,), sums (5,), hist (512,)) added over the frames, the regions of `region` and the depth bin
        `bin` (None: all of them)."""
        if region not in REGIONS:
            raise ValueError(f'region must be one of {sorted(REGIONS)}, got {region!r}')
        K = len(self.depth_edges) - 1
        if bin is not None and not 0 <= int(bin) < K:
            raise ValueError(f'bin {bin} outside 0..{K - 1}')
        bins = slice(None) if bin is None else slice(int(bin), int(bin) + 1)
        r = list(REGIONS[region])
        return tuple(a[:, r][:, :, bins].sum((0, 1, 2)) for a in (self.counts, self.sums, self.hist))

    def summary(self, invalid='skip', region='all', bin=None):
        return summarize_cell(*self.select(region, bin), self.bad_thresholds, invalid)

    def range_names(self):
        return ['%g-%g' % (a, b) for a, b in zip(self.depth_edges[:-1], self.depth_edges[1:])]

    def report(self, invalid='skip', prefix='stereo/'):
        """The flat result dict of StereoMetric: `prefix`KEY over everything, KEY@lo-hi per depth range, obj/KEY and
        bg/KEY for the object / background region."""
        out = {}
        for k, v in self.summary(invalid).items():
            out[prefix + k] = v
        for b, name in enumerate(self.range_names()):
            for k, v in self.summary(invalid, bin=b).items():
                out[f'{prefix}{k}@{name}'] = v
        for tag, region in (('obj', 'object'), ('bg', 'background')):
            for k, v in self.summary(invalid, region=region).items():
                out[f'{prefix}{tag}/{k}'] = v
        return out


class StereoMetric(GatheredVideoMetric):
    """Collects the per-frame `stereo_stats` (metainfo of the samples OCSORT_Disparity(stereo_eval=...) returns) per
    video; evaluate() -> dict(per_video={video: report}, combined=report of the sum over all videos).  Ranks hold whole
    videos; the small accumulator arrays are gathered, rank 0 summarises, the result is broadcast."""

    def __init__(self, invalid='skip', prefix='stereo/'):
        if invalid not in ('skip', 'bad'):
            raise ValueError(f"invalid must be 'skip' or 'bad', got {invalid!r}")
        self.invalid, self.prefix = invalid, prefix
        self.pred = defaultdict(list)      # video -> [StereoStats of one frame]
        self.gt = defaultdict(list)        # unused; GatheredVideoMetric.gather merges both

    def process(self, video, data_sample, gt_instances=None):
        meta = data_sample.metainfo if hasattr(data_sample, 'metainfo') else data_sample
        st = meta.get('stereo_stats')
        if st is None:
            raise KeyError("StereoMetric.process: the sample's metainfo has no 'stereo_stats'; build the model with "
                           "stereo_eval=dict(...) and pass 'depth_postp' in the inputs")
        if not isinstance(st, StereoStats):
            raise TypeError(f'stereo_stats must be a StereoStats, got {type(st).__name__}')
        if self.pred[video] and (self.pred[video][0].depth_edges, self.pred[video][0].bad_thresholds) != \
                (st.depth_edges, st.bad_thresholds):
            raise ValueError(f'video {video!r}: stereo_stats with different depth_edges / bad_thresholds')
        self.pred[video].append(st)

    def video_stats(self):
        """video -> StereoStats (one entry per collected frame)."""
        return {v: sum(frames[1:], frames[0]) for v, frames in self.pred.items() if frames}

    def _evaluate_local(self):
        stats = self.video_stats()
        per_video = {v: stats[v].report(self.invalid, self.prefix) for v in sorted(stats)}
        combined = {}
        if stats:
            allv = [stats[v] for v in sorted(stats)]
            combined = sum(allv[1:], allv[0]).report(self.invalid, self.prefix)
        return dict(per_video=per_video, combined=combined)


METRICS.register_module(name=['StereoMetric', 'mmtrack.StereoMetric'], module=StereoMetric)
