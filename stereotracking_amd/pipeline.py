"""The per-frame dense compute path as one device-resident pipeline.

   left/right (or left + disparity) --> [stem+stage1 features L,R] --> cost volume + soft-argmin
   --> disp_postp --> disparity branch + fused trunk + PAFPN + head --> decode + NMS --> per-box
   depth + depth-guided scaling  --> fixed-size detection buffer (ready for the RCCL all-gather)

Everything between the input tensors and the detection buffer is enqueued on the current stream
through the C ABI (include/stereotrack.h); no host synchronisation, no allocation after the
first call.  Mirrors the dense part of OCSORT_Disparity.predict (reference
mmtrack/models/mot/ocsort_disparity.py:50-83): detector.predict (:79) + bbox_postp_depth (:82-83).
"""
import ctypes as C

import torch

from . import _lib, records
from ._lib import check, current_stream, ptr
from .engine import HipDetector, HipDispHead, RawChunk, _require_cuda
from .stereo import StereoCostVolume


# per-box depth estimators (include/stereotrack.h ST_DEPTH_*): the reference's default extract_depth and the four
# alternatives of its depth-extraction comparison (mmtrack/models/mot/depth_extraction_comparison.py)
DEPTH_METHODS = {'reference': 0, 'truncated_mean': 1, 'mean': 2, 'median': 3, 'center': 4}


def depth_method_code(name):
    """ST_DEPTH_* code of a depth_method / depth_extraction name; ValueError for anything else."""
    if not isinstance(name, str) or name not in DEPTH_METHODS:
        raise ValueError(f'unknown depth extraction method {name!r}: one of {", ".join(DEPTH_METHODS)}')
    return DEPTH_METHODS[name]


# where box_depth() reads its disparity (include/stereotrack.h st_disp_fuse `mode`): the input map disp_postp, the
# disparity-completion head's prediction resized to the padded input, or the input with its invalid pixels (<= 0, NaN)
# taken from the head
DEPTH_SOURCES = {'input': 0, 'completed': 1, 'fused': 2}


def depth_source_code(name):
    """st_disp_fuse mode of a depth_source name (0: no launch); ValueError for anything else."""
    if not isinstance(name, str) or name not in DEPTH_SOURCES:
        raise ValueError(f'unknown depth_source {name!r}: one of {", ".join(DEPTH_SOURCES)}')
    return DEPTH_SOURCES[name]


def launch_box_depth(lib, disp, boxes, counts, baseline, focal, method, out, channel_stride):
    """ONE st_box_depth launch (st_box_depth_method for method != 0) on the current stream: disp (N,C,H,W) fp32, frames
    `channel_stride` floats apart, boxes (N,M,4), counts (N,) -> out = (depth, scales, scaled boxes), every row defined."""
    N, M = boxes.shape[0], boxes.shape[1]
    args = (ptr(disp), channel_stride, N, *disp.shape[-2:], ptr(boxes), ptr(counts), M, float(baseline), float(focal),
            None, 0, current_stream(), *(ptr(t) for t in out))
    if method == 0:
        check(lib.st_box_depth(*args), 'st_box_depth')
    else:
        check(lib.st_box_depth_method(*args, method), 'st_box_depth_method')


def committed_tuning_plans():
    """configs/tuning/mi355x.json: the plans committed with the repository.  READ-ONLY for the package - one committed
    plan per graph makes the kernel instances (and with them the fp32 summation order, i.e. every float the path
    returns) the same in the parity tests and in the bench run; nothing here ever writes to a tracked file."""
    import os
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs', 'tuning', 'mi355x.json')


def default_tuning_cache():
    """Where NEWLY measured plans are remembered: $ST_TUNE_CACHE, else $XDG_CACHE_HOME (or ~/.cache)
    /stereotracking_amd/tuning.json.  Lookups consult this file first when $ST_TUNE_CACHE names it explicitly (tools
    trying out a plan), otherwise the committed plans first."""
    import os
    explicit = os.environ.get('ST_TUNE_CACHE')
    if explicit:
        return explicit
    base = os.environ.get('XDG_CACHE_HOME') or os.path.join(os.path.expanduser('~'), '.cache')
    return os.path.join(base, 'stereotracking_amd', 'tuning.json')


def _read_plans(path):
    """-> (dict, ok).  ok is False when the file exists but cannot be parsed (then it must not be overwritten)."""
    import json
    import os
    if not path or not os.path.exists(path):
        return {}, True
    try:
        with open(path) as f:
            d = json.load(f)
        return (d, True) if isinstance(d, dict) else ({}, False)
    except (OSError, ValueError):
        return {}, False


def _store_plans(path, updates):
    """Merge `updates` into the JSON file at `path`: exclusive lock on a side file, RE-READ under the lock, write a
    temporary file, os.replace (atomic).  Concurrent ranks / test processes that tune at the same time cannot
    truncate each other's file; a file that exists but does not parse is left alone."""
    import fcntl
    import json
    import os
    import tempfile
    try:
        d = os.path.dirname(os.path.abspath(path))
        os.makedirs(d, exist_ok=True)
        with open(path + '.lock', 'w') as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            cur, ok = _read_plans(path)
            if not ok:
                return False
            cur.update(updates)
            fd, tmp = tempfile.mkstemp(prefix='.tuning.', dir=d)
            with os.fdopen(fd, 'w') as f:
                json.dump(cur, f, indent=0, sort_keys=True)
            os.replace(tmp, path)
        return True
    except OSError:
        return False    # a read-only install keeps working: the plan was measured, it is just not remembered


def _device_tag():
    """gfx architecture + CU count of the current device: part of every plan key (a plan measured on one part says
    nothing about another)."""
    p = torch.cuda.get_device_properties(torch.cuda.current_device())
    arch = str(getattr(p, 'gcnArchName', 'gpu')).split(':')[0]
    return f'{arch}_cu{p.multi_processor_count}'


class StereoDensePipeline:
    """Fixed-shape dense path for `batch` frames of `ori_shape` (H, W) pixels."""

    def __init__(self, batch, ori_shape=(720, 1280), widen_factor=0.5, deepen_factor=0.33, num_classes=1,
                 stereo=True, max_disp=192, feat_stride=4, temperature=32.0, score_thr=0.01, iou_thr=0.5,
                 max_det=1000, baseline=0.25, focal_length=640, pad_size_divisor=32, agg_layers=0, agg3d_layers=0,
                 split_bf16=None, multi_label=True, rgb_only=False, full_res=False, full_res_channels=8, sgbm=None,
                 depth_method='reference', lr_check=False, lr_max_diff=1.0, disp_head=None,
                 depth_source='input'):
        """max_det: rows of the fixed-size detection buffer per frame.  The reference applies NO cap on the
        kept boxes (yolox_style=True => max_per_img = len(results)), so this is a
        capacity, not a threshold: `run()` reports `overflow` whenever a frame kept more boxes than fit, and
        every consumer in this package (sequence drivers, MOT shell, bench.py) raises on it.

        sgbm: a StereoSGBM config dict (or module, whose configuration is copied: every context owns its workspace).
        The pipeline then takes left + right frames like the stereo mode, computes the disparity with OpenCV's
        SGBM_3WAY restated on the device (sgbm.py) into the same disp_postp ring, and runs the MONO detector plan
        (stereo must be False) on img + that disparity - the configuration the reference's detector was trained in.

        depth_method: the per-box depth estimator of box_depth() (DEPTH_METHODS; 'reference' = the reference's default
        extract_depth, launched through st_box_depth exactly as before).

        lr_check / lr_max_diff: the stereo module's left-right check (stereo.py): pixels that fail it are 0 in disp_postp -
        so they drop out of the per-box depth - and `run()` also returns `disp_mask` (N,1,H,W), 1 = valid.

        disp_head: dict(in_channels=, channels=, bn_eps=) - the disparity-completion head (DispHeadV2, engine.HipDispHead).
        The detector plan is then built with out_fd; the head runs on the context's stream right after the detector
        forward, on the 'p3' and 'stage1_disp' taps in the context's workspace (so before that workspace is reused), and
        `run()` also returns `dense_disp` (N,1,H/2,W/2), the completed disparity of the PADDED input at half resolution.
        Parameters: `disp_head.*`.  None: nothing changes.

        depth_source: 'input' (box_depth reads disp_postp; no buffer, no launch), or - with disp_head - 'completed' /
        'fused': one st_disp_fuse launch between the head and box_depth builds `disp_depth` (N,1,H,W), the head's
        prediction resized to the PADDED input (the pixels disp_postp and the boxes live in), 'fused' keeping disp_postp
        wherever it is > 0; box_depth reads that map, and `run()` also returns it and `disp_filled` (N,) int32, the
        pixels inside `ext` that came from the head.  The map rotates over the `disp_buffers` slots under `disp_guard`
        exactly like the stereo module's disp_postp: a consumer may read run k's map while run k + 1 is enqueued."""
        self.depth_source = str(depth_source)
        self._depth_src = depth_source_code(depth_source)
        if self._depth_src and disp_head is None:
            raise ValueError(f'depth_source={depth_source!r} reads the disparity-completion head: pass disp_head=')
        self.depth_method = str(depth_method)
        self._depth_code = depth_method_code(depth_method)
        self.lib = _lib.load()
        self.batch = int(batch)
        self.ori_h, self.ori_w = int(ori_shape[0]), int(ori_shape[1])
        d = pad_size_divisor
        self.height = (self.ori_h + d - 1) // d * d
        self.width = (self.ori_w + d - 1) // d * d
        self.stereo = bool(stereo)
        self.sgbm = None
        if sgbm is not None:
            from .sgbm import StereoSGBM
            if self.stereo:
                raise ValueError('sgbm= runs the mono detector plan on the SGBM disparity: pass stereo=False')
            self.sgbm = StereoSGBM(**(sgbm.config() if isinstance(sgbm, StereoSGBM) else
                                      {k: v for k, v in sgbm.items() if k != 'type'}))
        self.takes_right = self.stereo or self.sgbm is not None    # run() needs the right image
        # full_res: the stereo module's full-resolution mode (D = max_disp levels at image resolution, 3-D aggregation
        # only; stereo.py) - north_star's literal D x H x W sizing as a product path
        self.full_res = bool(full_res) and bool(stereo)
        import math
        feat_channels = int(math.ceil(128 * widen_factor / 8) * 8)
        self.stereo_module = StereoCostVolume(max_disp, feat_stride, temperature, agg_layers if stereo else 0,
                                              agg3d_layers if stereo else 0, full_res=self.full_res,
                                              full_res_channels=full_res_channels, feat_channels=feat_channels,
                                              lr_check=bool(lr_check) and bool(stereo), lr_max_diff=lr_max_diff)
        self.lr_check, self.lr_max_diff = self.stereo_module.lr_check, self.stereo_module.lr_max_diff
        self.agg_layers = self.stereo_module.agg_layers
        self.agg3d_layers = self.stereo_module.agg3d_layers
        # split_bf16: the autotuner may pick the split-operand (bf16x3) conv instances (fp32 operands as three bf16 terms,
        # six exact products on the bf16 MFMA, fp32 accumulate).  PARKED in round 5 (frozen parity gate not passed, +0.7 % in
        # flight: DESIGN.md 5): the instances exist in the TOOLS build of the library only ($ST_LIBRARY pointing at
        # libstereotrack_hip_ablation.so); with the product library the request is an error, not a silent fallback.
        if split_bf16 is None:
            import os
            split_bf16 = os.environ.get('ST_SPLIT_BF16', '0') == '1'
        self.split_bf16 = bool(split_bf16)
        if self.split_bf16 and not self.lib.st_split_instances_available():
            raise RuntimeError('split_bf16 / ST_SPLIT_BF16=1: the split-operand (bf16x3) conv instances are parked in the '
                               'tools build (make -C stereotracking_amd/csrc ABLATION=1; ST_LIBRARY=<...>_ablation.so)')
        self.max_disp, self.feat_stride = int(max_disp), int(feat_stride)
        self.disp_buffers, self.disp_guard, self.disp_slot, self._disp_turn = 1, [None], 0, 0
        self.D = self.stereo_module.levels
        self.temperature = float(temperature)
        self.score_thr, self.iou_thr, self.max_det = float(score_thr), float(iou_thr), int(max_det)
        self.baseline, self.focal_length = float(baseline), float(focal_length)
        # rgb_only: the single-branch detector (reference config yolox_s_mmyolo_mot_airdrone.py:40-42, backbone
        # mmtrack.CSPDarknet); the disparity (loaded, or from the stereo module) is then consumed by box_depth only
        self.rgb_only = bool(rgb_only)
        self.det = HipDetector(self.batch, self.height, self.width, widen_factor, deepen_factor, num_classes,
                               stereo=self.stereo, rgb_only=self.rgb_only, out_fd=disp_head is not None)
        self.disp_head = None
        if disp_head is not None:
            cfg = {k: v for k, v in dict(disp_head).items() if k != 'type'}
            self.disp_head = HipDispHead(self.batch, self.height // 8, self.width // 8, **cfg)
        self.det.multi_label = bool(multi_label)     # several classes: test_cfg.multi_label
        self._bufs = None

    # ---- parameters ------------------------------------------------------------------------------
    def param_table(self):
        """Detector parameters (reference state_dict names) + `stereo.agg.*` of the stereo module."""
        return (self.det.param_table() + [('stereo.' + n, shp) for n, shp in self.stereo_module.param_table()] +
                ([('disp_head.' + n, shp) for n, shp in self.disp_head.param_table()] if self.disp_head is not None else []))

    def load_state_dict(self, sd, prefix='', autotune=True, tuning_cache=None):
        """Upload weights; then pick conv tile variants by measurement, or restore them from
        a plan file (JSON keyed by graph signature + device) when one holds this graph: the COMMITTED plans
        (committed_tuning_plans(), read-only) and the user cache (default_tuning_cache(), where new measurements are
        merged atomically).  `tuning_cache=<path>` / $ST_TUNE_CACHE: that file is consulted first and receives new
        measurements.  tuning_cache=False: always measure, never read or write a cache."""
        self.det.load_state_dict(sd, prefix)
        pre = prefix + 'stereo.'
        self.stereo_module.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)})
        if self.disp_head is not None:
            self.disp_head.load_state_dict(sd, prefix + 'disp_head.')
        if not autotune:
            return
        import os
        key = (f'v{self.det.lib.st_version()}_b{self.batch}_{self.height}x{self.width}_w{self.det.widen_factor:g}'
               f'_d{self.det.deepen_factor:g}_s{int(self.stereo)}{"r" if self.rgb_only else ""}'
               f'{"f" if self.det.out_fd else ""}{"_ds%d" % self._depth_src if self._depth_src else ""}_a{self.agg_layers}'
               f'_D{self.max_disp // self.feat_stride if self.full_res else self.D}'
               f'{"_F%d" % self.stereo_module.reduce.out_channels if self.full_res else ""}'
               f'_ops{self.det.lib.st_detector_num_ops(self.det.handle)}_{_device_tag()}'
               + ('_split' + os.environ.get('ST_SPLIT_MASK', '') if self.split_bf16 else ''))
        # (the 3-D aggregation layers run on a kernel of their own: no tile choice, not part of the key)
        sources = []
        if tuning_cache is not False:
            explicit = tuning_cache or os.environ.get('ST_TUNE_CACHE')
            store = explicit or default_tuning_cache()
            sources = [store, committed_tuning_plans()] if explicit else [committed_tuning_plans(), store]
            # full_res: the key carries `_F<channels>`, so a plan tuned for this mode is never served to the default module
            # or back.  Where no such plan exists yet, the DEFAULT module's plan of the same detector graph (agg_layers = 0
            # needs no `_agg` entry) is taken on purpose: the detector launch plan is identical - the key pins the op
            # count, set_tuning() rejects a plan of another length - and the full-resolution stereo kernels have no tile
            # choice.  Anything tuned per mode later lands under the `_F` key and wins.
            keys = [key] + ([key.replace(f'_F{self.stereo_module.reduce.out_channels}', '', 1)] if self.full_res else [])
            for k in keys:
                for path in sources:
                    cache, _ = _read_plans(path)
                    if k in cache and (not self.agg_layers or k + '_agg' in cache):
                        if len(cache[k]) != self.det.lib.st_detector_num_ops(self.det.handle):
                            continue
                        self.det.set_tuning(cache[k])
                        if self.agg_layers:
                            self.stereo_module.variant = int(cache[k + '_agg'])
                        self.tuning_source = path
                        return
        self.det.set_split(self.split_bf16)
        self.det.autotune()
        if self.agg_layers:
            s = self.feat_stride
            dev = torch.device('cuda', torch.cuda.current_device())
            extra = (50, 51, 52) if self.split_bf16 else ()
            self.stereo_module.autotune(dev, self.batch, self.height // s, self.width // s,
                                        candidates=tuple(range(22)) + (42, 43) + extra)
        self.tuning_source = 'measured'
        if tuning_cache is not False:
            upd = {key: self.det.get_tuning()}
            if self.agg_layers:
                upd[key + '_agg'] = self.stereo_module.variant
            _store_plans(store, upd)     # never the committed file (unless a tool names it explicitly)

    # ---- buffers -----------------------------------------------------------------------------------
    def _buffers(self, dev):
        if (self._bufs is None or self._bufs['dev'] != dev or
                len(self._bufs['disp_ring']) != max(1, int(self.disp_buffers))):
            N, H, W, M = self.batch, self.height, self.width, self.max_det
            f32 = dict(dtype=torch.float32, device=dev)
            b = dict(dev=dev)
            b['head'] = torch.empty(self.det.head_floats, **f32)
            b['disp_lr'] = torch.empty(N, H // self.feat_stride, W // self.feat_stride, **f32)
            # disp_buffers > 1: the stereo module's output alternates between that many buffers, so a consumer may keep
            # reading run k's disparity (the MOT shell's track-box depth, on a side stream) while run k+1 writes the
            # next one; `disp_guard[i]` = event the consumer records after its last read of buffer i (waited on before
            # buffer i is rewritten)
            b['disp_ring'] = [torch.empty(N, 3, H, W, **f32) for _ in range(max(1, int(self.disp_buffers)))]
            b['disp_postp'] = b['disp_ring'][0]
            # left-right check: one validity mask beside every disparity buffer (same slot, same guard event)
            b['mask_ring'] = [torch.empty(N, 1, H, W, **f32) if self.lr_check else None for _ in b['disp_ring']]
            b['disp_mask'] = b['mask_ring'][0]
            self.disp_guard = [None] * len(b['disp_ring'])
            self._disp_turn = 0
            b['depth'] = torch.empty(N, M, **f32)       # rows past the count are written as 0 by st_box_depth
            b['scales'] = torch.empty(N, M, **f32)
            b['scaled_boxes'] = torch.empty(N, M, 4, **f32)
            b['decode'] = self.det.decode_buffers(M, dev)   # persistent: st_decode_nms defines every row itself
            b['overflow'] = torch.empty(N, dtype=torch.bool, device=dev)
            if self.disp_head is not None:
                b['dense_disp'] = torch.empty(N, 1, H // 2, W // 2, **f32)
            if self._depth_src:     # one map (and its counters) per disparity slot, under the same guard events
                b['depth_ring'] = [torch.empty(N, 1, H, W, **f32) for _ in b['disp_ring']]
                b['filled_ring'] = [torch.empty(N, dtype=torch.int32, device=dev) for _ in b['disp_ring']]
            self._bufs = b
        return self._bufs

    # ---- the hot path --------------------------------------------------------------------------------
    def disparity(self, img, right):
        """Stereo module: stem+stage1 features of left/right -> cost volume -> soft-argmin ->
        bilinear x4 -> disp_postp (N,3,H,W) in pixels, 0 outside the original image.  With sgbm: StereoSGBM of
        left/right (RawChunks or fp32 batches) -> disp_postp."""
        b = self._buffers(img.device)
        k = self._disp_turn % len(b['disp_ring'])
        self._disp_turn += 1
        self.disp_slot = k
        if self.disp_guard[k] is not None:
            torch.cuda.current_stream(img.device).wait_event(self.disp_guard[k])
            self.disp_guard[k] = None
        out = b['disp_postp'] = b['disp_ring'][k]
        mask = b['disp_mask'] = b['mask_ring'][k]
        if self.sgbm is not None:
            self.sgbm.compute(img, right, (self.ori_h, self.ori_w), out)
        else:
            self.stereo_module.compute(self.det, img, right, (self.ori_h, self.ori_w), b['disp_lr'], out, disp_mask=mask)
        return out

    def depth_map(self, disp_postp, ext=None):
        """st_disp_fuse: the head's `dense_disp` of this run (+ plane 0 of disp_postp) -> disp_depth (N,1,H,W), filled (N,).
        The stereo / SGBM pipeline writes the slot disparity() just took (its guard has been waited for); the mono
        pipeline, whose disp_postp is the caller's tensor, takes the next slot here."""
        b = self._buffers(disp_postp.device)
        N, H, W = self.batch, self.height, self.width
        if tuple(disp_postp.shape[-2:]) != (H, W) or disp_postp.shape[0] != N or not disp_postp.is_contiguous():
            raise ValueError(f'disp_postp: expected a contiguous ({N}, C, {H}, {W}) map, got {tuple(disp_postp.shape)}')
        if not self.takes_right:
            k = self._disp_turn % len(b['depth_ring'])
            self._disp_turn += 1
            self.disp_slot = k
            if self.disp_guard[k] is not None:
                torch.cuda.current_stream(disp_postp.device).wait_event(self.disp_guard[k])
                self.disp_guard[k] = None
        k = self.disp_slot
        eh, ew = (self.ori_h, self.ori_w) if ext is None else (int(ext[0]), int(ext[1]))
        out, filled = b['depth_ring'][k], b['filled_ring'][k]
        check(self.lib.st_disp_fuse(ptr(b['dense_disp']), ptr(disp_postp), disp_postp.shape[1] * H * W, N, H, W, eh, ew,
                                    self._depth_src, ptr(out), ptr(filled), current_stream()), 'st_disp_fuse')
        return out, filled

    def box_depth(self, disp_postp, boxes, counts, out=None):
        """bbox_postp_depth (ocsort_disparity.py:113-130) on device -> depth, scales, scaled boxes."""
        b = self._buffers(disp_postp.device)
        out = out if out is not None else (b['depth'], b['scales'], b['scaled_boxes'])
        _, Cc, H, W = disp_postp.shape      # the plan's (3, height, width): ONE source for the stride and the launch's H, W
        launch_box_depth(self.lib, disp_postp, boxes, counts, self.baseline, self.focal_length, self._depth_code, out,
                         Cc * H * W)
        return out

    def run(self, img, right=None, disp_postp=None, ext=None):
        """img (N,3,H,W) fp32 CUDA; stereo: right (N,3,H,W); mono: disp_postp (N,3,H,W).  img (and, stereo, right)
        may be engine.RawChunk (N uint8 frames each): the stem kernels cast + pad them while staging their windows.
        Returns a dict of device tensors (no host sync; the context's PERSISTENT buffers, overwritten by its next run): boxes (N,M,4) unscaled xyxy, scores, labels,
        prior_idx, counts (TRUE number kept per frame), overflow (N,) bool = counts > M, depth, scales,
        scaled_boxes, disp_postp, head (and, with lr_check, disp_mask (N,1,H,W): 1 = valid).  Rows past min(counts, M) are zero (prior_idx -1).  With disp_buffers > 1 the
        stereo module's disp_postp is buffer `self.disp_slot` of the ring (see _buffers).  ext: (h, w) of the frames inside
        the padded input (img_shape; default ori_shape) - with a depth_source other than 'input', where `disp_filled` counts."""
        if isinstance(img, RawChunk):
            if (self.stereo or self.sgbm is not None) and not isinstance(right, RawChunk):
                raise ValueError('the stereo pipeline takes left AND right as raw uint8 chunks (or both as fp32 tensors)')
        else:
            _require_cuda(img, 'img')
        b = self._buffers(img.device)
        if self.sgbm is not None:
            if right is None:
                raise ValueError('the SGBM pipeline needs the right image')
            disp_postp = self.disparity(img, right)
            self.det.forward(img, disp_postp, b['head'])
        elif self.stereo:
            if right is None:
                raise ValueError('stereo pipeline needs the right image')
            disp_postp = self.disparity(img, right)
            self.det.forward_phase(1, disp=disp_postp, head_out=b['head'])
        else:
            if disp_postp is None:
                raise ValueError('mono pipeline needs disp_postp')
            self.det.forward(img, disp_postp, b['head'])
        if self.disp_head is not None:     # reads the taps this forward left in the context's workspace
            self.disp_head.forward(self.det, out=b['dense_disp'])
        boxes, scores, labels, prior, counts = self.det.decode_nms(
            b['head'], self.score_thr, self.iou_thr, self.max_det, (self.ori_h, self.ori_w), out=b['decode'])
        disp_depth = filled = None
        if self._depth_src:
            disp_depth, filled = self.depth_map(disp_postp, ext)
        depth, scales, sboxes = self.box_depth(disp_postp if disp_depth is None else disp_depth, boxes, counts)
        torch.gt(counts, self.max_det, out=b['overflow'])
        out = dict(boxes=boxes, scores=scores, labels=labels, prior_idx=prior, counts=counts,
                   overflow=b['overflow'], depth=depth, scales=scales, scaled_boxes=sboxes,
                   disp_postp=disp_postp, head=b['head'])
        if self.lr_check:
            out['disp_mask'] = b['disp_mask']
        if self.disp_head is not None:
            out['dense_disp'] = b['dense_disp']
        if disp_depth is not None:
            out['disp_depth'], out['disp_filled'] = disp_depth, filled
        return out

    @staticmethod
    def pack_detections(out, scaled=False, n_real=None):
        """Fixed-size, self-describing frame records for the all-gather: (N, M + 1, 8) fp32.
        Row 0 = header [count kept (true, may exceed M = overflow), M, valid frame flag, 0...]; rows 1..M =
        x1,y1,x2,y2,score,label,depth,scale (`scaled`: the depth-scaled boxes the tracker consumes;
        scaled='both': 13 columns, the unscaled box first, then the scaled box and the kept prior index appended -
        what the MOT shell copies to the host in ONE transfer per batch).  A fresh tensor: safe to keep after the context's buffers are reused.
        Frames >= n_real are batch padding."""
        mode = 2 if scaled == 'both' else (1 if scaled is True else 0)
        N, M = out['boxes'].shape[0], out['boxes'].shape[1]
        rec = torch.empty(N, M + 1, records.REC_FLOATS_BOTH if mode == 2 else records.REC_FLOATS, dtype=torch.float32, device=out['boxes'].device)
        check(_lib.load().st_pack_records(ptr(out['boxes']), ptr(out['scores']), ptr(out['labels']), ptr(out['depth']),
                                          ptr(out['scales']), ptr(out['scaled_boxes']), ptr(out['prior_idx']),
                                          ptr(out['counts']), N, M, mode, N if n_real is None else int(n_real),
                                          ptr(rec), current_stream()), 'st_pack_records')
        return rec


class InflightPipelines:
    """`n` independent StereoDensePipeline contexts (own workspace, buffers and HIP stream each), fed round-robin.

    Consecutive batches are independent (the dense path is stateless per frame), so batch i+1 may start while
    batch i is still running: the tail of every kernel launch (the last partial wave of workgroups) and the
    latency-bound decode / NMS / per-box-depth kernels of one batch are filled by the convs of the next.
    Measured on MI355X (bench workload, round 3 library, one hardware queue per context): 1 context 1538-1568 pairs/s,
    3 contexts 1811, 4 contexts 1839-1843.

    submit() returns (out, event): `out` is that context's result dict (device tensors, overwritten when the same
    context is reused `n` submits later), `event` is recorded on the context's stream after the batch.
    """

    def __init__(self, n, *args, **kwargs):
        if n < 1:
            raise ValueError('need at least one context')
        self.pipes = [StereoDensePipeline(*args, **kwargs) for _ in range(int(n))]
        self.streams = None
        self._next = 0

    def __len__(self):
        return len(self.pipes)

    def __getattr__(self, name):   # geometry / thresholds of the (identical) contexts: batch, max_det, stereo, ...
        if name in ('batch', 'max_det', 'stereo', 'height', 'width', 'ori_h', 'ori_w', 'agg_layers', 'agg3d_layers', 'split_bf16',
                    'rgb_only', 'full_res', 'sgbm', 'takes_right', 'depth_method', 'lr_check', 'lr_max_diff', 'disp_head',
                    'depth_source'):
            return getattr(self.pipes[0], name)
        raise AttributeError(name)

    def param_table(self):
        return self.pipes[0].param_table()

    def load_state_dict(self, sd, prefix='', autotune=True, tuning_cache=None):
        first = self.pipes[0]
        first.load_state_dict(sd, prefix, autotune, tuning_cache)
        for p in self.pipes[1:]:   # same graph: reuse the measured tile choices instead of re-tuning
            p.load_state_dict(sd, prefix, autotune=False)
            if autotune:
                p.det.set_tuning(first.det.get_tuning())
                p.stereo_module.variant = first.stereo_module.variant

    def next_stream(self, device):
        """The stream of the context the NEXT submit() runs on: work that produces that batch's inputs may be enqueued
        there directly instead of on the caller's stream."""
        if self.streams is None:
            self.streams = [torch.cuda.Stream(device=device) for _ in self.pipes]
        return self.streams[self._next % len(self.pipes)]

    def submit(self, img, right=None, disp_postp=None, post=None, ext=None):
        """Enqueue one batch on the next context's stream (after everything already enqueued on the caller's
        current stream, where the inputs were produced).  `post(out)` runs under that stream too.  ext: run()'s."""
        if not isinstance(img, RawChunk):
            _require_cuda(img, 'img')
        if self.streams is None:
            self.streams = [torch.cuda.Stream(device=img.device) for _ in self.pipes]
        j = self._next % len(self.pipes)
        self._next += 1
        s = self.streams[j]
        s.wait_stream(torch.cuda.current_stream(img.device))
        for t in (img, right, disp_postp):   # the caller may drop its references while the batch is still running
            if t is not None:
                t.record_stream(s)
        with torch.cuda.stream(s):
            out = self.pipes[j].run(img, right, disp_postp, ext)
            if post is not None:
                out = post(out, j)
            ev = torch.cuda.Event()
            ev.record(s)
        return out, ev

    def synchronize(self):
        for s in self.streams or []:
            s.synchronize()
