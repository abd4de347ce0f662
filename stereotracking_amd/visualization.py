"""Annotated frames (ABI: include/stereotrack_vis.h): the track overlay in HIP, the reference's
TrackLocalVisualizer and TrackVisualizationHook above it.

  draw_tracks             st_draw_tracks (csrc/draw_tracks.hip) on uint8 planar device frames, in place
  TrackLocalVisualizer    reference mmtrack/visualization/local_visualizer.py:27-219: colour per instance id, label
                          `id | score`, score threshold, GT and prediction side by side; the painted frames are written
                          as JPEG by jpeg_write.JpegEncoder (forward path in HIP)
  TrackVisualizationHook  reference mmtrack/engine/hooks/visualization_hook.py:17-147: after_test_iter writes one painted
                          frame per test iteration into test_out_dir

Not restated: category names in the label and matplotlib's text rendering (a built-in 5x7 bitmap font takes their
place), masks (NotImplementedError), show=True (refused: there is no window), the vis backends (accepted and ignored).
"""
import ctypes as C
import os
import threading

import numpy as np

from . import _lib
from .jpeg import _check
from .registry import HOOKS, VISUALIZERS

LABEL_MAX = 15
# StDrawBox, field for field
BOX_DTYPE = np.dtype([('xyxy', np.float32, 4), ('colour', np.uint8, 3), ('zoom', np.uint8), ('label_len', np.uint8),
                      ('label', np.uint8, LABEL_MAX)])
assert BOX_DTYPE.itemsize == 36

_PROTOS = {
    'st_draw_tracks': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_ssize_t, C.c_ssize_t, C.c_ssize_t, C.c_void_p,
                                 C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
}
_bound = None
_bind_lock = threading.Lock()


def _api():
    """The library handle with the overlay's prototype of stereotrack_vis.h set on it (outside _lib._PROTOS, which
    mirrors stereotrack.h name for name)."""
    global _bound
    if _bound is None:
        with _bind_lock:
            if _bound is None:
                lib = _lib.load()
                for name, (res, args) in _PROTOS.items():
                    fn = getattr(lib, name)
                    fn.restype, fn.argtypes = res, args
                _bound = lib
    return _bound


# the ten colours of matplotlib's default cycle, which seaborn.color_palette() returns by default, as 8-bit RGB
# [upstream-memory: seaborn and matplotlib are absent here, the parity of these triples with int(255 * c) is unpinned]
PALETTE = ((31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194),
           (127, 127, 127), (188, 189, 34), (23, 190, 207))


def random_color(seed):
    """The reference's random_color (local_visualizer.py:18-24): seed numpy's legacy generator with the id and draw one
    of the ten palette entries -> an RGB triple.  A private RandomState gives the value np.random.seed(id) +
    np.random.choice would, without reseeding the process's global generator."""
    rs = np.random.RandomState(int(seed) % (1 << 32))
    return PALETTE[int(rs.choice(range(len(PALETTE))))]


def tag_zoom(area):
    """The reference's adaptive text scale (mmdet _get_adaptive_scales with its defaults: 0.5 + (area - 800) / (30000 -
    800), clipped to 0.5 .. 1.0, times the 13 pt font) mapped onto an integer zoom of the 7-pixel-high font: 2 from
    about 10900 px^2 on, else 1."""
    scale = min(max(0.5 + (float(area) - 800.0) / (30000.0 - 800.0), 0.5), 1.0)
    return max(1, (int(13 * scale) + 3) // 7)


def pack_boxes(per_frame):
    """per_frame: for each frame a list of (xyxy, colour per PLANE, label str) -> (boxes (N, K) BOX_DTYPE, counts (N,)
    int32), K the largest count.  The zoom follows tag_zoom of the box's area."""
    n = len(per_frame)
    k = max([len(f) for f in per_frame] + [0])
    boxes = np.zeros((n, k), BOX_DTYPE)
    counts = np.zeros(n, np.int32)
    for i, frame in enumerate(per_frame):
        counts[i] = len(frame)
        for j, (xyxy, colour, label) in enumerate(frame):
            b = boxes[i, j]
            b['xyxy'] = np.asarray(xyxy, np.float32)
            b['colour'] = colour
            x1, y1, x2, y2 = (float(v) for v in b['xyxy'])
            b['zoom'] = tag_zoom((y2 - y1) * (x2 - x1)) if np.isfinite([x1, y1, x2, y2]).all() else 1
            raw = label.encode('ascii', 'replace')[:LABEL_MAX]
            b['label_len'] = len(raw)
            b['label'][:len(raw)] = np.frombuffer(raw, np.uint8)
    return boxes, counts


def draw_tracks(frames, boxes, counts, line_width=3, alpha=0.8):
    """st_draw_tracks on the current stream: frames a uint8 (N, 3, H, W) device tensor (unit stride along W; it may be a
    view into a wider buffer), painted IN PLACE; boxes (N, K) BOX_DTYPE and counts (N,) int32 host arrays (pack_boxes).
    K == 0: no launch, no allocation."""
    import torch
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and
            frames.shape[1] == 3 and frames.stride(3) == 1):
        raise TypeError('draw_tracks takes a uint8 (N, 3, H, W) device tensor with unit stride along W')
    n, _, h, w = frames.shape
    boxes = np.ascontiguousarray(boxes, BOX_DTYPE)
    counts = np.ascontiguousarray(counts, np.int32)
    if boxes.ndim != 2 or boxes.shape[0] != n or counts.shape != (n,):
        raise ValueError(f'{n} frames, boxes {boxes.shape}, counts {counts.shape}')
    k = boxes.shape[1]
    if k == 0 or n == 0:
        return frames
    a256 = int(round(float(alpha) * 256))
    dev = frames.device
    with torch.cuda.device(dev):
        blob = np.concatenate([counts.view(np.uint8), np.zeros(-counts.nbytes % 16, np.uint8), boxes.reshape(-1).view(np.uint8)])
        blob_dev = torch.from_numpy(blob).to(dev, non_blocking=False)
        off = counts.nbytes + (-counts.nbytes % 16)
        rc = _api().st_draw_tracks(frames.data_ptr(), n, h, w, frames.stride(0), frames.stride(1), frames.stride(2),
                                   blob_dev.data_ptr() + off, blob_dev.data_ptr(), k, int(line_width), a256,
                                   torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, 'st_draw_tracks')
    return frames


# ---- the reference's visualizer --------------------------------------------------------------------------------------
_current = None


def instance_boxes(instances):
    """InstanceData -> [(xyxy, RGB colour, label)] by the rules of the reference's _draw_instances: colour
    random_color(id), label `id | score` (two decimals) or `id`; without instances_id (SOT / VOS) the colour of the
    instance's index and the score alone."""
    if 'masks' in instances:
        raise NotImplementedError('TrackLocalVisualizer: masks are not drawn')
    if 'bboxes' not in instances:
        return []
    bboxes = np.asarray(_host(instances.bboxes), np.float32)
    bboxes = bboxes.reshape(-1, bboxes.shape[-1] if bboxes.ndim == 2 and bboxes.shape[-1] >= 4 else 4)[:, :4]
    scores = _host(instances.scores) if 'scores' in instances else None
    if 'instances_id' in instances:
        ids = [int(i) for i in _host(instances.instances_id)]
        colours = [random_color(i) for i in ids]
        labels = [f'{i} | {float(s):.2f}' for i, s in zip(ids, scores)] if scores is not None else [f'{i}' for i in ids]
    else:
        colours = [random_color(i) for i in range(len(bboxes))]
        labels = [f'{float(s):.2f}' for s in scores] if scores is not None else [''] * len(bboxes)
    return list(zip(bboxes, colours, labels))


def _host(v):
    return v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)


@VISUALIZERS.register_module(name=['TrackLocalVisualizer'])
class TrackLocalVisualizer:
    """The reference's TrackLocalVisualizer on the device: boxes and id tags painted by st_draw_tracks, the result
    written as JPEG through JpegEncoder.

    name, vis_backends (accepted and ignored), save_dir, line_width, alpha as in the reference; quality / subsampling:
    the JPEG writer's; device: where host images are painted (default: the current GPU); chunk: frames per draw launch
    and encode call."""

    def __init__(self, name='visualizer', image=None, vis_backends=None, save_dir=None, line_width=3, alpha=0.8, quality=90,
                 subsampling='420', device=None, chunk=16):
        global _current
        if subsampling not in ('444', '422', '420'):
            raise ValueError(f"subsampling is '444', '422' or '420', not {subsampling!r}")
        self.name, self.save_dir = name, save_dir
        self.line_width, self.alpha = int(line_width), float(alpha)
        self.quality, self.subsampling = int(quality), subsampling
        self.device, self.chunk = device, max(int(chunk), 1)
        self.dataset_meta = {}
        self._encoder = None
        _current = self

    @classmethod
    def get_current_instance(cls):
        """The visualizer built last (mmengine's ManagerMixin.get_current_instance), a default one if none was."""
        return _current if _current is not None else cls()

    # the two seams to the device: tests without a GPU put the host routines here
    def _draw(self, frames, boxes, counts):
        return draw_tracks(frames, boxes, counts, self.line_width, self.alpha)

    def _encode(self, frames):
        from .jpeg_write import JpegEncoder
        if self._encoder is None or self._encoder.dev != frames.device:
            self.close()
            self._encoder = JpegEncoder(frames.device, quality=self.quality, subsampling=self.subsampling)
        return self._encoder.encode(frames, order='bgr')

    def close(self):
        """Stop the encoder's pool threads (idle ones also end with the interpreter)."""
        if self._encoder is not None:
            self._encoder.close()
            self._encoder = None

    def _to_device(self, image):
        """-> uint8 (3, H, W) planar BGR on the device (the caller's memory is never painted)."""
        import torch
        if isinstance(image, torch.Tensor):
            if image.dtype != torch.uint8 or image.dim() not in (3, 4) or image.shape[-3] != 3 or (image.dim() == 4 and image.shape[0] != 1):
                raise TypeError('an image tensor is uint8 (3, H, W) or (1, 3, H, W), planar BGR')
            image = image.reshape(3, *image.shape[-2:])
            return image if self.device is None and image.is_cuda else image.to(self._device())
        arr = np.asarray(image)
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
            raise TypeError('a host image is a uint8 (H, W, 3) RGB array')
        return torch.from_numpy(np.ascontiguousarray(arr[..., ::-1].transpose(2, 0, 1))).to(self._device())

    def _device(self):
        import torch
        return torch.device('cuda', torch.cuda.current_device()) if self.device is None else torch.device(self.device)

    def _sides(self, data_sample, draw_gt, draw_pred, pred_score_thr):
        """The box lists to paint, GT first: the reference's add_datasample rules."""
        sides = []
        if data_sample is None:
            return [[]]
        if draw_gt:
            assert 'gt_instances' in data_sample
            sides.append(instance_boxes(data_sample.gt_instances))
        if draw_pred:
            assert 'pred_track_instances' in data_sample
            pred = data_sample.pred_track_instances
            if 'scores' in pred:
                pred = pred[pred.scores > pred_score_thr]
            sides.append(instance_boxes(pred))
        return sides or [[]]

    def add_datasamples(self, images, data_samples, out_files=None, draw_gt=True, draw_pred=True, pred_score_thr=0.3):
        """The batched form: one draw launch and one encode call per chunk of equal-sized frames -> the JPEG bytes of
        every painted frame; out_files (one path or None per frame): where they are written."""
        import torch
        images, data_samples = list(images), list(data_samples)
        out_files = [None] * len(images) if out_files is None else list(out_files)
        if not len(images) == len(data_samples) == len(out_files):
            raise ValueError(f'{len(images)} images, {len(data_samples)} data samples, {len(out_files)} output files')
        frames = [self._to_device(im) for im in images]
        sides = [self._sides(ds, draw_gt, draw_pred, pred_score_thr) for ds in data_samples]
        blobs = []
        s = 0
        while s < len(frames):
            e = s + 1
            while (e < len(frames) and e - s < self.chunk and frames[e].shape == frames[s].shape and
                   frames[e].device == frames[s].device and len(sides[e]) == len(sides[s])):
                e += 1
            n, ns = e - s, len(sides[s])
            _, h, w = frames[s].shape
            canvas = torch.stack([frames[i] for i in range(s, e) for _ in range(ns)])          # (n * ns, 3, H, W), a copy
            per_frame = [[(xyxy, rgb[::-1], label) for xyxy, rgb, label in side] for i in range(s, e) for side in sides[i]]
            boxes, counts = pack_boxes(per_frame)
            canvas = self._draw(canvas, boxes, counts)
            if ns > 1:                                         # GT left, prediction right
                canvas = canvas.view(n, ns, 3, h, w).permute(0, 2, 3, 1, 4).reshape(n, 3, h, ns * w)
            blobs += self._encode(canvas)
            s = e
        for path, blob in zip(out_files, blobs):
            if path is not None:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, 'wb') as f:
                    f.write(blob)
        return blobs

    def add_datasample(self, name, image, data_sample=None, draw_gt=True, draw_pred=True, show=False, wait_time=0,
                       out_file=None, pred_score_thr=0.3, step=0):
        """The reference's signature.  -> the painted frame's JPEG bytes (also written to out_file, and to
        save_dir/vis_data/vis_image/<name>_<step>.jpg when save_dir is set, as the reference's LocalVisBackend names it)."""
        if show:
            raise NotImplementedError('TrackLocalVisualizer: show=True needs a window; pass out_file or save_dir')
        blob = self.add_datasamples([image], [data_sample], [out_file], draw_gt, draw_pred, pred_score_thr)[0]
        if self.save_dir is not None:
            path = os.path.join(self.save_dir, 'vis_data', 'vis_image', f'{name}_{step}.jpg')
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, 'wb') as f:
                f.write(blob)
        return blob


VISUALIZERS.register_module(name='mmtrack.TrackLocalVisualizer', module=TrackLocalVisualizer)


@HOOKS.register_module(name=['TrackVisualizationHook'])
class TrackVisualizationHook:
    """The reference's TrackVisualizationHook for the test loop: with draw=True every `interval`-th iteration's frames
    are painted with their predictions (score > score_thr) and written to test_out_dir/<basename>.jpg.  It sits outside
    the model: the caller's loop hands it what test_step took and returned."""

    def __init__(self, draw=False, interval=30, score_thr=0.3, show=False, wait_time=0., test_out_dir=None,
                 file_client_args=None, visualizer=None):
        if show:
            raise NotImplementedError('TrackVisualizationHook: show=True needs a window; set test_out_dir')
        self.draw, self.interval, self.score_thr = bool(draw), int(interval), float(score_thr)
        self.show, self.wait_time, self.test_out_dir = False, wait_time, test_out_dir
        self._visualizer_cfg = visualizer
        self._visualizer = None
        self._out_dir = None

    @property
    def visualizer(self):
        if self._visualizer is None:
            v = self._visualizer_cfg
            self._visualizer = (VISUALIZERS.build(v) if isinstance(v, dict) else v) or TrackLocalVisualizer.get_current_instance()
        return self._visualizer

    def every_n_inner_iters(self, batch_idx, n):
        return (batch_idx + 1) % n == 0 if n > 0 else False

    def out_dir(self, runner):
        """test_out_dir as given when there is no runner, else under the runner's work_dir / timestamp (joined once: the
        reference joins again on every iteration)."""
        if self.test_out_dir is None:
            return None
        if self._out_dir is None:
            self._out_dir = (self.test_out_dir if runner is None else
                             os.path.join(runner.work_dir, str(runner.timestamp), self.test_out_dir))
        return self._out_dir

    @staticmethod
    def out_name(sample, batch_idx, i):
        path = sample.get('img_path') if sample is not None else None
        if isinstance(path, (list, tuple)):
            path = path[0]
        if path:
            return os.path.splitext(os.path.basename(path))[0] + '.jpg'
        return f'{batch_idx:06d}_{i}.jpg'

    @staticmethod
    def frames_of(data_batch, n):
        """The n frames of data_batch['inputs']['img'] as uint8 (3, H, W) device tensors, or None when they are not there."""
        import torch
        from .shell_inputs import RawFrames
        inputs = data_batch.get('inputs') if isinstance(data_batch, dict) else None
        img = inputs.get('img') if isinstance(inputs, dict) else None
        if img is None:
            return None
        if isinstance(img, RawFrames):
            img = img.frames
        if isinstance(img, torch.Tensor):
            img = list(img.reshape(-1, *img.shape[-3:]))
        frames = []
        for f in img:
            f = f.reshape(-1, *f.shape[-3:])
            for g in f:
                if g.dtype != torch.uint8:
                    if not (g.is_floating_point() and bool(((g == g.round()) & (g >= 0) & (g <= 255)).all())):
                        raise TypeError('TrackVisualizationHook: frames must be uint8, or floating point holding the integers 0..255')
                    g = g.to(torch.uint8)
                frames.append(g)
        if len(frames) != n:
            raise ValueError(f"TrackVisualizationHook: data_batch['inputs']['img'] holds {len(frames)} frames for {n} outputs")
        return frames

    @staticmethod
    def read_image(path):
        """img_path through the project's own readers -> uint8 (H, W, 3) RGB."""
        from . import datasets, jpeg
        ext = os.path.splitext(path)[1].lower()
        if ext == '.png':
            arr = datasets.read_png(path)
        elif ext in ('.jpg', '.jpeg'):
            arr = jpeg.read_jpeg(path)
        else:
            raise ValueError(f'TrackVisualizationHook: no reader for {path!r} (.png, .jpg, .jpeg)')
        arr = np.asarray(arr)
        return np.repeat(arr[..., None], 3, -1) if arr.ndim == 2 else arr[..., :3]

    def after_test_iter(self, runner, batch_idx, data_batch, outputs):
        if not self.draw:
            return None
        if not self.every_n_inner_iters(batch_idx, self.interval):
            return None
        outputs = list(outputs)
        frames = self.frames_of(data_batch, len(outputs))
        if frames is None:
            frames = []
            for s in outputs:
                path = s.get('img_path')
                frames.append(self.read_image(path[0] if isinstance(path, (list, tuple)) else path))
        out_dir = self.out_dir(runner)
        files = [None if out_dir is None else os.path.join(out_dir, self.out_name(s, batch_idx, i)) for i, s in enumerate(outputs)]
        # GT beside the prediction only where the sample carries it (the reference asserts it does)
        with_gt = all('gt_instances' in s for s in outputs)
        self.visualizer.add_datasamples(frames, outputs, files, draw_gt=with_gt, draw_pred=True, pred_score_thr=self.score_thr)
        return files


HOOKS.register_module(name='mmtrack.TrackVisualizationHook', module=TrackVisualizationHook)
