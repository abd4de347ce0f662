"""The host path from a preprocessed call to a dense chunk's inputs.  OCSORT_Disparity (mot.py) and MultiStreamTracker
(multistream.py) both validate (plan_inputs) and feed their chunks (chunk_inputs) HERE: a stream sees what `test_step`
returns for its frames because there is one copy of this logic."""
import ctypes as C

import torch

from . import _lib
from . import sgbm as _sgbm
from ._lib import check, current_stream, ptr


class RawFrames:
    """N equal-sized uint8 CUDA frames (1,3,h,w) of one input key, NOT yet converted: what test_step hands to
    predict() for frames uploaded raw.  predict() converts a chunk at a time (torch.cat of the chunk's frames +
    st_pack_raw_inputs: cast + pad in one HIP pass) inside the pipelined submit, so the conversion
    of chunk i+3 overlaps the dense work of chunks i..i+2 and no (N,1,3,H,W) fp32 copy of the whole call exists.
    Values are exactly those of TrackDataPreprocessor_Disparity_V1.forward (reference
    data_preprocessor_disparity_v1.py:21-84 + utils/misc.py:13-64)."""

    def __init__(self, frames, pad_hw, pad_value):
        self.frames, self.pad_hw, self.pad_value = frames, (int(pad_hw[0]), int(pad_hw[1])), float(pad_value)
        self.hw = tuple(frames[0].shape[-2:])
        self.device = frames[0].device

    def __len__(self):
        return len(self.frames)

    def chunk(self, s, e, B):
        """frames [s, e) (+ the last one repeated up to B) -> (B,3,H,W) fp32, padded with pad_value."""
        fr = self.frames[s:e]
        fr = fr + [fr[-1]] * (B - len(fr))
        (h, w), (H, W) = self.hw, self.pad_hw
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=self.device)
        lib = _lib.load()
        if (B <= 32 and w % 4 == 0 and W % 4 == 0 and
                all(f.is_contiguous() and f.dtype == torch.uint8 and f.data_ptr() % 4 == 0 for f in fr)):
            # the frames stay where the dataloader put them: their pointers travel in the kernel arguments
            # (no torch.cat staging copy: 73 us per input and chunk at 8 x 720 x 1280)
            ptrs = (C.c_void_p * B)(*[f.data_ptr() for f in fr])
            check(lib.st_pack_raw_frames(ptrs, B, h, w, H, W, self.pad_value, ptr(out), current_stream()),
                  'st_pack_raw_frames')
            return out
        raw = torch.cat(fr, dim=0)
        check(lib.st_pack_raw_inputs(ptr(raw), None, B, h, w, H, W, self.pad_value, ptr(out), None, None,
                                     current_stream()), 'st_pack_raw_inputs')
        return out

    def raw_chunk(self, s, e, B, runner):
        """frames [s, e) (+ the last one repeated up to B) as an engine.RawChunk - the stem kernel casts + pads them while it
        stages its input windows (st_detector_forward_phase0_raw), no fp32 image exists - or None when the frames do
        not qualify (width % 4, alignment, non-integral pad value, padded size of another plan)."""
        from .engine import RawChunk
        fr = self.frames[s:e]
        fr = fr + [fr[-1]] * (B - len(fr))
        if self.pad_hw != (runner.height, runner.width) or not RawChunk.supported(fr, self.pad_value):
            return None
        return RawChunk(fr, self.pad_value)

    def dense(self):
        """The (N,1,3,H,W) fp32 tensor the preprocessor would have produced (for callers that want it)."""
        return self.chunk(0, len(self.frames), len(self.frames))[:, None]


def preprocess(model, data):
    if model._pre_lazy:     # decided once from the preprocessor's signature (__init__), not by catching TypeError
        return model.data_preprocessor(data, False, lazy_raw=True)
    return model.data_preprocessor(data, False)      # a preprocessor without the lazy option (e.g. mmengine's own class)


def _hw(shape):
    return tuple(int(v) for v in shape[:2])


def uniform_ori_shape(metas, default=None):
    """The ori_shape (h, w) the frames of one launch plan share: that of the first meta (`default` when it has none);
    a meta without the key takes it over, one with another shape raises."""
    ori = metas[0].get('ori_shape', default)
    ori = None if ori is None else _hw(ori)
    for m in metas[1:]:
        if 'ori_shape' in m:
            if ori is not None and _hw(m['ori_shape']) != ori:
                raise NotImplementedError('one batched launch plan needs a uniform ori_shape')
            ori = _hw(m['ori_shape'])
    return ori


def _unwrap(t, name):      # (N,1,C,H,W) tensor -> (N,C,H,W); RawFrames stay lazy (converted per chunk)
    if t is None or isinstance(t, RawFrames):
        return t
    assert t.dim() == 5, f'The {name} must be 5D Tensor (N, T, C, H, W).'
    assert t.size(1) == 1, 'one key frame per sample (T = 1)'
    return t[:, 0]


def plan_inputs(model, inputs, data_samples, who):
    """Validate one call's preprocessed inputs; nothing is launched.  -> (img, second input of the dense plan: the right
    images when `stereo`, else disp_postp, gt depth maps or None, stereo, the frames' ori_shape).  `who`: the entry
    point's name in the refusal of host tensors."""
    if getattr(model, 'rectify', None) is not None:
        check_rectify_inputs(model.rectify, inputs)
    img, disp_postp = _unwrap(inputs['img'], 'img'), inputs.get('disp_postp')
    assert len(data_samples) == len(img)
    if img.device.type != 'cuda':
        raise RuntimeError(f'{who} runs on the HIP path only: inputs must be CUDA tensors')
    stereo = disp_postp is None
    if stereo:
        if model.stereo is None or inputs.get('right') is None:
            raise KeyError("inputs need 'disp_postp', or 'right' with a stereo module configured")
        second = _unwrap(inputs['right'], 'right')
    else:
        second = _unwrap(disp_postp, 'disp_postp')
        if isinstance(second, RawFrames):
            second = second.dense()[:, 0]      # a uint8 disparity is unusual: convert it eagerly
    gt = _unwrap(inputs.get('depth_postp'), 'depth_postp')
    if isinstance(gt, RawFrames):
        gt = gt.dense()[:, 0]
    metas = [s.metainfo for s in data_samples]
    ori = uniform_ori_shape(metas, img.pad_hw if isinstance(img, RawFrames) else tuple(img.shape[-2:]))
    if stereo and isinstance(model.stereo, _sgbm.StereoSGBM):
        for m in metas:
            if 'img_shape' in m and _hw(m['img_shape']) != ori:
                raise NotImplementedError(
                    f"StereoSGBM matches at the original resolution: img_shape {tuple(m['img_shape'][:2])} differs "
                    f"from ori_shape {ori} (the reference matched before resizing; that order is not restated)")
    return img, second, gt, stereo, ori


def check_rectify_inputs(rect, inputs):
    """What a shell with `rectify` set takes: the stereo-input configuration (img + right) as raw uint8 frames of the
    calibration's size.  Everything else is refused here, before anything is launched."""
    if inputs.get('disp_postp') is not None:
        raise NotImplementedError("rectify is set but the inputs carry 'disp_postp': a disparity map is already in "
                                  "rectified coordinates and the raw image beside it is not; rectify applies to the "
                                  "stereo-input configuration ('img' + 'right')")
    for name in ('img', 'right'):
        t = inputs.get(name)
        if t is None:
            raise KeyError(f"rectify is set: the inputs need 'img' and 'right' (raw uint8 frames), '{name}' is missing")
        if not isinstance(t, RawFrames):
            raise NotImplementedError(f"rectify remaps raw uint8 frames (cv2.remap's 8-bit rule); '{name}' arrived as a "
                                      f"{getattr(t, 'dtype', type(t).__name__)} tensor - pass uint8 frames, or rectify "
                                      f"fp32 images before the call")
        if tuple(t.hw) != tuple(rect.size):
            raise ValueError(f"rectify: '{name}' frames are {tuple(t.hw)}, the calibration is for {tuple(rect.size)}")
    if len(inputs['img']) != len(inputs['right']):
        raise ValueError(f"rectify: {len(inputs['img'])} left frames, {len(inputs['right'])} right frames")


def rectified_chunk(rect, img, second, s, e):
    """Frames [s, e) of a raw stereo call, rectified: left and right frames in ONE st_rectify_remap launch on the current
    stream -> two RawFrames of e - s frames (views of one uint8 block), read by the raw stem and StereoSGBM unchanged."""
    left, right = rect.rectify_pairs(img.frames[s:e], second.frames[s:e])
    return RawFrames(left, img.pad_hw, img.pad_value), RawFrames(right, second.pad_hw, second.pad_value)


def padded(t, s, e, B):
    """frames [s, e) of a call's input as a (B, C, H, W) fp32 batch."""
    if isinstance(t, RawFrames):
        return t.chunk(s, e, B)
    t = t[s:e].float().contiguous()
    if e - s < B:      # last chunk: repeat its last frame (results of the padding are ignored)
        t = torch.cat([t, t[-1:].expand(B - (e - s), *t.shape[1:])])
    return t


def chunk_inputs(model, img, second, stereo, s, e, B, runner):
    """Frames [s, e) of a planned call -> the two inputs (a, b) of `runner.submit`.  With model.rectify set the chunk's
    raw pairs are rectified first, under the stream of the context the chunk is submitted to (so the pass is part of
    that context's pipelined work and overlaps the dense work of the other contexts)."""
    rect = getattr(model, 'rectify', None)
    if rect is None:
        return _chunk_inputs(model, img, second, stereo, s, e, B, runner)
    ctx = runner.next_stream(img.device)
    ctx.wait_stream(torch.cuda.current_stream(img.device))       # the raw frames were uploaded on the caller's stream
    for f in img.frames[s:e] + second.frames[s:e]:
        f.record_stream(ctx)
    with torch.cuda.stream(ctx):
        img, second = rectified_chunk(rect, img, second, s, e)
        return _chunk_inputs(model, img, second, stereo, 0, e - s, B, runner)


def _chunk_inputs(model, img, second, stereo, s, e, B, runner):
    a = b = None
    if model.raw_stem and isinstance(img, RawFrames):
        if stereo and isinstance(second, RawFrames):
            a, b = img.raw_chunk(s, e, B, runner), second.raw_chunk(s, e, B, runner)
        elif not stereo:      # disparity-input configuration: the image raw, the fp32 disparity as it is
            a = img.raw_chunk(s, e, B, runner)
            b = padded(second, s, e, B) if a is not None else None
    if a is None or b is None:      # fp32 tensors (or frames the stem cannot read raw): cast + pad as a pass of its own
        a, b = padded(img, s, e, B), padded(second, s, e, B)
    return a, b
