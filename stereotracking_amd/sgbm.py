"""StereoSGBM - OpenCV's StereoSGBM in mode SGBM_3WAY on the device (csrc/sgbm.hip), from uint8 left / right frames.

The reference's two-branch detector was trained on disparity PNGs that OpenCV StereoSGBM made offline with one fixed
configuration (reproducibility.md section 3; the defaults below).  This module computes that map from raw stereo
frames and writes `disp_postp` with the meaning the PNG loader gives it (LoadDisparityFromFile: invalid -> 0, values
/ 16, three identical channels, 0 in the padding), so the shipped stereo detector runs on live left / right video.

OpenCV is absent: the rules are restated from OpenCV 4.x [upstream-memory] and listed in tests/sgbm_ref.py (the numpy
restatement, the executable spec) and DESIGN.md "Stereo SGBM"; parity with cv2 itself is unpinned.  The image is one
stripe (OpenCV run with setNumThreads(1)); a multi-threaded cv2 restarts the top->bottom path per row stripe.
"""
import ctypes as C

import torch
from torch import nn

from . import _lib
from ._lib import StSgbmParams, check, current_stream, ptr
from .engine import RawChunk, _require_cuda
from .registry import MODELS

INT16_MAX = 32767
NUM_DISPARITIES = (16, 32, 48, 64, 128, 192, 256)


def ftzero_of(pre_filter_cap):
    return max(int(pre_filter_cap), 15) | 1


@MODELS.register_module()
class StereoSGBM(nn.Module):
    """Launcher with no parameters and no CPU forward.  compute() fills a (N, 3, H, W) disp_postp from N pairs.

    num_disparities: 16, 32, 48 or 64 (one level per lane of a wave) or 128, 192 or 256 (2, 3 or 4 levels per lane; the
    two cost volumes take 2 * 2 * N * h * (w - D) * D bytes of the workspace).  min_disparity is 0 and the mode SGBM_3WAY."""

    def __init__(self, min_disparity=0, num_disparities=48, block_size=3, P1=96, P2=384, disp12_max_diff=0,
                 uniqueness_ratio=10, speckle_window_size=400, speckle_range=10, pre_filter_cap=63, mode='SGBM_3WAY',
                 color=True):
        super().__init__()
        if mode != 'SGBM_3WAY':
            raise NotImplementedError(f"StereoSGBM: only mode='SGBM_3WAY' is implemented (got {mode!r})")
        if min_disparity != 0:
            raise NotImplementedError(f'StereoSGBM: only min_disparity=0 is implemented (got {min_disparity})')
        if num_disparities not in NUM_DISPARITIES:
            raise ValueError(f'StereoSGBM: num_disparities must be 16, 32, 48 or 64 (one level per lane of a wave) or '
                             f'128, 192 or 256 (whole 64-level slots: 2, 3 or 4 levels per lane), got {num_disparities}')
        if block_size < 1 or block_size % 2 != 1:
            raise ValueError(f'StereoSGBM: block_size must be odd and >= 1, got {block_size}')
        if not 1 <= pre_filter_cap <= 127:
            raise ValueError(f'StereoSGBM: pre_filter_cap must be in 1..127, got {pre_filter_cap}')
        if P1 < 0 or P2 < 0 or speckle_window_size < 0 or speckle_range < 0:
            raise ValueError('StereoSGBM: P1, P2, speckle_window_size and speckle_range must be >= 0')
        if not 0 <= uniqueness_ratio < 100:
            raise ValueError(f'StereoSGBM: uniqueness_ratio must be in 0..99, got {uniqueness_ratio}')
        cn = 3 if color else 1
        p2 = max(int(P2), int(P1) + 1)
        worst = 3 * (block_size ** 2 * cn * (2 * ftzero_of(pre_filter_cap) + 63) + p2)
        if worst > INT16_MAX:
            raise ValueError(f'StereoSGBM: worst-case aggregated cost {worst} leaves int16 (> {INT16_MAX}); OpenCV '
                             f'wraps around there and that is not restated.  Lower block_size, P2 or pre_filter_cap')
        self.min_disparity, self.num_disparities, self.block_size = 0, int(num_disparities), int(block_size)
        self.P1, self.P2, self.disp12_max_diff = int(P1), int(P2), int(disp12_max_diff)
        self.uniqueness_ratio, self.pre_filter_cap = int(uniqueness_ratio), int(pre_filter_cap)
        self.speckle_window_size, self.speckle_range = int(speckle_window_size), int(speckle_range)
        self.mode, self.color = mode, bool(color)
        self._ws = {}
        self.last_status = None

    def config(self):
        """The constructor arguments (a copy builds an independent module with its own workspace)."""
        return dict(min_disparity=0, num_disparities=self.num_disparities, block_size=self.block_size, P1=self.P1,
                    P2=self.P2, disp12_max_diff=self.disp12_max_diff, uniqueness_ratio=self.uniqueness_ratio,
                    speckle_window_size=self.speckle_window_size, speckle_range=self.speckle_range,
                    pre_filter_cap=self.pre_filter_cap, mode=self.mode, color=self.color)

    def forward(self, *args, **kwargs):
        raise RuntimeError('StereoSGBM has no CPU forward: call compute() with CUDA tensors')

    def params(self):
        return StSgbmParams(C.sizeof(StSgbmParams), self.num_disparities, self.block_size, self.P1, self.P2,
                            self.disp12_max_diff, self.uniqueness_ratio, self.speckle_window_size, self.speckle_range,
                            self.pre_filter_cap, int(self.color))

    def workspace(self, dev, N, h, w):
        """(workspace uint8 tensor, status int32 (1,)) owned per device and batch geometry."""
        if w <= self.num_disparities:
            raise ValueError(f'StereoSGBM: image width {w} must exceed num_disparities {self.num_disparities}')
        key = (str(dev), int(N), int(h), int(w))
        if key not in self._ws:
            nbytes = _lib.load().st_sgbm_workspace_bytes(N, h, w, self.num_disparities)
            self._ws[key] = (torch.empty(nbytes, dtype=torch.uint8, device=dev),
                             torch.zeros(1, dtype=torch.int32, device=dev))
        return self._ws[key]

    def compute(self, left, right, valid_hw, disp_postp):
        """left / right: RawChunk (N uint8 (3, h, w) frames each) or padded fp32 (N, 3, H, W) CUDA batches (integral
        values, the top-left valid_hw matched).  disp_postp: (N, 3, H, W) fp32, written in full.  Enqueued on the
        current stream; no host sync."""
        lib = _lib.load()
        h, w = int(valid_hw[0]), int(valid_hw[1])
        _require_cuda(disp_postp, 'disp_postp')
        N, _, H, W = disp_postp.shape
        if h > H or w > W:
            raise ValueError(f'valid_hw {valid_hw} exceeds the output ({H}, {W})')
        prm = self.params()
        if isinstance(left, RawChunk):
            if not isinstance(right, RawChunk) or len(left) != N or len(right) != N:
                raise ValueError('StereoSGBM: left and right must both be RawChunks of N frames (or both fp32 batches)')
            if left.hw != right.hw or h > left.hw[0] or w > left.hw[1]:
                raise ValueError(f'StereoSGBM: frame sizes {left.hw} / {right.hw} do not cover valid_hw {valid_hw}')
            ws, status = self.workspace(disp_postp.device, N, h, w)
            check(lib.st_sgbm_u8(left.table(), right.table(), N, left.hw[0], left.hw[1], h, w, C.byref(prm), ptr(ws),
                                 ws.numel(), ptr(disp_postp), H, W, ptr(status), current_stream()), 'st_sgbm_u8')
            self.last_status = status
        else:
            for t, nm in ((left, 'left'), (right, 'right')):
                _require_cuda(t, nm)
                if tuple(t.shape) != (N, 3, H, W):
                    raise ValueError(f'{nm} must be (N, 3, H, W) = {(N, 3, H, W)}, got {tuple(t.shape)}')
            ws, status = self.workspace(disp_postp.device, N, h, w)
            check(lib.st_sgbm_f32(ptr(left), ptr(right), N, H, W, h, w, C.byref(prm), ptr(ws), ws.numel(),
                                  ptr(disp_postp), ptr(status), current_stream()), 'st_sgbm_f32')
            self.last_status = status     # device int32 (1,): 0 = the speckle filter's union-find converged
        return disp_postp

    # ---- stage entry points (tests, tools) ---------------------------------------------------------------------
    def match(self, left, right, valid_hw, cost=True):
        """fp32 batches -> (block-summed cost (N, h, w - D, D) int16 or None, int16 map (N, h, w) before the median)."""
        lib = _lib.load()
        h, w = int(valid_hw[0]), int(valid_hw[1])
        _require_cuda(left, 'left')
        _require_cuda(right, 'right')
        N, _, H, W = left.shape
        D = self.num_disparities
        ws, _ = self.workspace(left.device, N, h, w)
        c = torch.empty(N, h, w - D, D, dtype=torch.int16, device=left.device) if cost else None
        raw = torch.empty(N, h, w, dtype=torch.int16, device=left.device)
        check(lib.st_sgbm_match_f32(ptr(left), ptr(right), N, H, W, h, w, C.byref(self.params()), ptr(ws), ws.numel(),
                                    ptr(c), ptr(raw), current_stream()), 'st_sgbm_match_f32')
        return c, raw

    @staticmethod
    def median(disp):
        """int16 (N, h, w) -> 3 x 3 median."""
        out = torch.empty_like(disp)
        N, h, w = disp.shape
        check(_lib.load().st_sgbm_median(ptr(disp), N, h, w, ptr(out), current_stream()), 'st_sgbm_median')
        return out

    def speckle(self, disp):
        """int16 (N, h, w) -> (filterSpeckles result int16, status int32 (1,))."""
        N, h, w = disp.shape
        ws = torch.empty(2 * ((N * h * w * 4 + 255) // 256 * 256), dtype=torch.uint8, device=disp.device)
        out = torch.empty_like(disp)
        status = torch.empty(1, dtype=torch.int32, device=disp.device)
        check(_lib.load().st_sgbm_speckle(ptr(disp), N, h, w, self.speckle_window_size, 16 * self.speckle_range,
                                          ptr(ws), ws.numel(), ptr(out), None, 0, 0, ptr(status), current_stream()),
              'st_sgbm_speckle')
        return out, status
