"""StereoRectify - from a stereo rig's calibration to rectified frames on the device (csrc/rectify.hip).

StereoCostVolume, StereoSGBM and the shell's `right` input assume RECTIFIED pairs (no distortion, horizontal epipolar
lines); the reference's AirSim renders are.  A physical rig delivers distorted, slightly rotated frames plus a
calibration.  This module turns the calibration into fixed-point maps ON THE HOST (numpy fp64, once) and remaps the
frames ON THE DEVICE (st_rectify_remap: left and right frames of a chunk in one launch).

OpenCV is absent: the map rule (cv2.initUndistortRectifyMap), the sampling rule (cv2.remap, 8-bit INTER_LINEAR on
CV_16SC2 maps) and Bouguet's construction (cv2.stereoRectify) are restated from OpenCV 4.x [upstream-memory]; parity
with cv2 itself is unpinned.  tests/rectify_ref.py is the independent numpy restatement of the sampling rule, DESIGN.md
"Stereo rectification" lists the rules.

Results of a rectified run (boxes, tracks) are in RECTIFIED-LEFT pixel coordinates; `to_raw_boxes` maps boxes back
into the raw left frame.
"""
import ctypes as C
import json

import numpy as np

from .registry import MODELS

MAP_BITS = 5
MAP_ONE = 1 << MAP_BITS          # a map unit is 1/32 px
MAP_OUTSIDE = -2 * MAP_ONE       # -64: x0 = -2, every tap outside the image
MAX_FRAMES = 32                  # frames of one st_rectify_remap launch (their pointers travel in the kernel arguments)
_CAMERA_KEYS = ('K', 'D', 'R', 'P')


# ---- the float rule ------------------------------------------------------------------------------------------------------
def _dist8(D):
    """[k1, k2, p1, p2[, k3[, k4, k5, k6]]] -> the eight coefficients (k1, k2, p1, p2, k3, k4, k5, k6)."""
    d = np.asarray(D, np.float64).reshape(-1)
    if d.size not in (4, 5, 8):
        raise ValueError(f'D needs 4, 5 or 8 distortion coefficients (k1, k2, p1, p2[, k3[, k4, k5, k6]]), got {d.size}')
    return np.concatenate([d, np.zeros(8 - d.size)])


def undistort_rectify_points(K, D, R, P, u, v):
    """Rectified pixel (u, v) -> raw pixel (mx, my), fp64 - cv2.initUndistortRectifyMap's rule [upstream-memory]:
    [x y w] = (P[:, :3] R)^-1 [u v 1], x /= w, y /= w, r2 = x^2 + y^2,
    kr = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3),
    xd = x kr + 2 p1 x y + p2 (r2 + 2 x^2), yd = y kr + p1 (r2 + 2 y^2) + 2 p2 x y, mx = fx xd + cx, my = fy yd + cy."""
    K, R, P = np.asarray(K, np.float64), np.asarray(R, np.float64), np.asarray(P, np.float64)
    k1, k2, p1, p2, k3, k4, k5, k6 = _dist8(D)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    iR = np.linalg.inv(P[:, :3] @ R)
    with np.errstate(all='ignore'):
        x = iR[0, 0] * u + iR[0, 1] * v + iR[0, 2]
        y = iR[1, 0] * u + iR[1, 1] * v + iR[1, 2]
        w = iR[2, 0] * u + iR[2, 1] * v + iR[2, 2]
        x, y = x / w, y / w
        r2 = x * x + y * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        return K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]


def quantise(m, dim):
    """A float map coordinate -> int32 in 1/32 px: rint (ties to even) of 32 m, clipped to [-64, 32 (dim + 1)] - both
    ends have every tap outside the image - and a non-finite m sent to -64."""
    m = np.asarray(m, np.float64)
    with np.errstate(all='ignore'):
        q = np.rint(MAP_ONE * m)
    q = np.where(np.isfinite(m), q, float(MAP_OUTSIDE))
    return np.clip(q, float(MAP_OUTSIDE), float(MAP_ONE * (dim + 1))).astype(np.int32)


def build_map(K, D, R, P, size, out_size=None):
    """(h2, w2, 2) int32 map of (qx, qy) for one camera: raw frame `size` = (h, w), rectified `out_size` (= size)."""
    h, w = size
    h2, w2 = out_size or size
    v, u = np.meshgrid(np.arange(h2, dtype=np.float64), np.arange(w2, dtype=np.float64), indexing='ij')
    mx, my = undistort_rectify_points(K, D, R, P, u, v)
    return np.stack([quantise(mx, w), quantise(my, h)], axis=-1)


def map_valid_mask(qmap, size):
    """(h2, w2) bool: every tap of non-zero bilinear weight lies inside the raw image of `size` = (h, w)."""
    h, w = size
    q = np.asarray(qmap).astype(np.int64)
    x0, a, y0, b = q[..., 0] >> MAP_BITS, q[..., 0] & (MAP_ONE - 1), q[..., 1] >> MAP_BITS, q[..., 1] & (MAP_ONE - 1)
    okx = (x0 >= 0) & (x0 < w) & ((a == 0) | (x0 + 1 < w))
    oky = (y0 >= 0) & (y0 < h) & ((b == 0) | (y0 + 1 < h))
    return okx & oky


# ---- Bouguet's construction ----------------------------------------------------------------------------------------------
def _rodrigues_matrix(om):
    om = np.asarray(om, np.float64).reshape(3)
    th = float(np.linalg.norm(om))
    if th < 1e-300:
        return np.eye(3)
    k = om / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def _rodrigues_vector(R):
    R = np.asarray(R, np.float64)
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = np.linalg.norm(axis) / 2, (np.trace(R) - 1) / 2
    th = float(np.arctan2(s, c))
    if s < 1e-12:
        if c > 0:
            return axis / 2          # theta -> 0: the first-order term
        raise NotImplementedError('stereo_rectify: a relative rotation of 180 degrees is not a stereo rig')
    return axis / (2 * s) * th


def stereo_rectify(K1, D1, K2, D2, size, R, T, new_focal=None, new_center=None):
    """Rectifying rotations and projections of a rig known by its extrinsics (x2 = R x1 + T, camera 1 the left one):
    -> (R1, R2, P1, P2, Q).  Bouguet's construction [upstream-memory]: R is split into two half rotations (Rodrigues of
    -/+ om / 2), the baseline is rotated onto the x axis (its sign kept), both cameras get the SAME intrinsics
    f = new_focal or min(fy1, fy2), centre new_center or ((w - 1) / 2, (h - 1) / 2), and P2[0, 3] = f * t_x with
    t = R2 T = (-/+ |T|, 0, 0) (a left-first rig: P2[0, 3] = -f |T|).  Q reprojects (u, v, disparity, 1) to 3-D.

    This is a stated choice of new intrinsics, NOT a claim to equal cv2.stereoRectify's P matrices: its alpha / ROI
    scaling and its principal point from the undistorted corners are not restated.  Users who hold cv2's R1, R2, P1,
    P2 pass them to StereoRectify directly.  D1 / D2 only validate here (the new intrinsics do not depend on them).
    A rig whose baseline is closer to vertical than to horizontal raises NotImplementedError."""
    K1, K2 = np.asarray(K1, np.float64), np.asarray(K2, np.float64)
    R, T = np.asarray(R, np.float64), np.asarray(T, np.float64).reshape(-1)
    if K1.shape != (3, 3) or K2.shape != (3, 3) or R.shape != (3, 3) or T.shape != (3,):
        raise ValueError('stereo_rectify: K1, K2, R must be 3x3 and T a 3-vector')
    _dist8(D1), _dist8(D2)
    h, w = size
    om = _rodrigues_vector(R)
    r_r = _rodrigues_matrix(-0.5 * om)            # each camera turns half of R towards the other
    t = r_r @ T
    if abs(t[1]) >= abs(t[0]):
        raise NotImplementedError('stereo_rectify: the baseline is closer to vertical than to horizontal; vertical '
                                  'stereo is not implemented')
    nt = float(np.linalg.norm(t))
    uu = np.array([1.0 if t[0] > 0 else -1.0, 0.0, 0.0])
    ww = np.cross(t, uu)
    nw = float(np.linalg.norm(ww))
    if nw > 0:
        ww = ww * (np.arccos(min(1.0, abs(t[0]) / nt)) / nw)
    wR = _rodrigues_matrix(ww)
    R1, R2 = wR @ r_r.T, wR @ r_r
    tx = float((R2 @ T)[0])
    f = float(new_focal) if new_focal is not None else float(min(K1[1, 1], K2[1, 1]))
    cx, cy = new_center if new_center is not None else ((w - 1) / 2.0, (h - 1) / 2.0)
    P1 = np.array([[f, 0, cx, 0], [0, f, cy, 0], [0, 0, 1, 0]], np.float64)
    P2 = P1.copy()
    P2[0, 3] = f * tx
    Q = np.array([[1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, 0, f], [0, 0, -1.0 / tx, 0]], np.float64)
    return R1, R2, P1, P2, Q


# ---- the module ----------------------------------------------------------------------------------------------------------
def _camera(cfg, name):
    if not isinstance(cfg, dict):
        raise ValueError(f'StereoRectify: {name} must be a dict with the keys K, D, R, P')
    if set(cfg) != set(_CAMERA_KEYS):
        raise ValueError(f'StereoRectify: {name} needs exactly the keys K, D, R, P, got {sorted(cfg)}')
    try:
        K, R, P = (np.asarray(cfg[k], np.float64) for k in ('K', 'R', 'P'))
    except (TypeError, ValueError) as e:
        raise ValueError(f'StereoRectify: {name}: {e}') from None
    if K.shape != (3, 3) or R.shape != (3, 3) or P.shape != (3, 4):
        raise ValueError(f'StereoRectify: {name}: K and R must be 3x3 and P 3x4, got {K.shape}, {R.shape}, {P.shape}')
    try:
        D = _dist8(cfg['D'])
    except (TypeError, ValueError) as e:
        raise ValueError(f'StereoRectify: {name}: {e}') from None
    if not all(np.isfinite(m).all() for m in (K, D, R, P)) or abs(np.linalg.det(P[:, :3] @ R)) < 1e-300:
        raise ValueError(f'StereoRectify: {name}: the calibration must be finite and P[:, :3] R invertible')
    return dict(K=K, D=D, R=R, P=P)


def _hw(v, name):
    try:
        h, w = (int(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(f'StereoRectify: {name} must be (h, w)') from None
    if h < 1 or w < 1:
        raise ValueError(f'StereoRectify: {name} must be positive, got {(h, w)}')
    return h, w


@MODELS.register_module()
class StereoRectify:
    """dict(type='StereoRectify', left=dict(K=3x3, D=[k1, k2, p1, p2[, k3[, k4, k5, k6]]], R=3x3, P=3x4),
    right=dict(...), size=(h, w), out_size=None, border=0), or calibration='file.json' holding `left`, `right` (and
    optionally size / out_size / border; arguments given next to it win).  R / P are a camera's rectifying rotation and
    new projection matrix (cv2.stereoRectify's R1, P1 / R2, P2, or `stereo_rectify` below).

    maps            (2, h2, w2, 2) int32: (qx, qy) in 1/32 px of the left [0] and the right [1] camera, built once
    focal_length    P_left[0, 0];   baseline  -P_right[0, 3] / P_right[0, 0]
    valid_mask(c)   (h2, w2) bool of camera c ('left' / 'right'): every tap of non-zero weight inside the raw image
    to_raw_boxes    rectified-left xyxy boxes -> bounding boxes in the raw left frame (host helper)
    remap / rectify_pairs   the device pass (st_rectify_remap); the maps are uploaded once per device"""

    def __init__(self, left=None, right=None, size=None, out_size=None, border=0, calibration=None):
        if calibration is not None:
            with open(calibration) as f:
                cal = json.load(f)
            if not isinstance(cal, dict) or not set(cal) <= {'left', 'right', 'size', 'out_size', 'border'}:
                raise ValueError(f'StereoRectify: {calibration} must hold a dict of left, right[, size, out_size, border]')
            left = cal.get('left') if left is None else left
            right = cal.get('right') if right is None else right
            size = cal.get('size') if size is None else size
            out_size = cal.get('out_size') if out_size is None else out_size
            border = cal.get('border', border)
        if left is None or right is None or size is None:
            raise ValueError('StereoRectify needs left, right and size (as arguments or in the calibration file)')
        self.left, self.right = _camera(left, 'left'), _camera(right, 'right')
        self.size = _hw(size, 'size')
        self.out_size = self.size if out_size is None else _hw(out_size, 'out_size')
        if isinstance(border, bool) or int(border) != border or not 0 <= int(border) <= 255:
            raise ValueError(f'StereoRectify: border must be an integer in [0, 255], got {border!r}')
        self.border = int(border)
        self.maps = np.stack([build_map(size=self.size, out_size=self.out_size, **c) for c in (self.left, self.right)])
        self._dev_maps = {}

    def _cam(self, camera):
        if camera not in ('left', 'right'):
            raise ValueError(f"camera must be 'left' or 'right', got {camera!r}")
        return (self.left, 0) if camera == 'left' else (self.right, 1)

    @property
    def focal_length(self):
        return float(self.left['P'][0, 0])

    @property
    def baseline(self):
        return float(-self.right['P'][0, 3] / self.right['P'][0, 0])

    def float_map(self, camera, u, v):
        """Raw pixel (mx, my) of rectified pixel (u, v) of `camera`: the unquantised rule, fp64."""
        return undistort_rectify_points(u=u, v=v, **self._cam(camera)[0])

    def valid_mask(self, camera='left'):
        return map_valid_mask(self.maps[self._cam(camera)[1]], self.size)

    def to_raw_boxes(self, boxes_xyxy):
        """(n, 4) xyxy boxes in rectified-left pixels -> (n, 4) fp64 in the RAW left frame: the bounding box of the
        four corners and the four edge midpoints pushed through the float rule."""
        b = np.asarray(boxes_xyxy, np.float64).reshape(-1, 4)
        x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        xm, ym = (x1 + x2) / 2, (y1 + y2) / 2
        u = np.stack([x1, xm, x2, x1, x2, x1, xm, x2], axis=1)
        v = np.stack([y1, y1, y1, ym, ym, y2, y2, y2], axis=1)
        mx, my = self.float_map('left', u, v)
        return np.stack([mx.min(1), my.min(1), mx.max(1), my.max(1)], axis=1)

    # ---- device ----------------------------------------------------------------------------------------------------------
    def device_maps(self, device):
        import torch
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('StereoRectify remaps on the HIP path only: frames must be CUDA tensors')
        key = (device.type, torch.cuda.current_device() if device.index is None else device.index)
        m = self._dev_maps.get(key)
        if m is None:
            m = self._dev_maps[key] = torch.from_numpy(np.ascontiguousarray(self.maps)).to(device)
        return m

    def remap(self, frames, map_index, bilinear=True, out=None):
        """One st_rectify_remap launch on the current stream: `frames` = F <= 32 contiguous planar (P, h, w) /
        (1, P, h, w) CUDA tensors of one dtype and size, map_index[f] = 0 (left) or 1 (right) -> one (F, P, h2, w2) block
        (`out` or a new tensor).  bilinear: uint8 only; False = nearest for 1-, 2- and 4-byte elements."""
        import torch
        from . import _lib
        f0 = frames[0]
        F, (h, w), (h2, w2) = len(frames), self.size, self.out_size
        if not 1 <= F <= MAX_FRAMES or len(map_index) != F:
            raise ValueError(f'StereoRectify.remap: 1..{MAX_FRAMES} frames and one map index each, got {F} / {len(map_index)}')
        if f0.dim() < 3 or f0.numel() != f0.shape[-3] * h * w or tuple(f0.shape[-2:]) != (h, w) or f0.shape[-3] not in (1, 3):
            raise ValueError(f'StereoRectify.remap: frames must be (P, {h}, {w}) with P in (1, 3), got {tuple(f0.shape)}')
        for f in frames:
            if not (f.is_cuda and f.is_contiguous() and f.dtype == f0.dtype and f.shape == f0.shape and f.device == f0.device):
                raise ValueError('StereoRectify.remap: frames must be contiguous CUDA tensors of one dtype, size and device')
        P = int(f0.shape[-3])
        if out is None:
            out = torch.empty(F, P, h2, w2, dtype=f0.dtype, device=f0.device)
        elif not (out.is_contiguous() and out.dtype == f0.dtype and out.numel() == F * P * h2 * w2 and out.device == f0.device):
            raise ValueError(f'StereoRectify.remap: out must be a contiguous ({F}, {P}, {h2}, {w2}) block of the frames\' dtype')
        maps = self.device_maps(f0.device)
        src = (C.c_void_p * F)(*[f.data_ptr() for f in frames])
        idx = (C.c_int * F)(*[int(i) for i in map_index])
        _lib.check(_lib.load().st_rectify_remap(src, F, P, h, w, _lib.ptr(maps), int(maps.shape[0]), idx, None, _lib.ptr(out),
                                                h2, w2, f0.element_size(), 1 if bilinear else 0, self.border,
                                                _lib.current_stream()), 'st_rectify_remap')
        return out

    def rectify_pairs(self, left, right):
        """n <= 16 left and n right uint8 frames -> (list of n rectified left, list of n rectified right (1, 3, h2, w2)
        views of ONE block), in one launch on the current stream."""
        n = len(left)
        out = self.remap(list(left) + list(right), [0] * n + [1] * len(right))
        return [out[i:i + 1] for i in range(n)], [out[i:i + 1] for i in range(n, n + len(right))]
