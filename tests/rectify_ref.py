"""Numpy restatement of the remap rule of st_rectify_remap (test infrastructure, the executable spec; it imports nothing
from stereotracking_amd.rectify).  int64 arithmetic, fancy indexing with explicit masks.

A map cell (qx, qy) is in 1/32 px.  With floor division / modulo (= arithmetic shift / mask on two's complement):
  x0 = qx // 32, a = qx % 32, y0 = qy // 32, b = qy % 32
  bilinear (uint8):  out = ((32-a)(32-b) p00 + a(32-b) p01 + (32-a)b p10 + ab p11 + 512) // 1024
                     p.. = the taps at (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1); outside the image: border
  nearest:           the element at ((qx + 16) // 32, (qy + 16) // 32); outside: border (1-byte elements) or 0
cv2.remap's 8-bit INTER_LINEAR over CV_16SC2 maps [upstream-memory; cv2 absent: parity unpinned]."""
import numpy as np


def _tap(plane, xs, ys, border):
    h, w = plane.shape
    inside = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
    vals = plane[np.where(inside, ys, 0), np.where(inside, xs, 0)].astype(np.int64)
    return np.where(inside, vals, np.int64(border)), inside


def taps_read(qmap, h, w):
    """(h2, w2, 4) bool: which of the four taps a bilinear remap READS - inside the image and of non-zero weight."""
    q = np.asarray(qmap).astype(np.int64)
    x0, a, y0, b = q[..., 0] // 32, q[..., 0] % 32, q[..., 1] // 32, q[..., 1] % 32
    out = []
    for dx, dy, wt in ((0, 0, (32 - a) * (32 - b)), (1, 0, a * (32 - b)), (0, 1, (32 - a) * b), (1, 1, a * b)):
        xs, ys = x0 + dx, y0 + dy
        out.append((xs >= 0) & (xs < w) & (ys >= 0) & (ys < h) & (wt != 0))
    return np.stack(out, axis=-1)


def remap(frame, qmap, bilinear=True, border=0):
    """frame (P, h, w) of uint8 (bilinear) or any 1- / 2- / 4-byte dtype (nearest); qmap (h2, w2, 2) int -> (P, h2, w2)."""
    frame = np.asarray(frame)
    q = np.asarray(qmap).astype(np.int64)
    qx, qy = q[..., 0], q[..., 1]
    out = np.empty((frame.shape[0],) + q.shape[:2], frame.dtype)
    if bilinear:
        assert frame.dtype == np.uint8
        x0, a, y0, b = qx // 32, qx % 32, qy // 32, qy % 32
        for p, plane in enumerate(frame):
            acc = np.full(q.shape[:2], 512, np.int64)
            for dx, dy, wt in ((0, 0, (32 - a) * (32 - b)), (1, 0, a * (32 - b)), (0, 1, (32 - a) * b), (1, 1, a * b)):
                acc += wt * _tap(plane, x0 + dx, y0 + dy, border)[0]
            out[p] = (acc // 1024).astype(np.uint8)
        return out
    sx, sy = (qx + 16) // 32, (qy + 16) // 32
    outside = border if frame.dtype.itemsize == 1 else 0
    for p, plane in enumerate(frame):
        h, w = plane.shape
        inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        vals = plane[np.where(inside, sy, 0), np.where(inside, sx, 0)]
        out[p] = np.where(inside, vals, np.asarray(outside, frame.dtype))
    return out
