"""Executable spec of the per-box depth estimators (csrc/box_depth.hip): the four alternatives of st_box_depth_method -
the reference's depth-extraction comparison (mmtrack/models/mot/depth_extraction_comparison.py: truncated_mean_decorator,
mean_decorator, median_decorator, center_decorator) - and the default estimator of st_box_depth (DEFAULT = 'reference',
mmtrack/models/mot/ocsort_disparity.py extract_depth; line-by-line restatement: oracle/depth.py), restated in numpy from
the rules below.  DESIGN.md section 11.

Front end, shared with the default extract_depth (oracle/depth.py):
  R1  depth map: disparity input -> depth = (float32(1) / (disp + float32(1e-6))) * float32(baseline * focal): an fp32
      IEEE reciprocal, then the product (two roundings).  torch evaluates `python_float / tensor` as
      tensor.reciprocal() * python_float, so this is the reference's disp2depth bit for bit
      (tests/golden/reference/depth.npz); one divide bf / (disp + 1e-6) is 1 ulp away on about one pixel in four;
      gt-depth input (baseline < 0 at the ABI) -> the raw map as given.  Channel 0 of (C, H, W), H x W = the padded
      map the model holds.
  R2  box.astype(np.int): every coordinate truncated toward zero.
  R3  window = depth[y1:y2, x1:x2] with Python slice rules (negative indices wrap once, out of range clamps, start >=
      stop is empty).
  R4  valid pixels v = window[(window < 150) & (window > 0)], n = len(v), s = sort(v).
  R5  n < 1 or (x2 - x1) > 800 -> depth -1, scale 1.0.
Values (n >= 1 and w <= 800):
  R6  truncated_mean: s[int(0.1 n) : int((1 - 0.1) n)] with the bounds computed in doubles; if that is empty,
      s[:-1]; its mean.  Only n == 1 is still empty after the fallback: NaN (np.mean of an empty slice).
  R7  mean: mean(v).
  R8  median: np.median(v) = s[n // 2] for odd n; for even n (s[n/2 - 1] + s[n/2]) added in fp32, then halved.
  R9  center: depth[cy, cx] of the RAW map (no validity filter), cx = (x1 + x2) // 2, cy = (y1 + y2) // 2 (floor
      division of the truncated ints); a negative index wraps once as in numpy.  Still gated by R5.
  R10 (stated deviation) center index out of range after the wrap: numpy raises IndexError; here depth -1, scale 1.0.
      Unscaled Kalman track boxes can reach past the map.
  R11 means (R6, R7) are accumulated in float64 and rounded to float32 once.  numpy sums float32 pairwise in
      float32; the device accumulates in float64 too, and may differ from this restatement by 1 fp32 ulp (the order
      of the float64 sum).
Scale:
  R12 scale = max(min(d * d / 400, 3.), 1.) with Python's min / max: NaN passes through both.
  R13 (uncertain) numpy promotion: the reference pins numpy < 1.24, where d is an np.float32 scalar, d * d an
      np.float32 product, and `/ 400` (all-scalar operands, Python int) promotes to float64.  So: float32 product,
      float64 quotient, float64 clamps, float32 when the list becomes a tensor.  NumPy >= 2 (NEP 50) would keep
      float32 for the quotient; this restatement spells the legacy reading out and does not depend on the
      installed numpy.
The default estimator ('reference'; n >= 1 and w <= 800, front end R1-R5):
  R14 mid = s[n // 2] (the upper middle element for even n; not np.median).
  R15 four corner means on the RAW map (no validity filter): depth[y1:y1+2, x1:x1+2], depth[y1:y1+2, x2-2:x2],
      depth[y2-2:y2, x1:x1+2], depth[y2-2:y2, x2-2:x2], Python slice rules on the literal bounds (x1 = -3 wraps to two
      columns, x1 in (-2, -1) and x2 in (0, 1) give an empty slice, an edge clamps to one row / column).  An empty slice
      gives NaN.  The mean is float32, summed in row-major sequential order ((a + b) + c) + d, then / count: what np.mean
      of the 2 x 2 view computes (checked on numpy 2.2.6; the pairwise order (a + b) + (c + d) differs on 24 % of
      random blocks).
  R16 cnt = the number of corner means > mid (strict; NaN > mid is False).
  R17 w_start = min(1 - cnt / 4, 0.4) * n, w_end = w_start + 0.6 * n, both in Python doubles: the fraction is 0.4 for
      cnt <= 2, 0.25 for cnt == 3 and 0 for cnt == 4.  seg = s[int(w_start):int(w_end)]; if that is empty, s[:-1]; if
      that is empty too, NaN.  (Only n == 1 with cnt >= 3 is empty, and then s[:-1] is empty as well.)  The bounds do
      not depend on floating-point contraction: int(w_start + 0.6 * n) evaluated with one fused multiply-add gives the
      same integer for every n < 200 000 and all three fractions (tests/test_cpu_box_depth_ref.py re-checks a part).
      Ties need no rule of their own: the slice holds a value tied with s[a] or s[b - 1] exactly as often as the sorted
      positions [a, b) do.
  R18 value = float64 sum of seg / len(seg), rounded to float32 once (R11).
  R19 scale = max(min(d * d, 3.), 1.): float32 product, Python min / max, so NaN passes through (scale_of_default).
"""
from collections import namedtuple

import numpy as np

METHODS = ('truncated_mean', 'mean', 'median', 'center')
DEFAULT = 'reference'
MAX_DEPTH = 150
MAX_WIDTH = 800


def depth_map(disp, baseline=0.25, focal=640.0, is_depth=False):
    """R1: (H, W) float32 depth of a disparity map (or the gt-depth map itself)."""
    d = np.asarray(disp, np.float32)
    if is_depth:
        return d
    bf = np.float32(float(baseline) * float(focal))
    return ((np.float32(1.0) / (d + np.float32(1e-6))) * bf).astype(np.float32)


def _mean64(a):
    """R11: float64 accumulation, one rounding."""
    return np.float32(np.sum(a, dtype=np.float64) / len(a))


# What value(..., trace=True) adds for the default estimator: the corner count, the number of valid depths, the
# segment [a, b) of s that was averaged (after the fallback; a == b for the NaN row), whether the s[:-1] fallback was
# taken, the number of window pixels, the box width x2 - x1, and s itself.  cnt is None for a (-1, 1.0) row.
Trace = namedtuple('Trace', 'cnt n a b fallback window width s')


def corner_mean(block):
    """R15: float32 mean of a (<= 2) x (<= 2) view in row-major sequential order; NaN for an empty view."""
    if block.size == 0:
        return np.float32(np.nan)
    acc = np.float32(0.0)
    with np.errstate(over='ignore', invalid='ignore'):
        for v in block.ravel():                                               # ravel of a view: row-major
            acc = np.float32(acc + v)
        return np.float32(acc / np.float32(block.size))


def _default_value(depth, s, n, x1, y1, x2, y2):
    """R14-R18 -> (float32 value, cnt, a, b, fallback)."""
    mid = s[n // 2]                                                           # R14
    corners = [corner_mean(depth[y1:y1 + 2, x1:x1 + 2]), corner_mean(depth[y1:y1 + 2, x2 - 2:x2]),      # R15
               corner_mean(depth[y2 - 2:y2, x1:x1 + 2]), corner_mean(depth[y2 - 2:y2, x2 - 2:x2])]
    cnt = sum(bool(c > mid) for c in corners)                                 # R16
    w_start = min(1 - cnt / 4, 0.4) * n                                       # R17
    w_end = w_start + 0.6 * n
    a, b = min(int(w_start), n), min(int(w_end), n)
    fallback = b <= a
    if fallback:
        a, b = 0, n - 1
    if b <= a:
        return np.float32(np.nan), cnt, a, a, fallback
    return _mean64(s[a:b]), cnt, a, b, fallback                               # R18


def value(depth, box, method, trace=False):
    """R2-R10, R14-R18 for one box -> (float32 depth value, estimated?)  estimated False = the (-1, 1.0) row.
    trace=True (the default estimator only) appends a Trace."""
    H, W = depth.shape
    x1, y1, x2, y2 = (int(c) for c in np.asarray(box, np.float32))          # R2: int() truncates toward zero
    win = depth[y1:y2, x1:x2]                                                 # R3
    v = win[(win < MAX_DEPTH) & (win > 0)]                                    # R4
    n = len(v)
    if n < 1 or (x2 - x1) > MAX_WIDTH:                                        # R5
        if trace:
            return np.float32(-1.0), False, Trace(None, n, 0, 0, False, win.size, x2 - x1, np.sort(v))
        return np.float32(-1.0), False
    if method == DEFAULT:
        s = np.sort(v)
        d, cnt, a, b, fallback = _default_value(depth, s, n, x1, y1, x2, y2)
        if trace:
            return d, True, Trace(cnt, n, a, b, fallback, win.size, x2 - x1, s)
        return d, True
    if method == 'center':                                                    # R9
        cx, cy = (x1 + x2) // 2, (y1 + y2) // 2
        cx, cy = cx + W if cx < 0 else cx, cy + H if cy < 0 else cy
        if not (0 <= cx < W and 0 <= cy < H):                                 # R10
            return np.float32(-1.0), False
        return np.float32(depth[cy, cx]), True
    if method == 'mean':                                                      # R7
        return _mean64(v), True
    s = np.sort(v)
    if method == 'median':                                                    # R8
        if n % 2:
            return np.float32(s[n // 2]), True
        return np.float32(np.float32(s[n // 2 - 1]) + np.float32(s[n // 2])) / np.float32(2), True
    if method == 'truncated_mean':                                            # R6
        seg = s[int(0.1 * n):int((1 - 0.1) * n)]
        if len(seg) == 0:
            seg = s[:-1]
        if len(seg) == 0:
            return np.float32(np.nan), True
        return _mean64(seg), True
    raise ValueError(f'unknown method {method!r}')


def scale_of(d):
    """R12-R13: float32 product, float64 quotient and clamps (Python min / max), float32 result."""
    d = np.float32(d)
    with np.errstate(over='ignore', invalid='ignore'):
        dd = np.float32(d * d)
    s = float(dd) / 400.0
    s = min(s, 3.)
    s = max(s, 1.)
    return np.float32(s)


def scale_of_default(d):
    """R19: float32 product, Python min / max (NaN passes through both), float32 result."""
    d = np.float32(d)
    with np.errstate(over='ignore', invalid='ignore'):
        s = float(np.float32(d * d))
    s = min(s, 3.)
    s = max(s, 1.)
    return np.float32(s)


def extract_depth(depth, boxes, method):
    """(H, W) float32 depth map, (M, 4) boxes -> depth values (M,) float32, scales (M,) float32."""
    vals, scales = [], []
    scale = scale_of_default if method == DEFAULT else scale_of
    for box in np.asarray(boxes, np.float32).reshape(-1, 4):
        d, ok = value(depth, box, method)
        vals.append(d)
        scales.append(scale(d) if ok else np.float32(1.0))
    return np.asarray(vals, np.float32), np.asarray(scales, np.float32)


def scale_bbox(boxes, scales):
    """trackers/utils.py:58-73 in float32 (what the kernel writes as the scaled boxes)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    sc = np.asarray(scales, np.float32)
    two = np.float32(2.0)
    cx, cy = (b[:, 0] + b[:, 2]) / two, (b[:, 1] + b[:, 3]) / two
    w, h = (b[:, 2] - b[:, 0]) * sc, (b[:, 3] - b[:, 1]) * sc
    return np.stack([cx - w / two, cy - h / two, cx + w / two, cy + h / two], axis=1).astype(np.float32)
