"""Seeded inputs for the default per-box depth estimator (st_box_depth; rules R1-R5 and R14-R19 of
tests/depth_methods_ref.py), shared by tests/test_cpu_box_depth_ref.py (the restatement against oracle/depth.py,
coverage facts, mutants) and tests/test_box_depth_default_gpu.py (the kernel against the restatement).

A builder returns a tuple of Case: maps (N, C, H, W) float32, boxes (N, M, 4) float32, counts (N,) int32 and is_depth
(True: gt-depth input, baseline -1, the map's float32 values ARE the depths, so exact bit patterns can be placed; False:
disparity input, baseline 0.25, focal 640).  Every builder is cached and its arrays are read-only; reference(case) is
computed once per case.  Channels past the first hold other data: a wrong image pitch or channel shows."""
import functools
from collections import namedtuple

import numpy as np

import depth_methods_ref as R

BD_CACHE = 2560     # csrc/box_depth.hip: windows of up to BD_CACHE pixels are cached in LDS, larger ones are streamed
Case = namedtuple('Case', 'name maps boxes counts is_depth')
BUILDERS = ('branch_grid', 'tie_maps', 'strict_compare', 'radix_levels', 'geometry', 'near_depth')
ABOVE, BELOW = np.float32(1000.0), np.float32(-5.0)   # invalid raw values: above / not above any median


def _case(name, maps, boxes, counts, is_depth):
    maps = np.ascontiguousarray(maps, np.float32)
    boxes = np.ascontiguousarray(boxes, np.float32)
    counts = np.ascontiguousarray(counts, np.int32)
    assert maps.ndim == 4 and boxes.shape[0] == maps.shape[0] == len(counts) and boxes.shape[2] == 4
    for a in (maps, boxes, counts):
        a.setflags(write=False)
    return Case(name, maps, boxes, counts, is_depth)


def _channels(first, C, other=77.0):
    """(N, H, W) -> (N, C, H, W): channel 0 = the map, the others a constant valid value nobody may read."""
    out = np.full((first.shape[0], C) + first.shape[1:], other, np.float32)
    out[:, 0] = first
    return out


def _force_cnt(d, x1, y1, x2, y2, k, rot=0):
    """The four 2 x 2 corner blocks of the box hold invalid raw values: k of them (starting at corner `rot`) above any
    median, the rest below.  So cnt == k whatever the valid depths are."""
    blocks = [(y1, x1), (y1, x2 - 2), (y2 - 2, x1), (y2 - 2, x2 - 2)]
    for i, (y, x) in enumerate(blocks):
        d[y:y + 2, x:x + 2] = ABOVE if (i - rot) % 4 < k else BELOW


def _inner(x1, y1, x2, y2):
    """Row-major (y, x) of the box's pixels outside its four corner blocks."""
    return [(y, x) for y in range(y1, y2) for x in range(x1, x2)
            if not ((y < y1 + 2 or y >= y2 - 2) and (x < x1 + 2 or x >= x2 - 2))]


def _place(d, rng, pix, values, fill=0.0):
    """values at a random subset of pix, the rest fill."""
    order = rng.permutation(len(pix))
    for j, i in enumerate(order):
        y, x = pix[i]
        d[y, x] = values[j] if j < len(values) else fill


# ---- every branch of the segment choice -----------------------------------------------------------------------------
GRID_N = tuple(range(1, 65)) + (127, 128, 129, 255, 256, 257, 283, 284)


@functools.lru_cache(maxsize=None)
def branch_grid():
    """10 x 30 boxes on a grid, one map, one launch: cnt = 0..4 (forced by the corner blocks) x n valid depths, n in
    GRID_N.  The n depths are distinct, in (1, 140), at random pixels among the 284 outside the corner blocks; the rest
    are 0.  Sweeps int(w_start) and int(w_end) of all three fractions, the s[:-1] fallback and the NaN row (n = 1, cnt >=
    3), and the per-thread element boundaries of the 128-thread workgroup."""
    rng = np.random.RandomState(101)
    cols = 36
    rows = (5 * len(GRID_N) + cols - 1) // cols
    d = np.zeros((30 * rows, 10 * cols), np.float32)
    boxes = []
    for i, (n, k) in enumerate((n, k) for n in GRID_N for k in range(5)):
        x1, y1 = 10 * (i % cols), 30 * (i // cols)
        x2, y2 = x1 + 10, y1 + 30
        vals = np.unique(rng.uniform(1.0, 140.0, 4 * n).astype(np.float32))
        vals = rng.permutation(vals[(vals > 1) & (vals < 140)])[:n]
        assert len(vals) == n
        pix = _inner(x1, y1, x2, y2)
        assert len(pix) == 284
        _place(d, rng, pix, vals)
        _force_cnt(d, x1, y1, x2, y2, k, rot=n)
        boxes.append([x1, y1, x2, y2])
    boxes = np.asarray(boxes, np.float32)[None]
    return (_case('branch_grid', d[None, None], boxes, [boxes.shape[1]], True),)


# ---- ties: the product's disparity is a 16-bit code / 16 -----------------------------------------------------------
def _make_disp(rng, H, W):
    """Background far, a few nearer rectangles, invalid holes (the structure the older box-depth tests use)."""
    disp = np.full((H, W), 2.0, np.float32) + rng.uniform(0, 0.5, (H, W)).astype(np.float32)
    for _ in range(12):
        y, x = rng.randint(0, H - 40), rng.randint(0, W - 60)
        h, w = rng.randint(6, 40), rng.randint(6, 60)
        disp[y:y + h, x:x + w] = rng.uniform(3, 40) + rng.uniform(0, 0.3, (h, w))
    disp[rng.uniform(size=(H, W)) < 0.05] = 0.0
    return disp


@functools.lru_cache(maxsize=None)
def tie_maps():
    """Disparity input quantised to 1/16 px as the PNG loader delivers it, random boxes; boxes over constant patches
    (all 7 ranks select one value; with the corners inside the patch the corner means equal the median); and 12 x 12
    windows with cnt forced to 3 (fraction 0.25: 0 < a and b < n) or 0 whose sorted valid depths hold a run of equal
    values straddling a, straddling b - 1, and spanning both."""
    rng = np.random.RandomState(102)
    N, H, W = 2, 120, 232
    disp = np.stack([_make_disp(rng, H, W) for _ in range(N)])
    disp = (np.round(disp * 16) / 16).astype(np.float32)
    boxes = [[] for _ in range(N)]
    for n in range(N):
        for _ in range(28):
            x1, y1 = rng.uniform(0, W - 8), rng.uniform(0, H - 8)
            boxes[n].append([x1, y1, min(W, x1 + rng.uniform(1, 90)), min(H, y1 + rng.uniform(1, 70))])
    disp[:, 4:30, 4:40] = 8.0                                   # constant patches
    disp[1, 40:60, 4:30] = np.float32(5.0625)
    for n in range(N):
        boxes[n] += [[4, 4, 40, 30], [10.5, 8.2, 31.9, 22.7], [6, 6, 7, 7], [0, 0, 60, 50], [4, 40, 30, 60]]
    # crafted runs: window (x0, y0, x0 + 12, y0 + 12), 128 valid pixels outside the corner blocks, distinct disparities
    # 30 - i / 16 (depth rises with i) except the run [lo, hi) of sorted positions, which shares one disparity
    m = 128
    n25 = (int(0.25 * m), int(0.25 * m + 0.6 * m))             # (32, 108)
    n40 = (int(0.4 * m), int(0.4 * m + 0.6 * m))               # (51, 128)
    runs = [(3, n25[0] - 2, n25[0] + 3), (3, n25[1] - 3, n25[1] + 2), (3, n25[0] - 2, n25[1] + 2),
            (3, n25[0] - 1, n25[0] + 1), (3, n25[1] - 1, n25[1] + 1), (0, n40[0] - 3, n40[0] + 4),
            (0, n40[0] - 1, m), (4, 40, 80), (4, 0, 77)]
    for j, (k, lo, hi) in enumerate(runs):
        x0, y0 = 64 + 14 * j, 100
        codes = 30.0 - np.arange(m) / 16.0
        codes[lo:hi] = codes[lo]
        win = np.zeros((12, 12), np.float32)
        # invalid corners in disparity terms: 0 -> depth 1.6e8 (above every median), -2 -> depth < 0 (below)
        for i, (y, x) in enumerate([(0, 0), (0, 10), (10, 0), (10, 10)]):
            win[y:y + 2, x:x + 2] = 0.0 if i < k else -2.0
        _place(win, rng, _inner(0, 0, 12, 12), codes.astype(np.float32))
        for n in range(N):
            disp[n, y0:y0 + 12, x0:x0 + 12] = win if n == 0 else win[::-1, ::-1]
            boxes[n].append([x0, y0, x0 + 12, y0 + 12])
    boxes = np.asarray(boxes, np.float32)
    M = boxes.shape[1]
    return (_case('tie_maps', _channels(disp, 3, other=3.0), boxes, [M, M], False),)


# ---- strict comparisons ---------------------------------------------------------------------------------------------
def _pairwise_differs(rng):
    """A 2 x 2 block whose sequential mean ((a + b) + c) + d) / 4 and pairwise mean ((a + b) + (c + d)) / 4 differ."""
    f = np.float32
    while True:
        a, b, c, d = rng.uniform(2.0, 120.0, 4).astype(np.float32)
        seq = f(f(f(f(a + b) + c) + d) / f(4))
        pair = f(f(f(a + b) + f(c + d)) / f(4))
        if seq != pair:
            return np.asarray([[a, b], [c, d]], np.float32), min(seq, pair)


@functools.lru_cache(maxsize=None)
def strict_compare():
    """gt-depth windows on one 24 x 96 map, each decided by one strict comparison:
    6 x 6, corner blocks == the median exactly (> gives cnt 0, >= gives 4); 6 x 6, even n, corner means strictly between
    s[n/2 - 1] and s[n/2]; 6 x 6, median == the smaller of the corner blocks' sequential and pairwise means; one-row
    windows holding 150.0, nextafter(150, 0), 0.0, the smallest positive float32, negatives, NaN and +-inf, few enough
    pixels that taking or dropping one moves the segment."""
    rng = np.random.RandomState(103)
    d = np.zeros((24, 96), np.float32)
    boxes = []

    def window(x0, corner, others):
        win = np.zeros((6, 6), np.float32)
        for y, x in [(0, 0), (0, 4), (4, 0), (4, 4)]:
            win[y:y + 2, x:x + 2] = corner
        _place(win, rng, _inner(0, 0, 6, 6), np.asarray(others, np.float32))
        d[2:8, x0:x0 + 6] = win
        boxes.append([x0, 2, x0 + 6, 8])

    # n = 36: 10 below, 16 x 20.0 (the corners), 10 above: s[18] = 20.0 = every corner mean
    window(2, np.float32(20.0), list(np.arange(5, 15)) + list(np.arange(60, 140, 8)))
    # n = 36: 8 x 10, 11..19.5, | 21..29.5, 8 x 30: s[17] = 19.5, s[18] = 21, corner means = 20
    window(10, np.asarray([[10, 30], [10, 30]], np.float32),
           list(np.linspace(11, 19.5, 10)) + list(np.linspace(21, 29.5, 10)))
    blk, mid = _pairwise_differs(rng)
    window(18, blk, [mid] * 20)                                   # 20 x mid covers sorted position 18 in any case
    tiny = np.float32(1e-45)                                      # 2**-149
    below150 = np.nextafter(np.float32(150), np.float32(0))
    rows = [[150.0, below150, 10, 20, 30, 40], [0.0, tiny, 10, 20, 30], [-3, np.nan, np.inf, -np.inf, 5, 7, 9, 11],
            [tiny, tiny, 0.0, -0.0, 1.0], [150.0, 150.0, below150, below150, 149.0],
            [np.nan, 150.0, below150, 0.0, tiny, -1.0, np.inf, 3.0, 4.0, 5.0, 6.0], [below150], [tiny], [150.0, 0.0]]
    x0 = 2
    for r in rows:
        d[14, x0:x0 + len(r)] = np.asarray(r, np.float32)
        boxes.append([x0, 14, x0 + len(r), 15])
        x0 += len(r) + 1
    assert x0 <= 96
    d[13, :], d[15, :] = 50.0, -7.0                               # the rows the one-row windows' corner slices reach
    boxes = np.asarray(boxes, np.float32)[None]
    return (_case('strict_compare', d[None, None], boxes, [boxes.shape[1]], True),)


# ---- radix select: where the 7 ranks stop sharing a histogram ------------------------------------------------------
def _bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def radix_levels():
    """20 x 20 gt-depth windows built from bit patterns, each with cnt forced to 0, 3 and 4 (all three pairs of bounds
    are returned): valid depths that differ only in the lowest byte (one shared histogram until the last pass; 256
    patterns on 384 pixels, so ties), that diverge in the second-lowest byte, in the third byte, in the top byte (1e-3
    to 149), and two mixed windows - the low third of the sorted depths spread over the top byte and the rest in one
    lowest-byte cluster, and the mirror image - where some ranks get a histogram of their own in the first pass and the
    others share one until the last."""
    rng = np.random.RandomState(104)
    m = 384                                                       # 400 - 16 corner pixels
    base = 0x41A00000                                             # 20.0
    spread = np.exp(rng.uniform(np.log(1e-3), np.log(149.0), m)).astype(np.float32)
    sets = [_bits(base | rng.randint(0, 1 << 8, m)), _bits(base | rng.randint(0, 1 << 16, m)),
            _bits(0x41000000 | rng.randint(0, 1 << 24, m)), spread,
            np.concatenate([np.exp(rng.uniform(np.log(1e-3), np.log(1.0), m // 3)).astype(np.float32),
                            _bits(base | rng.randint(0, 1 << 8, m - m // 3))]),
            np.concatenate([_bits(0x3F800000 | rng.randint(0, 1 << 8, m - m // 3)),
                            np.exp(rng.uniform(np.log(2.0), np.log(149.0), m // 3)).astype(np.float32)])]
    d = np.zeros((22 * 3, 22 * len(sets)), np.float32)
    boxes = []
    for i, vals in enumerate(sets):
        assert np.all((vals > 0) & (vals < 150))
        for j, k in enumerate((0, 3, 4)):
            x1, y1 = 22 * i + 1, 22 * j + 1
            _place(d, rng, _inner(x1, y1, x1 + 20, y1 + 20), vals)
            _force_cnt(d, x1, y1, x1 + 20, y1 + 20, k, rot=i)
            boxes.append([x1, y1, x1 + 20, y1 + 20])
    boxes = np.asarray(boxes, np.float32)[None]
    return (_case('radix_levels', d[None, None], boxes, [boxes.shape[1]], True),)


# ---- window geometry ----------------------------------------------------------------------------------------------
def _geo_maps(rng, N, H, W):
    """gt depth: ~25 % above 150 m, zeros, negatives; image 1 quantised to 0.5 m (ties)."""
    d = rng.uniform(0.0, 200.0, (N, H, W)).astype(np.float32)
    d[rng.uniform(size=d.shape) < 0.05] = 0.0
    d[rng.uniform(size=d.shape) < 0.02] = -4.0
    d[1:] = np.round(d[1:] * 2) / 2
    return d


def _geo_case(name, rng, d, boxes, C):
    """N = 2; 5 random filler boxes last; image 0 counts fewer boxes than max_det (the fillers are not evaluated and
    their rows must be 0), image 1 more than max_det (clamps)."""
    N, H, W = d.shape
    for _ in range(5):
        x1, y1 = rng.uniform(0, W - 2), rng.uniform(0, H - 2)
        boxes.append([x1, y1, x1 + rng.uniform(1, 30), y1 + rng.uniform(1, 30)])
    b = np.repeat(np.asarray(boxes, np.float32)[None], N, axis=0)
    M = b.shape[1]
    return _case(name, _channels(d, C), b, [M - 5, M + 9], True)


@functools.lru_cache(maxsize=None)
def geometry():
    """Three gt-depth maps, N = 2 each.
    wide (48 x 900, 3 channels): windows of 2560 and 2561 pixels; streamed windows (more than BD_CACHE pixels) of 63,
    64, 65, 255, 256, 257, 513 and 800 columns whose row count leaves 1, 2 and 3 rows for the last group of 4 (the
    streaming loop takes 2 rows per wave, 4 per step: one row alone, one pair, a pair and a row); the same column counts
    with 1, 2 and 5 rows (cached unless 513 or 800 x 5); x2 - x1 = 800 and 801.
    tall (2600 x 8, 1 channel): the window of 2559 pixels (3 x 853: the only shape with x2 - x1 <= 800), 2560 as 5 x 512,
    one-column windows of 2561, 2562, 2563, 1, 2 and 5 rows, boxes past the right and bottom edges and row wraps.
    general (96 x 160, 3 channels): boxes past every edge, wraps to a non-empty window, corner slices that wrap or are
    empty, empty and inverted windows, all-invalid windows, fractional coordinates on both sides of zero."""
    rng = np.random.RandomState(105)
    cases = []
    # wide
    H, W = 48, 900
    d = _geo_maps(rng, 2, H, W)
    boxes = [[10, 3, 90, 35], [100, 2, 297, 15]]                              # 80 x 32 = 2560, 197 x 13 = 2561
    for cols, rows in ((63, (41, 42, 43)), (64, (41, 42, 43)), (65, (41, 42, 43)), (255, (13, 14, 11)),
                       (256, (13, 14, 11)), (257, (13, 10, 11)), (513, (5, 6, 7)), (800, (5, 6, 7))):
        for r in rows:
            assert cols * r > BD_CACHE and r <= H
            x1, y1 = rng.randint(0, W - cols + 1), rng.randint(0, H - r + 1)
            boxes.append([x1, y1, x1 + cols, y1 + r])
        for r in (1, 2, 5):
            x1, y1 = rng.randint(0, W - cols + 1), rng.randint(0, H - r + 1)
            boxes.append([x1, y1, x1 + cols, y1 + r])
    boxes += [[50, 0, 850, 5], [50, 0, 851, 5], [-100, 4, 700, 9], [-100.5, 4, 701.2, 9],   # w = 800, 801, 800, 801
              [99.9, 40, 900.2, 48], [120, 44, 1500, 60]]
    cases.append(_geo_case('geometry_wide', rng, d, boxes, 3))
    # tall
    H, W = 2600, 8
    d = _geo_maps(rng, 2, H, W)
    boxes = [[2, 100, 5, 953], [1, 1000, 6, 1512], [3, 20, 16, 217], [0, 20, 13, 217],
             [4, 10, 5, 2571], [7, 30, 8, 2592], [0, 37, 1, 2600], [3, 5, 4, 6], [3, 5, 4, 7], [3, 5, 4, 10],
             [0, 0, 8, 2600], [0, -2600, 8, 2600], [2, 2598, 6, 2700], [2, -3, 6, 2600]]
    cases.append(_geo_case('geometry_tall', rng, d, boxes, 1))
    # general
    H, W = 96, 160
    d = _geo_maps(rng, 2, H, W)
    d[:, 30:44, 60:90] = 0.0
    d[:, 50:58, 60:90] = 170.0
    boxes = [[-10.7, -3.2, 40.9, 30.5], [W - 20.5, H - 15.2, W + 30, H + 40], [-5, 70, 30, H + 9],    # past the corners
             [W - 9, -8, W + 9, 12], [-400, -400, 400, 400], [0, 0, W, H],
             [-50, 10, W, 40], [20, -30, 60, H], [-50, -30, W, H], [-W + 5, 10, 30, 40],               # window wraps
             [-3, 10, W, 40], [-2, 10, W, 40], [-1, 10, W, 40], [10, -3, 40, H], [10, -2, 40, H],      # corner wraps
             [10, -1, 40, H], [-3, -3, W, H], [-3, 10, -1, 40], [10, -3, 40, -1], [-30, -20, -3, -2],
             [0, 10, 1, 40], [0, 10, 2, 40], [10, 0, 40, 1], [10, 0, 40, 2], [0, 0, 1, 1], [0, 0, 2, 2],   # x2 - 2 <= 0
             [-1, 10, 20, 40], [-2, 10, 20, 40],                                                         # wraps to empty
             [30, 30, 25, 60], [40, 40, 40, 50], [30, 60, 50, 20], [W, 10, W + 20, 30], [10, H, 30, H + 9],   # empty
             [60, 30, 90, 44], [62, 51, 80, 57], [60, 30, 90, 58],                                       # all invalid
             [-0.7, -0.2, 20.9, 12.5], [-1.2, -1.9, 20.2, 12.9], [0.9, 0.99, 1.01, 30.5],                # fractions
             [-3.9, 5.5, W + 0.9, 9.1], [7.5, 8.5, 9.5, 10.5], [150.2, 90.7, 161.9, 97.3], [5, 5, 95, 75]]
    cases.append(_geo_case('geometry_general', rng, d, boxes, 3))
    return tuple(cases)


# ---- the scale's clamps ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def near_depth():
    """Disparity input, 32 x 96: patches whose depths lie below 1 m (scale clamps to 1), with d * d in (1, 3) (scale =
    d * d) and above sqrt(3) m (clamps to 3), boxes inside each patch and across two."""
    rng = np.random.RandomState(106)
    H, W = 32, 96
    depth = np.empty((1, H, W), np.float32)
    depth[:, :, :32] = rng.uniform(0.3, 0.98, (1, H, 32))
    depth[:, :, 32:64] = rng.uniform(1.02, 1.7, (1, H, 32))
    depth[:, :, 64:] = rng.uniform(1.75, 9.0, (1, H, 32))
    disp = (np.float32(160.0) / depth).astype(np.float32)
    disp[rng.uniform(size=disp.shape) < 0.03] = 0.0
    disp = np.where(rng.uniform(size=disp.shape) < 0.5, np.round(disp * 16) / 16, disp).astype(np.float32)
    boxes = []
    for x0 in (0, 32, 64):
        for _ in range(6):
            x1, y1 = x0 + rng.uniform(0, 20), rng.uniform(0, 20)
            boxes.append([x1, y1, x1 + rng.uniform(2, 11), y1 + rng.uniform(2, 11)])
    boxes += [[20, 4, 44, 20], [50, 6, 80, 30], [0, 0, W, H], [33, 3, 34, 4], [30.5, 10, 33.5, 13]]
    boxes = np.asarray(boxes, np.float32)[None]
    return (_case('near_depth', _channels(disp, 3, other=100.0), boxes, [boxes.shape[1]], False),)


# ---- the restatement on a case --------------------------------------------------------------------------------------
def cases(builder):
    return globals()[builder]()


def depth_maps(case):
    """(N, H, W) float32 depths of the case (R1)."""
    return np.stack([R.depth_map(m[0], is_depth=case.is_depth) for m in case.maps])


_REF = {}


def reference(case):
    """Per image: (values, scales, traces) of the restatement for the boxes below min(count, max_det).  Computed once."""
    if case.name not in _REF:
        out = []
        M = case.boxes.shape[1]
        for dmap, boxes, count in zip(depth_maps(case), case.boxes, case.counts):
            vals, scales, traces = [], [], []
            for box in boxes[:min(int(count), M)]:
                v, ok, t = R.value(dmap, box, R.DEFAULT, trace=True)
                vals.append(v)
                scales.append(R.scale_of_default(v) if ok else np.float32(1.0))
                traces.append(t)
            vals, scales = np.asarray(vals, np.float32), np.asarray(scales, np.float32)
            vals.setflags(write=False)
            scales.setflags(write=False)
            out.append((vals, scales, tuple(traces)))
        _REF[case.name] = tuple(out)
    return _REF[case.name]
