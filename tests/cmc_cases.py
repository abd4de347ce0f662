"""TEST INFRASTRUCTURE: the scenarios the camera-motion kernels (csrc/cmc_flow.hip) are pinned on, with no GPU in them.

tests/test_cmc_kernels_gpu.py runs them on the device against the restatement (tests/cmc_ref.py); tests/test_cpu_cmc.py
asserts, with the restatement alone, the preconditions that make each of them able to tell right from wrong: a front
frame that equalises to at least two grey levels, a point set whose winning hypothesis, inlier set and ratio do not
depend on rounding (float32 restatement == float64 restatement, no residual near the threshold but the ones put on it).
Nothing under stereotracking_amd/ imports this.
"""
import functools

import numpy as np

import cmc_ref as R

SIDE = R.SIDE
IMG_H, IMG_W = 720, 1280

# ---- front: frame geometries (fh, fw, h, w) and contents ------------------------------------------------------------------
GEOMETRIES = [
    (736, 1280, 720, 1280),      # the shipped crop (landscape, down-scaling)
    (1080, 1920, 1080, 1920),
    (1280, 720, 1280, 720),      # portrait
    (480, 640, 480, 640),
    (96, 160, 96, 160),          # up-scaling (what the MOT shell test feeds)
    (255, 255, 255, 255),        # identity
    (333, 517, 333, 517),        # odd sizes
    (64, 96, 50, 70),            # crop in both axes, w < fw
    (2, 3, 2, 3),
]
FRONT_KINDS = ('random', 'constant', 'two-valued', 'one-off')
FRONT_BATCH = 33                 # frames of the uint8 list that crosses the 32-frame chunk of st_cmc_front_u8
FRONT_BATCH_GEOMETRY = (96, 160, 96, 160)
PAD_VALUE = 114.0


def geometry_id(g):
    return '%dx%d-crop%dx%d' % g


def _tap(d, n_dst, n_src):
    """source index the 8-bit resize reads first for destination index d"""
    return int(np.clip(np.floor((d + 0.5) * n_src / n_dst - 0.5), 0, n_src - 1))


def front_frame(kind, geometry, seed=0):
    """uint8 (3, fh, fw) BGR frame with differing channels; the content outside the (h, w) crop is random."""
    fh, fw, h, w = geometry
    rng = np.random.default_rng(1000 + seed)
    f = rng.integers(0, 256, (3, fh, fw), dtype=np.uint8)
    lo = np.array([10, 12, 14], np.uint8)[:, None, None]
    if kind == 'random':
        return f
    if kind == 'constant':
        f[:, :h, :w] = np.array([90, 80, 120], np.uint8)[:, None, None]
    elif kind == 'two-valued':
        f[:, :h, :w] = lo
        f[:, :h, w // 2:w] = np.array([200, 150, 100], np.uint8)[:, None, None]
    elif kind == 'one-off':       # every pixel the lowest grey but one, placed where the resize samples it
        f[:, :h, :w] = lo
        f[:, _tap(100, SIDE, h), _tap(100, SIDE, w)] = (250, 240, 230)
    else:
        raise KeyError(kind)
    return f


def canvas_f32(frame, h, w, pad=(5, 3)):
    """The crop of a uint8 (3, fh, fw) frame strictly inside a padded fp32 canvas (pad value 114, as the preprocessor)."""
    c = np.full((3, h + pad[0], w + pad[1]), PAD_VALUE, np.float32)
    c[:, :h, :w] = frame[:, :h, :w]
    return c


def out_of_range_f32(geometry, seed=0):
    """Integral fp32 (3, fh, fw) frame with values outside 0..255 (-7 and 300 among them)."""
    fh, fw, h, w = geometry
    rng = np.random.default_rng(2000 + seed)
    f = rng.integers(-7, 301, (3, fh, fw)).astype(np.float32)
    f[0, 0, 0], f[1, 0, 0], f[2, h - 1, w - 1] = -7.0, 300.0, 300.0
    return f


# ---- fit: point sets -------------------------------------------------------------------------------------------------------
MOTION = R.similarity(tx=11.0, ty=-6.0, deg=1.2, scale=1.02, cx=640, cy=360)
STEP_OF_SIDE = {15: 16, 31: 8, 28: 9, 20: 12}       # grid side -> cell step (255 // step == side, but 20: a sub-grid)
NOISE = 0.05                                       # px, per coordinate, at most


def grid(side):
    """Centres of the side x side cells of the mesh on 1280 x 720 -> (side^2, 2) float32, as the mesh kernel writes them."""
    step = STEP_OF_SIDE[side]
    ys, xs = np.mgrid[0:side, 0:side]
    return np.stack([(xs + 0.5) * step * (IMG_W / SIDE), (ys + 0.5) * step * (IMG_H / SIDE)], -1).reshape(-1, 2).astype(
        np.float32)


def noisy_set(side, n_outliers, seed, thr=5.0):
    """Inliers follow MOTION with noise <= NOISE px; n_outliers random points are displaced by 10..20 x thr per
    coordinate.  -> points (P, 4) float32, outlier indices."""
    rng = np.random.default_rng(seed)
    src = grid(side)
    dst = src.astype(np.float64) @ MOTION[:, :2].T + MOTION[:, 2] + rng.uniform(-NOISE, NOISE, src.shape)
    out = np.sort(rng.permutation(len(src))[:n_outliers])
    dst[out] += rng.uniform(10 * thr, 20 * thr, (len(out), 2)) * rng.choice([-1.0, 1.0], (len(out), 2))
    return np.concatenate([src, dst.astype(np.float32)], 1), out


def _case(points, thr=5.0, min_ratio=0.3, **expect):
    return dict(points=np.ascontiguousarray(points, np.float32), thr=float(thr), min_ratio=float(min_ratio),
                on_threshold=(), **expect)


def _set_a(side=15, seed=11, thr=5.0):
    pts, out = noisy_set(side, int(0.4 * side * side), seed)
    return _case(pts, thr, outliers=out)


def _set_c(side=28, seed=13):
    pts, _ = noisy_set(side, 0, seed)
    return _case(pts, winner=(0, 1), n_inliers=side * side, motion=MOTION)


def _set_d(side=15):
    """Integer coordinates under the identity: a displacement of exactly (3, 4) sits ON thr = 5 (inlier, `<=`),
    (3, 4.01) lies outside."""
    ys, xs = np.mgrid[0:side, 0:side]
    src = np.stack([40 + 80 * xs, 22 + 45 * ys], -1).reshape(-1, 2).astype(np.float32)
    dst = src.copy()
    dst[7] += np.array([3, 4], np.float32)
    dst[11] += np.array([3, 4.01], np.float32)
    c = _case(np.concatenate([src, dst], 1), winner=(0, 1), n_inliers=side * side - 1, inlier=(7,), outlier=(11,))
    c['on_threshold'] = (7,)
    return c


def _set_e(seed=17):
    """200 distinct points (40 % outliers) followed by 25 whose source repeats one of them and whose target is far off:
    the den == 0 hypotheses are skipped, the added points join no consensus, the answer over the first 200 stays."""
    pts, out = noisy_set(15, 90, seed)
    base = pts[:200]
    rng = np.random.default_rng(seed + 1)
    dup = base[rng.permutation(np.setdiff1d(np.arange(200), out))[:25]].copy()       # copies of inliers
    dup[:, 2:] += rng.uniform(50, 100, (25, 2)).astype(np.float32) * rng.choice([-1, 1], (25, 2)).astype(np.float32)
    return _case(np.concatenate([base, dup]), base_points=200)


def _set_f(side=15, seed=19):
    """Every source point coincident: no usable hypothesis."""
    rng = np.random.default_rng(seed)
    P = side * side
    src = np.tile(np.array([[640.0, 360.0]], np.float32), (P, 1))
    dst = src + rng.uniform(-30, 30, (P, 2)).astype(np.float32)
    return _case(np.concatenate([src, dst], 1), n_inliers=0, valid=False)


def _set_g(n_inliers, seed=23):
    """P = 400 with exactly n_inliers inliers against min_inlier_ratio 0.3: 120 / 400 >= 0.3f holds in float32."""
    pts, _ = noisy_set(20, 400 - n_inliers, seed)
    return _case(pts, 5.0, 0.3, n_inliers=n_inliers, valid=n_inliers >= 120)


FIT_CASES = {
    'a': _set_a,                                           # P = 225, 40 % outliers
    'b': lambda: _case(noisy_set(31, int(0.6 * 961), 29)[0]),    # P = 961, 60 % outliers
    'c': _set_c,                                           # P = 784, none: every inlier pair ties, (0, 1) wins
    'd': _set_d,
    'e': _set_e,
    'f': _set_f,
    'g120': lambda: _set_g(120),
    'g119': lambda: _set_g(119),
    'h1': lambda: _set_a(thr=1.0),
    'h3': lambda: _set_a(thr=3.0),
    # the same constructions at another point count, so that a batch of one P can hold them
    'c225': lambda: _set_c(15),
    'a784': lambda: _set_a(28, seed=31),
    'd784': lambda: _set_d(28),
    'f784': lambda: _set_f(28),
}
# one call of N = 5 (the entry point takes one P per call, so each batch holds the constructions at its own P):
# every row must equal its own N = 1 result bit for bit
FIT_BATCHES = {'batch225': ('a', 'c225', 'f', 'd', 'a'), 'batch784': ('a784', 'c', 'f784', 'd784', 'a784')}


@functools.lru_cache(maxsize=None)
def fit_case(name):
    return FIT_CASES[name]()


@functools.lru_cache(maxsize=None)
def fit_reference(name, dtype=np.float32):
    """R.consensus_fit of a case -> (warp or None, ratio, inliers, winner (i, j, residuals) or None)."""
    c = fit_case(name)
    p = c['points']
    return R.consensus_fit(p[:, :2], p[:, 2:], c['thr'], c['min_ratio'], dtype, with_winner=True)


# ---- mesh: flow fields ---------------------------------------------------------------------------------------------------
MESH_STEPS = (8, 9, 11, 12, 15, 16)          # cell counts odd and even, 255 // step from 31 down to 15
MESH_SIZES = ((720, 1280), (1080, 1920), (333, 517), (96, 160))


def flow_fields():
    """name -> (255, 255, 2) float32.  Exact ties (zeros; two values per cell, in equal numbers where the cell count is
    even), -0.0 among zeros, a smooth ramp, and white noise (no ties at all)."""
    rng = np.random.default_rng(41)
    y, x = np.mgrid[0:SIDE, 0:SIDE]
    two = np.stack([np.where((x + y) % 2 == 0, 1.25, -0.75), np.where((x + y) % 2 == 1, 0.5, 2.5)], -1)
    negz = np.zeros((SIDE, SIDE, 2), np.float32)
    negz[rng.random((SIDE, SIDE, 2)) < 0.5] = -0.0
    ramp = np.stack([0.011 * x - 0.023 * y + 0.4, 0.017 * y + 0.005 * x - 1.3], -1)
    return {'zeros': np.zeros((SIDE, SIDE, 2), np.float32), 'two-valued': two.astype(np.float32), 'neg-zero': negz,
            'ramp': ramp.astype(np.float32), 'noise': rng.normal(0, 3, (SIDE, SIDE, 2)).astype(np.float32)}


# ---- flow: frame pairs -----------------------------------------------------------------------------------------------------
FLOW_WINSIZES = (5, 15, 31, 63)
# the scenes of test_cpu_cmc.test_farneback_recovers_known_camera_motion: (motion, region moving on its own);
# together they are the N = 3 batch of different motions
FLOW_SCENES = {
    'shift': (R.similarity(tx=7.3, ty=-4.6), None),
    'similarity': (R.similarity(tx=3.0, deg=0.5, scale=1.01, cx=640, cy=360), None),
    'moving-region': (R.similarity(tx=5.0, deg=0.5, scale=1.01, cx=640, cy=360), (300, 720, 600, 1280)),
}


@functools.lru_cache(maxsize=None)
def scene_frames(name):
    """Two grey uint8 (720, 1280) frames of a scene."""
    from test_cpu_cmc import moving_pair
    A, moving = FLOW_SCENES[name]
    return moving_pair(A, moving=moving)


def grey_to_bgr(g):
    """grey uint8 (h, w) -> uint8 (3, h, w) BGR with differing channels."""
    g = g.astype(np.int32)
    return np.stack([np.clip(g - 9, 0, 255), g, np.clip(255 - g // 2, 0, 255)]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scene_planes(name):
    """The restatement's equalised planes of a scene's two frames."""
    return tuple(R.front(grey_to_bgr(f), IMG_H, IMG_W) for f in scene_frames(name))


# ---- options end to end --------------------------------------------------------------------------------------------------
OPTIONS = dict(step=8, winsize=15, ransac_thr=3.0, min_inlier_ratio=0.5)
OPTIONS_SCENE = 'similarity'
