"""TEST INFRASTRUCTURE: the scenarios the StereoSGBM kernels (csrc/sgbm.hip) are pinned on, with no GPU in them.

tests/test_sgbm_edges_gpu.py runs them on the device against the restatement (tests/sgbm_ref.py); tests/test_cpu_sgbm.py
asserts, with the restatement alone, the preconditions that make each of them able to tell right from wrong: tied
minima of the aggregated cost S that are decided (not invalidated), unique pixels of one row that claim the same disp2
entry at the same cost, geometries whose cost is not flat, options that reach the final map, an S above 2^14.
Everything is deterministic.  Nothing under stereotracking_amd/ imports this.
"""
import functools

import numpy as np

import sgbm_ref as R

# ---- TIES: inputs whose aggregated cost has several minima --------------------------------------------------------------
TIES_HW = (24, 120)
TIES_D = (16, 48, 64)
TIES_UNIQ = (10, 0)


def _bgr(plane):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(plane, np.uint8), (3,) + TIES_HW))


def _rolled(img, d):
    """The right view of a left image at disparity d everywhere (wrapping): right[x - d] = left[x]."""
    return np.ascontiguousarray(np.roll(img, -d, axis=-1))


def _ties():
    h, w = TIES_HW
    y, x = np.mgrid[0:h, 0:w]
    same = lambda p: (_bgr(p), _bgr(p))                                        # noqa: E731
    stripes = _bgr((x // 4) % 2 * 255)
    half = _bgr((x > 70) * 255)
    fine = _bgr((x // 2) % 2 * 255)
    rng = np.random.RandomState(7)
    noise = (rng.randint(0, 2, (3, h, w + 9)) * 255).astype(np.uint8)
    return {
        'const63': same(np.full(TIES_HW, 63)),
        'const120': same(np.full(TIES_HW, 120)),
        'const0': same(np.zeros(TIES_HW)),
        'const255': same(np.full(TIES_HW, 255)),
        'stripes-self': (stripes, stripes),
        'stripes-rolled': (stripes, _rolled(stripes, 5)),
        'period3': same((x % 3 == 0) * 255),
        'checkerboard': same((x + y) % 2 * 255),
        'rows': same(y % 2 * 255),
        'halfplane-rolled': (half, _rolled(half, 5)),
        'inverse': (fine, 255 - fine),
        'noise-shift9': (np.ascontiguousarray(noise[:, :, :w]), np.ascontiguousarray(noise[:, :, 9:])),
    }


TIES = _ties()
# the scenarios that test_cpu_sgbm holds to "at least half of the computed pixels have two or more minima of S"
TIES_TIED = ('const63', 'stripes-rolled', 'period3', 'inverse', 'halfplane-rolled')


def ties_partner(name):
    """The different scenario of the same size that fills the second slot of the N = 2 batch."""
    names = list(TIES)
    return names[(names.index(name) + 1) % len(names)]


def ties_kw(D, uniq):
    return dict(num_disparities=D, uniqueness_ratio=uniq)


def tied_minima(S):
    """S (h, w', D) -> bool (h, w'): the pixels whose minimum of S is attained at two or more levels."""
    return (S == S.min(-1, keepdims=True)).sum(-1) >= 2


def disp2_ties(S, D, uniqueness_ratio):
    """Number of disp2 entries (row, x - best) whose lowest claiming cost comes from two or more unique pixels with
    different best: there 'ties go to the highest x' (rule 6) decides what disp2 holds."""
    minS, best = S.min(-1), S.argmin(-1)
    if uniqueness_ratio > 0:
        thresh = (100 * minS) // (100 - uniqueness_ratio)
        bad = ((np.abs(np.arange(D)[None, None] - best[..., None]) > 1) & (S <= thresh[..., None])).any(-1)
    else:
        bad = np.zeros(best.shape, bool)
    n = 0
    for y in range(S.shape[0]):
        claims = {}
        for xi in np.nonzero(~bad[y])[0]:
            claims.setdefault(int(xi) + D - int(best[y, xi]), []).append((int(minS[y, xi]), int(best[y, xi])))
        for c in claims.values():
            lo = min(c)[0]
            n += len({b for cost, b in c if cost == lo}) > 1
    return n


# ---- GEOMETRY: edge sizes on synthetic_stereo_pair texture -------------------------------------------------------------
# (h, w, D, block_size, extra module arguments).  block_size >= 5 needs grey (the int16 bound of the constructor).
# The speckle windows are small, so that the few computed pixels of these sizes are not all removed.
GEOMETRY = [
    (1, 17, 16, 1, dict(speckle_window_size=0)),                 # w = D + 1: one computed column, one row
    (1, 17, 16, 3, dict(speckle_window_size=0)),
    (2, 18, 16, 5, dict(color=False, speckle_window_size=1)),    # h < block radius
    (3, 81, 64, 3, dict(speckle_window_size=4)),                 # w - D = 17: a partial block of 4 waves, a partial chunk
    (5, 65, 64, 3, dict(speckle_window_size=1)),                 # one computed column, all 64 lanes
    (7, 300, 32, 7, dict(color=False, speckle_window_size=50)),  # ring slots 0..6
    (4, 100, 16, 9, dict(color=False, pre_filter_cap=15, speckle_window_size=20)),   # ring slots 0..8, h < radius
    (40, 83, 48, 3, dict(speckle_window_size=50)),               # w - D = 35: odd
    (33, 67, 48, 3, dict(speckle_window_size=20)),               # w - D = 19
]


def geometry_id(g):
    h, w, D, bs, extra = g
    return '%dx%d-D%d-b%d%s' % (h, w, D, bs, '' if extra.get('color', True) else '-grey')


def geometry_kw(g):
    h, w, D, bs, extra = g
    return dict(num_disparities=D, block_size=bs, **extra)


@functools.lru_cache(maxsize=None)
def texture_pair(seed, h, w, D):
    from stereotracking_amd.synthetic import synthetic_stereo_pair
    p = synthetic_stereo_pair(seed, h, w, max_disp=D)
    return p['left'], p['right']


_GEOMETRY_SEED = {(2, 18): 4}       # a pair whose two rows decide valid and invalid pixels (most seeds: one level)


def geometry_pairs(g):
    """The two pairs of the N = 2 batch of a geometry: the scenario, then another pair of its size."""
    h, w, D = g[:3]
    seed = _GEOMETRY_SEED.get((h, w), 100 + h + w)
    return [texture_pair(seed, h, w, D), texture_pair(seed + 1, h, w, D)]


# ---- OPTIONS: each changed alone from the defaults, on one pair ---------------------------------------------------------
OPTIONS_HW, OPTIONS_SEED = (48, 150), 3
OPTIONS = [
    dict(uniqueness_ratio=0), dict(uniqueness_ratio=50), dict(uniqueness_ratio=99),
    dict(disp12_max_diff=-1), dict(disp12_max_diff=1000),
    dict(speckle_window_size=0), dict(speckle_window_size=5000),
    dict(speckle_range=0),
    dict(P1=0, P2=0), dict(P1=400, P2=100),
    dict(P2=5819),
    dict(pre_filter_cap=1), dict(pre_filter_cap=31),
    dict(pre_filter_cap=127, block_size=1),
]
# rule 6 maps disp12_max_diff <= 0 to 1, so -1 computes what the default 0 computes on every input; every other
# option has to change the final map of the pair
OPTIONS_SAME_AS_DEFAULT = [dict(disp12_max_diff=-1)]


def options_id(kw):
    return '-'.join('%s=%s' % kv for kv in kw.items())


def options_pairs():
    h, w = OPTIONS_HW
    return [texture_pair(OPTIONS_SEED + i, h, w, 48) for i in range(2)]


# ---- BOUND: the largest P2 the constructor admits, on unmatched binary noise ---------------------------------------------
BOUND_KW = dict(P2=5819)


@functools.lru_cache(maxsize=None)
def bound_pairs():
    """Independent {0, 255} noise in the left and the right image, the same in the three channels (RandomState(0),
    then RandomState(1) for the second slot of the batch)."""
    out = []
    for seed in range(2):
        rng = np.random.RandomState(seed)
        out.append(tuple(_bgr(rng.randint(0, 2, TIES_HW) * 255) for _ in range(2)))
    return out


# ---- the restatement's stages, computed once per (pair, options) ---------------------------------------------------------
_REFS = {}


def reference(left, right, kw):
    """R.sgbm(stages=True) of a pair, cached by content and options; the arrays are read-only."""
    key = (left.tobytes(), right.tobytes(), left.shape, tuple(sorted(kw.items())))
    if key not in _REFS:
        st = R.sgbm(left, right, stages=True, **kw)
        for a in st.values():
            a.setflags(write=False)
        _REFS[key] = st
    return _REFS[key]


# ---- SPECKLE: int16 maps ------------------------------------------------------------------------------------------------
SPECKLE_HW = (32, 48)
SPECKLE_WINDOWS = (0, 1, 400, 900, 32 * 48)
SPECKLE_RANGES = (0, 10)
SERPENTINE_PIXELS = 784


def _serpentine(step):
    """One-pixel-wide path: even rows full, odd rows one joining pixel at alternating ends; row y holds 320 + step y."""
    h, w = SPECKLE_HW
    m = np.full((h, w), R.INVALID, np.int16)
    for y in range(h):
        v = 320 + step * y
        if y % 2 == 0:
            m[y] = v
        else:
            m[y, w - 1 if y % 4 == 1 else 0] = v
    return m


def _batch3():
    """Three maps; map n ends (its last 5 rows, the last pixel among them) on the value that map n + 1 begins on (its
    first 4 rows).  Alone, each map holds components of 192 and 240 pixels (both <= 400); an edge from the last row or
    the last pixel of map n into map n + 1 would make one of 432."""
    h, w = SPECKLE_HW
    vals = [160, 480, 800, 1120]
    maps = np.full((3, h, w), R.INVALID, np.int16)
    for n in range(3):
        maps[n, :4] = vals[n]
        maps[n, h - 5:] = vals[n + 1]
        maps[n, 10:20, 5:40] = 2000 + 16 * n          # 350 pixels, away from the seams
    return maps


def _speckle_maps():
    h, w = SPECKLE_HW
    y, x = np.mgrid[0:h, 0:w]
    return {
        'serpentine': _serpentine(0)[None],
        'serpentine-rising': _serpentine(160)[None],         # steps of exactly max_diff at speckle_range 10
        'checkerboard': ((x + y) % 2 * 1600).astype(np.int16)[None],
        'constant': np.full((1, h, w), 320, np.int16),
        'batch3': _batch3(),
        'all-invalid': np.full((1, h, w), R.INVALID, np.int16),
    }


SPECKLE = _speckle_maps()


def speckle_reference(maps, window, rng):
    """The restatement's filter of every map of a batch on its own."""
    return np.stack([R.speckles(m.astype(np.int64), window, 16 * rng) for m in maps]).astype(np.int16)


# ---- MEDIAN: int16 maps, N = 3 ------------------------------------------------------------------------------------------
MEDIAN_HW = ((1, 1), (1, 9), (9, 1), (2, 300))


def median_maps(hw):
    """(3, h, w) int16 from a few values (ties in every window), -16 among them."""
    rng = np.random.RandomState(hw[0] * 1000 + hw[1])
    return rng.choice(np.array([-16, -16, 0, 16, 17, 320, 1008], np.int16), size=(3,) + tuple(hw))


# ---- a second compute() on a dirty workspace: a TIES scenario valid nearly everywhere, then one valid nowhere ---------
DIRTY = ('noise-shift9', 'const63')
