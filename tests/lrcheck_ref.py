"""Test infrastructure: the executable form of the stereo module's left-right check (DESIGN.md "Left-right check of the
stereo module"; kernels in stereotracking_amd/csrc/lr_check.hip).  No reference function exists for it - the five rules
are the specification, restated here in numpy on top of the C oracle:

  1  dL = oracle softargmin(V)                       (or the module's own left disparity where that is what it ships)
  2  VR[n][y][x'][d] = V[n][y][x'+d][d] if x'+d < W else 0                                            -> shear()
  3  dR = oracle softargmin(VR): the oracle's own operation order applied to the sheared array
  4  float32, one operation each: r = (int)floorf(dL + 0.5f), xr = x - r; invalid if dL is not finite, xr < 0 (or
     xr >= W, which a soft-argmin result cannot produce), or !(|dL - dR[y][xr]| * s <= lr_max_diff)   -> check()
  5  disp_postp = valid ? oracle disp_upsample : +0 on the nearest-expanded mask; disp_mask = that mask inside valid_hw
                                                                                                      -> pack()
Also the test scenes: a two-plane disparity field turned into a volume with positive, peaked costs."""
import numpy as np

from oracle import c_oracle

# (H, W, D) of the scenes every GPU test of the check uses; tests/test_cpu_lrcheck.py asserts their preconditions
SCENE_SHAPES = [(6, 40, 16), (5, 100, 48), (4, 12, 16), (3, 300, 192), (4, 70, 64), (2, 9, 16)]
SCENE_T = 32.0
SCENE_SCALE = 4
SCENE_MAX_DIFFS = (1.0, 4.0)


def shear(V):
    """Rule 2: the right view's volume of V (N,H,W,D)."""
    V = np.ascontiguousarray(V, np.float32)
    W, D = V.shape[2], V.shape[3]
    VR = np.zeros_like(V)
    for d in range(min(D, W)):
        VR[:, :, :W - d, d] = V[:, :, d:, d]
    return VR


def disparities(V, T):
    """Rules 1 and 3 -> (dL, dR), each (N,H,W) float32."""
    return c_oracle.softargmin(V, T), c_oracle.softargmin(shear(V), T)


def check(dL, dR, s, lr_max_diff):
    """Rule 4 -> dict(valid, by_xr, by_diff, diff): boolean (N,H,W) maps, and the float32 difference in image pixels
    (NaN where no right pixel was looked up)."""
    dL = np.asarray(dL, np.float32)
    dR = np.asarray(dR, np.float32)
    N, H, W = dL.shape
    finite = np.isfinite(dL)
    r = np.floor(np.where(finite, dL, np.float32(0)) + np.float32(0.5)).astype(np.float32)
    xr = np.arange(W, dtype=np.int64)[None, None, :] - r.astype(np.int64)
    inside = finite & (xr >= 0) & (xr < W)
    n, y = np.meshgrid(np.arange(N), np.arange(H), indexing='ij')
    dRm = dR[n[:, :, None], y[:, :, None], np.clip(xr, 0, W - 1)]
    with np.errstate(invalid='ignore'):
        diff = (np.abs(dL - dRm).astype(np.float32) * np.float32(s)).astype(np.float32)
        ok = diff <= np.float32(lr_max_diff)          # a NaN fails; equality is valid
    diff = np.where(inside, diff, np.float32('nan')).astype(np.float32)
    return dict(valid=inside & ok, by_xr=finite & (xr < 0), by_diff=inside & ~ok, diff=diff)


def pack(dL, valid, s, valid_hw):
    """Rule 5 -> disp_postp (N,3,H*s,W*s), disp_mask (N,1,H*s,W*s)."""
    u = c_oracle.disp_upsample(dL, s, int(valid_hw[0]), int(valid_hw[1]))
    m = np.repeat(np.repeat(valid, s, axis=1), s, axis=2)
    m[:, valid_hw[0]:, :] = False
    m[:, :, valid_hw[1]:] = False
    disp = np.where(m[:, None], u, np.float32(0)).astype(np.float32)
    return disp, m[:, None].astype(np.float32)


def restate(V, T, s, lr_max_diff, valid_hw, dL=None):
    """All five rules on the volume V.  dL: the left disparity to use instead of the oracle's (the module without
    aggregation ships the fused kernel's, which equals the oracle's to 1e-3 only; rule 1 keeps what the module ships)."""
    oL, dR = disparities(V, T)
    dL = oL if dL is None else np.asarray(dL, np.float32)
    c = check(dL, dR, s, lr_max_diff)
    disp, mask = pack(dL, c['valid'], s, valid_hw)
    return dict(dL=dL, dR=dR, disp_postp=disp, disp_mask=mask, **c)


def two_plane_field(H, W, D, N=2, seed=0):
    """Disparity field in levels: background max(1, D/4), the middle third of the columns min(D-2, W/4, 0.6 D), each
    plus uniform +-0.3: a near object in front of a far plane, with a half-occluded band at its left edge."""
    rng = np.random.RandomState(1000 + seed)
    g = np.full((N, H, W), max(1.0, D / 4.0), np.float64)
    g[:, :, W // 3:(2 * W) // 3] = min(D - 2.0, W / 4.0, 0.6 * D)
    return (g + rng.uniform(-0.3, 0.3, g.shape)).astype(np.float32)


def scene_volume(H, W, D, N=2, seed=0):
    """Volume (N,H,W,D) of the two-plane field: exp(-(d - g)^2 / 2) + 0.02 randn.  The peak cost is positive (about 1):
    with negative scores the zero cost of the out-of-range levels of rule 2 would win the soft-argmin."""
    g = two_plane_field(H, W, D, N, seed)
    rng = np.random.RandomState(2000 + seed)
    d = np.arange(D, dtype=np.float32)
    vol = np.exp(-(d[None, None, None, :] - g[..., None]) ** 2 / 2.0) + 0.02 * rng.standard_normal((N, H, W, D))
    return vol.astype(np.float32)


def noise_volume(H, W, D, N=2, seed=0):
    return np.random.RandomState(3000 + seed + 7 * W + D).normal(0, 0.6, (N, H, W, D)).astype(np.float32)


_SCENES = {}


def scene(shape, lr_max_diff, s=SCENE_SCALE):
    """The restatement of one scene, computed once and shared (read-only) by every test that needs it."""
    key = (tuple(shape), float(lr_max_diff), int(s))
    if key not in _SCENES:
        H, W, D = shape
        V = scene_volume(H, W, D)
        out = restate(V, SCENE_T, s, lr_max_diff, (H * s, W * s))
        out['V'] = V
        for v in out.values():
            v.setflags(write=False)
        _SCENES[key] = out
    return _SCENES[key]


def equality_scene(shape=(6, 40, 16), s=SCENE_SCALE):
    """-> (scene volume, dL, dR, v, at): v is a difference value the restatement observes (the median of the positive
    ones), `at` the pixels sitting exactly at it: valid at lr_max_diff = v, invalid at the next float below."""
    H, W, D = shape
    V = scene_volume(H, W, D)
    dL, dR = disparities(V, SCENE_T)
    diff = check(dL, dR, s, 0.0)['diff']
    pos = np.sort(diff[np.isfinite(diff) & (diff > 0)])
    v = np.float32(pos[len(pos) // 2])
    return V, dL, dR, v, diff == v
