"""Camera-motion compensation (CMC) of the tracker: the device half (estimate: Mesh-Affine, and ECC further down -
csrc/cmc_ecc.hip, DESIGN.md "ECC camera-motion compensation") and the host half (apply).  The tracker and the MOT shell
reach either estimate through one small object per method (`estimator(cmc)`: plane_shape, front, estimate).

Reference: OCSORTTracker_Disparity(cmc=dict(method='glme_affine', glme=dict(step, winsize, ransac_thr,
min_inlier_ratio))) - mmtrack/models/trackers/ocsort_tracker_disparity.py:62-97, gmc.py:7-45, utils.py:6-55.  The
estimate runs in csrc/cmc_flow.hip (front -> Farneback flow -> per-cell medians -> consensus similarity fit, every
OpenCV rule restated, the RANSAC draw replaced by a deterministic exhaustive fit: DESIGN.md "Camera-motion
compensation"); `apply_warp` is gmc.apply_gmc_to_tracks_cxcyah on one Kalman state, the same arithmetic the native
tracker applies (csrc/ocsort_tracker.cpp).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream, ptr

SIDE = 255
WARP_FLOATS = 8          # valid, inlier ratio, a00, a01, a02, a10, a11, a12
DEFAULTS = dict(step=16, winsize=31, ransac_thr=5.0, min_inlier_ratio=0.3)


def glme_params(glme=None):
    """cmc['glme'] overrides on the reference defaults (utils.py:6-7) -> dict."""
    p = dict(DEFAULTS)
    for k, v in (glme or {}).items():
        if k not in p:
            raise ValueError(f"unknown glme option '{k}' (expected one of {sorted(p)})")
        p[k] = v
    if not 8 <= int(p['step']) <= 16:
        raise ValueError(f"glme step {p['step']} is not supported (8..16)")
    if int(p['winsize']) % 2 != 1:
        raise ValueError(f"glme winsize {p['winsize']} must be odd")
    return p


def _params(p):
    return _lib.StCmcParams(C.sizeof(_lib.StCmcParams), int(p['step']), int(p['winsize']), float(p['ransac_thr']),
                            float(p['min_inlier_ratio']))


def front(img, h, w, out=None):
    """Equalised 255 x 255 grey planes of N frames on the device (one launch).
    img: (N, 3, H, W) fp32 or uint8 CUDA tensor (BGR, as the preprocessor leaves it), or a list of N uint8 (1, 3, fh, fw)
    CUDA frames; cropped to (h, w).  -> uint8 (N, 255, 255) (written into `out` when given)."""
    lib = _lib.load()
    if isinstance(img, (list, tuple)):
        fr = [f.contiguous() for f in img]
        if any(f.dtype != torch.uint8 or f.dim() != 4 or f.shape[:2] != (1, 3) for f in fr):
            raise ValueError('CMC front: frames must be uint8 (1, 3, h, w) tensors')
        N, fh, fw = len(fr), int(fr[0].shape[-2]), int(fr[0].shape[-1])
        dev = fr[0].device
        out = torch.empty(N, SIDE, SIDE, dtype=torch.uint8, device=dev) if out is None else out
        ptrs = (C.c_void_p * N)(*[f.data_ptr() for f in fr])
        check(lib.st_cmc_front_u8(ptrs, N, fh, fw, int(h), int(w), ptr(out), current_stream()), 'st_cmc_front_u8')
        return out
    if img.dim() != 4 or img.shape[1] < 3 or not img.is_cuda:
        raise ValueError('CMC front: img must be a (N, 3, H, W) CUDA tensor')
    N, H, W = int(img.shape[0]), int(img.shape[2]), int(img.shape[3])
    out = torch.empty(N, SIDE, SIDE, dtype=torch.uint8, device=img.device) if out is None else out
    if img.dtype == torch.uint8:
        return front([img[i:i + 1, :3] for i in range(N)], h, w, out)
    x = img[:, :3].float().contiguous()
    check(lib.st_cmc_front_f32(ptr(x), N, H, W, int(h), int(w), ptr(out), current_stream()), 'st_cmc_front_f32')
    return out


def _workspace(n, dev):
    return torch.empty(int(_lib.load().st_cmc_workspace_bytes(n)), dtype=torch.uint8, device=dev)


def flow(prev, curr, winsize=31, per_level=False):
    """Dense Farneback flow prev[n] -> curr[n] (uint8 (N, 255, 255) planes) -> (N, 255, 255, 2) fp32; per_level: also
    every pyramid level's final flow, a list finest first."""
    N, dev = int(prev.shape[0]), prev.device
    lib = _lib.load()
    ws = _workspace(N, dev)
    out = torch.empty(N, SIDE, SIDE, 2, device=dev)
    sides = (C.c_int * 8)()
    L = lib.st_cmc_num_levels(sides)
    tot = sum(s * s for s in sides[:L])
    lev = torch.empty(N, tot, 2, device=dev) if per_level else None
    check(lib.st_cmc_flow(ptr(prev.contiguous()), ptr(curr.contiguous()), N, int(winsize), ptr(ws), ws.numel(),
                          ptr(out), ptr(lev), current_stream()), 'st_cmc_flow')
    if not per_level:
        return out
    res, o = [], 0
    for s in sides[:L]:
        res.append(lev[:, o:o + s * s].view(N, s, s, 2))
        o += s * s
    return out, res


def estimate(prev, curr, img_h, img_w, params=None, with_mesh=False, ws=None):
    """Warps of the plane pairs (prev[n], curr[n]) on the device -> (N, 8) fp32 device tensor
    [valid, inlier ratio, 2 x 3 warp] (+ mesh (N, P, 4) and inliers (N, P) uint8 with with_mesh)."""
    p = glme_params(params)
    N, dev = int(prev.shape[0]), prev.device
    ws = _workspace(N, dev) if ws is None else ws
    warps = torch.empty(N, WARP_FLOATS, device=dev)
    P = (SIDE // int(p['step'])) ** 2
    mesh = torch.empty(N, P, 4, device=dev) if with_mesh else None
    inl = torch.empty(N, P, dtype=torch.uint8, device=dev) if with_mesh else None
    prm = _params(p)
    check(_lib.load().st_cmc_estimate(ptr(prev.contiguous()), ptr(curr.contiguous()), N, int(img_h), int(img_w),
                                      C.byref(prm), ptr(ws), ws.numel(), ptr(warps), ptr(mesh), ptr(inl),
                                      current_stream()), 'st_cmc_estimate')
    return (warps, mesh, inl) if with_mesh else warps


def mesh_fit(flow, img_h, img_w, params=None, with_mesh=False, ws=None):
    """The estimate entered after the flow (st_cmc_mesh_fit): flow (N, 255, 255, 2) fp32 device tensor -> what
    estimate() returns for planes with that flow.  Test-facing; the flow must be free of NaN."""
    p = glme_params(params)
    if flow.dim() != 4 or tuple(flow.shape[1:]) != (SIDE, SIDE, 2) or flow.dtype != torch.float32 or not flow.is_cuda:
        raise ValueError('CMC mesh_fit: flow must be a (N, 255, 255, 2) fp32 CUDA tensor')
    N, dev = int(flow.shape[0]), flow.device
    ws = _workspace(N, dev) if ws is None else ws
    warps = torch.empty(N, WARP_FLOATS, device=dev)
    P = (SIDE // int(p['step'])) ** 2
    mesh = torch.empty(N, P, 4, device=dev) if with_mesh else None
    inl = torch.empty(N, P, dtype=torch.uint8, device=dev) if with_mesh else None
    prm = _params(p)
    check(_lib.load().st_cmc_mesh_fit(ptr(flow.contiguous()), N, int(img_h), int(img_w), C.byref(prm), ptr(ws),
                                      ws.numel(), ptr(warps), ptr(mesh), ptr(inl), current_stream()), 'st_cmc_mesh_fit')
    return (warps, mesh, inl) if with_mesh else warps


def fit(points, ransac_thr=DEFAULTS['ransac_thr'], min_inlier_ratio=DEFAULTS['min_inlier_ratio'], ws=None):
    """The consensus fit alone (st_cmc_fit): points (N, P, 4) fp32 device tensor {src x, src y, dst x, dst y},
    2 <= P <= 1024 -> warps (N, 8) as estimate(), inliers (N, P) uint8.  Test-facing."""
    if points.dim() != 3 or points.shape[2] != 4 or points.dtype != torch.float32 or not points.is_cuda:
        raise ValueError('CMC fit: points must be a (N, P, 4) fp32 CUDA tensor')
    N, P, dev = int(points.shape[0]), int(points.shape[1]), points.device
    ws = _workspace(N, dev) if ws is None else ws
    warps = torch.empty(N, WARP_FLOATS, device=dev)
    inl = torch.empty(N, P, dtype=torch.uint8, device=dev)
    check(_lib.load().st_cmc_fit(ptr(points.contiguous()), N, P, float(ransac_thr), float(min_inlier_ratio), ptr(ws),
                                 ws.numel(), ptr(warps), ptr(inl), current_stream()), 'st_cmc_fit')
    return warps, inl


def warp_or_none(row):
    """One (8,) host row of estimate() -> 2 x 3 float32 warp, or None (fit failed / inlier ratio too low)."""
    row = np.asarray(row, np.float32)
    return row[2:8].reshape(2, 3).copy() if row[0] != 0 else None


def apply_warp(mean, cov, warp):
    """gmc.apply_gmc_to_tracks_cxcyah for one cxcyah Kalman state -> (mean, covariance), float64."""
    w = np.asarray(warp)
    R = w[:2, :2].astype(np.float64)
    t = w[:2, 2].astype(np.float64)
    s = float(np.sqrt(max(np.linalg.det(R), 1e-12)))
    mean = mean.copy()
    mean[0:2] = R.dot(mean[0:2]) + t
    mean[3] *= s
    mean[4:6] = R.dot(mean[4:6])
    mean[7] *= s
    M = np.eye(8, dtype=float)
    M[0:2, 0:2] = R
    M[4:6, 4:6] = R
    M[3, 3] = s
    M[7, 7] = s
    return mean, M.dot(cov).dot(M.T)


# ---- ECC (cmc=dict(method='ecc')): csrc/cmc_ecc.hip, rules in tests/ecc_ref.py and DESIGN.md -------------------------
ECC_MODES = dict(MOTION_TRANSLATION=0, MOTION_EUCLIDEAN=1, MOTION_AFFINE=2)
ECC_DEFAULTS = dict(warp_mode='MOTION_EUCLIDEAN', num_iters=50, stop_eps=1e-3, gauss_filt_size=1, downscale=2)
ECC_STEP_DOUBLES = 72
# field -> (offset, length) of one st_cmc_ecc_step row (include/stereotrack.h, ST_ECC_STEP_*)
ECC_STEP_FIELDS = dict(valid=(0, 1), n=(1, 1), mean_i=(2, 1), mean_t=(3, 1), std_i=(4, 1), std_t=(5, 1),
                       img_norm=(6, 1), tmp_norm=(7, 1), corr=(8, 1), rho=(9, 1), lam=(10, 1), H=(12, 36), iP=(48, 6),
                       tP=(54, 6), dp=(60, 6), warp=(66, 6))


def ecc_params(ecc=None):
    """cmc['ecc'] overrides on the reference defaults (camera_motion_compensation.py:21-27; downscale is this
    package's) -> dict; warp_mode comes back as its bare name ('cv2.MOTION_EUCLIDEAN' and 'MOTION_EUCLIDEAN' parse)."""
    p = dict(ECC_DEFAULTS)
    for k, v in (ecc or {}).items():
        if k not in p:
            raise ValueError(f"unknown ecc option '{k}' (expected one of {sorted(p)})")
        p[k] = v
    mode = p['warp_mode']
    name = mode[len('cv2.'):] if isinstance(mode, str) and mode.startswith('cv2.') else mode
    if name == 'MOTION_HOMOGRAPHY':
        raise ValueError('ecc warp_mode MOTION_HOMOGRAPHY is not supported: the Kalman application takes a 2 x 3 warp')
    if not isinstance(name, str) or name not in ECC_MODES:
        raise ValueError(f"unknown ecc warp_mode {mode!r} (expected one of {sorted(ECC_MODES)})")
    p['warp_mode'] = name
    for k in ('num_iters', 'gauss_filt_size', 'downscale'):
        if isinstance(p[k], bool) or int(p[k]) != p[k]:
            raise ValueError(f'ecc {k} {p[k]!r} must be an integer')
        p[k] = int(p[k])
    if p['num_iters'] < 1:
        raise ValueError(f"ecc num_iters {p['num_iters']} must be >= 1")
    if p['gauss_filt_size'] not in (1, 3, 5):
        raise ValueError(f"ecc gauss_filt_size {p['gauss_filt_size']} is not supported (1, 3 or 5)")
    if p['downscale'] not in (1, 2, 4):
        raise ValueError(f"ecc downscale {p['downscale']} is not supported (1, 2 or 4)")
    p['stop_eps'] = float(p['stop_eps'])
    if not p['stop_eps'] == p['stop_eps']:
        raise ValueError('ecc stop_eps is NaN')
    return p


def ecc_plane_shape(h, w, downscale):
    return int(h) // int(downscale), int(w) // int(downscale)


def ecc_to_image(warp, downscale):
    """Plane warp [A | t] (2 x 3) -> image warp: plane pixel i sits at image coordinate s i + c, c = (s - 1) / 2, so
    t -> s t + c - A (c, c).  float64."""
    M = np.asarray(warp, np.float64).reshape(2, 3)
    c = (downscale - 1) / 2.0
    return np.hstack([M[:, :2], (downscale * M[:, 2] + c - M[:, :2] @ np.array([c, c]))[:, None]])


def _ecc_struct(p):
    return _lib.StEccParams(C.sizeof(_lib.StEccParams), ECC_MODES[p['warp_mode']], p['num_iters'], p['stop_eps'],
                            p['gauss_filt_size'], p['downscale'])


def ecc_front(img, h, w, downscale=2, out=None):
    """Grey fp32 planes (N, h // downscale, w // downscale) of N frames on the device: crop to (h, w), fixed-point grey,
    downscale x downscale box mean.  img as front(): a (N, 3, H, W) fp32 / uint8 BGR CUDA batch or a list of N uint8
    (1, 3, fh, fw) CUDA frames; both give the same bits."""
    lib = _lib.load()
    ph, pw = ecc_plane_shape(h, w, downscale)
    if isinstance(img, (list, tuple)):
        fr = [f.contiguous() for f in img]
        if any(f.dtype != torch.uint8 or f.dim() != 4 or f.shape[:2] != (1, 3) or f.shape != fr[0].shape for f in fr):
            raise ValueError('ECC front: frames must be uint8 (1, 3, h, w) tensors of one size')
        N, fh, fw = len(fr), int(fr[0].shape[-2]), int(fr[0].shape[-1])
        out = torch.empty(N, ph, pw, device=fr[0].device) if out is None else out
        ptrs = (C.c_void_p * N)(*[f.data_ptr() for f in fr])
        check(lib.st_cmc_ecc_front_u8(ptrs, N, fh, fw, int(h), int(w), int(downscale), ptr(out), current_stream()),
              'st_cmc_ecc_front_u8')
        return out
    if img.dim() != 4 or img.shape[1] < 3 or not img.is_cuda:
        raise ValueError('ECC front: img must be a (N, 3, H, W) CUDA tensor')
    N, H, W = int(img.shape[0]), int(img.shape[2]), int(img.shape[3])
    if img.dtype == torch.uint8:
        return ecc_front([img[i:i + 1, :3] for i in range(N)], h, w, downscale, out)
    out = torch.empty(N, ph, pw, device=img.device) if out is None else out
    x = img[:, :3].float().contiguous()
    check(lib.st_cmc_ecc_front_f32(ptr(x), N, H, W, int(h), int(w), int(downscale), ptr(out), current_stream()),
          'st_cmc_ecc_front_f32')
    return out


def _ecc_planes(prev, curr, img_h, img_w, p):
    """The two contiguous plane batches, checked against the plane size the library derives from (img_h, img_w)."""
    shape = ecc_plane_shape(img_h, img_w, p['downscale'])
    for t in (prev, curr):
        if t.dim() != 3 or tuple(t.shape[1:]) != shape or t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f'ECC: planes must be (N, {shape[0]}, {shape[1]}) fp32 CUDA tensors, got {tuple(t.shape)} '
                             f'{t.dtype}')
    if prev.shape[0] != curr.shape[0]:
        raise ValueError('ECC: template and input batches differ in N')
    return prev.contiguous(), curr.contiguous(), int(prev.shape[0]), shape


def ecc_workspace(n, plane_shape, dev):
    return torch.empty(int(_lib.load().st_cmc_ecc_workspace_bytes(int(n), int(plane_shape[0]), int(plane_shape[1]))),
                       dtype=torch.uint8, device=dev)


def ecc_prepare(prev, curr, img_h, img_w, params=None, ws=None):
    """Rules E1 / E2 -> (blurred template, blurred input, gx, gy), each (N, ph, pw) fp32.  Test-facing."""
    p = ecc_params(params)
    prev, curr, N, shape = _ecc_planes(prev, curr, img_h, img_w, p)
    ws = ecc_workspace(N, shape, prev.device) if ws is None else ws
    outs = [torch.empty_like(prev) for _ in range(4)]
    prm = _ecc_struct(p)
    check(_lib.load().st_cmc_ecc_prepare(ptr(prev), ptr(curr), N, int(img_h), int(img_w), C.byref(prm), ptr(ws),
                                         ws.numel(), *[ptr(o) for o in outs], current_stream()), 'st_cmc_ecc_prepare')
    return tuple(outs)


def ecc_step(prev, curr, img_h, img_w, params=None, warps=None, ws=None):
    """ONE iteration (rules E3 .. E8) from the plane warps `warps` ((N, 2, 3) float64, None: identity) -> (N, 72)
    float64 device tensor; ecc_step_fields() names its columns.  Test-facing, the launches of ecc_estimate."""
    p = ecc_params(params)
    prev, curr, N, shape = _ecc_planes(prev, curr, img_h, img_w, p)
    ws = ecc_workspace(N, shape, prev.device) if ws is None else ws
    win = None
    if warps is not None:
        win = torch.as_tensor(np.asarray(warps, np.float64).reshape(N, 6)).to(prev.device)
    out = torch.empty(N, ECC_STEP_DOUBLES, dtype=torch.float64, device=prev.device)
    prm = _ecc_struct(p)
    check(_lib.load().st_cmc_ecc_step(ptr(prev), ptr(curr), N, int(img_h), int(img_w), C.byref(prm), ptr(win), ptr(ws),
                                      ws.numel(), ptr(out), current_stream()), 'st_cmc_ecc_step')
    return out


def ecc_step_fields(row, warp_mode='MOTION_EUCLIDEAN'):
    """One host row of ecc_step() -> dict (H (K, K), iP / tP / dp (K,), warp (2, 3), scalars as floats)."""
    row = np.asarray(row, np.float64)
    K = (2, 3, 6)[ECC_MODES[warp_mode]]
    d = {}
    for k, (o, n) in ECC_STEP_FIELDS.items():
        d[k] = float(row[o]) if n == 1 else row[o:o + n].copy()
    d['H'] = d['H'].reshape(6, 6)[:K, :K]
    for k in ('iP', 'tP', 'dp'):
        d[k] = d[k][:K]
    d['warp'] = d['warp'].reshape(2, 3)
    d['valid'], d['n'] = bool(d['valid']), int(d['n'])
    return d


def ecc_estimate(prev, curr, img_h, img_w, params=None, with_iters=False, ws=None):
    """ECC warps of the plane pairs (template prev[n], input curr[n]) on the device -> (N, 8) fp32 device tensor
    [valid, rho, 2 x 3 warp in image coordinates] (+ the iterations run, (N,) int32, with with_iters).  Every round is
    enqueued on the current stream; the host does not wait."""
    p = ecc_params(params)
    prev, curr, N, shape = _ecc_planes(prev, curr, img_h, img_w, p)
    ws = ecc_workspace(N, shape, prev.device) if ws is None else ws
    warps = torch.empty(N, WARP_FLOATS, device=prev.device)
    iters = torch.empty(N, dtype=torch.int32, device=prev.device) if with_iters else None
    prm = _ecc_struct(p)
    check(_lib.load().st_cmc_ecc_estimate(ptr(prev), ptr(curr), N, int(img_h), int(img_w), C.byref(prm), ptr(ws),
                                          ws.numel(), ptr(warps), ptr(iters), current_stream()), 'st_cmc_ecc_estimate')
    return (warps, iters) if with_iters else warps


# ---- one estimator object per method: what the tracker and the MOT shell call ------------------------------------------
class MeshAffineEstimator:
    """cmc=dict(method='glme_affine', glme=...): equalised 255 x 255 uint8 planes, Farneback flow, consensus fit."""
    mode, plane_dtype = 'mesh_affine', torch.uint8

    def __init__(self, options=None):
        self.params = glme_params(options)

    def plane_shape(self, h, w):
        return SIDE, SIDE

    def front(self, img, h, w, out=None):
        return front(img, h, w, out=out)

    def estimate(self, prev, curr, h, w):
        return estimate(prev, curr, h, w, self.params)


class EccEstimator:
    """cmc=dict(method='ecc', ecc=...): fp32 grey planes of the frame / downscale, ECC iterations."""
    mode, plane_dtype = 'ecc', torch.float32

    def __init__(self, options=None):
        self.params = ecc_params(options)

    def plane_shape(self, h, w):
        return ecc_plane_shape(h, w, self.params['downscale'])

    def front(self, img, h, w, out=None):
        return ecc_front(img, h, w, self.params['downscale'], out=out)

    def estimate(self, prev, curr, h, w):
        return ecc_estimate(prev, curr, h, w, self.params)


def estimator(cmc):
    """The tracker option cmc=dict(method=..., <method's options>) -> estimator object, None when CMC is off."""
    method = cmc.get('method') if cmc is not None else None
    if method is None:
        return None
    if method == 'glme_affine':
        return MeshAffineEstimator(cmc.get('glme'))
    if method == 'ecc':
        return EccEstimator(cmc.get('ecc'))
    raise ValueError(f"Unknown cmc method '{method}', expected 'glme_affine', 'ecc' or None.")


class CmcFrame:
    """One frame's CMC input as the MOT shell's chunk path hands it to the tracker: its grey plane (already on the
    device), its frame id, and the speculative warp of the pair (warp_src, this frame) computed with the chunk."""
    __slots__ = ('plane', 'fid', 'warp', 'warp_src')

    def __init__(self, plane, fid, warp=None, warp_src=-2):
        self.plane, self.fid, self.warp, self.warp_src = plane, int(fid), warp, int(warp_src)
