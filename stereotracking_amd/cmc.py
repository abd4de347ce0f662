"""Mesh-Affine camera-motion compensation (CMC) of the tracker: the device half (estimate) and the host half (apply).

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


class CmcFrame:
    """One frame's CMC input as the MOT shell's chunk path hands it to the tracker: its grey plane (already on the
    device), its frame id, and the speculative warp of the pair (warp_src, this frame) computed with the chunk."""
    __slots__ = ('plane', 'fid', 'warp', 'warp_src')

    def __init__(self, plane, fid, warp=None, warp_src=-2):
        self.plane, self.fid, self.warp, self.warp_src = plane, int(fid), warp, int(warp_src)
