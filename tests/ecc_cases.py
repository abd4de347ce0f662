"""Scenarios of the ECC tests (tests/test_cpu_ecc.py asserts their preconditions from the restatement alone,
tests/test_ecc_gpu.py runs them on the device).  Planes are 48 x 80 and 90 x 160: 2 and 8 workgroups of the iterate
kernel (2048 template pixels each), neither a multiple of it."""
import functools

import numpy as np

import cmc_ref as C
import ecc_ref as E

SIZES = ((48, 80), (90, 160))
MODES = (E.TRANSLATION, E.EUCLIDEAN, E.AFFINE)
MODE_NAMES = {E.TRANSLATION: 'MOTION_TRANSLATION', E.EUCLIDEAN: 'MOTION_EUCLIDEAN', E.AFFINE: 'MOTION_AFFINE'}
CUTOFF = 0.04          # band limit of the texture (cycles / px): smooth at the scale of the motions below


def motion(name, ph, pw):
    cx, cy = pw / 2, ph / 2
    return dict(shift=C.similarity(tx=2.3, ty=-1.4),
                rot=C.similarity(tx=1.5, ty=0.8, deg=1.0, cx=cx, cy=cy),
                big=C.similarity(tx=-9.0, ty=4.0, deg=-1.5, cx=cx, cy=cy),
                far=C.similarity(tx=-0.3 * pw, ty=0.2 * ph, deg=2.0, cx=cx, cy=cy))[name]


@functools.lru_cache(maxsize=None)
def pair(size, seed, name):
    """(template, input) fp32 planes with integral values: the texture, and the texture moved by motion(name)."""
    ph, pw = size
    T = C.warp_texture(ph, pw, C.similarity(), seed=seed, cutoff=CUTOFF).astype(np.float32)
    I = C.warp_texture(ph, pw, motion(name, ph, pw), seed=seed, cutoff=CUTOFF).astype(np.float32)
    T.setflags(write=False)
    I.setflags(write=False)
    return T, I


# ---- estimate: name -> size, texture seed, motion, warp mode, gauss_filt_size, num_iters, downscale ----------------------
# `kind`: early = stops on the rho test well before the cap; capped = runs into num_iters; masked = part of the template
# is warped outside the input (tx = -9: a band of about 9 columns), so the mask of rule E3 matters
ESTIMATE = dict(
    early=dict(size=(90, 160), seed=1, motion='rot', mode=E.EUCLIDEAN, gauss=1, num_iters=50, downscale=1, kind='early'),
    capped=dict(size=(90, 160), seed=2, motion='big', mode=E.EUCLIDEAN, gauss=1, num_iters=4, downscale=1, kind='capped'),
    masked=dict(size=(90, 160), seed=1, motion='big', mode=E.EUCLIDEAN, gauss=1, num_iters=50, downscale=1, kind='masked'),
    affine=dict(size=(90, 160), seed=3, motion='rot', mode=E.AFFINE, gauss=1, num_iters=50, downscale=1, kind='early'),
    affine_small=dict(size=(48, 80), seed=2, motion='rot', mode=E.AFFINE, gauss=1, num_iters=50, downscale=2, kind='early'),
    translation=dict(size=(90, 160), seed=1, motion='shift', mode=E.TRANSLATION, gauss=5, num_iters=50, downscale=4,
                     kind='early'),
    blur3=dict(size=(48, 80), seed=3, motion='rot', mode=E.EUCLIDEAN, gauss=3, num_iters=50, downscale=1, kind='early'),
    blur5=dict(size=(48, 80), seed=2, motion='rot', mode=E.EUCLIDEAN, gauss=5, num_iters=50, downscale=1, kind='early'),
)
# one batch of the early-stopping, the capped and the masked pair (one plane size, one option set: the cap of `capped`)
MIXED_BATCH = ('early', 'capped', 'masked')
MIXED_ITERS = 4


def estimate_inputs(name):
    c = ESTIMATE[name]
    T, I = pair(c['size'], c['seed'], c['motion'])
    return T, I, motion(c['motion'], *c['size'])


@functools.lru_cache(maxsize=None)
def estimate_reference(name, dt, num_iters=None):
    """(valid, rho, plane warp, iterations, gaps) of the restatement in dtype `dt` ('f64' / 'f32')."""
    c = ESTIMATE[name]
    T, I, _ = estimate_inputs(name)
    return E.estimate(T, I, c['mode'], num_iters or c['num_iters'], 1e-3, c['gauss'],
                      np.float64 if dt == 'f64' else np.float32, trace=True)


def image_size(name):
    """An (img_h, img_w) whose plane at the case's downscale is the case's size (odd remainders: floor)."""
    c = ESTIMATE[name]
    s = c['downscale']
    return c['size'][0] * s + (s - 1), c['size'][1] * s + (s - 1)


# ---- failures (E10) --------------------------------------------------------------------------------------------------------
def constant_pair(size=(48, 80)):
    return np.full(size, 77.0, np.float32), np.full(size, 77.0, np.float32)


UNCORRELATED_MODE = E.AFFINE


def uncorrelated_pair(size=(48, 80)):
    """Two unrelated textures: under UNCORRELATED_MODE the iteration runs into a failure of rule E10 (cv2 raises
    there)."""
    return pair(size, 5, 'shift')[0], pair(size, 11, 'shift')[1]


# ---- one step: (size, mode) -> three (pair, warp) rows of one batch -------------------------------------------------------
def step_warps(size):
    """identity; a known warp near the truth of `rot`; a warp near the truth of `far`, which throws more than a third
    of the template outside the input."""
    ph, pw = size
    near = C.similarity(tx=1.2, ty=0.6, deg=0.8, cx=pw / 2, cy=ph / 2)
    out = C.similarity(tx=-0.3 * pw + 0.4, ty=0.2 * ph - 0.3, deg=1.8, cx=pw / 2, cy=ph / 2)
    return E.IDENTITY.copy(), near, out


def step_rows(size):
    """[(T, I, M)] x 3: different pairs, one per warp."""
    warps = step_warps(size)
    pairs = (pair(size, 1, 'rot'), pair(size, 2, 'rot'), pair(size, 3, 'far'))
    return [(p[0], p[1], M) for p, M in zip(pairs, warps)]


@functools.lru_cache(maxsize=None)
def step_reference(size, mode, gauss, dt):
    out = []
    for T, I, M in step_rows(size):
        d = np.float64 if dt == 'f64' else np.float32
        out.append(E.step(*E.prepare(T, I, gauss, d), M, mode, d))
    return out


STEP_GAUSS = 3          # the step cases run behind the 3-tap blur
STEP_FIELDS = ('mean_i', 'mean_t', 'std_i', 'std_t', 'img_norm', 'tmp_norm', 'corr', 'rho', 'lam', 'H', 'iP', 'tP', 'dp',
               'warp')


# ---- front -----------------------------------------------------------------------------------------------------------------
# (frame h, frame w, crop h, crop w, downscale)
FRONT = ((48, 80, 48, 80, 1), (97, 163, 97, 163, 2), (97, 163, 97, 163, 4), (100, 170, 97, 163, 2), (100, 170, 90, 161, 4))
FRONT_BATCH = 33       # crosses the 32-frame chunk of the pointer table


def front_frame(fh, fw, seed):
    return np.random.default_rng(seed).integers(0, 256, (3, fh, fw), dtype=np.uint8)


def canvas_f32(frame, pad=16, value=114.0):
    """The padded fp32 batch entry of a uint8 frame."""
    _, fh, fw = frame.shape
    out = np.full((3, (fh + pad - 1) // pad * pad + pad, (fw + pad - 1) // pad * pad), value, np.float32)
    out[:, :fh, :fw] = frame
    return out
