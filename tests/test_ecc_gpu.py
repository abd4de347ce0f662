"""GPU: ECC camera-motion compensation (csrc/cmc_ecc.hip) against the numpy restatement (tests/ecc_ref.py) on the
scenarios of tests/ecc_cases.py (their preconditions: tests/test_cpu_ecc.py), its refusals, and its purpose: identities
kept through camera pans, the MOT shell's chunk path, and the registered CameraMotionCompensation.

Bounds.  Front and prepare are exact (rules E0 - E2).  A float the device derives from fp32 per-pixel arithmetic lies
within 4 x |fp32 restatement - float64 restatement| + floor of the float64 restatement.  The floor covers what the two
fp32 computations share exactly (the identity warp: every bilinear weight is 0 or 1, the two restatements agree to the
bit) but float64 sums do not: the device sums in another order and derives the zero-mean sums from raw moments, which
cancels up to 4 digits (raw J^T Iw against J^T Iz) before the solve (condition up to 1e5 for AFFINE) - 1e-16 x 1e4 x
1e5 = 1e-7 of the field's largest magnitude."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cmc_ref as R
import ecc_cases as K
import ecc_ref as E

pytestmark = pytest.mark.gpu
FLOOR = 1e-7


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order='C')).to(cuda)      # a copy: the cached scenario planes are read-only


def _within(got, r64, r32, what):
    got, r64, r32 = (np.asarray(a, np.float64) for a in (got, r64, r32))
    d_gpu, d_32 = np.abs(got - r64).max(), np.abs(r32 - r64).max()
    bound = 4 * d_32 + FLOOR * max(1.0, np.abs(r64).max())
    print(f'{what}: |gpu - f64| = {d_gpu:.3g}, |f32 - f64| = {d_32:.3g}, bound {bound:.3g}')
    assert d_gpu <= bound, f'{what}: gpu {d_gpu:.3g} vs fp32 restatement {d_32:.3g} (bound {bound:.3g})'


# ---- front ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geometry', K.FRONT, ids=lambda g: 'x'.join(map(str, g)))
def test_front_bit_exact_both_forms(geometry, cuda):
    from stereotracking_amd import cmc
    fh, fw, h, w, s = geometry
    frames = [K.front_frame(fh, fw, seed=10 * s + i) for i in range(3)]
    want = np.stack([E.front(f, h, w, s) for f in frames])
    a = cmc.ecc_front([_dev(f[None], cuda) for f in frames], h, w, s).cpu().numpy()
    b = cmc.ecc_front(_dev(np.stack([K.canvas_f32(f) for f in frames]), cuda), h, w, s).cpu().numpy()
    assert a.dtype == np.float32 and a.shape == want.shape
    assert np.array_equal(a, want) and np.array_equal(b, want)


def test_front_list_crosses_the_pointer_chunk(cuda):
    from stereotracking_amd import cmc
    frames = [K.front_frame(48, 80, seed=100 + i) for i in range(K.FRONT_BATCH)]
    want = np.stack([E.front(f, 47, 79, 2) for f in frames])
    got = cmc.ecc_front([_dev(f[None], cuda) for f in frames], 47, 79, 2).cpu().numpy()
    assert np.array_equal(got, want) and len({p.tobytes() for p in got}) == K.FRONT_BATCH


# ---- prepare ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gauss', [1, 3, 5])
@pytest.mark.parametrize('size', K.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_prepare_bit_exact(size, gauss, cuda):
    from stereotracking_amd import cmc
    ph, pw = size
    # templates with fractional values (multiples of 1 / 16: a downscale-4 front), inputs with integral values
    T = np.stack([E.front(K.front_frame(4 * ph, 4 * pw, seed=7 + i), 4 * ph, 4 * pw, 4) for i in range(2)])
    I = np.stack([K.pair(size, 1, 'rot')[1], K.pair(size, 2, 'big')[1]])
    got = cmc.ecc_prepare(_dev(T, cuda), _dev(I, cuda), ph, pw, dict(gauss_filt_size=gauss, downscale=1))
    for n in range(2):
        want = E.prepare(T[n], I[n], gauss, np.float32)
        for g, w, what in zip(got, want, ('template', 'input', 'gx', 'gy')):
            assert np.array_equal(g[n].cpu().numpy(), w), f'{what} of pair {n}'


# ---- one step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', K.MODES, ids=lambda m: K.MODE_NAMES[m])
@pytest.mark.parametrize('size', K.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_step_vs_restatement_batch_and_repeat(size, mode, cuda):
    from stereotracking_amd import cmc
    ph, pw = size
    rows = K.step_rows(size)
    r64 = K.step_reference(size, mode, K.STEP_GAUSS, 'f64')
    r32 = K.step_reference(size, mode, K.STEP_GAUSS, 'f32')
    prm = dict(warp_mode=K.MODE_NAMES[mode], gauss_filt_size=K.STEP_GAUSS, downscale=1)
    T, I = _dev(np.stack([r[0] for r in rows]), cuda), _dev(np.stack([r[1] for r in rows]), cuda)
    M = np.stack([r[2] for r in rows])
    batch = cmc.ecc_step(T, I, ph, pw, prm, warps=M).cpu().numpy()
    for n in range(3):
        d = cmc.ecc_step_fields(batch[n], K.MODE_NAMES[mode])
        assert d['valid'] and d['n'] == r64[n]['n'] == r32[n]['n']
        for f in K.STEP_FIELDS:
            _within(d[f], r64[n][f], r32[n][f], f'row {n} {f}')
    # a pair's row does not depend on N
    for n in range(3):
        one = cmc.ecc_step(T[n:n + 1], I[n:n + 1], ph, pw, prm, warps=M[n:n + 1]).cpu().numpy()
        assert np.array_equal(one[0], batch[n]), f'row {n} differs between N = 3 and N = 1'
    # a repeat over a workspace of stale bits
    ws = cmc.ecc_workspace(3, size, cuda)
    ws.fill_(0xA5)
    again = cmc.ecc_step(T, I, ph, pw, prm, warps=M, ws=ws).cpu().numpy()
    ws.view(torch.float64)[:].fill_(float('nan'))
    third = cmc.ecc_step(T, I, ph, pw, prm, warps=M, ws=ws).cpu().numpy()
    assert np.array_equal(again, batch) and np.array_equal(third, batch)
    if mode == E.EUCLIDEAN:       # warps=None is the identity
        ident = cmc.ecc_step(T[:1], I[:1], ph, pw, prm).cpu().numpy()
        assert np.array_equal(ident[0], batch[0])


# ---- estimate -----------------------------------------------------------------------------------------------------------------
def _row_bound(got, name, r64, r32, s):
    row64 = np.concatenate([[1.0, r64[1]], E.to_image(r64[2], s).ravel()])
    row32 = np.concatenate([[1.0, r32[1]], E.to_image(r32[2], s).ravel()])
    d_gpu, d_32 = np.abs(got.astype(np.float64) - row64), np.abs(row32 - row64)
    # + the rounding of the fp32 output
    bound = 4 * d_32.max() + FLOOR + 2.0 ** -23 * np.maximum(1.0, np.abs(row64))
    print(f'{name}: |gpu - f64| = {d_gpu.max():.3g}, |f32 - f64| = {d_32.max():.3g}')
    assert np.all(d_gpu <= bound), f'{name}: gpu {d_gpu.max():.3g} vs fp32 restatement {d_32.max():.3g}'


@pytest.mark.parametrize('name', list(K.ESTIMATE))
def test_estimate_vs_restatement(name, cuda):
    from stereotracking_amd import cmc
    c = K.ESTIMATE[name]
    T, I, A = K.estimate_inputs(name)
    r64, r32 = K.estimate_reference(name, 'f64'), K.estimate_reference(name, 'f32')
    img_h, img_w = K.image_size(name)
    prm = dict(warp_mode=K.MODE_NAMES[c['mode']], num_iters=c['num_iters'], gauss_filt_size=c['gauss'],
               downscale=c['downscale'])
    warps, iters = cmc.ecc_estimate(_dev(T[None], cuda), _dev(I[None], cuda), img_h, img_w, prm, with_iters=True)
    row, it = warps[0].cpu().numpy(), int(iters[0])
    assert row[0] == 1 and it == r64[3], f'{it} iterations, the restatement runs {r64[3]}'
    _row_bound(row, name, r64, r32, c['downscale'])
    # the corner error to the truth, in plane pixels: the truth in image coordinates, compared at the image corners
    s = c['downscale']
    truth = E.to_image(A, s)
    ih, iw = c['size'][0] * s, c['size'][1] * s
    assert E.corner_error(row[2:].reshape(2, 3), truth, ih, iw) / s <= 0.25
    again = cmc.ecc_estimate(_dev(T[None], cuda), _dev(I[None], cuda), img_h, img_w, prm)[0].cpu().numpy()
    assert np.array_equal(again, row), 'not bit-identical from run to run'


def test_estimate_mixed_batch_equals_single_runs(cuda):
    from stereotracking_amd import cmc
    prm = dict(num_iters=K.MIXED_ITERS, downscale=1)
    pairs = [K.estimate_inputs(n) for n in K.MIXED_BATCH]
    T, I = _dev(np.stack([p[0] for p in pairs]), cuda), _dev(np.stack([p[1] for p in pairs]), cuda)
    warps, iters = cmc.ecc_estimate(T, I, 90, 160, prm, with_iters=True)
    warps, iters = warps.cpu().numpy(), iters.cpu().numpy()
    for n, name in enumerate(K.MIXED_BATCH):
        w1, i1 = cmc.ecc_estimate(T[n:n + 1], I[n:n + 1], 90, 160, prm, with_iters=True)
        assert np.array_equal(w1[0].cpu().numpy(), warps[n]) and int(i1[0]) == iters[n], name
        r64 = K.estimate_reference(name, 'f64', K.MIXED_ITERS)
        assert iters[n] == r64[3] and warps[n, 0] == 1
        _row_bound(warps[n], name, r64, K.estimate_reference(name, 'f32', K.MIXED_ITERS), 1)
    assert iters[0] < K.MIXED_ITERS == iters[1]


def test_estimate_failures_are_finite_and_invalid(cuda):
    from stereotracking_amd import cmc
    fail = np.array([0, 0, 1, 0, 0, 0, 1, 0], np.float32)
    for mode in K.MODES:
        T, I = K.constant_pair()
        w, it = cmc.ecc_estimate(_dev(T[None], cuda), _dev(I[None], cuda), 48, 80,
                                 dict(warp_mode=K.MODE_NAMES[mode], downscale=1), with_iters=True)
        assert np.array_equal(w[0].cpu().numpy(), fail) and int(it[0]) == 1
    T, I = K.uncorrelated_pair()
    ref = E.estimate(T, I, K.UNCORRELATED_MODE)
    # beside a good pair: the failed row fails alone
    Tg, Ig, _ = K.estimate_inputs('affine_small')
    w, it = cmc.ecc_estimate(_dev(np.stack([T, Tg]), cuda), _dev(np.stack([I, Ig]), cuda), 48, 80,
                             dict(warp_mode=K.MODE_NAMES[K.UNCORRELATED_MODE], downscale=1), with_iters=True)
    w = w.cpu().numpy()
    assert np.isfinite(w).all() and np.array_equal(w[0], fail) and int(it[0]) == ref[3]
    assert w[1, 0] == 1


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(cuda):
    from stereotracking_amd import _lib, cmc
    from stereotracking_amd._lib import current_stream, ptr
    lib = _lib.load()
    N, ph, pw = 2, 48, 80
    T = torch.rand(N, ph, pw, device=cuda)
    I = torch.rand(N, ph, pw, device=cuda)
    ws = cmc.ecc_workspace(N, (ph, pw), cuda)
    assert ws.numel() > 0 and lib.st_cmc_ecc_workspace_bytes(0, ph, pw) == 0
    a, b = C.c_int(), C.c_int()
    assert lib.st_cmc_ecc_plane_size(97, 163, 4, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (24, 40)
    assert lib.st_cmc_ecc_plane_size(97, 163, 3, C.byref(a), C.byref(b)) != 0
    SENT = 123.0
    warps = torch.full((N, 8), SENT, device=cuda)
    iters = torch.full((N,), 77, dtype=torch.int32, device=cuda)
    step = torch.full((N, cmc.ECC_STEP_DOUBLES), SENT, dtype=torch.float64, device=cuda)
    outs = [torch.full((N, ph, pw), SENT, device=cuda) for _ in range(4)]
    planes = torch.full((N, ph, pw), SENT, device=cuda)

    def P(**kw):
        p = dict(struct_size=C.sizeof(_lib.StEccParams), warp_mode=1, num_iters=50, stop_eps=1e-3, gauss_filt_size=1,
                 downscale=1)
        p.update(kw)
        return _lib.StEccParams(p['struct_size'], p['warp_mode'], p['num_iters'], p['stop_eps'], p['gauss_filt_size'],
                                p['downscale'])

    def calls(prm, t=T, i=I, w=ws, nbytes=None, h=ph, wd=pw, wout=warps, sout=step, which=(0, 1, 2)):
        """Return codes of st_cmc_ecc_estimate / _step / _prepare (those in `which`) on one bad argument set."""
        nbytes = w.numel() if nbytes is None and w is not None else (nbytes or 0)
        pp = C.byref(prm) if prm is not None else None
        s = current_stream()
        fns = [lambda: lib.st_cmc_ecc_estimate(ptr(t), ptr(i), N, h, wd, pp, ptr(w), nbytes, ptr(wout), ptr(iters), s),
               lambda: lib.st_cmc_ecc_step(ptr(t), ptr(i), N, h, wd, pp, None, ptr(w), nbytes, ptr(sout), s),
               lambda: lib.st_cmc_ecc_prepare(ptr(t), ptr(i), N, h, wd, pp, ptr(w), nbytes, *[ptr(o) for o in outs], s)]
        return [fns[k]() for k in which]

    bad = [calls(P(struct_size=8)), calls(None), calls(P(), t=None), calls(P(), i=None), calls(P(), w=None),
           calls(P(), nbytes=ws.numel() - 1), calls(P(warp_mode=3)), calls(P(warp_mode=-1)), calls(P(downscale=3)),
           calls(P(downscale=0)), calls(P(gauss_filt_size=2)), calls(P(gauss_filt_size=7)), calls(P(num_iters=0)),
           calls(P(), h=7), calls(P(downscale=4), h=31, wd=80), calls(P(), wout=None, which=(0,)),
           calls(P(), sout=None, which=(1,))]
    assert all(rc != 0 for group in bad for rc in group), bad
    frame = torch.zeros(1, 3, 48, 80, dtype=torch.uint8, device=cuda)
    ok = (C.c_void_p * 2)(frame.data_ptr(), frame.data_ptr())
    null2 = (C.c_void_p * 2)(frame.data_ptr(), None)
    s = current_stream()
    assert lib.st_cmc_ecc_front_u8(null2, 2, 48, 80, 48, 80, 1, ptr(planes), s) != 0      # every pointer before a launch
    assert lib.st_cmc_ecc_front_u8(ok, 2, 48, 80, 48, 80, 3, ptr(planes), s) != 0
    assert lib.st_cmc_ecc_front_u8(ok, 2, 48, 80, 49, 80, 1, ptr(planes), s) != 0         # crop larger than the frame
    assert lib.st_cmc_ecc_front_u8(None, 2, 48, 80, 48, 80, 1, ptr(planes), s) != 0
    assert lib.st_cmc_ecc_front_u8(ok, 2, 48, 80, 48, 80, 1, None, s) != 0
    assert lib.st_cmc_ecc_front_f32(ptr(T), 1, 16, 80, 16, 80, 3, ptr(planes), s) != 0
    assert lib.st_cmc_ecc_front_f32(None, 1, 16, 80, 16, 80, 1, ptr(planes), s) != 0
    torch.cuda.synchronize()
    for t in [warps, step, planes] + outs:
        assert bool((t == SENT).all())
    assert bool((iters == 77).all())
    # the Python layer refuses planes that are not the size the library derives
    with pytest.raises(ValueError):
        cmc.ecc_estimate(T, I, 96, 160, dict(downscale=1))
    with pytest.raises(ValueError):
        cmc.ecc_estimate(T, I[:1], 48, 80, dict(downscale=1))


# ---- purpose: a panning camera over static objects ----------------------------------------------------------------------------
H, W = 192, 320


def _bgr(gray_frames, pad=(192, 320)):
    """grey uint8 (h, w) frames -> padded fp32 (N, 3, H, W) BGR batch whose channels differ."""
    u8 = []
    for g in gray_frames:
        g = g.astype(np.int32)
        u8.append(np.stack([np.clip(g - 9, 0, 255), g, np.clip(255 - g // 2, 0, 255)]).astype(np.uint8))
    h, w = gray_frames[0].shape
    f32 = np.full((len(u8), 3) + pad, 114.0, np.float32)
    for i, f in enumerate(u8):
        f32[i, :, :h, :w] = f
    return f32


def _panning_scene(T=30, K=12, seed=6, pan=8.0):
    rng = np.random.default_rng(seed)
    objs = rng.uniform([90, 50], [375, 212], (K, 2))        # world positions of static small objects
    # camera offset: still (tracks confirmed, CMC images established), then pans that start and reverse abruptly
    vel = [np.zeros(2)] * 6 + [np.array([pan, 0.0])] * 8 + [np.array([-pan, 0.0])] * 8 + [np.array([0.0, pan])] * T
    cam = np.cumsum([np.zeros(2)] + vel[:T - 1], 0) + np.array([25.0, 12.0])
    return objs, cam


def _track_panning(backend, with_cmc, cuda, frames, objs, cam, box=12.0):
    from stereotracking_amd.motion import KalmanFilter
    from stereotracking_amd.structures import InstanceData, TrackDataSample
    from stereotracking_amd.trackers import OCSORTTracker_Disparity

    class _M:
        motion = KalmanFilter()
    trk = OCSORTTracker_Disparity(obj_score_thr=0.3, init_track_thr=0.7, weight_iou_with_det_scores=False,
                                  match_iou_thr=0.3, num_tentatives=3, vel_delta_t=3, num_frames_retain=30,
                                  backend=backend, cmc=dict(method='ecc') if with_cmc else None)
    gt, pred = [], []
    for t, img in enumerate(frames):
        p = objs - cam[t]
        vis = (p[:, 0] > 8) & (p[:, 0] < W - 8) & (p[:, 1] > 8) & (p[:, 1] < H - 8)
        boxes = np.concatenate([p - box / 2, p + box / 2], 1)[vis].astype(np.float32)
        n = len(boxes)
        s = TrackDataSample(dict(frame_id=t, img_shape=(H, W)))
        s.pred_det_instances = InstanceData(bboxes=torch.from_numpy(boxes), scores=torch.full((n,), 0.9),
                                            labels=torch.zeros(n, dtype=torch.long), depth=torch.full((n,), 10.0),
                                            scales=torch.ones(n))
        out = trk.track(_M(), img, None, s)
        for k, i in enumerate(np.nonzero(vis)[0]):
            gt.append([t + 1, i + 1, boxes[k, 0], boxes[k, 1], box, box])
        b = out.bboxes.cpu().numpy()
        for k, tid in enumerate(out.instances_id.cpu().tolist()):
            pred.append([t + 1, tid + 1, b[k, 0], b[k, 1], b[k, 2] - b[k, 0], b[k, 3] - b[k, 1]])
    return np.array(gt), np.array(pred)


def test_ecc_keeps_identities_through_camera_pans(cuda):
    from stereotracking_amd.metrics import clear_identity
    objs, cam = _panning_scene()
    frames = [_dev(_bgr([R.warp_texture(H, W, R.similarity(tx=-c[0], ty=-c[1]), seed=4, cutoff=0.02)]), cuda)
              for c in cam]
    res = {}
    for backend in ('native', 'python'):
        for on in (False, True):
            res[backend, on] = _track_panning(backend, on, cuda, frames, objs, cam)
    for on in (False, True):
        assert np.array_equal(res['native', on][1], res['python', on][1]), 'backends differ'
    off = clear_identity(*res['native', False])
    on = clear_identity(*res['native', True])
    assert off['IDSW'] > 0, 'the scene does not challenge the tracker without CMC'
    assert on['IDSW'] < off['IDSW'] and on['IDF1'] > off['IDF1'], (off, on)


# ---- the shell's chunk path -----------------------------------------------------------------------------------------------------
def test_shell_chunk_path_equals_per_frame_tracking(cuda):
    """test_step over 64 frames in 8 chunks with method='ecc' (speculative warps per chunk, on-demand pairs after
    detection-free frames) gives the ids and rows of per-frame tracker.track(img=...) calls on the same detections."""
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.motion import KalmanFilter
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.structures import InstanceData, TrackDataSample
    from stereotracking_amd.synthetic import synthetic_batch, synthetic_state_dict
    from stereotracking_amd.trackers import OCSORTTracker_Disparity
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(root, 'configs', 'stereo_tracking', 'ocsort',
                                       'stereo_yolox_s_mot_airdrone_costvolume.py'))
    for part in ('backbone', 'neck'):
        cfg.model.detector[part]['widen_factor'] = 0.375
    cfg.model.detector.bbox_head.head_module['widen_factor'] = 0.375
    cfg.model.stereo['max_disp'] = 32
    cfg.model.tracker['init_track_thr'] = 0.03
    cfg.model.tracker['obj_score_thr'] = 0.02
    cfg.model.tracker['cmc'] = dict(method='ecc', ecc=dict(downscale=2))
    model = MODELS.build(dict(cfg.model, autotune=False, dense_batch=8, inflight=2))
    table = list(model.detector._table) + [('stereo.' + n, shp) for n, shp in model.stereo.param_table()]
    sd = synthetic_state_dict(table, seed=5, prior_prob=0.2, logit_std=2.5)
    model.detector.load_state_dict(sd, strict=False)
    model.stereo.load_state_dict({k[len('stereo.'):]: v for k, v in sd.items() if k.startswith('stereo.')})
    ori, T = (96, 160), 64
    fr = synthetic_batch(list(range(T)), ori[0], ori[1], 32)
    left = [fr['img'][i:i + 1, :, :ori[0]].to(torch.uint8).to(cuda) for i in range(T)]
    right = [fr['right'][i:i + 1, :, :ori[0]].to(torch.uint8).to(cuda) for i in range(T)]
    # detection-free frames (their records are emptied on the way to the tracker): the next frame's pair is not
    # consecutive, so the chunk path estimates it on demand
    blank = set(range(13, 17)) | {30, 41}
    captured, demands = [], []
    orig = model.tracker.track_records
    est = model.tracker.cmc_estimator
    orig_estimate = est.estimate

    def spy_estimate(prev, curr, h, w):
        demands.append(int(prev.shape[0]))
        return orig_estimate(prev, curr, h, w)
    est.estimate = spy_estimate

    def spy(fids, records, cmc=None):
        records = records.copy()
        for i, f in enumerate(fids):
            if f in blank:
                records[i, 0, 0] = 0
        captured.append((list(fids), records.copy()))
        return orig(fids, records, cmc=cmc)
    model.tracker.track_records = spy
    samples = [TrackDataSample(dict(frame_id=t, ori_shape=ori, img_shape=ori, scale_factor=(1.0, 1.0))) for t in range(T)]
    outs = model.test_step(dict(inputs=dict(img=left, right=right), data_samples=samples))
    torch.cuda.synchronize()
    assert sum(len(o.pred_track_instances) for o in outs) > 0
    recs = {f: r for fids, rr in captured for f, r in zip(fids, rr)}
    assert all(int(recs[t][0, 0]) == 0 for t in blank) and model.tracker.prev_cmc_fid == T - 1
    assert demands.count(8) == T // 8 and demands.count(1) >= 3, 'no on-demand pair was estimated'
    assert tuple(model.tracker.prev_cmc_img.shape) == (1, 48, 80) and model.tracker.prev_cmc_img.dtype == torch.float32

    class _M:
        motion = KalmanFilter()
    used = 0
    for backend in ('native', 'python'):
        trk = OCSORTTracker_Disparity(**{k: v for k, v in cfg.model.tracker.items() if k != 'type'}, backend=backend)
        valid = []
        real = trk.cmc_estimator.estimate
        trk.cmc_estimator.estimate = lambda p, c, h, w: (valid.append(real(p, c, h, w)), valid[-1])[1]
        for t in range(T):
            r = recs[t]
            k = int(r[0, 0])
            rows = torch.from_numpy(r[1:1 + k])
            s = TrackDataSample(dict(frame_id=t, img_shape=ori))
            s.pred_det_instances = InstanceData(bboxes=rows[:, 8:12], scores=rows[:, 4], labels=rows[:, 5].long(),
                                                depth=rows[:, 6], scales=rows[:, 7])
            tr = trk.track(_M(), left[t], None, s)
            got = outs[t].pred_track_instances
            assert tr.instances_id.cpu().tolist() == got.instances_id.tolist(), f'{backend} frame {t}: ids differ'
            assert torch.allclose(tr.scores.cpu(), got.scores), f'{backend} frame {t}: rows differ'
        used += sum(int(v[0, 0]) for v in valid)
    print(f'valid ECC warps applied in the per-frame runs: {used}')


# ---- the registered utility -----------------------------------------------------------------------------------------------------
def test_camera_motion_compensation_recovers_euclidean_motion(cuda):
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.registry import TASK_UTILS
    c = TASK_UTILS.build(dict(type='CameraMotionCompensation'))
    T, I = K.pair((90, 160), 1, 'rot')
    A = K.motion('rot', 90, 160)
    img, ref = (np.repeat(p.astype(np.uint8)[:, :, None], 3, 2) for p in (T, I))      # RGB HWC, grey = the plane
    w = c.get_warp_matrix(img, ref)
    assert isinstance(w, torch.Tensor) and w.shape == (2, 3) and w.dtype == torch.float32
    assert E.corner_error(w.numpy(), A, 90, 160) <= 0.25
    w2 = c.get_warp_matrix(torch.from_numpy(img).to(cuda), torch.from_numpy(ref).to(cuda))
    assert torch.equal(w, w2)
    r64 = K.estimate_reference('early', 'f64')
    assert np.abs(w.numpy() - E.to_image(r64[2], 1)).max() <= 1e-4
    # the boxes follow the motion
    boxes = torch.tensor([[20.0, 30.0, 40.0, 50.0]])
    moved = c.warp_bboxes(boxes, w).numpy()[0]
    want = np.concatenate([A @ [20, 30, 1], A @ [40, 50, 1]])
    assert np.abs(moved - want).max() <= 0.25
    flat = np.full((90, 160, 3), 80, np.uint8)
    with pytest.raises(RuntimeError):
        c.get_warp_matrix(flat, flat)
