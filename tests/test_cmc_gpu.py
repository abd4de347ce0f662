"""GPU: Mesh-Affine camera-motion compensation (csrc/cmc_flow.hip) against the numpy restatement (tests/cmc_ref.py),
on known camera motion, for its purpose (identities kept through camera pans), and through the MOT shell's chunk path."""
import numpy as np
import pytest
import torch

import cmc_ref as R
from test_cpu_cmc import CORNER_TOL, CORNER_TOL_MOVING, MOVING, _corner_error, moving_pair

pytestmark = pytest.mark.gpu
H, W = 720, 1280


def _bgr(gray_frames, pad=(736, 1280)):
    """grey uint8 (h, w) frames -> padded fp32 (N, 3, H, W) BGR batch (channels differ) and the uint8 (1, 3, h, w) frames."""
    u8 = []
    for g in gray_frames:
        g = g.astype(np.int32)
        u8.append(np.stack([np.clip(g - 9, 0, 255), g, np.clip(255 - g // 2, 0, 255)]).astype(np.uint8))
    h, w = gray_frames[0].shape
    f32 = np.full((len(u8), 3) + pad, 114.0, np.float32)
    for i, f in enumerate(u8):
        f32[i, :, :h, :w] = f
    return f32, u8


def test_front_bit_exact_u8_and_f32(cuda):
    from stereotracking_amd import cmc
    frames = [R.warp_texture(H, W, R.similarity(tx=3 * i), seed=2) for i in range(3)]
    frames.append(np.full((H, W), 90, np.uint8))                          # constant frame: equalizeHist keeps it
    f32, u8 = _bgr(frames)
    want = np.stack([R.front(f, H, W) for f in u8])
    a = cmc.front(torch.from_numpy(f32).to(cuda), H, W).cpu().numpy()
    b = cmc.front([torch.from_numpy(f)[None].to(cuda) for f in u8], H, W).cpu().numpy()
    assert np.array_equal(a, want) and np.array_equal(b, want)
    assert np.array_equal(want[3], np.full((255, 255), want[3, 0, 0]))


def _planes(cuda, A, seed=1, moving=None):
    from stereotracking_amd import cmc
    f0, f1 = moving_pair(A, seed, moving)
    _, u8 = _bgr([f0, f1])
    p = cmc.front([torch.from_numpy(f)[None].to(cuda) for f in u8], H, W)
    return p[0:1], p[1:2]


def test_flow_field_vs_float64_restatement_per_level(cuda):
    from stereotracking_amd import cmc
    prev, curr = _planes(cuda, R.similarity(tx=6.5, ty=-3.2, deg=0.4, scale=1.005, cx=640, cy=360))
    _, lev = cmc.flow(prev, curr, 31, per_level=True)
    pp, pc = prev[0].cpu().numpy(), curr[0].cpu().numpy()
    ref64 = R.farneback(pp, pc, 31, np.float64, per_level=True)
    ref32 = R.farneback(pp, pc, 31, np.float32, per_level=True)
    assert len(lev) == len(ref64) == 3
    for k, (g, r64, r32) in enumerate(zip(lev, ref64, ref32)):
        g = g[0].cpu().numpy().astype(np.float64)
        d_gpu = np.abs(g - r64).max()
        d_32 = np.abs(r32.astype(np.float64) - r64).max()
        assert d_gpu <= 2 * d_32 + 1e-5, f'level {k}: gpu {d_gpu:.3g} vs fp32 restatement {d_32:.3g}'


def test_mesh_and_fit_vs_restatement(cuda):
    from stereotracking_amd import cmc
    prev, curr = _planes(cuda, R.similarity(tx=9.0, ty=4.0, deg=-0.3, cx=640, cy=360), moving=(0, 400, 0, 700))
    fl = cmc.flow(prev, curr, 31)[0].cpu().numpy()
    warps, mesh, inl = cmc.estimate(prev, curr, H, W, None, with_mesh=True)
    mesh, inl, row = mesh[0].cpu().numpy(), inl[0].cpu().numpy().astype(bool), warps[0].cpu().numpy()
    src, dst = R.mesh(fl, H, W, 16)
    assert np.array_equal(mesh[:, 0:2], src) and np.array_equal(mesh[:, 2:4], dst)
    warp, ratio, rinl = R.consensus_fit(src, dst, 5.0, 0.3, np.float32)
    res = R.residuals(src, dst, R.lsq_similarity(src[rinl], dst[rinl]))
    # whatever the flags: the warp is the least-squares refit over the device's own inlier set, the ratio its size
    own = R.lsq_similarity(src[inl], dst[inl])
    np.testing.assert_allclose(row[2:].reshape(2, 3), own, rtol=1e-4, atol=1e-4 * np.abs(own).max())
    assert row[1] == np.float32(inl.sum()) / np.float32(len(inl)) and row[0] == (1.0 if row[1] >= np.float32(0.3) else 0.0)
    differ = inl != rinl
    if differ.any():     # only points whose residual sits on the threshold may differ
        assert np.all(np.abs(res[differ] - 5.0) <= 1e-3 + 1e-3 * 5), f'{differ.sum()} inlier flags differ'
    else:
        assert row[0] == 1 and abs(row[1] - ratio) < 1e-6
        np.testing.assert_allclose(row[2:].reshape(2, 3), warp, rtol=1e-4, atol=1e-4 * np.abs(warp).max())


@pytest.mark.parametrize('A,moving', [
    (R.similarity(tx=7.3, ty=-4.6), None),
    (R.similarity(deg=0.5, cx=640, cy=360), None),
    (R.similarity(scale=1.01, cx=640, cy=360), None),
    (R.similarity(tx=5.0, deg=0.5, scale=1.01, cx=640, cy=360), MOVING),
], ids=['translation', 'rotation', 'scale', 'moving-region'])
def test_known_camera_motion(A, moving, cuda):
    from stereotracking_amd import cmc
    prev, curr = _planes(cuda, A, moving=moving)
    row = cmc.estimate(prev, curr, H, W)[0].cpu().numpy()
    warp = cmc.warp_or_none(row)
    assert warp is not None and row[1] >= (0.5 if moving else 0.9)
    assert _corner_error(warp, A) <= (CORNER_TOL_MOVING if moving else CORNER_TOL)


def test_constant_frame_gives_identity(cuda):
    from stereotracking_amd import cmc
    _, u8 = _bgr([np.full((H, W), 120, np.uint8)] * 2)
    p = cmc.front([torch.from_numpy(f)[None].to(cuda) for f in u8], H, W)
    warp = cmc.warp_or_none(cmc.estimate(p[0:1], p[1:2], H, W)[0].cpu().numpy())
    assert warp is not None and np.abs(warp - np.array([[1, 0, 0], [0, 1, 0]])).max() < 1e-5


# ---- purpose: a panning camera over static objects ------------------------------------------------------------------------
def _panning_scene(T=30, K=12, seed=4):
    rng = np.random.default_rng(seed)
    objs = rng.uniform([350, 200], [1500, 850], (K, 2))     # world positions of static small objects
    # camera offset: still (tracks confirmed, CMC images established), then pans that start and reverse abruptly
    vel = [np.zeros(2)] * 6 + [np.array([12.0, 0.0])] * 8 + [np.array([-12.0, 0.0])] * 8 + [np.array([0.0, 12.0])] * T
    cam = np.cumsum([np.zeros(2)] + vel[:T - 1], 0) + np.array([100.0, 50.0])
    return objs, cam


def _render(cam, seed=4):
    A = R.similarity(tx=-cam[0], ty=-cam[1])
    return R.warp_texture(H, W, A, seed=seed, cutoff=0.05)


def _track_panning(backend, with_cmc, cuda, frames, objs, cam):
    from stereotracking_amd.motion import KalmanFilter
    from stereotracking_amd.structures import InstanceData, TrackDataSample
    from stereotracking_amd.trackers import OCSORTTracker_Disparity

    class _M:
        motion = KalmanFilter()
    trk = OCSORTTracker_Disparity(obj_score_thr=0.3, init_track_thr=0.7, weight_iou_with_det_scores=False,
                                  match_iou_thr=0.3, num_tentatives=3, vel_delta_t=3, num_frames_retain=30,
                                  backend=backend, cmc=dict(method='glme_affine') if with_cmc else None)
    gt, pred = [], []
    for t, f in enumerate(frames):
        p = objs - cam[t]
        vis = (p[:, 0] > 20) & (p[:, 0] < W - 20) & (p[:, 1] > 20) & (p[:, 1] < H - 20)
        boxes = np.concatenate([p - 10, p + 10], 1)[vis].astype(np.float32)        # 20 x 20 px boxes
        n = len(boxes)
        s = TrackDataSample(dict(frame_id=t, img_shape=(H, W)))
        s.pred_det_instances = InstanceData(bboxes=torch.from_numpy(boxes), scores=torch.full((n,), 0.9),
                                            labels=torch.zeros(n, dtype=torch.long), depth=torch.full((n,), 10.0),
                                            scales=torch.ones(n))
        img = torch.from_numpy(_bgr([f])[0]).to(cuda)
        out = trk.track(_M(), img, None, s)
        for k, i in enumerate(np.nonzero(vis)[0]):
            gt.append([t + 1, i + 1, boxes[k, 0], boxes[k, 1], 20, 20])
        b = out.bboxes.cpu().numpy()
        for k, tid in enumerate(out.instances_id.cpu().tolist()):
            pred.append([t + 1, tid + 1, b[k, 0], b[k, 1], b[k, 2] - b[k, 0], b[k, 3] - b[k, 1]])
    return np.array(gt), np.array(pred)


def test_cmc_keeps_identities_through_camera_pans(cuda):
    from stereotracking_amd.metrics import clear_identity
    objs, cam = _panning_scene()
    frames = [_render(c) for c in cam]
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


# ---- the shell's chunk path -----------------------------------------------------------------------------------------------
def test_shell_chunk_path_equals_per_frame_tracking(cuda):
    """test_step over 64 frames with CMC on (speculative warps per chunk, on-demand pairs after detection-free frames)
    gives the ids and rows of per-frame tracker.track(img=...) calls on the same detections."""
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.structures import InstanceData, TrackDataSample
    from stereotracking_amd.synthetic import synthetic_batch, synthetic_state_dict
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(root, 'configs', 'stereo_tracking', 'ocsort',
                                       'stereo_yolox_s_mot_airdrone_costvolume.py'))
    for part in ('backbone', 'neck'):
        cfg.model.detector[part]['widen_factor'] = 0.375
    cfg.model.detector.bbox_head.head_module['widen_factor'] = 0.375
    cfg.model.stereo['max_disp'] = 32
    cfg.model.tracker['init_track_thr'] = 0.03
    cfg.model.tracker['obj_score_thr'] = 0.02
    cfg.model.tracker['cmc'] = dict(method='glme_affine')
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
    captured = []
    orig = model.tracker.track_records

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

    from stereotracking_amd.motion import KalmanFilter
    from stereotracking_amd.trackers import OCSORTTracker_Disparity

    class _M:
        motion = KalmanFilter()
    for backend in ('native', 'python'):
        trk = OCSORTTracker_Disparity(**{k: v for k, v in cfg.model.tracker.items() if k != 'type'}, backend=backend)
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
