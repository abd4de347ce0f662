"""CPU suite: Mesh-Affine camera-motion compensation (CMC) of the tracker - the option, the warp application to the
Kalman states (Python and native backends), the reference's bookkeeping of the previous CMC image, and the numpy
restatement (tests/cmc_ref.py) the GPU kernels are held to (tests/test_cmc_gpu.py)."""
import os

import numpy as np
import pytest
import torch

import cmc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone_disp.py')
# corner error (px, 1280 x 720) within which the float32 restatement recovers a known camera motion from rendered
# frames (measured here: 0.04 px translation, 0.13 px rotation 0.5 deg + scale 1.01); tests/test_cmc_gpu.py uses it
CORNER_TOL = 0.5
# the same with about 30 % of the frame moving on its own (measured here: 2.50 px - the cells straddling the moving
# region's border carry blended medians within the 5 px inlier threshold and pull the least-squares refit)
CORNER_TOL_MOVING = 3.0
MOVING = (300, 720, 600, 1280)     # rows / columns of the region that moves by (-25, 18) instead


def moving_pair(A, seed=1, moving=MOVING, h=720, w=1280):
    """Two grey frames: the texture, and the texture moved by A with the `moving` region moved on its own."""
    f0 = R.warp_texture(h, w, R.similarity(), seed=seed)
    f1 = R.warp_texture(h, w, A, seed=seed)
    if moving is not None:
        y0, y1, x0, x1 = moving
        f1[y0:y1, x0:x1] = R.warp_texture(h, w, R.similarity(tx=-25, ty=18), seed=seed + 7)[y0:y1, x0:x1]
    return f0, f1


class _M:
    from stereotracking_amd.motion import KalmanFilter
    motion = KalmanFilter()


def _tracker(backend, **kw):
    from stereotracking_amd.trackers import OCSORTTracker_Disparity
    return OCSORTTracker_Disparity(obj_score_thr=0.3, init_track_thr=0.7, weight_iou_with_det_scores=False,
                                   match_iou_thr=0.1, num_tentatives=3, vel_consist_weight=0.2, vel_delta_t=3,
                                   num_frames_retain=30, backend=backend, **kw)


# ---- the option -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', ['native', 'python'])
def test_cmc_option_builds(backend):
    t = _tracker(backend, cmc=dict(method='glme_affine'))
    assert t.with_cmc and t.prev_cmc_img is None
    assert t.cmc_params == dict(step=16, winsize=31, ransac_thr=5.0, min_inlier_ratio=0.3)
    t = _tracker(backend, cmc=dict(method='glme_affine', glme=dict(winsize=21, ransac_thr=3.0)))
    assert t.cmc_params['winsize'] == 21 and t.cmc_params['ransac_thr'] == 3.0
    assert not _tracker(backend).with_cmc and not _tracker(backend, cmc=dict(method=None)).with_cmc
    with pytest.raises(ValueError):
        _tracker(backend, cmc=dict(method='orb'))


def test_config_builds_with_cmc():
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    cfg = Config.fromfile(CFG)
    cfg.merge_from_dict({'model.tracker.cmc': dict(method='glme_affine', glme=dict(step=16, winsize=31))})
    model = MODELS.build(cfg.model)
    assert model.tracker.with_cmc and model.tracker.cmc_mode == 'mesh_affine'


def test_batched_association_refuses_cmc():
    from stereotracking_amd.batched_assoc import BatchedGpuTracker
    with pytest.raises(NotImplementedError, match='camera-motion'):
        BatchedGpuTracker(2, cmc=dict(method='glme_affine'))


def test_sharded_driver_refuses_cmc():
    from stereotracking_amd.sequence import track_gathered
    with pytest.raises(NotImplementedError, match='sharded'):
        track_gathered(torch.zeros(1, 2, 13), None, 1, _tracker('native', cmc=dict(method='glme_affine')), _M())


# ---- warp application: known answers --------------------------------------------------------------------------------------
def _state(seed=0):
    rng = np.random.default_rng(seed)
    mean = rng.normal(0, 1, 8) * np.array([300, 200, 0.3, 40, 2, 2, 0.01, 1]) + np.array([600, 400, 0.7, 60, 0, 0, 0, 0])
    A = rng.normal(0, 1, (8, 8))
    return mean, A @ A.T + np.eye(8)


def test_apply_warp_identity_bit_identical():
    from stereotracking_amd.cmc import apply_warp
    mean, cov = _state()
    m2, c2 = apply_warp(mean, cov, np.array([[1, 0, 0], [0, 1, 0]], np.float32))
    assert np.array_equal(m2, mean) and np.array_equal(c2, cov)


def test_apply_warp_translation_moves_only_centre():
    from stereotracking_amd.cmc import apply_warp
    mean, cov = _state(1)
    m2, c2 = apply_warp(mean, cov, np.array([[1, 0, 7.5], [0, 1, -3.25]], np.float32))
    assert m2[0] == mean[0] + 7.5 and m2[1] == mean[1] - 3.25
    assert np.array_equal(m2[2:], mean[2:]) and np.array_equal(c2, cov)


def test_apply_warp_rotation_scale_matches_float64_hand_computation():
    from stereotracking_amd.cmc import apply_warp
    mean, cov = _state(2)
    th, s = np.deg2rad(3.0), 1.04
    W = np.array([[s * np.cos(th), -s * np.sin(th), 12.0], [s * np.sin(th), s * np.cos(th), -5.0]])
    m2, c2 = apply_warp(mean, cov, W)
    Rm = W[:, :2]
    sc = np.sqrt(np.linalg.det(Rm))
    M = np.eye(8)
    M[0:2, 0:2] = Rm
    M[4:6, 4:6] = Rm
    M[3, 3] = M[7, 7] = sc
    want = mean.copy()
    want[0:2] = Rm @ mean[0:2] + W[:, 2]
    want[4:6] = Rm @ mean[4:6]
    want[3] *= sc
    want[7] *= sc
    np.testing.assert_allclose(m2, want, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(c2, M @ cov @ M.T, rtol=1e-12, atol=1e-9)
    assert abs(sc - s) < 1e-12


# ---- the reference's bookkeeping ------------------------------------------------------------------------------------------
def _sample(fid, rows):
    from stereotracking_amd.structures import InstanceData, TrackDataSample
    s = TrackDataSample(dict(frame_id=fid, img_shape=(720, 1280)))
    r = torch.from_numpy(np.asarray(rows, np.float32).reshape(-1, 8))
    s.pred_det_instances = InstanceData(bboxes=r[:, 0:4], scores=r[:, 4], labels=r[:, 5].long(), depth=r[:, 6],
                                        scales=r[:, 7])
    return s


def _frames(seed=77, T=40, K=6):
    from stereotracking_amd.synthetic import synthetic_detection_stream
    st = synthetic_detection_stream(seed, T, K=K, occlusion=(2, 10, 14))
    out = []
    for t in range(T):
        r = st[st[:, 0] == t]
        rows = np.zeros((len(r), 8), np.float32)
        rows[:, 0:4] = r[:, 1:5]
        rows[:, 4] = r[:, 5]
        rows[:, 6] = r[:, 6]
        rows[:, 7] = r[:, 7]
        out.append(rows)
    return out


class _FakeDevice:
    """Stands in for the device estimate: front() -> a plane tagged with its frame, estimate() -> a warp that encodes
    the pair, so that every call the tracker makes is recorded."""

    def __init__(self, monkeypatch, warp_of):
        from stereotracking_amd import cmc
        self.calls, self.warp_of = [], warp_of
        monkeypatch.setattr(cmc, 'front', self.front)
        monkeypatch.setattr(cmc, 'estimate', self.estimate)

    def front(self, img, h, w, out=None):
        return torch.full((1, 1), float(img.view(-1)[0]))

    def estimate(self, prev, curr, h, w, params=None, **kw):
        a, b = int(prev.view(-1)[0]), int(curr.view(-1)[0])
        self.calls.append((a, b))
        wp = self.warp_of(a, b)
        row = np.zeros(8, np.float32) if wp is None else np.concatenate([[1, 1], np.asarray(wp, np.float32).ravel()])
        return torch.from_numpy(row.astype(np.float32))[None]


def _img(fid):
    return torch.full((1, 3, 4, 4), float(fid))


@pytest.mark.parametrize('backend', ['native', 'python'])
def test_bookkeeping_of_previous_cmc_image(backend, monkeypatch):
    dev = _FakeDevice(monkeypatch, lambda a, b: [[1, 0, 0.5 * (b - a)], [0, 1, 0]])
    trk = _tracker(backend, cmc=dict(method='glme_affine'))
    fr = _frames(T=12)
    fr[5] = fr[5][:0]          # a frame without detections: no estimate, the previous image stays frame 4
    for t in range(12):
        trk.track(_M(), _img(t), None, _sample(t, fr[t]))
    # frame 0 is the empty branch (reset, no tracks), frame 1 is the first estimate after the reset: no previous
    # image, so no call (the warp is None); afterwards every non-empty frame estimates from the previous CMC image
    assert dev.calls == [(1, 2), (2, 3), (3, 4), (4, 6), (6, 7), (7, 8), (8, 9), (9, 10), (10, 11)]
    assert trk.prev_cmc_fid == 11
    dev.calls.clear()
    trk.track(_M(), _img(0), None, _sample(0, fr[0]))          # frame 0 again: reset
    assert trk.prev_cmc_img is None and dev.calls == []
    trk.track(_M(), _img(1), None, _sample(1, fr[1]))
    assert dev.calls == [] and trk.prev_cmc_fid == 1


def test_first_estimate_after_reset_returns_none(monkeypatch):
    _FakeDevice(monkeypatch, lambda a, b: [[1, 0, 1], [0, 1, 0]])
    trk = _tracker('python', cmc=dict(method='glme_affine'))
    meta = dict(frame_id=3, img_shape=(720, 1280))
    assert trk.estimate_camera_motion(_img(3), meta) is None
    w = trk.estimate_camera_motion(_img(4), dict(meta, frame_id=4))
    assert np.array_equal(w, np.array([[1, 0, 1], [0, 1, 0]], np.float32))
    trk.reset_cmc()
    assert trk.estimate_camera_motion(_img(5), dict(meta, frame_id=5)) is None


def _run(backend, frames, warp_of, monkeypatch):
    _FakeDevice(monkeypatch, warp_of)
    trk = _tracker(backend, cmc=dict(method='glme_affine'))
    out = []
    for t, rows in enumerate(frames):
        res = trk.track(_M(), _img(t), None, _sample(t, rows))
        out.append((res.instances_id.tolist(), res.bboxes.numpy().copy(), res.scores.numpy().copy()))
    return trk, out


def test_native_equals_python_with_injected_warps(monkeypatch):
    rng = np.random.default_rng(5)
    pans = {}

    def warp_of(a, b):            # a pan with occasional rotation / scale; every 9th pair fails the fit (None)
        if (a, b) not in pans:
            th, s = rng.normal(0, 0.01), 1 + rng.normal(0, 0.01)
            pans[(a, b)] = None if b % 9 == 0 else [[s * np.cos(th), -s * np.sin(th), rng.normal(0, 6)],
                                                    [s * np.sin(th), s * np.cos(th), rng.normal(0, 4)]]
        return pans[(a, b)]
    fr = _frames(T=48, K=8)
    fr[17] = fr[17][:0]
    tn, on = _run('native', fr, warp_of, monkeypatch)
    tp, op = _run('python', fr, warp_of, monkeypatch)
    assert len({i for ids, _, _ in on for i in ids}) >= 8
    for t, (a, b) in enumerate(zip(on, op)):
        assert a[0] == b[0], f'frame {t}: ids differ'
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), f'frame {t}: rows differ'
    ns = {s['id']: s for s in tn.native_state()}
    assert sorted(ns) == sorted(tp.tracks)
    for i, t in tp.tracks.items():
        np.testing.assert_allclose(ns[i]['mean'], t.mean, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(ns[i]['covariance'], t.covariance, rtol=1e-9, atol=1e-9)


def test_warps_change_the_association(monkeypatch):
    """The warps reach the states: a large pan separates the runs with and without CMC."""
    fr = _frames(T=30, K=8)
    _, with_w = _run('native', fr, lambda a, b: [[1, 0, 40.0], [0, 1, 25.0]], monkeypatch)
    _, no_w = _run('native', fr, lambda a, b: None, monkeypatch)
    assert any(a[0] != b[0] for a, b in zip(with_w, no_w))


def test_native_records_call_stops_for_non_consecutive_pair(monkeypatch):
    """st_tracker_track_records_cmc: a speculative warp is used only for the pair (previous CMC image, frame); any other
    frame stops the call, the pair is estimated on demand, and the result equals the per-frame path."""
    fr = _frames(T=24, K=6)
    fr[9] = fr[9][:0]              # the pair of frame 10 reaches back to 8 (inside a chunk)
    fr[14] = fr[14][:0]            # ... and that of frame 15, the last of its chunk; frame 16 then starts a chunk
    warp_of = lambda a, b: [[1, 0, 0.7 * (b - a)], [0, 1, -0.3 * (b - a)]]  # noqa: E731
    _, ref = _run('native', fr, warp_of, monkeypatch)
    M = max(len(r) for r in fr) + 2
    rec = np.zeros((len(fr), M + 1, 13), np.float32)
    for t, rows in enumerate(fr):
        rec[t, 0, :3] = (len(rows), M, 1)
        rec[t, 1:1 + len(rows), 4:8] = rows[:, 4:8]
        rec[t, 1:1 + len(rows), 8:12] = rows[:, 0:4]
        # unscaled box: the records path unscales the tracker's output again (scale_bbox(b, 1 / scale))
        c, wh = (rows[:, 0:2] + rows[:, 2:4]) / 2, (rows[:, 2:4] - rows[:, 0:2]) / rows[:, 7:8]
        rec[t, 1:1 + len(rows), 0:4] = np.concatenate([c - wh / 2, c + wh / 2], 1)
    trk = _tracker('native', cmc=dict(method='glme_affine'))
    demands = []

    chunk = [0]

    def on_demand(i, prev):       # i: index of the frame inside the chunk
        f = chunk[0] + i
        demands.append((prev, f))
        return np.concatenate([[1, 1], np.asarray(warp_of(prev, f), np.float32).ravel()]).astype(np.float32)
    got_ids = []
    for s in range(0, len(fr), 8):
        e = min(s + 8, len(fr))
        chunk[0] = s
        spec = np.stack([np.concatenate([[1, 1], np.asarray(warp_of(t - 1, t), np.float32).ravel()]) for t in range(s, e)])
        rows, ids, cnt = trk.track_records(list(range(s, e)), rec[s:e].copy(),
                                           cmc=(spec.astype(np.float32), np.arange(s - 1, e - 1), on_demand))
        got_ids += [ids[i, :cnt[i]].tolist() for i in range(e - s)]
    assert demands == [(8, 10), (13, 15)]
    assert got_ids == [r[0] for r in ref]


# ---- the restatement itself -------------------------------------------------------------------------------------------------
def test_equalize_hist_constant_and_ramp():
    c = np.full((255, 255), 77, np.uint8)
    assert np.array_equal(R.equalize_hist(c), c)
    ramp = np.tile(np.arange(255, dtype=np.uint8), (255, 1))
    eq = R.equalize_hist(ramp)
    assert eq[0, 0] == 0 and eq[0, -1] == 255
    assert np.all(np.diff(eq[0].astype(int)) >= 0)
    # 255 equally full bins: lut[i] = round(i * 255 / 254 * 255 / 255)
    want = np.rint(np.arange(255, dtype=np.float32) * np.float32(255) * np.float32(255.0 / (255 * 254))).astype(np.uint8)
    assert np.abs(eq[0].astype(int) - want.astype(int)).max() <= 1


def test_median_of_even_count_is_mean_of_middle_pair():
    flow = np.zeros((255, 255, 2), np.float32)
    cell = np.arange(256, dtype=np.float32).reshape(16, 16)
    flow[:16, :16, 0] = cell
    src, dst = R.mesh(flow, 255, 255, 16)
    assert dst[0, 0] - src[0, 0] == np.float32(127.5)


def test_fit_recovers_similarity_with_40_percent_outliers():
    rng = np.random.default_rng(3)
    src, _ = R.mesh(np.zeros((255, 255, 2), np.float32), 720, 1280, 16)
    A = R.similarity(tx=11.0, ty=-6.0, deg=1.2, scale=1.02, cx=640, cy=360)
    dst = (src.astype(np.float64) @ A[:, :2].T + A[:, 2]).astype(np.float32)
    out = rng.permutation(len(src))[:int(0.4 * len(src))]
    dst[out] += rng.uniform(15, 60, (len(out), 2)).astype(np.float32) * rng.choice([-1, 1], (len(out), 2))
    for dt in (np.float32, np.float64):
        warp, ratio, inl = R.consensus_fit(src, dst, 5.0, 0.3, dt)
        assert ratio == pytest.approx(1 - len(out) / len(src), abs=1 / len(src))
        assert not inl[out].any()
        np.testing.assert_allclose(warp, A, rtol=0, atol=2e-3 * np.abs(A).max())
    # the same scene with fewer inliers than min_inlier_ratio: no warp
    dst2 = dst.copy()
    bad = rng.permutation(len(src))[:int(0.8 * len(src))]
    dst2[bad] = src[bad] + rng.uniform(-200, 200, (len(bad), 2)).astype(np.float32)
    warp, ratio, _ = R.consensus_fit(src, dst2, 5.0, 0.3)
    assert warp is None and ratio < 0.3


def _corner_error(warp, A, h=720, w=1280):
    c = np.array([[0, 0], [w, 0], [0, h], [w, h]], float)
    return np.abs((c @ np.asarray(warp, float)[:, :2].T + np.asarray(warp, float)[:, 2]) - (c @ A[:, :2].T + A[:, 2])).max()


@pytest.mark.parametrize('A,moving', [(R.similarity(tx=7.3, ty=-4.6), None),
                                      (R.similarity(tx=3.0, deg=0.5, scale=1.01, cx=640, cy=360), None),
                                      (R.similarity(tx=5.0, deg=0.5, scale=1.01, cx=640, cy=360), MOVING)],
                         ids=['shift', 'similarity', 'moving-region'])
def test_farneback_recovers_known_camera_motion(A, moving):
    h, w = 720, 1280
    f0, f1 = moving_pair(A, moving=moving)
    p0, p1 = (R.front(np.repeat(f[None], 3, 0), h, w) for f in (f0, f1))
    warp, ratio, _, _, _ = R.estimate(p0, p1, h, w, dtype=np.float32)
    assert warp is not None and ratio > (0.5 if moving else 0.9)
    assert _corner_error(warp, A) <= (CORNER_TOL_MOVING if moving else CORNER_TOL)


# ---- the scenarios of tests/test_cmc_kernels_gpu.py: preconditions, from the restatement alone --------------------------
import cmc_cases as K  # noqa: E402


@pytest.mark.parametrize('geometry', K.GEOMETRIES, ids=K.geometry_id)
def test_front_cases_equalise_to_two_grey_levels(geometry):
    """A frame whose plane is constant cannot tell a wrong resize or LUT from a right one: every non-constant front
    case yields at least 2 grey levels, through the uint8 frame and through the padded fp32 canvas alike."""
    fh, fw, h, w = geometry
    for kind in K.FRONT_KINDS:
        f = K.front_frame(kind, geometry)
        plane = R.front(f, h, w)
        assert plane.shape == (255, 255) and plane.dtype == np.uint8
        assert np.array_equal(R.front(K.canvas_f32(f, h, w), h, w), plane)
        levels = len(np.unique(plane))
        assert levels == 1 if kind == 'constant' else levels >= 2, (kind, levels)
    if h * w > 255 * 255:     # down-scaling: the one differing pixel stays one plane pixel, the extreme of equalizeHist
        assert (R.front(K.front_frame('one-off', geometry), h, w) != 0).sum() <= 4
    o = K.out_of_range_f32(geometry)
    assert o.min() == -7 and o.max() == 300 and len(np.unique(R.front(o, h, w))) >= 2 or h * w < 8


def test_front_batch_crosses_the_chunk():
    assert K.FRONT_BATCH > 32
    fh, fw, h, w = K.FRONT_BATCH_GEOMETRY
    planes = [R.front(K.front_frame('random', K.FRONT_BATCH_GEOMETRY, seed=i), h, w) for i in range(K.FRONT_BATCH)]
    # no two planes alike: a plane written to the wrong slot cannot pass for the right one
    assert len({p.tobytes() for p in planes}) == K.FRONT_BATCH


@pytest.mark.parametrize('name', list(K.FIT_CASES))
def test_fit_cases_do_not_depend_on_rounding(name):
    """float32 restatement == float64 restatement in winner, inlier set and ratio; under the float64 winner no residual
    lies within 1e-3 thr of thr, but the ones a case puts exactly on it; and what each case was built to show."""
    c = K.fit_case(name)
    P, thr = len(c['points']), c['thr']
    assert 2 <= P <= 1024
    w32, r32, i32, win32 = K.fit_reference(name, np.float32)
    w64, r64, i64, win64 = K.fit_reference(name, np.float64)
    assert np.array_equal(i32, i64) and r32 == r64 and (w32 is None) == (w64 is None)
    assert (win32 is None) == (win64 is None)
    if win64 is not None:
        assert win32[:2] == win64[:2], 'winning hypothesis differs between float32 and float64'
        free = np.ones(P, bool)
        free[list(c['on_threshold'])] = False
        assert np.abs(win64[2][free] - thr).min() > 1e-3 * thr
        for k in c['on_threshold']:
            assert win64[2][k] == thr and win32[2][k] == np.float32(thr)
    if 'winner' in c:
        assert win32[:2] == c['winner']
    if 'n_inliers' in c:
        assert int(i32.sum()) == c['n_inliers']
    if 'valid' in c:
        assert (w32 is not None) == c['valid']
        # the device decides in float32
        assert (np.float32(i32.sum()) / np.float32(P) >= np.float32(c['min_ratio'])) == c['valid']
    if 'outliers' in c:
        assert not i32[c['outliers']].any() and int(i32.sum()) == P - len(c['outliers'])
        assert np.all(R.residuals(c['points'][:, :2], c['points'][:, 2:], K.MOTION)[c['outliers']] >= 10 * thr)
    for k in c.get('inlier', ()):
        assert i32[k]
    for k in c.get('outlier', ()):
        assert not i32[k]
    if 'motion' in c:
        np.testing.assert_allclose(w32, c['motion'], rtol=1e-3, atol=0)      # a, b, tx, ty each to 1e-3 of itself
    if 'base_points' in c:       # (e): the repeated sources add den == 0 hypotheses and change nothing
        n = c['base_points']
        p = c['points']
        d = p[:, None, :2] - p[None, :, :2]
        assert ((d ** 2).sum(-1) == 0).sum() > P, 'no coincident source points'
        wb, rb, ib, winb = R.consensus_fit(p[:n, :2], p[:n, 2:], thr, c['min_ratio'], np.float32, with_winner=True)
        assert winb[:2] == win32[:2] and np.array_equal(ib, i32[:n]) and not i32[n:].any()
        assert np.array_equal(wb, w32)


def test_ratio_boundary_in_float32():
    assert np.float32(120) / np.float32(400) >= np.float32(0.3)
    assert not np.float32(119) / np.float32(400) >= np.float32(0.3)
    assert K.fit_reference('g120')[0] is not None and K.fit_reference('g119')[0] is None


def test_fit_batches_share_a_point_count():
    for names in K.FIT_BATCHES.values():
        assert len(names) == 5 and len({len(K.fit_case(n)['points']) for n in names}) == 1
        assert names[0] == names[4]       # the same set twice: its two rows must agree, whatever the keys held between


def test_mesh_fields_hold_ties_and_odd_cells():
    f = K.flow_fields()
    assert {s * s % 2 for s in K.MESH_STEPS} == {0, 1}
    assert sorted(255 // s for s in K.MESH_STEPS)[0] == 15 and sorted(255 // s for s in K.MESH_STEPS)[-1] == 31
    assert np.signbit(f['neg-zero']).any() and not np.signbit(f['neg-zero']).all() and not f['neg-zero'].any()
    for s in K.MESH_STEPS:
        cell = f['two-valued'][:s, :s]
        for c in range(2):
            v, n = np.unique(cell[..., c], return_counts=True)
            assert len(v) == 2 and abs(int(n[0]) - int(n[1])) == (s * s) % 2
        src, dst = R.mesh(f['two-valued'], 255, 255, s)
        want = (0.25, 1.5) if s % 2 == 0 else None     # even count: the mean of the two values
        if want:
            assert np.all(dst[:, 0] - src[:, 0] == np.float32(want[0])) and np.all(dst[:, 1] - src[:, 1] == want[1])
    assert len(np.unique(f['noise'])) > 0.99 * f['noise'].size


def test_options_scene_is_recovered_by_the_restatement():
    """The glme overrides the end-to-end GPU test uses (step 8, winsize 15, thr 3, ratio 0.5) recover the known motion
    in the float32 restatement within the tolerance of the default options."""
    A, moving = K.FLOW_SCENES[K.OPTIONS_SCENE]
    p0, p1 = K.scene_planes(K.OPTIONS_SCENE)
    warp, ratio, src, _, _ = R.estimate(p0, p1, K.IMG_H, K.IMG_W, dtype=np.float32, **K.OPTIONS)
    assert len(src) == 961 and warp is not None and ratio >= 0.9
    assert _corner_error(warp, A) <= CORNER_TOL
