"""GPU: StereoSGBM (csrc/sgbm.hip) bit for bit against the numpy restatement (tests/sgbm_ref.py), stage by stage and end
to end, from both input forms; then through the dense pipeline, the MOT shell and the offline PNG path."""
import numpy as np
import pytest
import torch

import sgbm_ref as R
from sgbm_check import assert_stages_bit_exact, batch as _batch, up as _up

pytestmark = pytest.mark.gpu


def _pairs(N, h, w, D, seed=0):
    from stereotracking_amd.synthetic import synthetic_stereo_pair
    ps = [synthetic_stereo_pair(seed + i, h, w, max_disp=D) for i in range(N)]
    return [p['left'] for p in ps], [p['right'] for p in ps]


CASES = [  # N, h, w, module kwargs
    (1, 720, 1280, {}),
    (3, 96, 200, {}),                                             # width not a multiple of 64
    (8, 48, 150, dict(num_disparities=32)),
    (2, 64, 130, dict(num_disparities=16, block_size=1, uniqueness_ratio=15, disp12_max_diff=2)),
    (2, 70, 160, dict(num_disparities=64, block_size=5, color=False, P1=8, P2=32, speckle_window_size=50)),
]


@pytest.mark.parametrize('N,h,w,kw', CASES)
def test_stages_bit_exact(cuda, N, h, w, kw):
    L, Rt = _pairs(N, h, w, kw.get('num_disparities', 48), seed=N * 7 + h)
    refs, _ = assert_stages_bit_exact(cuda, L, Rt, kw)
    valid = np.mean([(r['final'] > 0).mean() for r in refs])
    assert valid > 0.3, f'scenario has too few valid pixels ({valid:.2f}) to test anything'


def test_u8_frames_equal_f32_batch(cuda):
    from stereotracking_amd.engine import RawChunk
    from stereotracking_amd.sgbm import StereoSGBM
    m = StereoSGBM()
    N, h, w = 3, 120, 224
    L, Rt = _pairs(N, h, w, 48, seed=11)
    H, W = _up(h), _up(w)
    a = torch.zeros(N, 3, H, W, device=cuda)
    b = torch.zeros(N, 3, H, W, device=cuda)
    m.compute(_batch(L, H, W, cuda), _batch(Rt, H, W, cuda), (h, w), a)
    lc = RawChunk([torch.from_numpy(f).to(cuda) for f in L], 114.0)
    rc = RawChunk([torch.from_numpy(f).to(cuda) for f in Rt], 114.0)
    m.compute(lc, rc, (h, w), b)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert np.array_equal(a[0].cpu().numpy(), R.disp_postp(R.sgbm(L[0], Rt[0]), H, W))


def test_speckle_status_and_rule(cuda):
    """Squares of 400 and 401 pixels and a chain joined by steps of <= maxDiff through the kernel."""
    from stereotracking_amd.sgbm import StereoSGBM
    m = StereoSGBM()
    d = np.full((1, 64, 96), -16, np.int16)
    d[0, 2:22, 2:22] = 320                      # 400 pixels: removed
    d[0, 30:50, 2:22] = 320
    d[0, 50, 2] = 320                           # 401 pixels: kept
    d[0, 2:12, 40:90] = (np.arange(50) * 100 + 160).astype(np.int16)[None]   # 500-pixel ramp, steps of 100 <= 160
    d[0, 20:40, 40:60] = 300
    d[0, 20:40, 60:80] = 600                    # two 400-pixel blocks differing by 300 > 160: both removed
    out, status = m.speckle(torch.from_numpy(d).to(cuda))
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert np.array_equal(out.cpu().numpy()[0], R.speckles(d[0], 400, 160))
    o = out.cpu().numpy()[0]
    assert (o[2:22, 2:22] == -16).all() and (o[30:50, 2:22] == 320).all() and (o[2:12, 40:90] > 0).all()
    assert (o[20:40, 40:80] == -16).all()


# ---- through the layers above --------------------------------------------------------------------------------------------
def _clone(out, ctx):
    return {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor)}


@pytest.mark.parametrize('contexts', [1, 3])
def test_pipeline_sgbm_equals_mono_fed_its_own_disparity(cuda, contexts):
    """StereoDensePipeline(sgbm=...): detections, depths and scaled boxes are those of the mono pipeline given the
    module's own disp_postp, bit for bit, through 1 and 3 in-flight contexts (each with its own SGBM workspace)."""
    from stereotracking_amd.pipeline import InflightPipelines
    from stereotracking_amd.synthetic import synthetic_state_dict
    N, h, w = 2, 96, 160
    sg = InflightPipelines(contexts, N, (h, w), 0.375, 0.33, 1, stereo=False, sgbm=dict(type='StereoSGBM'), max_det=256)
    mono = InflightPipelines(contexts, N, (h, w), 0.375, 0.33, 1, stereo=False, max_det=256)
    assert sg.takes_right and not mono.takes_right
    sd = synthetic_state_dict(sg.param_table(), seed=0, prior_prob=0.2, logit_std=2.5)
    sg.load_state_dict(sd, autotune=False)
    mono.load_state_dict(sd, autotune=False)
    got = []
    for k in range(4):
        L, Rt = _pairs(N, h, w, 48, seed=40 + 3 * k)
        img, right = _batch(L, h, w, cuda), _batch(Rt, h, w, cuda)
        got.append((img, right, sg.submit(img, right=right, post=_clone)[0]))
    sg.synchronize()
    kept = 0
    for img, right, a in got:
        b = mono.submit(img, disp_postp=a['disp_postp'], post=_clone)[0]
        mono.synchronize()
        for key in ('counts', 'boxes', 'scores', 'labels', 'prior_idx', 'depth', 'scales', 'scaled_boxes'):
            assert torch.equal(a[key].nan_to_num(-7.0), b[key].nan_to_num(-7.0)), key   # NaN depth: equal positions
        kept += int(a['counts'].sum())
    assert kept > 0, 'scenario kept no boxes'
    L, Rt = _pairs(N, h, w, 48, seed=40)
    want = np.stack([R.disp_postp(R.sgbm(x, y), h, w) for x, y in zip(L, Rt)])
    assert np.array_equal(got[0][2]['disp_postp'].cpu().numpy(), want)


def _sgbm_model(cuda, dense_batch=4, inflight=2):
    import os
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.synthetic import synthetic_state_dict
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(root, 'configs', 'stereo_tracking', 'ocsort', 'stereo_yolox_s_mot_airdrone_sgbm.py'))
    for part in ('backbone', 'neck'):
        cfg.model.detector[part]['widen_factor'] = 0.375
    cfg.model.detector.bbox_head.head_module['widen_factor'] = 0.375
    cfg.model.tracker['init_track_thr'] = 0.03
    cfg.model.tracker['obj_score_thr'] = 0.02
    model = MODELS.build(dict(cfg.model, autotune=False, dense_batch=dense_batch, inflight=inflight))
    sd = synthetic_state_dict(list(model.detector._table), seed=5, prior_prob=0.2, logit_std=2.5)
    model.detector.load_state_dict(sd, strict=False)
    return model


def _sequence(cuda, T, h, w):
    from stereotracking_amd.sequence import synthetic_sequence
    fr = list(synthetic_sequence(T, 3, h, w, 48, seed=2))
    left = [torch.from_numpy(f['left'])[None].to(cuda) for f in fr]
    right = [torch.from_numpy(f['right'])[None].to(cuda) for f in fr]
    return left, right


def _samples(lo, hi, ori, img_shape=None):
    from stereotracking_amd.structures import TrackDataSample
    return [TrackDataSample(dict(frame_id=t, ori_shape=ori, img_shape=img_shape or ori, scale_factor=(1.0, 1.0)))
            for t in range(lo, hi)]


def test_shell_sgbm_config_test_step_equals_per_chunk_calls(cuda):
    ori, T = (96, 160), 12          # whole chunks of 4: every call runs the same batch-4 launch plan
    left, right = _sequence(cuda, T, *ori)
    one = _sgbm_model(cuda)
    whole = one.test_step(dict(inputs=dict(img=left, right=right), data_samples=_samples(0, T, ori)))
    per = _sgbm_model(cuda)
    chunks = []
    for lo in range(0, T, 4):
        hi = min(lo + 4, T)
        chunks += per.test_step(dict(inputs=dict(img=left[lo:hi], right=right[lo:hi]), data_samples=_samples(lo, hi, ori)))
    torch.cuda.synchronize()
    assert len(whole) == len(chunks) == T
    n = 0
    for a, b in zip(whole, chunks):
        ta, tb = a.pred_track_instances, b.pred_track_instances
        assert ta.instances_id.tolist() == tb.instances_id.tolist()
        for key in ('bboxes', 'scores', 'depth', 'scales'):
            assert torch.equal(ta[key].nan_to_num(-7.0), tb[key].nan_to_num(-7.0)), key
        assert torch.equal(a.pred_det_instances.bboxes, b.pred_det_instances.bboxes)
        n += len(ta)
    assert n > 0, 'no tracks in the scenario'


def test_shell_refuses_resized_frames(cuda):
    ori = (96, 160)
    left, right = _sequence(cuda, 2, *ori)
    model = _sgbm_model(cuda)
    with pytest.raises(NotImplementedError, match='original resolution'):
        model.test_step(dict(inputs=dict(img=left, right=right), data_samples=_samples(0, 2, ori, img_shape=(48, 80))))


def test_end_to_end_sgbm_from_right_images_equals_the_png_disparity_path(cuda, tmp_path):
    """The user-facing promise: a dataset whose disparity PNGs hold the restatement's SGBM codes (d16, 65535 invalid)
    gives, through the PNG-disparity pipeline, exactly the tracks that the SGBM pipeline gives from the right images."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    from make_tiny_airdrone import make
    from stereotracking_amd import datasets as ds
    from stereotracking_amd.motion import KalmanFilter
    from stereotracking_amd.pipeline import StereoDensePipeline
    from stereotracking_amd.sequence import run_video_replicas, synthetic_sequence
    from stereotracking_amd.synthetic import synthetic_state_dict
    from stereotracking_amd.trackers import OCSORTTracker_Disparity
    h, w, D, T, V = 96, 160, 48, 8, 2
    base, _ = make(str(tmp_path), videos=V, frames=T, height=h, width=w, max_disp=D, objects=3)
    for v in range(V):
        for t, f in enumerate(synthetic_sequence(T, 3, h, w, D, seed=v)):
            fin = R.sgbm(f['left'], f['right'])
            codes = np.where(fin >= 0, fin, 65535).astype(np.uint16)
            ds.write_png(os.path.join(base, 'val', f'seq{v:02d}', 'disparity', f'{t:06d}.png'), codes)
    dataset = ds.MOTDispDataset(ann_file='annotations/val_cocoformat_80.json', data_root=base + os.sep,
                                data_prefix=dict(img_path='val/'), depth_dir_name='depth')

    class _Model:
        motion = KalmanFilter()

    def make_tracker():
        return OCSORTTracker_Disparity(obj_score_thr=0.02, init_track_thr=0.03, weight_iou_with_det_scores=False,
                                       match_iou_thr=0.1, num_tentatives=3, vel_consist_weight=0.2, vel_delta_t=3,
                                       num_frames_retain=30)

    png = StereoDensePipeline(4, (h, w), 0.375, 0.33, 1, stereo=False, max_det=256)
    sg = StereoDensePipeline(4, (h, w), 0.375, 0.33, 1, stereo=False, max_det=256, sgbm=dict(type='StereoSGBM'))
    sd = synthetic_state_dict(png.param_table(), seed=9, prior_prob=0.2, logit_std=2.5)
    png.load_state_dict(sd, autotune=False)
    sg.load_state_dict(sd, autotune=False)
    va, _ = ds.load_videos(dataset, False)
    vb, _ = ds.load_videos(dataset, True)
    ra, _ = run_video_replicas(png, va, make_tracker, _Model(), cuda, already_sharded=True)
    rb, _ = run_video_replicas(sg, vb, make_tracker, _Model(), cuda, already_sharded=True)
    n = 0
    for name in va:
        assert len(ra[name]) == len(rb[name]) == T
        for a, b in zip(ra[name], rb[name]):
            assert a.instances_id.tolist() == b.instances_id.tolist()
            for key in ('bboxes', 'scores', 'depth', 'scales'):    # NaN where a box sees no valid disparity
                assert torch.equal(a[key].nan_to_num(-7.0), b[key].nan_to_num(-7.0)), key
            n += len(a)
    assert n > 0, 'no tracks in the scenario'
