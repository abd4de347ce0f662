"""GPU: the per-box depth estimators (csrc/box_depth.hip, st_box_depth_method) against the numpy restatement
(tests/depth_methods_ref.py) - on random and crafted maps, on the loader's disparity, on StereoSGBM's disparity and in
the gt-depth mode - then through the dense pipeline (cost-volume and SGBM modes) and the MOT shell on a tiny AirDrone
dataset with gt depth: the option reaches every depth call, chunked test_step equals per-frame predict, and
depth_extraction='reference' changes nothing."""
import os
import sys

import numpy as np
import pytest
import torch

import depth_methods_ref as R
import guard_memory as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
CFG_DISP = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone_disp.py')

pytestmark = pytest.mark.gpu
CODES = {'truncated_mean': 1, 'mean': 2, 'median': 3, 'center': 4}


def run_method(disp, boxes, counts, method, baseline=0.25, focal=640.0):
    """st_box_depth_method on (N, C, H, W) maps, (N, M, 4) boxes, (N,) counts (CUDA) -> numpy depth, scale, boxes."""
    from stereotracking_amd import _lib
    from stereotracking_amd._lib import check, current_stream, ptr
    N, Cc, H, W = disp.shape
    M = boxes.shape[1]
    d = gm.device_output((N, M), disp.device, 7.0)           # poisoned: every row must be written
    s = gm.device_output((N, M), disp.device, 7.0)
    b = gm.device_output((N, M, 4), disp.device, 7.0)
    check(_lib.load().st_box_depth_method(ptr(disp.contiguous()), Cc * H * W, N, H, W, ptr(boxes.contiguous()),
                                          ptr(counts), M, baseline, focal, None, 0, current_stream(), ptr(d), ptr(s),
                                          ptr(b), CODES[method]), 'st_box_depth_method')
    torch.cuda.synchronize()
    return d.cpu().numpy(), s.cpu().numpy(), b.cpu().numpy()


def assert_matches(method, dmap, boxes, got_d, got_s, got_b, where=''):
    """One frame: dmap (H, W) float32 depth (R1 already applied), boxes (k, 4) -> the kernel's k rows."""
    rd, rs = R.extract_depth(dmap, boxes, method)
    gd, gs = got_d[:len(boxes)], got_s[:len(boxes)]
    assert np.array_equal(np.isnan(gd), np.isnan(rd)), f'{where}: NaN decisions differ'
    assert np.array_equal(gd == -1, rd == -1) and np.array_equal(np.isnan(gs), np.isnan(rs)), f'{where}: -1 decisions'
    if method in ('median', 'center'):
        assert np.array_equal(gd, rd, equal_nan=True), f'{where}: depth not bit-exact'
        assert np.array_equal(gs, rs, equal_nan=True), f'{where}: scale not bit-exact'
    else:   # fp64 sums in another order: within 1 fp32 ulp of the float64 restatement; the scale follows the value
        fin = np.isfinite(rd)
        assert np.all(np.abs(gd[fin] - rd[fin]) <= np.spacing(np.abs(rd[fin]))), f'{where}: mean beyond 1 ulp'
        est = (rd != -1) & fin
        want = np.where(est, [R.scale_of(v) for v in gd], rs).astype(np.float32)
        assert np.array_equal(gs, want, equal_nan=True), f'{where}: scale of the value'
    assert np.array_equal(got_b[:len(boxes)], R.scale_bbox(boxes, gs), equal_nan=True), f'{where}: scaled boxes'


def _boxes(rng, H, W, M):
    """Random boxes + the crafted cases: past every edge, fractional and negative coordinates, windows larger than
    the kernel's LDS cache (2560 px), w > 800, empty windows, centres out of range (tall track boxes)."""
    out = []
    for _ in range(M - 16):
        w, h = rng.uniform(1, 60), rng.uniform(1, 60)
        x1, y1 = rng.uniform(-30, W + 5), rng.uniform(-30, H + 5)
        out.append([x1, y1, x1 + w, y1 + h])
    out += [[-10.7, -3.2, 40.9, 30.5], [W - 20.5, H - 15.2, W + 30, H + 40],       # past the corners
            [5, 5, 95, 75], [0, 0, W, H], [20.2, 10.9, 120.7, 70.1],               # 6300, all, 6000 px windows
            [-500, 0, 401, 40], [-500, 0, 300, 40],                                # w = 901 (discard), w = 800
            [30, 30, 25, 60], [40, 40, 40, 50],                                    # empty windows
            [10, H - 12, 30, 4 * H], [W - 12, 10, 3 * W, 30],                      # centre past bottom / right
            [-3 * W, 5, 10, 25], [-W - 40, 5, 12, 20],                             # centre wraps to negative / wraps
            [7.5, 8.5, 9.5, 10.5],                                                 # 2 x 2
            [7, 22, 8, 23], [5, 20, 10, 25]]                                       # n == 1 (see _random_disp)
    return np.asarray(out, np.float32)


def _random_disp(rng, N, H, W):
    """Disparity with invalid regions: 0 (depth 1.6e8), negative, tiny (depth > 150), and single valid pixels."""
    d = rng.uniform(1.0, 40.0, (N, H, W)).astype(np.float32)
    d[:, 10:40, 50:120] = 0.0
    d[:, 60:70, :] = rng.choice([0.0, -2.0, 0.5, 1.05], size=(N, 10, W)).astype(np.float32)
    d[:, :, 100:104] = 0.0
    d[:, 20:25, 5:10] = 0.0
    d[:, 22, 7] = 12.0                                        # one valid pixel in an invalid 5 x 5 patch
    d[:, 80:, 140:] = np.round(d[:, 80:, 140:] / 8) * 8       # ties for the order statistics
    return d


def _check_maps(disp_np, method, cuda, rng, is_depth=False, M=64, cc=3):
    N, H, W = disp_np.shape
    boxes = np.stack([_boxes(rng, H, W, M) for _ in range(N)])
    counts = np.asarray([M - 3 * i for i in range(N)], np.int32)
    dev_map = gm.device_planes(np.repeat(disp_np[:, None], cc, axis=1), cuda)    # channel 0 is the map
    base = (-1.0, 1.0) if is_depth else (0.25, 640.0)
    gd, gs, gb = run_method(dev_map, gm.device_input(boxes, cuda), gm.device_input(counts, cuda), method, *base)
    for n in range(N):
        k = counts[n]
        dmap = disp_np[n] if is_depth else R.depth_map(disp_np[n])
        assert_matches(method, dmap, boxes[n, :k], gd[n], gs[n], gb[n], where=f'frame {n}')
        assert not gd[n, k:].any() and not gs[n, k:].any() and not gb[n, k:].any(), 'rows past the count are not 0'
    return gd


@pytest.mark.parametrize('method', R.METHODS)
def test_kernel_on_random_maps(method, cuda):
    rng = np.random.RandomState(3)
    gd = _check_maps(_random_disp(rng, 3, 96, 160), method, cuda, rng)
    assert (gd == -1).any() and (gd > 0).any()
    if method == 'truncated_mean':
        assert np.isnan(gd).any(), 'the single-valid-pixel box must give NaN'


@pytest.mark.parametrize('method', R.METHODS)
def test_kernel_in_gt_depth_mode(method, cuda):
    rng = np.random.RandomState(4)
    depth = rng.uniform(0.0, 200.0, (2, 96, 160)).astype(np.float32)     # ~25 % above 150 m: invalid
    depth[:, 30:50, 30:90] = 0.0
    depth[0, 40, 60] = -5.0
    _check_maps(depth, method, cuda, rng, is_depth=True, cc=1)


@pytest.mark.parametrize('method', R.METHODS)
def test_kernel_on_loader_and_sgbm_disparity(method, cuda):
    """The two disparity producers of the product: PNG codes through the device loader (st_pack_raw_inputs: invalid
    code -> 0, /16) and StereoSGBM (holes where the left-right check fails)."""
    from stereotracking_amd.mot import pack_raw_inputs
    from stereotracking_amd.sequence import synthetic_sequence
    from stereotracking_amd.sgbm import StereoSGBM
    h, w = 96, 160
    fr = list(synthetic_sequence(3, 3, h, w, 48, seed=7))
    codes = np.stack([(f['disp'] * 16.0).astype(np.uint16) for f in fr])
    codes[:, 10:20, 10:40] = 65535
    loaded = pack_raw_inputs(disp_u16=torch.from_numpy(codes.view(np.int16)).to(cuda))['disp_postp']
    sg = torch.zeros(3, 3, h, w, device=cuda)
    StereoSGBM().compute(*[torch.from_numpy(np.stack([f[k] for f in fr])).float().to(cuda) for k in ('left', 'right')],
                         (h, w), sg)
    torch.cuda.synchronize()
    rng = np.random.RandomState(5)
    for disp in (loaded, sg):
        _check_maps(disp[:, 0].cpu().numpy(), method, cuda, rng)
    assert (sg[:, 0] == 0).any() and (sg[:, 0] > 0).any()


# ---- the dense pipeline in both stereo modes ---------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['costvolume', 'sgbm'])
@pytest.mark.parametrize('method', R.METHODS)
def test_pipeline_depth_method(mode, method, cuda):
    from stereotracking_amd.pipeline import StereoDensePipeline
    from stereotracking_amd.synthetic import synthetic_batch, synthetic_state_dict
    h, w = 96, 160
    kw = dict(stereo=True, max_disp=32) if mode == 'costvolume' else dict(stereo=False, sgbm=dict(type='StereoSGBM'))
    pipe = StereoDensePipeline(2, (h, w), 0.375, 0.33, 1, max_det=300, depth_method=method, **kw)
    pipe.load_state_dict(synthetic_state_dict(pipe.param_table(), seed=2, prior_prob=0.2, logit_std=2.5),
                         autotune=False)
    batch = synthetic_batch([3, 4], h, w, 32)
    out = pipe.run(batch['img'].to(cuda), batch['right'].to(cuda))
    torch.cuda.synchronize()
    counts = out['counts'].cpu().numpy()
    assert counts.sum() > 0
    for n in range(2):
        k = int(counts[n])
        dmap = R.depth_map(out['disp_postp'][n, 0].cpu().numpy())
        assert_matches(method, dmap, out['boxes'][n, :k].cpu().numpy(), out['depth'][n].cpu().numpy(),
                       out['scales'][n].cpu().numpy(), out['scaled_boxes'][n].cpu().numpy(), where=f'{mode} {n}')


# ---- the MOT shell on a tiny AirDrone dataset with gt depth -------------------------------------------------------
H, W, T = 96, 160, 10


@pytest.fixture(scope='module')
def airdrone(tmp_path_factory):
    from make_tiny_airdrone import make
    from stereotracking_amd import datasets as ds
    base, _ = make(str(tmp_path_factory.mktemp('airdrone')), videos=1, frames=T, height=H, width=W, max_disp=32,
                   objects=4)
    dataset = ds.MOTDispDataset(ann_file='annotations/val_cocoformat_80.json', data_root=base + os.sep,
                                data_prefix=dict(img_path='val/'), depth_dir_name='depth')
    (_, idx), = dataset.video_indices()
    seq, _, _, depth = ds.load_video(dataset, idx, False, with_depth=True, pin=False)
    codes = seq.codes.numpy().view(np.uint16)
    disp = np.where(codes == 65535, 0.0, codes / 16.0).astype(np.float32)
    assert (depth > 0).any() and (disp == 0).any()       # gt depth everywhere, disparity with an invalid patch
    return seq.left.numpy(), disp, depth.astype(np.float32)


def _model(cuda, cfg_path=CFG_DISP, **kw):
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.synthetic import synthetic_state_dict
    cfg = Config.fromfile(cfg_path)
    for part in ('backbone', 'neck'):
        cfg.model.detector[part]['widen_factor'] = 0.375
    cfg.model.detector.bbox_head.head_module['widen_factor'] = 0.375
    cfg.model.tracker['init_track_thr'] = 0.03
    cfg.model.tracker['obj_score_thr'] = 0.02
    model = MODELS.build(dict(cfg.model, autotune=False, dense_batch=4, inflight=2, **kw))
    sd = synthetic_state_dict(list(model.detector._table), seed=5, prior_prob=0.2, logit_std=2.5)
    model.detector.load_state_dict(sd, strict=False)
    return model


def _data(airdrone, lo, hi, cuda):
    from stereotracking_amd.structures import TrackDataSample
    left, disp, depth = airdrone
    inputs = dict(img=[torch.from_numpy(left[t:t + 1]).to(cuda) for t in range(lo, hi)],
                  disp_postp=[torch.from_numpy(np.repeat(disp[t:t + 1, None], 3, axis=1)).to(cuda) for t in range(lo, hi)],
                  depth_postp=[torch.from_numpy(depth[t:t + 1, None]).to(cuda) for t in range(lo, hi)])
    samples = [TrackDataSample(dict(frame_id=t, ori_shape=(H, W), img_shape=(H, W), scale_factor=(1.0, 1.0)))
               for t in range(lo, hi)]
    return dict(inputs=inputs, data_samples=samples)


def _fields(sample):
    trk, det = sample.pred_track_instances, sample.pred_det_instances
    out = {k: trk[k].cpu().numpy() for k in ('bboxes', 'scores', 'depth', 'gt_depth', 'scales')}
    out['ids'] = trk.instances_id.cpu().numpy()
    out['det_bboxes'], out['det_scores'] = det.bboxes.cpu().numpy(), det.scores.cpu().numpy()
    return out


def test_reference_option_is_byte_identical(airdrone, cuda):
    a = _model(cuda).test_step(_data(airdrone, 0, T, cuda))
    b = _model(cuda, depth_extraction='reference').test_step(_data(airdrone, 0, T, cuda))
    torch.cuda.synchronize()
    n = 0
    for sa, sb in zip(a, b):
        fa, fb = _fields(sa), _fields(sb)
        for k in fa:
            assert fa[k].dtype == fb[k].dtype and fa[k].tobytes() == fb[k].tobytes(), k
        n += len(fa['ids'])
    assert n > 0, 'no tracks in the scenario'


@pytest.mark.parametrize('method', R.METHODS)
def test_shell_chunked_equals_per_frame_and_restatement(method, airdrone, cuda):
    """Chunked test_step (chunks of 4, the last one padded) equals per-frame predict; the tracks' depth and gt depth
    are the restatement on the unscaled track boxes (the disparity map and the gt map); the single-frame
    bbox_postp_depth uses the estimator too."""
    from stereotracking_amd.structures import InstanceData
    left, disp, depth = airdrone
    chunked = _model(cuda, depth_extraction=method)
    whole = chunked.test_step(_data(airdrone, 0, T, cuda))
    per = _model(cuda, depth_extraction=method)
    frames = []
    for t in range(T):
        frames += per.test_step(_data(airdrone, t, t + 1, cuda))
    torch.cuda.synchronize()
    n = 0
    for t, (a, b) in enumerate(zip(whole, frames)):
        fa, fb = _fields(a), _fields(b)
        assert fa['ids'].tolist() == fb['ids'].tolist(), f'frame {t}: track ids'
        for k in ('depth', 'gt_depth', 'scales', 'bboxes'):
            assert np.array_equal(fa[k], fb[k], equal_nan=True), f'frame {t}: {k}'
        k = len(fa['ids'])
        n += k
        if k:
            dmap = R.depth_map(disp[t])
            rd, _ = R.extract_depth(dmap, fa['bboxes'], method)
            rg, _ = R.extract_depth(depth[t], fa['bboxes'], method)
            for got, ref, what in ((fa['depth'], rd, 'depth'), (fa['gt_depth'], rg, 'gt_depth')):
                assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got == -1, ref == -1), what
                if method in ('median', 'center'):
                    assert np.array_equal(got, ref, equal_nan=True), f'frame {t}: {what}'
                else:
                    fin = np.isfinite(ref)
                    assert np.all(np.abs(got[fin] - ref[fin]) <= np.spacing(np.abs(ref[fin]))), f'frame {t}: {what}'
    assert n > 0, 'no tracks in the scenario'
    # the single-frame form (reference bbox_postp_depth) on frame 0's detections
    boxes = torch.from_numpy(_fields(whole[0])['det_bboxes']).to(cuda)
    assert len(boxes) > 0
    inst, dv = chunked.bbox_postp_depth(InstanceData(bboxes=boxes.clone()),
                                        torch.from_numpy(np.repeat(disp[0:1, None], 3, axis=1)).to(cuda),
                                        torch.from_numpy(depth[0:1, None]).to(cuda))
    torch.cuda.synchronize()
    assert_matches(method, R.depth_map(disp[0]), boxes.cpu().numpy(), inst['depth'].cpu().numpy(),
                   inst['scales'].cpu().numpy(), inst['bboxes'].cpu().numpy(), where='bbox_postp_depth')
    rg, _ = R.extract_depth(depth[0], boxes.cpu().numpy(), method)
    g = dv['gt_d_values'].cpu().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(rg))
    fin = np.isfinite(rg)
    assert np.all(np.abs(g[fin] - rg[fin]) <= np.spacing(np.abs(rg[fin])))


def test_median_config_builds_and_tracks(airdrone, cuda):
    model = _model(cuda, os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort',
                                      'yolox_s_mmyolo_mot_airdrone_disp_median.py'))
    assert model.depth_extraction == 'median'
    out = model.test_step(_data(airdrone, 0, T, cuda))
    torch.cuda.synchronize()
    assert sum(len(s.pred_track_instances) for s in out) > 0
    runner = next(iter(model._dense.values()))[0]
    assert runner.depth_method == 'median' and all(p.depth_method == 'median' for p in runner.pipes)


GUARDED = [test_kernel_on_random_maps, test_kernel_in_gt_depth_mode]      # st_box_depth_method, every estimator
NAN_BY_CONTRACT = GUARDED                                                  # a NaN depth is one of their decisions


# ---- the same entry points over hostile surroundings (tests/guard_memory.py) -------------------------------------------
test_entry_points_are_blind_to_guard_bands = gm.guarded_test(GUARDED, NAN_BY_CONTRACT, doc="""st_box_depth_method twice (guard_memory.run_both): as it stands, and with the map between guard bands of 0xFF
    bytes and NaN in its planes 1 and 2.  The hostile run passes the test's own bar against the restatement and equals
    the friendly run bit for bit.""")
