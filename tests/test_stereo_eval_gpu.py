"""GPU: the dense stereo evaluator (csrc/stereo_eval.hip, stereo_eval.stereo_error_stats, OCSORT_Disparity(stereo_eval=...),
StereoMetric) against tests/stereo_eval_ref.py: counts and histogram EQUAL, the fp64 sums within 2 n_both 2^-53 S per cell
(two summation orders of n_both non-negative doubles - nothing else differs), two calls byte-identical, exact known answers
on synthetic truth, the memory contract, and the shell option against a plain run of the same model."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_memory as gm          # noqa: E402
import stereo_eval_ref as R       # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort')
ORI = (96, 160)

K8 = (0, 3, 6, 10, 15, 20, 40, 60, 80)
T6 = (0.25, 0.5, 1, 2, 3, 5)
BOXES3 = [[3.0, 1.0, 40.0, 4.0], [30.0, 0.0, 66.0, 31.0], [float('nan')] * 4]      # overlapping; the third row is not counted

# name: (N, C, Cg, H, W, extent, boxes (M rows per frame) / None, count, depth_edges, bad_thresholds, gt_kind)
CASES = {
    'one_pixel': (1, 1, 1, 1, 1, None, None, 0, (0, 20, 40, 80), (0.5, 1, 2, 3), 'depth'),
    'padded_extents': (3, 3, 1, 32, 96, [(5, 67), (32, 96), (1, 1)], BOXES3, 2, (0, 20, 40, 80), (0.5, 1, 2, 3), 'depth'),
    'several_ranges_k8_t6': (2, 3, 2, 70, 130, None, None, 0, K8, T6, 'disp'),
    'k1_t1': (1, 1, 1, 9, 33, None, None, 0, (0, 80), (3,), 'disp'),
    'ranges_boxes_depth': (2, 1, 1, 70, 130, [(70, 130), (69, 129)], BOXES3, 2, (0, 20, 40, 80), (0.5, 1, 2, 3), 'depth'),
    'full_size': (8, 1, 1, 736, 1280, [(720, 1280)] * 8, [[100.0, 50.0, 400.0, 300.0], [350.0, 250.0, 900.0, 700.0]], 2,
                  (0, 20, 40, 80), (0.5, 1, 2, 3), 'depth'),
}


def _case(name):
    N, C, Cg, H, W, extent, boxes, count, edges, taus, kind = CASES[name]
    pred, gt = R.seeded_maps(len(name), N, C, Cg, H, W, kind)
    bx = None if boxes is None else np.repeat(np.asarray(boxes, np.float32)[None], N, 0)
    return pred, gt, kind, extent, bx, None if boxes is None else [count] * N, edges, taus


def _run(cuda, pred, gt, kind, extent, bx, cnt, edges, taus):
    from stereotracking_amd.stereo_eval import stereo_error_stats
    return stereo_error_stats(torch.from_numpy(pred).to(cuda), torch.from_numpy(gt).to(cuda), kind, 0.25, 640,
                              extent=extent, boxes=None if bx is None else torch.from_numpy(bx).to(cuda),
                              box_counts=cnt, depth_edges=edges, bad_thresholds=taus)


@pytest.mark.parametrize('name', list(CASES))
def test_kernel_equals_the_numpy_definitions_and_repeats_its_bytes(cuda, name):
    pred, gt, kind, extent, bx, cnt, edges, taus = _case(name)
    got = _run(cuda, pred, gt, kind, extent, bx, cnt, edges, taus)
    counts, sums, hist = R.accumulate(pred, gt, kind, R.BF, extent, bx, cnt, edges, taus)
    assert got.counts.shape == counts.shape and got.sums.shape == sums.shape and got.hist.shape == hist.shape
    assert np.array_equal(got.counts, counts)
    assert np.array_equal(got.hist, hist)
    err, bound = np.abs(got.sums - sums), R.sum_bound(counts, sums)
    print(name, 'n_both', int(counts[..., 1].sum()), 'worst sums error / bound',
          float((err / np.where(bound > 0, bound, 1)).max()))
    assert (err <= bound).all()
    if name != 'one_pixel':
        assert counts[..., 1].sum() > 0 and (name == 'k1_t1' or (counts[:, :, :, 1].sum((0, 1)) > 0).all())
    if bx is not None:
        assert counts[:, 1, :, 0].sum() > 0                       # the object region is populated
    again = _run(cuda, pred, gt, kind, extent, bx, cnt, edges, taus)
    for a, b in ((got.counts, again.counts), (got.sums, again.sums), (got.hist, again.hist)):
        assert a.tobytes() == b.tobytes()


def test_boundary_pixels_alone(cuda):
    """The boundary pixels of the CPU test, as one row: the device decides each the stated way (the expectations are
    asserted on the reference in tests/test_cpu_stereo_eval.py)."""
    px = R.boundary_pixels()
    pred = np.array([[p for _, p, _ in px]], np.float32)[None, None]
    gt = np.array([[g for _, _, g in px]], np.float32)[None, None]
    got = _run(cuda, pred, gt, 'depth', None, None, None, (0, 20, 40, 80), (0.5, 1, 2, 3))
    counts, sums, hist = R.accumulate(pred, gt, 'depth', R.BF)
    assert np.array_equal(got.counts, counts) and np.array_equal(got.hist, hist)
    assert (np.abs(got.sums - sums) <= R.sum_bound(counts, sums)).all()


def test_exact_known_answers_on_synthetic_truth(cuda):
    from stereotracking_amd.stereo_eval import stereo_error_stats
    from stereotracking_amd.synthetic import synthetic_stereo_pair
    truth = synthetic_stereo_pair(3, height=64, width=96, max_disp=32, block=16)['disp'].copy()
    ys, xs = np.nonzero(truth > 0)
    drop = len(ys) % 4
    truth[ys[:drop], xs[:drop]] = 0                               # the number of valid pixels: a multiple of 4
    ys, xs = np.nonzero(truth > 0)
    n = len(ys)
    assert n > 1000 and n % 4 == 0 and truth.max() <= 28 and truth[truth > 0].min() >= 4    # gz = 160 / d in [5.7, 40]
    gt = torch.from_numpy(truth)[None, None].to(cuda)

    def summary(pred, invalid='skip'):
        st = stereo_error_stats(torch.from_numpy(pred)[None, None].to(cuda), gt, gt_kind='disp', baseline=0.25,
                                focal_length=640)
        assert st.counts[0, :, :, 0].sum() == n
        return st.summary(invalid)
    s = summary(truth)
    assert s['EPE'] == 0 and s['density'] == 1 and s['D1'] == 0 and s['A50'] == 1 / 16
    assert all(s[k] == 0 for k in ('bad_0.5', 'bad_1', 'bad_2', 'bad_3')) and s['delta1'] == 1 and s['abs_rel'] == 0
    s = summary(np.where(truth > 0, truth + 2, 0).astype(np.float32))
    assert s['EPE'] == 2 and s['RMSE'] == 2 and s['bad_1'] == 1 and s['bad_2'] == 0 and s['D1'] == 0 and s['density'] == 1
    quarter = truth.copy()
    quarter[ys[::4], xs[::4]] = 0
    skip, bad = summary(quarter), summary(quarter, 'bad')
    assert skip['density'] == 0.75 and bad['density'] == 0.75
    for k in ('bad_0.5', 'bad_1', 'bad_2', 'bad_3', 'D1'):
        assert skip[k] == 0 and bad[k] == 0.25


def test_cpu_tensors_and_bad_options_are_refused(cuda, stlib):
    import ctypes as C
    from stereotracking_amd import _lib
    from stereotracking_amd.stereo_eval import stereo_error_stats
    z = torch.zeros(1, 1, 4, 4)
    with pytest.raises(RuntimeError, match='CUDA'):
        stereo_error_stats(z, z.to(cuda))
    with pytest.raises(RuntimeError, match='CUDA'):
        stereo_error_stats(z.to(cuda), z)
    with pytest.raises(ValueError, match='ascend'):
        stereo_error_stats(z.to(cuda), z.to(cuda), depth_edges=(0, 20, 20))
    with pytest.raises(ValueError, match='thresholds'):
        stereo_error_stats(z.to(cuda), z.to(cuda), bad_thresholds=(1,) * 7)
    with pytest.raises(ValueError, match='gt_kind'):
        stereo_error_stats(z.to(cuda), z.to(cuda), gt_kind='depth_m')
    a = _lib.StStereoEvalArgs()
    a.struct_size = C.sizeof(_lib.StStereoEvalArgs) - 4
    assert stlib.st_stereo_eval_workspace_bytes(C.byref(a)) == 0
    assert stlib.st_stereo_eval(C.byref(a), *([None] * 10)) == -1 and b'struct_size' in stlib.st_last_error()


def test_memory_contract_hostile_padding_planes_and_stale_outputs(cuda):
    """pred / gt / boxes inside arenas between 0xFF bands; what the call may not read - the padding outside every extent,
    planes 1 and 2, the box rows past the count - holds NaN in one run and plausible finite values in the other; the
    outputs and the workspace come pre-filled with 0x00, 0xFF and 0x7F.  All six results: the same bytes; bands intact."""
    pred, gt, kind, extent, bx, cnt, edges, taus = _case('padded_extents')
    want = R.accumulate(pred, gt, kind, R.BF, extent, bx, cnt, edges, taus)
    results = []
    for hostile in (float('nan'), 9.0):
        p, g, b = pred.copy(), gt.copy(), bx.copy()
        p[:, 1:] = hostile
        b[:, 2:] = [0.0, 0.0, 1000.0, 1000.0] if hostile == 9.0 else hostile
        for n, (h, w) in enumerate(extent):
            for arr in (p, g):
                arr[n, :, h:, :] = hostile
                arr[n, :, :, w:] = hostile
        dp, dg, db = (gm.arena(torch.from_numpy(a), device=cuda) for a in (p, g, b))
        for fill in (0x00, 0xFF, 0x7F):
            with gm.poisoned_empty(fill) as poison:
                from stereotracking_amd.stereo_eval import stereo_error_stats
                st = stereo_error_stats(dp, dg, kind, 0.25, 640, extent=extent, boxes=db, box_counts=cnt,
                                        depth_edges=edges, bad_thresholds=taus)
            assert poison.device_count >= 2                       # the packed outputs and the workspace
            results.append(st)
        torch.cuda.synchronize()
        assert gm.bands_intact(dp, dg, db)
        assert gm.same_bits(dp.cpu(), torch.from_numpy(p)) and gm.same_bits(dg.cpu(), torch.from_numpy(g))
    for st in results:
        assert st.counts.tobytes() == results[0].counts.tobytes() and st.hist.tobytes() == results[0].hist.tobytes()
        assert st.sums.tobytes() == results[0].sums.tobytes()
    assert np.array_equal(results[0].counts, want[0]) and np.array_equal(results[0].hist, want[2])


# ---- the shell -----------------------------------------------------------------------------------------------------------
def _model(cfg_name, **kw):
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.synthetic import synthetic_state_dict
    cfg = Config.fromfile(os.path.join(CFG_DIR, cfg_name))
    for part in ('backbone', 'neck'):
        cfg.model.detector[part]['widen_factor'] = 0.375
    cfg.model.detector.bbox_head.head_module['widen_factor'] = 0.375
    cfg.model.tracker['init_track_thr'] = 0.03
    cfg.model.tracker['obj_score_thr'] = 0.02
    model = MODELS.build(dict(cfg.model, autotune=False, dense_batch=8, inflight=2, **kw))
    sd = synthetic_state_dict(list(model.detector._table), seed=5, prior_prob=0.2, logit_std=2.5)
    model.detector.load_state_dict(sd, strict=False)
    return model


_SEQ = {}


def _sequence():
    """ONE 11-frame synthetic stereo sequence (numpy, built once and left unchanged): frames, true disparity -> depth
    maps (with holes), ground-truth boxes."""
    if not _SEQ:
        from stereotracking_amd.sequence import synthetic_sequence
        fr = list(synthetic_sequence(11, 3, ORI[0], ORI[1], 48, seed=2))
        depth = [np.where(f['disp'] > 0, R.BF / np.maximum(f['disp'], 1e-3), 0).astype(np.float32) for f in fr]
        for t, d in enumerate(depth):
            d[t:t + 5, 10:40] = 0.0                                # holes in the ground truth
        _SEQ.update(left=[f['left'] for f in fr], right=[f['right'] for f in fr], depth=depth,
                    disp=[f['disp'] for f in fr], boxes=[f['gt'][:, 1:5].copy() for f in fr])
    return _SEQ


def _data(cuda, mono=False, with_depth=True):
    from stereotracking_amd.structures import InstanceData, TrackDataSample
    seq = _sequence()
    def dev(frames):
        return [torch.from_numpy(f)[None].to(cuda) for f in frames]
    inputs = dict(img=dev(seq['left']))
    if mono:
        inputs['disp_postp'] = [torch.from_numpy(np.repeat(d[None, None], 3, axis=1)).to(cuda) for d in seq['disp']]
    else:
        inputs['right'] = dev(seq['right'])
    if with_depth:
        inputs['depth_postp'] = [torch.from_numpy(d[None, None]).to(cuda) for d in seq['depth']]
    samples = []
    for t in range(11):
        s = TrackDataSample(dict(frame_id=t, ori_shape=ORI, img_shape=ORI, scale_factor=(1.0, 1.0)))
        s.gt_instances = InstanceData(bboxes=torch.from_numpy(seq['boxes'][t]))
        samples.append(s)
    return dict(inputs=inputs, data_samples=samples)


def _same_results(a_list, b_list):
    assert len(a_list) == len(b_list)
    n = 0
    for a, b in zip(a_list, b_list):
        ta, tb = a.pred_track_instances, b.pred_track_instances
        assert ta.instances_id.tolist() == tb.instances_id.tolist()
        for key in ('bboxes', 'scores', 'depth', 'gt_depth', 'scales', 'labels'):
            assert torch.equal(ta[key].nan_to_num(-7.0), tb[key].nan_to_num(-7.0)), key
        for key in ('bboxes', 'scores', 'labels'):
            assert torch.equal(a.pred_det_instances[key], b.pred_det_instances[key]), key
        n += len(ta)
    assert n > 0, 'no tracks in the scenario'


def _stats_equal(a, b):
    return (np.array_equal(a.counts, b.counts) and np.array_equal(a.hist, b.hist) and
            a.sums.tobytes() == b.sums.tobytes() and (a.depth_edges, a.bad_thresholds) == (b.depth_edges, b.bad_thresholds))


@pytest.fixture(scope='module')
def sgbm_run(cuda):
    """The stereo-input configuration with StereoSGBM over 11 frames at dense_batch 8 (a ragged second chunk), with the
    evaluator on and off."""
    cfg = 'stereo_yolox_s_mot_airdrone_sgbm.py'
    on = _model(cfg, stereo_eval=dict(boxes='gt'))
    off = _model(cfg)
    assert off.stereo_eval is None
    got = on.test_step(_data(cuda))
    plain = off.test_step(_data(cuda))
    torch.cuda.synchronize()
    return on, off, got, plain


def test_shell_stats_equal_the_function_on_a_plain_pipeline_run_and_nothing_else_moves(cuda, sgbm_run):
    from stereotracking_amd.stereo_eval import stereo_error_stats
    on, off, got, plain = sgbm_run
    _same_results(got, plain)
    assert all('stereo_stats' not in s.metainfo for s in plain)
    seq = _sequence()
    pipe = off.dense_runner(ORI, True, 8).pipes[0]                 # a plain StereoDensePipeline of the same model
    total_both = 0
    for s, e in ((0, 8), (8, 11)):
        idx = list(range(s, e)) + [e - 1] * (8 - (e - s))
        left = torch.from_numpy(np.stack([seq['left'][i] for i in idx])).to(cuda).float()
        right = torch.from_numpy(np.stack([seq['right'][i] for i in idx])).to(cuda).float()
        disp = pipe.run(left, right)['disp_postp'].clone()
        depth = torch.from_numpy(np.stack([seq['depth'][i] for i in idx]))[:, None].to(cuda)
        M = max(len(seq['boxes'][i]) for i in idx)
        bx = torch.zeros(8, max(M, 1), 4)
        for k, i in enumerate(idx):
            bx[k, :len(seq['boxes'][i])] = torch.from_numpy(seq['boxes'][i])
        want = stereo_error_stats(disp, depth, 'depth', on.baseline, on.focal_length, extent=[ORI] * 8, boxes=bx.to(cuda),
                                  box_counts=[len(seq['boxes'][i]) for i in idx]).frames()
        for k in range(e - s):
            st = got[s + k].metainfo['stereo_stats']
            assert len(st) == 1 and _stats_equal(st, want[k]), s + k
            total_both += int(st.counts[0, :, :, 1].sum())
    assert total_both > 11 * 1000                                  # SGBM found most of every frame
    assert sum(int(s.metainfo['stereo_stats'].counts[0, 1, :, 0].sum()) for s in got) > 0     # ... and the gt boxes count


def test_stereo_metric_fed_from_the_shell_equals_the_reference_summary(cuda, sgbm_run):
    from stereotracking_amd.registry import METRICS
    on, off, got, _ = sgbm_run
    metric = METRICS.build(dict(type='mmtrack.StereoMetric'))
    for t, s in enumerate(got):
        metric.process('a' if t < 6 else 'b', s)
    res = metric.evaluate()
    assert sorted(res['per_video']) == ['a', 'b']
    tot = [np.sum([s.metainfo['stereo_stats'].__dict__[k] for s in got], axis=0)[0] for k in ('counts', 'sums', 'hist')]
    want = R.summarize(tot[0].sum((0, 1)), tot[1].sum((0, 1)), tot[2].sum((0, 1)))
    for k, v in want.items():
        assert res['combined']['stereo/' + k] == pytest.approx(v, rel=1e-12, nan_ok=True), k
    want = R.summarize(tot[0][1].sum(0), tot[1][1].sum(0), tot[2][1].sum(0))
    assert res['combined']['stereo/obj/EPE'] == pytest.approx(want['EPE'], rel=1e-12, nan_ok=True)
    assert res['combined']['stereo/n_both'] == sum(res['per_video'][v]['stereo/n_both'] for v in 'ab')
    assert 0 < res['combined']['stereo/density'] <= 1 and 'stereo/EPE@20-40' in res['combined']


def test_mono_png_disparity_configuration_scores_the_dataset_maps(cuda):
    model = _model('yolox_s_mmyolo_mot_airdrone_disp.py', stereo_eval=dict(depth_edges=(0, 40, 80), bad_thresholds=(1, 3)))
    got = model.test_step(_data(cuda, mono=True))
    seq = _sequence()
    for t, s in enumerate(got):
        st = s.metainfo['stereo_stats']
        assert st.counts.shape == (1, 2, 2, 8) and st.counts[0, 1].sum() == 0          # boxes=None: no object region
        pred, gt = np.repeat(seq['disp'][t][None, None], 3, 1), seq['depth'][t][None, None]
        counts, sums, hist = R.accumulate(pred, gt, 'depth', R.BF, depth_edges=(0, 40, 80), bad_thresholds=(1, 3))
        assert np.array_equal(st.counts, counts) and np.array_equal(st.hist, hist)
        assert (np.abs(st.sums - sums) <= R.sum_bound(counts, sums)).all()
        assert st.summary()['bad_3'] == 0 and st.counts[0, 0, :, 1].sum() > 10000      # the truth against itself
    with pytest.raises(KeyError, match='depth_postp'):
        model.test_step(_data(cuda, mono=True, with_depth=False))
