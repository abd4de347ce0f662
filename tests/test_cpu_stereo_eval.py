"""CPU suite: the dense stereo evaluator without a device - the numpy definitions (tests/stereo_eval_ref.py, to which the
kernel is held in tests/test_stereo_eval_gpu.py) on hand-derived answers and on every boundary, the summary formulas of
stereo_eval.StereoStats, StereoMetric (single process and a gloo world of 2), the config, the refusals and the ABI."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo_eval_ref as R       # noqa: E402

from stereotracking_amd import _lib, mot  # noqa: E402,F401
from stereotracking_amd import stereo_eval as S  # noqa: E402
from stereotracking_amd.config import Config  # noqa: E402
from stereotracking_amd.registry import METRICS, MODELS  # noqa: E402
from stereotracking_amd.structures import TrackDataSample  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'stereo_yolox_s_mot_airdrone_sgbm_dispeval.py')
N_GT, N_BOTH, BAD, D1, DELTA = 0, 1, slice(2, 6), 6, slice(7, 10)       # counter columns at T = 4


def maps(rows_p, rows_g):
    return np.asarray(rows_p, np.float32)[None, None], np.asarray(rows_g, np.float32)[None, None]


# ---- hand-derived answers ---------------------------------------------------------------------------------------------------
def test_known_answers_on_a_2x3_map():
    """bf = 160.  (0,0) g 20 -> gd 8, p 8.5: e 0.5;  (0,1) p 11: e 3;  (0,2) g 16 -> gd 10, p 8: e 2, pz 20, r 1.25;
    (1,0) p 0: ground truth only;  (1,1) p 40: e 32;  (1,2) g NaN: nothing.  All of it in depth bin 0."""
    pred, gt = maps([[8.5, 11, 8], [0, 40, 5]], [[20, 20, 16], [20, 20, np.nan]])
    counts, sums, hist = R.accumulate(pred, gt, 'depth', 160.0)
    assert counts.shape == (1, 2, 3, 10) and sums.shape == (1, 2, 3, 5) and hist.shape == (1, 2, 3, 512)
    assert counts[0, 0, 0].tolist() == [5, 4, 3, 3, 2, 1, 1, 1, 3, 3]
    assert counts[0, 0, 1:].sum() == 0 and counts[0, 1].sum() == 0
    assert sums[0, 0, 0, 0] == 37.5 and sums[0, 0, 0, 1] == 0.25 + 9 + 4 + 1024
    assert np.nonzero(hist[0, 0, 0])[0].tolist() == [8, 32, 48, 511] and hist.sum() == 4
    f = np.float32
    dz = [float(f(160) / f(p)) - g for p, g in ((8.5, 20.0), (11, 20.0), (8, 16.0), (40, 20.0))]
    gz = [20.0, 20.0, 16.0, 20.0]
    assert sums[0, 0, 0, 2] == pytest.approx(sum(abs(d) / g for d, g in zip(dz, gz)), rel=1e-15)
    assert sums[0, 0, 0, 3] == pytest.approx(sum(d * d / g for d, g in zip(dz, gz)), rel=1e-15)
    assert sums[0, 0, 0, 4] == pytest.approx(sum(d * d for d in dz), rel=1e-15)
    # a box over column 1 (x1 = 1 is inside, x2 = 2 is outside), twice: the pixels count once
    boxes = np.array([[[1, 0, 2, 2], [1, 0, 2, 5], [0, 0, 3, 2]]], np.float32)
    c2, s2, h2 = R.accumulate(pred, gt, 'depth', 160.0, boxes=boxes, box_counts=[2])
    assert c2[0, 1, 0].tolist() == [2, 2, 2, 2, 2, 1, 1, 0, 1, 1] and c2[0, 0, 0].tolist() == [3, 2, 1, 1, 0, 0, 0, 1, 2, 2]
    assert np.array_equal(c2.sum(1), counts.sum(1)) and np.array_equal(h2.sum(1), hist.sum(1))
    assert s2[0, 1, 0, 0] == 35.0 and s2[0, 0, 0, 0] == 2.5
    # the same maps as disparity ground truth
    c3, _, h3 = R.accumulate(pred, maps([[0]], [[8, 8, 10], [8, 8, np.nan]])[1], 'disp', 160.0)
    assert np.array_equal(c3, counts) and np.array_equal(h3, hist)


def _one(name):
    (p, g), = [(p, g) for n, p, g in R.boundary_pixels() if n == name]
    counts, _, hist = R.accumulate(*maps([[p]], [[g]]), 'depth', R.BF)
    assert counts.sum((0, 1, 2))[N_GT] <= 1
    return counts[0, 0], hist[0, 0]


def test_every_boundary_is_decided_the_stated_way():
    assert len({n for n, _, _ in R.boundary_pixels()}) == len(R.boundary_pixels())
    tot = lambda name: _one(name)[0].sum(0)      # noqa: E731
    assert tot('e==0.5')[BAD].tolist() == [0, 0, 0, 0]            # e == tau is not bad
    assert tot('e==1')[BAD].tolist() == [1, 0, 0, 0]
    assert tot('e==2')[BAD].tolist() == [1, 1, 0, 0]
    assert tot('e==3')[BAD].tolist() == [1, 1, 1, 0] and tot('e==3')[D1] == 0
    assert tot('e>3,rel<e')[BAD].tolist() == [1, 1, 1, 1] and tot('e>3,rel<e')[D1] == 1
    assert tot('e==3.5,rel>e')[BAD].tolist() == [1, 1, 1, 1] and tot('e==3.5,rel>e')[D1] == 0
    assert tot('e==4==rel')[D1] == 0 and tot('e==5,rel<e')[D1] == 1
    assert np.float32(0.05) * np.float32(80) == np.float32(4)
    # depth bins: upper edge inclusive
    assert _one('gz==20')[0][:, N_GT].tolist() == [1, 0, 0] and _one('gz>20')[0][:, N_GT].tolist() == [0, 1, 0]
    assert _one('gz==40')[0][:, N_GT].tolist() == [0, 1, 0] and _one('gz>40')[0][:, N_GT].tolist() == [0, 0, 1]
    assert _one('gz==80')[0][:, N_GT].tolist() == [0, 0, 1] and _one('gz>80')[0].sum() == 0
    assert tot('r==1.25')[DELTA].tolist() == [0, 1, 1] and tot('r<1.25')[DELTA].tolist() == [1, 1, 1]
    assert tot('r==1.5625')[DELTA].tolist()[0] == 0
    for name in ('p==0', 'p==-1', 'p==nan', 'p==inf'):
        assert tot(name).tolist() == [1] + [0] * 9, name           # ground truth counted, nothing else
    for name in ('g==0', 'g==nan', 'g==inf', 'g<0'):
        assert tot(name).sum() == 0, name
    assert np.nonzero(_one('e==31.875')[1].sum(0))[0].tolist() == [510]
    for name in ('e==31.9375', 'e==32', 'e==500'):
        assert np.nonzero(_one(name)[1].sum(0))[0].tolist() == [511], name
    assert np.nonzero(_one('e==0.5')[1].sum(0))[0].tolist() == [8]


def test_extent_and_other_planes_are_not_read():
    pred, gt = R.seeded_maps(4, 2, 3, 2, 6, 10)
    ext = [(4, 7), (6, 10)]
    a = R.accumulate(pred, gt, 'depth', R.BF, ext)
    pred2, gt2 = pred.copy(), gt.copy()
    pred2[:, 1:], gt2[:, 1:] = 9.0, 17.0
    pred2[0, :, 4:], pred2[0, :, :, 7:], gt2[0, :, 4:], gt2[0, :, :, 7:] = 9.0, 9.0, 17.0, 17.0
    b = R.accumulate(pred2, gt2, 'depth', R.BF, ext)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    full = R.accumulate(pred2, gt2, 'depth', R.BF)
    assert full[0][0, :, :, N_GT].sum() > a[0][0, :, :, N_GT].sum()


# ---- summary --------------------------------------------------------------------------------------------------------------
def _stats_2x3():
    pred, gt = maps([[8.5, 11, 8], [0, 40, 5]], [[20, 20, 16], [20, 20, np.nan]])
    return S.StereoStats(*R.accumulate(pred, gt, 'depth', 160.0))


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])), (k, a[k], b[k])


def test_summary_formulas_under_both_policies():
    st = _stats_2x3()
    s = st.summary('skip')
    assert (s['n_gt'], s['n_both'], s['EPE'], s['density']) == (5, 4, 37.5 / 4, 0.8)
    assert s['RMSE'] == math.sqrt(1037.25 / 4)
    assert [s[k] for k in ('bad_0.5', 'bad_1', 'bad_2', 'bad_3', 'D1')] == [0.75, 0.75, 0.5, 0.25, 0.25]
    assert (s['delta1'], s['delta2'], s['delta3']) == (0.25, 0.75, 0.75)
    assert (s['A50'], s['A90'], s['A99']) == (33 / 16, 32.0, 32.0)       # ceil(q * 4) = 2, 4, 4 -> bins 32, 511, 511
    b = st.summary('bad')
    assert [b[k] for k in ('bad_0.5', 'bad_1', 'bad_2', 'bad_3', 'D1')] == [0.8, 0.8, 0.6, 0.4, 0.4]
    assert b['EPE'] == s['EPE'] and b['density'] == 0.8
    for invalid in ('skip', 'bad'):
        _same(st.summary(invalid), R.summarize(*st.select(), invalid=invalid))
    with pytest.raises(ValueError, match='invalid'):
        st.summary('drop')


def test_quantiles_from_a_known_histogram_and_nan_on_empty_cells():
    hist = np.zeros(512, np.int64)
    hist[[0, 3, 100]] = [50, 40, 10]
    counts = np.array([100, 100, 0, 0, 0, 0, 0, 0, 0, 0])
    s = S.summarize_cell(counts, np.zeros(5), hist, (0.5, 1, 2, 3))
    assert (s['A50'], s['A90'], s['A99']) == (1 / 16, 4 / 16, 101 / 16)
    hist[3] = 39
    hist[100] = 11
    assert S.summarize_cell(counts, np.zeros(5), hist, (0.5, 1, 2, 3))['A90'] == 101 / 16
    empty = _stats_2x3().summary(bin=2)
    assert empty['n_gt'] == 0 and all(math.isnan(v) for k, v in empty.items() if k not in ('n_gt', 'n_both'))
    _same(empty, R.summarize(np.zeros(10, np.int64), np.zeros(5), np.zeros(512, np.int64)))
    nopred = S.summarize_cell(np.array([7, 0] + [0] * 8), np.zeros(5), np.zeros(512, np.int64), (0.5, 1, 2, 3), 'bad')
    assert nopred['density'] == 0 and nopred['bad_3'] == 1.0 and math.isnan(nopred['EPE'])


def test_stats_merge_select_and_refusals():
    pred, gt = R.seeded_maps(7, 3, 1, 1, 12, 20)
    boxes = np.repeat(np.array([[[2, 1, 9, 8]]], np.float32), 3, 0)
    acc = R.accumulate(pred, gt, 'depth', R.BF, boxes=boxes, box_counts=[1, 1, 1])
    st = S.StereoStats(*acc)
    assert len(st) == 3 and len(st.frames()) == 3 and len(st.total()) == 1
    a, b = S.StereoStats(*(x[:1] for x in acc)), S.StereoStats(*(x[1:] for x in acc))
    merged = a + b
    assert all(np.array_equal(getattr(merged, k), getattr(st, k)) for k in ('counts', 'sums', 'hist'))
    assert np.array_equal(sum(st.frames()[1:], st.frames()[0]).total().counts, st.total().counts)
    c_all, s_all, h_all = st.select()
    c_obj, _, _ = st.select('object')
    c_bg, _, _ = st.select('background')
    assert np.array_equal(c_obj + c_bg, c_all) and c_obj[0] > 0 and np.array_equal(c_all, acc[0].sum((0, 1, 2)))
    assert np.array_equal(sum(st.select(bin=k)[2] for k in range(3)), h_all)
    assert st.summary(region='object')['n_gt'] == int(c_obj[0])
    rep = st.report()
    assert {'stereo/EPE', 'stereo/bad_3', 'stereo/D1', 'stereo/density', 'stereo/abs_rel', 'stereo/EPE@20-40',
            'stereo/obj/EPE', 'stereo/bg/D1', 'stereo/A90@0-20'} <= set(rep)
    with pytest.raises(ValueError, match='merge'):
        a + S.StereoStats(*R.accumulate(pred, gt, 'depth', R.BF, depth_edges=(0, 80)), depth_edges=(0, 80))
    with pytest.raises(ValueError, match='fit'):
        S.StereoStats(acc[0], acc[1], acc[2], depth_edges=(0, 80))
    with pytest.raises(ValueError, match='region'):
        st.select('sky')
    with pytest.raises(ValueError, match='bin'):
        st.select(bin=3)
    for bad in (dict(depth_edges=(0,)), dict(depth_edges=(0, 20, 20)), dict(depth_edges=tuple(range(10))),
                dict(bad_thresholds=()), dict(bad_thresholds=(1,) * 7), dict(bad_thresholds=(float('nan'),))):
        with pytest.raises(ValueError):
            S.check_options(**bad)
    with pytest.raises(RuntimeError, match='CUDA'):       # no host fall-back
        S.stereo_error_stats(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2))


# ---- StereoMetric -----------------------------------------------------------------------------------------------------------
VIDEOS = {'v0': (11, 4), 'v1': (12, 3), 'v2': (13, 2)}      # name -> (seed, frames)


def _video(name):
    seed, frames = VIDEOS[name]
    pred, gt = R.seeded_maps(seed, frames, 1, 1, 16, 24)
    boxes = np.repeat(np.array([[[3, 2, 15, 11]]], np.float32), frames, 0)
    return pred, gt, boxes, [1] * frames


def _fill(metric, name):
    pred, gt, boxes, cnt = _video(name)
    st = S.StereoStats(*R.accumulate(pred, gt, 'depth', R.BF, boxes=boxes, box_counts=cnt))
    for t, frame in enumerate(st.frames()):
        metric.process(name, TrackDataSample(dict(frame_id=t, stereo_stats=frame)))


def _reference_report(names, invalid='skip'):
    """The summary over ALL pixels of the videos at once (one call of the reference on the stacked frames)."""
    parts = [_video(n) for n in names]
    pred, gt, boxes = (np.concatenate([p[i] for p in parts]) for i in range(3))
    counts, sums, hist = R.accumulate(pred, gt, 'depth', R.BF, boxes=boxes, box_counts=[1] * len(pred))
    c, s, h = counts.sum(0), sums.sum(0), hist.sum(0)
    out = {'stereo/' + k: v for k, v in R.summarize(c.sum((0, 1)), s.sum((0, 1)), h.sum((0, 1)), invalid=invalid).items()}
    for b, name in enumerate(('0-20', '20-40', '40-80')):
        out.update({f'stereo/{k}@{name}': v for k, v in R.summarize(c[:, b].sum(0), s[:, b].sum(0), h[:, b].sum(0),
                                                                    invalid=invalid).items()})
    for r, tag in ((1, 'obj'), (0, 'bg')):
        out.update({f'stereo/{tag}/{k}': v for k, v in R.summarize(c[r].sum(0), s[r].sum(0), h[r].sum(0),
                                                                   invalid=invalid).items()})
    return out


def _close(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k] == pytest.approx(b[k], rel=1e-12, nan_ok=True), k


@pytest.mark.parametrize('invalid', ['skip', 'bad'])
def test_metric_process_evaluate_equals_the_reference_over_all_pixels(invalid):
    m = METRICS.build(dict(type='mmtrack.StereoMetric', invalid=invalid))
    assert isinstance(m, S.StereoMetric)
    for name in ('v0', 'v1'):
        _fill(m, name)
    res = m.evaluate()
    assert sorted(res['per_video']) == ['v0', 'v1']
    _close(res['combined'], _reference_report(['v0', 'v1'], invalid))
    _close(res['per_video']['v1'], _reference_report(['v1'], invalid))
    assert res['combined']['stereo/n_gt'] == res['per_video']['v0']['stereo/n_gt'] + res['per_video']['v1']['stereo/n_gt']
    with pytest.raises(KeyError, match='stereo_stats'):
        m.process('v0', TrackDataSample(dict(frame_id=9)))
    with pytest.raises(ValueError, match='invalid'):
        S.StereoMetric(invalid='zero')
    assert S.StereoMetric().evaluate() == dict(per_video={}, combined={})


def _metric_worker(rank, world, port, q):
    import torch.distributed as dist
    from stereotracking_amd import dist as sdist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    names = sorted(VIDEOS)
    m = S.StereoMetric()
    for i in sdist.shard_videos(len(names)):
        _fill(m, names[i])
    res = m.evaluate()
    q.put((rank, res['combined'], sorted(res['per_video'])))
    dist.barrier()
    dist.destroy_process_group()


def test_metric_gather_world2_gloo_equals_single_process():
    import multiprocessing as mp
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_metric_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    single = S.StereoMetric()
    for name in sorted(VIDEOS):
        _fill(single, name)
    want = single.evaluate()
    _close(want['combined'], _reference_report(sorted(VIDEOS)))
    for rank, combined, videos in got:
        _same(combined, want['combined'])
        assert videos == sorted(VIDEOS)


# ---- config, shell option, ABI ---------------------------------------------------------------------------------------------
def test_config_parses_and_builds_its_evaluator_and_model():
    cfg = Config.fromfile(CFG)
    assert cfg.val_evaluator == cfg.test_evaluator and len(cfg.test_evaluator) == 3
    assert [dict(e)['type'] for e in cfg.test_evaluator] == ['mmdet.CocoMetric', 'mmtrack.MOTDroneMetrics',
                                                             'mmtrack.StereoMetric']
    m = METRICS.build(dict(cfg.test_evaluator[2]))
    assert isinstance(m, S.StereoMetric) and m.invalid == 'skip'
    assert cfg.model.stereo['type'] == 'StereoSGBM' and dict(cfg.model.stereo_eval)['boxes'] == 'gt'
    model = MODELS.build(dict(cfg.model, autotune=False))
    assert model.stereo_eval == dict(depth_edges=(0.0, 20.0, 40.0, 80.0), bad_thresholds=(0.5, 1.0, 2.0, 3.0), boxes='gt')
    base = Config.fromfile(CFG.replace('_dispeval', ''))
    assert MODELS.build(dict(base.model, autotune=False)).stereo_eval is None            # the default is off


def test_constructor_refusals():
    from stereotracking_amd.multistream import MultiStreamTracker
    from stereotracking_amd.sequence import track_gathered
    cfg = Config.fromfile(CFG)
    for bad, exc in ((dict(boxes='pred'), ValueError), (dict(edges=(0, 80)), ValueError), ('on', TypeError),
                     (dict(depth_edges=(0, 20, 10)), ValueError), (dict(bad_thresholds=(1,) * 7), ValueError)):
        with pytest.raises(exc):
            MODELS.build(dict(cfg.model, autotune=False, stereo_eval=bad))
    model = MODELS.build(dict(cfg.model, autotune=False))
    with pytest.raises(NotImplementedError, match='stereo_eval'):
        MultiStreamTracker(model, streams=2)
    with pytest.raises(NotImplementedError, match='stereo_eval'):
        track_gathered(torch.zeros(1, 2, 8), None, 1, model.tracker, model)


def test_abi_declares_the_entries_and_refuses_bad_arguments(stlib):
    for name in ('st_stereo_eval_workspace_bytes', 'st_stereo_eval'):
        assert hasattr(stlib, name) and name in _lib._PROTOS
    assert stlib.st_version() == 430
    a = _lib.StStereoEvalArgs()
    a.struct_size = C.sizeof(_lib.StStereoEvalArgs)
    a.N, a.H, a.W, a.gt_kind, a.num_bins, a.num_thresholds, a.max_boxes = 8, 736, 1280, 0, 3, 4, 0
    a.pred_img_pitch, a.gt_img_pitch, a.bf = 3 * 736 * 1280, 736 * 1280, 160.0
    for k, v in enumerate((0, 20, 40, 80)):
        a.depth_edges[k] = v
    for k, v in enumerate((0.5, 1, 2, 3)):
        a.bad_thresholds[k] = v
    need = stlib.st_stereo_eval_workspace_bytes(C.byref(a))
    assert need > 0 and need % 4 == 0 and need < 8 << 20
    assert stlib.st_stereo_eval(C.byref(a), *([None] * 10)) == -1 and b'null' in stlib.st_last_error()
    for field, value in (('num_bins', 9), ('num_thresholds', 0), ('max_boxes', 257), ('gt_kind', 2), ('bf', 0.0),
                         ('pred_img_pitch', 100), ('N', 0)):
        old = getattr(a, field)
        setattr(a, field, value)
        assert stlib.st_stereo_eval_workspace_bytes(C.byref(a)) == 0, field
        setattr(a, field, old)
    a.depth_edges[2] = 20
    assert stlib.st_stereo_eval_workspace_bytes(C.byref(a)) == 0 and b'ascend' in stlib.st_last_error()
    a.depth_edges[2] = 40
    a.struct_size -= 4
    assert stlib.st_stereo_eval_workspace_bytes(C.byref(a)) == 0 and b'struct_size' in stlib.st_last_error()
