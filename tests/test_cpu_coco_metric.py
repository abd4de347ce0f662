"""CPU: the numpy restatement of COCO bbox evaluation (tests/coco_eval_ref.py, the yardstick of the GPU tests) against
answers derived by hand, and the host side of stereotracking_amd.coco_metric.CocoMetric: registry names, the `_eval`
config, unsupported metrics, format_only, the two-rank gather.  The evaluation itself needs the device and is covered by
tests/test_coco_metric_gpu.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import coco_eval_ref as ref  # noqa: E402
from stereotracking_amd import coco_metric  # noqa: E402
from stereotracking_amd.config import Config  # noqa: E402
from stereotracking_amd.registry import METRICS  # noqa: E402
from stereotracking_amd.structures import InstanceData, TrackDataSample  # noqa: E402

CFG_EVAL = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone_disp_eval.py')


def run(dets, gts, num_images=1, num_cats=1, **kw):
    """dets: (img, [x, y, w, h], score[, label]); gts: (img, [x, y, w, h][, crowd[, area[, cat]]]).  Integer boxes, so
    the float32 xyxy form is exact."""
    db = np.array([[d[1][0], d[1][1], d[1][0] + d[1][2], d[1][1] + d[1][3]] for d in dets], dtype=np.float32).reshape(-1, 4)
    gb = np.array([g[1] for g in gts], dtype=np.float64).reshape(-1, 4)
    return ref.evaluate(db, [d[2] for d in dets], [d[3] if len(d) > 3 else 0 for d in dets], [d[0] for d in dets], gb,
                        [g[3] if len(g) > 3 and g[3] is not None else g[1][2] * g[1][3] for g in gts],
                        [g[2] if len(g) > 2 else 0 for g in gts], [g[4] if len(g) > 4 else 0 for g in gts],
                        [g[0] for g in gts], num_images, num_cats, **kw)


def test_three_detections_two_boxes():
    """gt (0,0,40,40), (100,100,40,40), both area 1600 = medium.  Detections by score: hit .9, miss .8, hit .7.
    tp = 1,1,2  fp = 0,1,1 -> precision 1, 1/2, 2/3 -> from the right 1, 2/3, 2/3; recall 1/2, 1/2, 1.
    Recall points 0 .. .50 (51 of them) first reach rc at index 0 -> 1; .51 .. 1 (50) at index 2 -> 2/3.  Same at every
    IoU threshold (the IoUs are 1), so mAP = mAP_50 = mAP_75 = mAP_m = (51 + 50 * 2/3) / 101.  No small or large ground
    truth: -1.  Recall 1 wherever it is defined."""
    r = run([(0, [0, 0, 40, 40], .9), (0, [300, 300, 40, 40], .8), (0, [100, 100, 40, 40], .7)],
            [(0, [0, 0, 40, 40]), (0, [100, 100, 40, 40])])
    want = (51 + 50 * 2 / 3) / 101
    s = r['stats']
    assert abs(want - 0.83498) < 1e-5
    for i in (0, 1, 2, 4):
        assert s[i] == pytest.approx(want, abs=1e-12)
    assert s[3] == -1 and s[5] == -1 and s[9] == -1 and s[11] == -1
    assert s[6] == 1 and s[7] == 1 and s[8] == 1 and s[10] == 1
    assert np.array_equal(r['precision'][0, :51, 0, 0, 2], np.full(51, 1 / (0 + 1 + np.spacing(1))))   # the 2^-52 term
    assert np.array_equal(r['precision'][9, 51:, 0, 2, 0], np.full(50, 2 / (1 + 2 + np.spacing(1))))
    assert np.array_equal(r['scores'][0, :, 0, 0, 2], np.r_[np.full(51, np.float32(.9)), np.full(50, np.float32(.7))])
    assert r['npig'].tolist() == [[2, 0, 2, 0]]
    out = ref.mmdet_results(s, r['precision'])
    assert out == {'coco/bbox_mAP': 0.835, 'coco/bbox_mAP_50': 0.835, 'coco/bbox_mAP_75': 0.835, 'coco/bbox_mAP_s': -1.0,
                   'coco/bbox_mAP_m': 0.835, 'coco/bbox_mAP_l': -1.0}


def test_crowd_box_absorbs_two_detections():
    """gt A (0,0,40,40); crowd C (100,100,100,100).  d1 = A .9: tp.  d2 (110,110,40,40) .8 and d3 (150,150,40,40) .7 lie
    inside C: IoU against a crowd box = inter / det area = 1, and a crowd box can be matched again, so both are matched
    to C and ignored - neither is a false positive.  npig = 1 (C does not count): tp 1, fp 0 -> precision 1 at every
    recall point, recall 1, mAP 1."""
    r = run([(0, [0, 0, 40, 40], .9), (0, [110, 110, 40, 40], .8), (0, [150, 150, 40, 40], .7)],
            [(0, [0, 0, 40, 40]), (0, [100, 100, 100, 100], 1)])
    assert r['matched'][:, :, 0].all()
    assert not r['ignored'][0, :, 0].any() and r['ignored'][1:, :, 0].all()
    assert r['npig'][0, 0] == 1
    assert np.array_equal(r['precision'][:, :, 0, 0, 2], np.full((10, 101), 1 / (1 + np.spacing(1))))
    assert r['stats'][0] == pytest.approx(1.0, abs=1e-12) and r['stats'][8] == 1
    # without the crowd flag the same box is ordinary ground truth: IoU(d2, C) = 1600 / 10000 < .5 -> two misses
    r2 = run([(0, [0, 0, 40, 40], .9), (0, [110, 110, 40, 40], .8), (0, [150, 150, 40, 40], .7)],
             [(0, [0, 0, 40, 40]), (0, [100, 100, 100, 100], 0)])
    assert not r2['matched'][1:, :, 0].any() and r2['recall'][0, 0, 0, 2] == .5


def test_equal_iou_takes_the_later_box():
    """g0 (0,0,10,10), g1 (10,0,10,10); d1 (5,0,10,10) .9 overlaps each by 50 of a union of 150: IoU 1/3 with both, the
    same double.  At the single threshold .3 the walk moves on to the later box at equal IoU, so d1 takes g1.
    d2 (10,0,10,10) .8 is exactly g1, which is taken, and does not touch g0: unmatched.  Had d1 taken g0, d2 would have
    matched g1.  So: matched = [True, False], recall 1/2."""
    r = run([(0, [5, 0, 10, 10], .9), (0, [10, 0, 10, 10], .8)], [(0, [0, 0, 10, 10]), (0, [10, 0, 10, 10])],
            iou_thrs=[.3])
    assert r['matched'][:, 0, 0].tolist() == [True, False]
    assert r['recall'][0, 0, 0, 2] == .5
    # a strictly better box earlier is kept: d1 moved left by 1 overlaps g0 more
    r = run([(0, [4, 0, 10, 10], .9), (0, [10, 0, 10, 10], .8)], [(0, [0, 0, 10, 10]), (0, [10, 0, 10, 10])],
            iou_thrs=[.3])
    assert r['matched'][:, 0, 0].tolist() == [True, True] and r['recall'][0, 0, 0, 2] == 1


def test_equal_scores_across_images_image_order_decides():
    """Two images, one box each, both detections score .5.  Miss in image 0, hit in image 1: order miss, hit ->
    precision 0, 1/2 -> from the right 1/2, 1/2; recall 0, 1/2 -> the 51 points up to .5 read 1/2, the rest 0:
    AP = 51/2 / 101.  Hit in image 0, miss in image 1: precision 1, 1/2, recall 1/2, 1/2 -> 51 points read 1:
    AP = 51 / 101."""
    gts = [(0, [0, 0, 40, 40]), (1, [0, 0, 40, 40])]
    a = run([(0, [200, 200, 40, 40], .5), (1, [0, 0, 40, 40], .5)], gts, num_images=2)
    b = run([(0, [0, 0, 40, 40], .5), (1, [200, 200, 40, 40], .5)], gts, num_images=2)
    assert a['stats'][0] == pytest.approx(25.5 / 101, abs=1e-12)
    assert b['stats'][0] == pytest.approx(51 / 101, abs=1e-12)
    assert a['recall'][0, 0, 0, 2] == .5 and b['recall'][0, 0, 0, 2] == .5


def test_area_range_of_detection_and_of_its_match():
    """gt (0,0,30,30) area 900 = small; detection (0,0,34,34) area 1156 = medium; IoU = 900 / 1156 = .7785: a match at
    the six thresholds .5 .. .75, none at .8 .. .95.
      all:    matched, counted / unmatched, counted (fp)
      small:  matched to an in-range box: counted although its own area is outside / unmatched and outside: ignored
      medium: the box is out of range = ignored, the detection inherits it / unmatched, inside: counted (fp)
      large:  matched to an ignored box: ignored / unmatched and outside: ignored
    And the reverse (gt medium, detection small): small and medium swap roles."""
    lo, hi = slice(0, 6), slice(6, 10)
    r = run([(0, [0, 0, 34, 34], .9)], [(0, [0, 0, 30, 30])])
    m, ig = r['matched'][0], r['ignored'][0]
    assert m[lo].all() and not m[hi].any()
    assert not ig[:, 0].any()
    assert not ig[lo, 1].any() and ig[hi, 1].all()
    assert ig[lo, 2].all() and not ig[hi, 2].any()
    assert ig[:, 3].all()
    assert r['npig'].tolist() == [[1, 1, 0, 0]]
    assert r['recall'][:, 0, 1, 2].tolist() == [1] * 6 + [0] * 4 and (r['recall'][:, 0, 2, 2] == -1).all()
    r = run([(0, [0, 0, 30, 30], .9)], [(0, [0, 0, 34, 34])])
    m, ig = r['matched'][0], r['ignored'][0]
    assert m[lo].all() and not m[hi].any()
    assert ig[lo, 1].all() and not ig[hi, 1].any()
    assert not ig[lo, 2].any() and ig[hi, 2].all()
    assert r['npig'].tolist() == [[1, 0, 1, 0]]


def test_image_with_detections_and_no_ground_truth():
    """Image 0: one box, hit at .9.  Image 1: no ground truth, one detection at .95: a false positive that sorts first.
    precision 0, 1/2 -> 1/2, 1/2; recall 0, 1 -> all 101 points read 1/2: AP = 1/2, recall 1."""
    r = run([(0, [0, 0, 40, 40], .9), (1, [0, 0, 40, 40], .95)], [(0, [0, 0, 40, 40])], num_images=2)
    assert r['stats'][0] == pytest.approx(.5, abs=1e-12) and r['stats'][8] == 1
    assert r['scores'][0, 0, 0, 0, 2] == np.float32(.95) and r['scores'][0, 1, 0, 0, 2] == np.float32(.9)


def test_no_countable_ground_truth_leaves_minus_one():
    """Detections only, or only a crowd box: npig = 0 everywhere, every cell stays -1, every summary number is -1."""
    for gts in ([], [(0, [0, 0, 40, 40], 1)]):
        r = run([(0, [0, 0, 40, 40], .9)], gts)
        assert (r['precision'] == -1).all() and (r['recall'] == -1).all() and (r['scores'] == -1).all()
        assert (r['stats'] == -1).all()
        assert set(ref.mmdet_results(r['stats'], r['precision']).values()) == {-1.0}
    # ground truth and no detection at all: recall 0, precision 0 (not -1)
    r = run([], [(0, [0, 0, 40, 40])])
    assert (r['precision'][:, :, 0, 0, :] == 0).all() and (r['recall'][:, 0, 0, :] == 0).all()
    # a second category that nothing belongs to stays -1 next to one that is evaluated
    r = run([(0, [0, 0, 40, 40], .9)], [(0, [0, 0, 40, 40])], num_cats=2)
    assert (r['precision'][:, :, 1] == -1).all() and r['stats'][0] == pytest.approx(1.0, abs=1e-12)


def test_max_dets_cuts_a_true_positive_off():
    """Boxes A, B; detections miss .9, A .8, B .7.  max_dets (1, 2, 3): one detection per image keeps only the miss:
    AR 0; two keep the hit on A: AR 1/2; three: AR 1.  max_dets (1, 1, 2): the match is made on the first two, the third
    row gets rank -1; AP at two detections: precision 0, 1/2 -> 1/2, 1/2, recall 0, 1/2: 51 points read 1/2."""
    dets = [(0, [300, 300, 40, 40], .9), (0, [0, 0, 40, 40], .8), (0, [100, 100, 40, 40], .7)]
    gts = [(0, [0, 0, 40, 40]), (0, [100, 100, 40, 40])]
    r = run(dets, gts, max_dets=(1, 2, 3))
    assert r['stats'][6:9].tolist() == [0, .5, 1]
    r = run(dets, gts, max_dets=(1, 1, 2))
    assert r['rank'].tolist() == [0, 1, -1] and not r['matched'][2].any()
    assert r['stats'][0] == pytest.approx(25.5 / 101, abs=1e-12) and r['stats'][6:9].tolist() == [0, 0, .5]


def test_stable_order_inside_a_group_and_iou_on_a_threshold():
    """Equal scores inside one image keep arrival order: two detections of the same box at .5, the first one takes it.
    IoU exactly on a threshold is a match: (0,0,2,1) on (0,0,1,1) has IoU 1/2, (0,0,4,1) on (0,0,3,1) has 3/4, and
    np.linspace(.5, .95, 10)[5] is exactly .75."""
    r = run([(0, [0, 0, 40, 40], .5), (0, [0, 0, 40, 40], .5)], [(0, [0, 0, 40, 40])])
    assert r['rank'].tolist() == [0, 1] and r['matched'][0].all() and not r['matched'][1].any()
    assert ref.IOU_THRS[5] == .75 and ref.IOU_THRS[0] == .5
    r = run([(0, [0, 0, 2, 1], .9)], [(0, [0, 0, 1, 1])])
    assert r['recall'][:, 0, 0, 2].tolist() == [1] + [0] * 9
    r = run([(0, [0, 0, 4, 1], .9)], [(0, [0, 0, 3, 1])])
    assert r['recall'][:, 0, 0, 2].tolist() == [1] * 6 + [0] * 4


# ---- host side of the product ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['CocoMetric', 'mmdet.CocoMetric', 'CocoVideoMetric'])
def test_build_from_the_eval_config_under_each_registered_name(name):
    cfg = Config.fromfile(CFG_EVAL)
    assert cfg.val_evaluator == cfg.test_evaluator and len(cfg.test_evaluator) == 1
    entry = dict(cfg.test_evaluator[0])
    assert entry == dict(type='mmdet.CocoMetric', ann_file='data/AirSim_drone/annotations/val_cocoformat_80.json',
                         metric='bbox', format_only=False)
    assert cfg.model.type == 'OCSORT_Disparity' and cfg.DEPTH_RANGE == 80 and cfg.data_root == 'data/AirSim_drone/'
    m = METRICS.build(dict(entry, type=name))
    assert isinstance(m, coco_metric.CocoMetric)
    assert m.metrics == ['bbox'] and m.proposal_nums == [100, 300, 1000] and m.prefix == 'coco' and not m.format_only
    assert np.array_equal(m.iou_thrs, np.linspace(.5, .95, 10))
    assert METRICS.build(dict(entry, collect_device='cpu', backend_args=None, file_client_args=dict(backend='disk')))


@pytest.mark.parametrize('metric', ['segm', 'proposal', 'proposal_fast', ['bbox', 'segm'], 'keypoints'])
def test_unsupported_metric_is_refused_at_construction(metric):
    with pytest.raises((KeyError, NotImplementedError), match='bbox'):
        coco_metric.CocoMetric(metric=metric)


def test_bad_arguments():
    with pytest.raises(ValueError, match='outfile_prefix'):
        coco_metric.CocoMetric(format_only=True)
    with pytest.raises(ValueError, match='proposal_nums'):
        coco_metric.CocoMetric(proposal_nums=(100, 10, 1))
    with pytest.raises(KeyError, match='mAP_x'):
        coco_metric.CocoMetric(metric_items=['mAP_x'])
    m = coco_metric.CocoMetric()
    assert m.classes == ('drone',) and m.cat_ids == [1]          # MOTDispDataset.METAINFO
    m.dataset_meta = dict(classes=('drone', 'bird'))
    assert m.dataset_meta == dict(classes=('drone', 'bird')) and m.cat_ids == [1, 2]


def _sample(img_id, boxes, scores, labels=None):
    s = TrackDataSample(dict(img_id=img_id, ori_shape=(96, 160), frame_id=0))
    n = len(scores)
    s.pred_det_instances = InstanceData(bboxes=torch.tensor(boxes, dtype=torch.float32).reshape(n, 4),
                                        scores=torch.tensor(scores, dtype=torch.float32),
                                        labels=torch.tensor(labels if labels is not None else [0] * n, dtype=torch.long))
    return s


def test_format_only_writes_the_result_file(tmp_path):
    m = coco_metric.CocoMetric(format_only=True, outfile_prefix=str(tmp_path / 'out' / 'res'))
    m.process(_sample(7, [[1, 2, 11, 22]], [.5]))
    m.process([_sample(3, [[0, 0, 4, 4], [1.5, 1, 3, 5]], [.25, .75])])
    assert m.evaluate() == {}
    got = json.load(open(tmp_path / 'out' / 'res.bbox.json'))
    assert got == [dict(image_id=3, bbox=[0, 0, 4, 4], score=.25, category_id=1),
                   dict(image_id=3, bbox=[1.5, 1, 1.5, 4], score=.75, category_id=1),
                   dict(image_id=7, bbox=[1, 2, 10, 20], score=.5, category_id=1)]


def test_process_needs_ground_truth_or_an_annotation_file_and_keeps_references():
    m = coco_metric.CocoMetric()
    s = _sample(1, [[0, 0, 4, 4]], [.5])
    with pytest.raises(ValueError, match='instances'):
        m.process(s)
    m.process(s, [dict(bbox=[0, 0, 4, 6], ignore_flag=1, bbox_label=0)])
    rec = m.records[0]
    assert rec['bboxes'] is s.pred_det_instances.bboxes and rec['scores'] is s.pred_det_instances.scores
    assert rec['gt'] == [(0.0, 0.0, 4.0, 6.0, 24.0, 1, 0)] and rec['img_id'] == 1 and rec['ori_shape'] == (96, 160)


def test_evaluate_without_a_device_fails_loudly(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    m = coco_metric.CocoMetric()
    m.process(_sample(1, [[0, 0, 4, 4]], [.5]), [dict(bbox=[0, 0, 4, 4])])
    with pytest.raises(RuntimeError, match='no host implementation'):
        m.evaluate()


def _gather_worker(rank, world, port, q, duplicate):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    m = coco_metric.CocoMetric()
    ids = ([10, 11], [20, 10 if duplicate else 21])[rank]
    for i in ids:
        m.process(_sample(i, [[0, 0, float(i), 4]], [i / 100]), [dict(bbox=[0, 0, 4, 4])])
    try:
        m.gather()
        q.put((rank, 'ok', [(r['img_id'], type(r['bboxes']).__name__, r['bboxes'].tolist(), r['gt']) for r in m.records]))
    except RuntimeError as e:
        q.put((rank, 'error', str(e)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('duplicate', [False, True])
def test_gather_world2_gloo(duplicate):
    """The records of both ranks end up on both, in rank order, as host arrays; an image held twice is refused."""
    import multiprocessing as mp
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q, duplicate)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, state, payload in got:
        if duplicate:
            assert state == 'error' and 'more than one rank' in payload and '10' in payload
        else:
            assert state == 'ok'
            assert [r[0] for r in payload] == [10, 11, 20, 21]
            assert all(r[1] == 'ndarray' for r in payload) and payload[2][2] == [[0, 0, 20, 4]]
            assert payload[0][3] == [(0.0, 0.0, 4.0, 4.0, 16.0, 0, 0)]
