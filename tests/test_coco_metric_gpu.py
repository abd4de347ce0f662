"""GPU: the device evaluation (csrc/coco_eval.hip through stereotracking_amd.coco_metric) against the numpy restatement
tests/coco_eval_ref.py on the same inputs.  np.array_equal throughout - rank, matched / ignored tables, npig, precision,
recall, scores, the 12 stats and the returned dict: the outputs are integer counts and single fp64 divisions of them, so
no tolerance is needed and none is used.  Output buffers are poisoned before every launch: a cell that the contract
says is written and is not fails the comparison (NaN / -77 / all-ones never equal the restatement)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import coco_eval_ref as ref  # noqa: E402

CFG_EVAL = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone_disp_eval.py')
H, W, T = 96, 160, 10

pytestmark = pytest.mark.gpu


# ---- inputs ---------------------------------------------------------------------------------------------------------
def random_set(seed, num_images, num_cats, max_gt=12, max_det=60, empty_every=7):
    """Flat rows.  Box sides are log-uniform over 4 .. 250 (all three area ranges), a tenth of the ground truth is
    crowd, scores have two decimals (ties inside and across images), most detections are jittered copies of ground
    truth (shift up to a quarter of the side, scale .8 .. 1.25: IoUs on both sides of every threshold).  Image kinds:
    every `empty_every`-th has no ground truth, the next one no detections, the one after neither."""
    rng = np.random.RandomState(seed)
    db, dsc, dl, di, gb, ga, gc, gk, gi = [], [], [], [], [], [], [], [], []
    for img in range(num_images):
        kind = img % empty_every
        ng = 0 if kind in (0, 2) else rng.randint(0, max_gt + 1)
        nd = 0 if kind in (1, 2) else rng.randint(0, max_det + 1)
        boxes = []
        for _ in range(ng):
            w, h = np.exp(rng.uniform(np.log(4), np.log(250), 2))
            x, y = rng.uniform(0, 1000, 2)
            boxes.append((x, y, w, h))
            gb.append((x, y, w, h))
            ga.append(w * h * rng.choice([1.0, 0.8]))
            gc.append(int(rng.rand() < 0.1))
            gk.append(rng.randint(num_cats))
            gi.append(img)
        for _ in range(nd):
            if boxes and rng.rand() < 0.8:
                j = rng.randint(len(boxes))
                x, y, w, h = boxes[j]
                x, y = x + rng.uniform(-.25, .25) * w, y + rng.uniform(-.25, .25) * h
                w, h = w * rng.uniform(.8, 1.25), h * rng.uniform(.8, 1.25)
                k = gk[len(gk) - len(boxes) + j] if rng.rand() < 0.9 else rng.randint(num_cats)
            else:
                w, h = np.exp(rng.uniform(np.log(4), np.log(250), 2))
                x, y = rng.uniform(0, 1000, 2)
                k = rng.randint(num_cats)
            db.append((x, y, x + w, y + h))
            dsc.append(round(rng.rand(), 2))
            dl.append(k)
            di.append(img)
    return dict(det_boxes=np.array(db, dtype=np.float32).reshape(-1, 4), det_scores=np.array(dsc, dtype=np.float32),
                det_labels=np.array(dl, dtype=np.int32), det_img=np.array(di, dtype=np.int32),
                gt_boxes=np.array(gb, dtype=np.float64).reshape(-1, 4), gt_area=np.array(ga, dtype=np.float64),
                gt_crowd=np.array(gc, dtype=np.int32), gt_cat=np.array(gk, dtype=np.int32),
                gt_img=np.array(gi, dtype=np.int32), num_images=num_images, num_cats=num_cats)


def unpack_bits(words, T_, A_):
    w = np.asarray(words).astype(np.uint64)
    return np.stack([np.stack([((w >> np.uint64(t * A_ + a)) & np.uint64(1)).astype(bool) for a in range(A_)], axis=1)
                     for t in range(T_)], axis=1)


def run_device(s, cuda, **kw):
    from stereotracking_amd.coco_metric import coco_eval_device, default_params
    p = default_params()
    T_ = len(kw.get('iou_thrs') if kw.get('iou_thrs') is not None else p['iou_thrs'])
    A_, R_, M_ = len(p['area_rngs']), len(p['rec_thrs']), len(kw.get('max_dets', (100, 300, 1000)))
    D, K = len(s['det_scores']), s['num_cats']
    poison = dict(rank=torch.full((D,), -77, dtype=torch.int32, device=cuda),
                  matched=torch.full((D,), -1, dtype=torch.int64, device=cuda),
                  ignored=torch.full((D,), -1, dtype=torch.int64, device=cuda),
                  npig=torch.full((K, A_), -77, dtype=torch.int32, device=cuda),
                  precision=torch.full((T_, R_, K, A_, M_), float('nan'), dtype=torch.float64, device=cuda),
                  recall=torch.full((T_, K, A_, M_), float('nan'), dtype=torch.float64, device=cuda),
                  scores=torch.full((T_, R_, K, A_, M_), float('nan'), dtype=torch.float64, device=cuda),
                  status=torch.full((4,), -77, dtype=torch.int32, device=cuda))
    out = coco_eval_device(torch.from_numpy(s['det_boxes']).to(cuda), torch.from_numpy(s['det_scores']).to(cuda),
                           torch.from_numpy(s['det_labels']).to(cuda), torch.from_numpy(s['det_img']), s['gt_boxes'],
                           s['gt_area'], s['gt_crowd'], s['gt_cat'], s['gt_img'], s['num_images'], K, out=poison, **kw)
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy() for k in poison}
    got['matched'], got['ignored'] = unpack_bits(got['matched'], T_, A_), unpack_bits(got['ignored'], T_, A_)
    return got


def compare(s, cuda, **kw):
    from stereotracking_amd.coco_metric import summarize, default_params
    want = ref.evaluate(s['det_boxes'], s['det_scores'], s['det_labels'], s['det_img'], s['gt_boxes'], s['gt_area'],
                        s['gt_crowd'], s['gt_cat'], s['gt_img'], s['num_images'], s['num_cats'], **kw)
    got = run_device(s, cuda, **kw)
    assert got['status'].tolist() == [0, 0, 0, 0]
    for k in ('rank', 'matched', 'ignored', 'npig', 'precision', 'recall', 'scores'):
        assert got[k].shape == want[k].shape, k
        bad = int(np.sum(got[k] != want[k]))
        print(f'{k}: {got[k].size} cells, {bad} differ')
        assert np.array_equal(got[k], want[k]), k
    iou = kw.get('iou_thrs')
    iou = default_params()['iou_thrs'] if iou is None else np.asarray(iou, dtype=np.float64)
    stats = summarize(got['precision'], got['recall'], iou, list(kw.get('max_dets', (100, 300, 1000))))
    print('stats', stats.tolist())
    assert np.array_equal(stats, want['stats'])
    return want, got


# ---- random sets ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed,num_images,num_cats', [(0, 220, 1), (1, 260, 3)])
def test_random_sets_equal_the_restatement(cuda, seed, num_images, num_cats):
    s = random_set(seed, num_images, num_cats)
    want, _ = compare(s, cuda)
    # the set is not trivial: every area range has ground truth, hits and misses exist, ties exist
    assert (want['npig'] > 0).all()
    assert want['matched'].any() and not want['matched'].all() and want['ignored'].any()
    assert 0 < want['stats'][0] < 1 and len(np.unique(s['det_scores'])) < len(s['det_scores']) / 4


def test_custom_thresholds_and_proposal_nums_that_bite(cuda):
    """proposal_nums (1, 10, 100) with up to 150 detections per image (one category: every image is one group), so the
    cut at max_dets[-1] drops rows and the prefixes at 1 and 10 differ; thresholds that are not the default ten."""
    s = random_set(2, 60, 1, max_gt=12, max_det=150)
    want, got = compare(s, cuda, iou_thrs=[.3, .5, .77, .9], max_dets=(1, 10, 100))
    assert (want['rank'] == -1).sum() > 50                       # rows beyond the 100th of their group
    r = want['recall'][:, 0, 0, :]
    assert (r[:, 0] < r[:, 1]).all() and (r[:, 1] < r[:, 2]).all()
    assert want['stats'][2] == -1                               # .75 is not among the thresholds


def test_ground_truth_cap_is_supported_and_refused_above(cuda):
    from stereotracking_amd import _lib
    from stereotracking_amd.coco_metric import max_gt_per_group
    cap = max_gt_per_group()
    assert cap >= 128
    rng = np.random.RandomState(3)

    def one_image(ng, nd=40):
        xy = rng.uniform(0, 900, (ng, 2))
        wh = rng.uniform(8, 120, (ng, 2))
        gb = np.concatenate([xy, wh], axis=1)
        pick = rng.randint(0, ng, nd)
        d = gb[pick] + rng.uniform(-3, 3, (nd, 4))
        db = np.stack([d[:, 0], d[:, 1], d[:, 0] + d[:, 2], d[:, 1] + d[:, 3]], axis=1).astype(np.float32)
        return dict(det_boxes=db, det_scores=np.round(rng.rand(nd), 2).astype(np.float32),
                    det_labels=np.zeros(nd, dtype=np.int32), det_img=np.zeros(nd, dtype=np.int32), gt_boxes=gb,
                    gt_area=gb[:, 2] * gb[:, 3], gt_crowd=(rng.rand(ng) < .1).astype(np.int32),
                    gt_cat=np.zeros(ng, dtype=np.int32), gt_img=np.zeros(ng, dtype=np.int32), num_images=1, num_cats=1)
    want, _ = compare(one_image(cap), cuda)
    assert want['matched'].any()
    with pytest.raises(_lib.StError, match='ST_ERR_INVALID'):
        run_device(one_image(cap + 1), cuda)


def test_empty_inputs_of_each_kind(cuda):
    s = random_set(4, 30, 2)
    none = np.zeros(0, dtype=np.int32)
    no_det = dict(s, det_boxes=np.zeros((0, 4), dtype=np.float32), det_scores=np.zeros(0, dtype=np.float32),
                  det_labels=none, det_img=none)
    no_gt = dict(s, gt_boxes=np.zeros((0, 4)), gt_area=np.zeros(0), gt_crowd=none, gt_cat=none, gt_img=none)
    want, _ = compare(no_det, cuda)
    assert (want['recall'][:, :, 0, :] == 0).all()
    want, _ = compare(no_gt, cuda)
    assert (want['precision'] == -1).all()
    compare(dict(no_det, **{k: no_gt[k] for k in ('gt_boxes', 'gt_area', 'gt_crowd', 'gt_cat', 'gt_img')}), cuda)


def test_iou_exactly_on_a_threshold_is_a_match(cuda):
    """(0,0,2,1) on (0,0,1,1): IoU 1/2; (0,0,4,1) on (0,0,3,1): IoU 3/4; np.linspace(.5, .95, 10)[5] is exactly .75."""
    def one(dw, gw):
        return dict(det_boxes=np.array([[0, 0, dw, 1]], dtype=np.float32), det_scores=np.array([.9], dtype=np.float32),
                    det_labels=np.zeros(1, dtype=np.int32), det_img=np.zeros(1, dtype=np.int32),
                    gt_boxes=np.array([[0., 0., gw, 1.]]), gt_area=np.array([float(gw)]), gt_crowd=np.zeros(1, dtype=np.int32),
                    gt_cat=np.zeros(1, dtype=np.int32), gt_img=np.zeros(1, dtype=np.int32), num_images=1, num_cats=1)
    _, got = compare(one(2, 1), cuda)
    assert got['recall'][:, 0, 0, 2].tolist() == [1] + [0] * 9
    _, got = compare(one(4, 3), cuda)
    assert got['recall'][:, 0, 0, 2].tolist() == [1] * 6 + [0] * 4


# ---- the metric class -----------------------------------------------------------------------------------------------
def _sample(img_id, boxes, scores, labels, cuda):
    from stereotracking_amd.structures import InstanceData, TrackDataSample
    s = TrackDataSample(dict(img_id=img_id, ori_shape=(1000, 1000), frame_id=0))
    s.pred_det_instances = InstanceData(bboxes=torch.from_numpy(boxes).to(cuda), scores=torch.from_numpy(scores).to(cuda),
                                        labels=torch.from_numpy(labels).to(cuda).long())
    return s


def test_metric_dict_classwise_items_and_bad_rows(cuda):
    """CocoMetric fed per image, in shuffled order with non-contiguous image ids: the returned dict (rounded the mmdet
    way), stats and arrays equal the restatement's; a NaN score raises ValueError naming the image."""
    from stereotracking_amd.coco_metric import CocoMetric
    s = random_set(5, 80, 3)
    classes = ('drone', 'bird', 'kite')
    img_id_of = [10 + 3 * i for i in range(s['num_images'])]
    items = ['mAP', 'mAP_s', 'AR@100', 'AR_l@1000']

    def fill(metric, poison_image=None):
        for img in np.random.RandomState(0).permutation(s['num_images']):
            d, g = s['det_img'] == img, s['gt_img'] == img
            sc = s['det_scores'][d].copy()
            if img == poison_image:
                sc[0] = np.nan
            inst = [dict(bbox=[b[0], b[1], b[0] + b[2], b[1] + b[3]], ignore_flag=int(c), bbox_label=int(k))
                    for b, c, k in zip(s['gt_boxes'][g], s['gt_crowd'][g], s['gt_cat'][g])]
            metric.process(_sample(img_id_of[img], s['det_boxes'][d], sc, s['det_labels'][d], cuda), inst)
    m = CocoMetric(classes=classes, classwise=True, metric_items=items)
    fill(m)
    got = m.evaluate()
    # ground truth as the metric builds it from `instances`: xyxy -> xywh by subtraction, area = w * h
    gb = s['gt_boxes'].copy()
    x2, y2 = gb[:, 0] + gb[:, 2], gb[:, 1] + gb[:, 3]
    gb[:, 2], gb[:, 3] = x2 - gb[:, 0], y2 - gb[:, 1]
    want = ref.evaluate(s['det_boxes'], s['det_scores'], s['det_labels'], s['det_img'], gb, gb[:, 2] * gb[:, 3],
                        s['gt_crowd'], s['gt_cat'], s['gt_img'], s['num_images'], 3)
    assert np.array_equal(m.precision, want['precision']) and np.array_equal(m.recall, want['recall'])
    assert np.array_equal(m.scores, want['scores']) and np.array_equal(m.stats, want['stats'])
    want_dict = ref.mmdet_results(want['stats'], want['precision'], classes, items, classwise=True)
    print(got)
    assert got == want_dict and list(got) == list(want_dict)
    assert set(got) == {'coco/bbox_mAP', 'coco/bbox_mAP_s', 'coco/bbox_AR@100', 'coco/bbox_AR_l@1000',
                        'coco/drone_precision', 'coco/bird_precision', 'coco/kite_precision'}
    bad_img = int(s['det_img'][len(s['det_img']) // 2])
    m = CocoMetric(classes=classes)
    fill(m, poison_image=bad_img)
    with pytest.raises(ValueError, match=f'image {img_id_of[bad_img]}\\b'):
        m.evaluate()


# ---- through the product --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def airdrone(tmp_path_factory):
    from make_tiny_airdrone import make
    from stereotracking_amd import datasets as ds
    base, _ = make(str(tmp_path_factory.mktemp('airdrone_coco')), videos=1, frames=T, height=H, width=W, max_disp=32,
                   objects=4)
    ann = os.path.join(base, 'annotations', 'val_cocoformat_80.json')
    dataset = ds.MOTDispDataset(ann_file='annotations/val_cocoformat_80.json', data_root=base + os.sep,
                                data_prefix=dict(img_path='val/'))
    (_, idx), = dataset.video_indices()
    seq = ds.load_video(dataset, idx, False, pin=False)[0]
    codes = seq.codes.numpy().view(np.uint16)
    disp = np.where(codes == 65535, 0.0, codes / 16.0).astype(np.float32)
    infos = [dataset.get_data_info(i) for i in idx]
    return seq.left.numpy(), disp, infos, ann


def _detect(airdrone, cuda):
    """make_tiny_airdrone -> MOTDispDataset -> MODELS.build(cfg.model).test_step: the data samples with
    pred_det_instances on the device, and the evaluator entry of the config."""
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.structures import TrackDataSample
    from stereotracking_amd.synthetic import synthetic_state_dict
    cfg = Config.fromfile(CFG_EVAL)
    for part in ('backbone', 'neck'):
        cfg.model.detector[part]['widen_factor'] = 0.375
    cfg.model.detector.bbox_head.head_module['widen_factor'] = 0.375
    model = MODELS.build(dict(cfg.model, autotune=False, dense_batch=4, inflight=2))
    model.detector.load_state_dict(synthetic_state_dict(list(model.detector._table), seed=5, prior_prob=0.2,
                                                        logit_std=2.5), strict=False)
    left, disp, infos, _ = airdrone
    inputs = dict(img=[torch.from_numpy(left[t:t + 1]).to(cuda) for t in range(T)],
                  disp_postp=[torch.from_numpy(np.repeat(disp[t:t + 1, None], 3, axis=1)).to(cuda) for t in range(T)])
    samples = [TrackDataSample(dict(frame_id=t, img_id=infos[t]['img_id'], ori_shape=(H, W), img_shape=(H, W),
                                    scale_factor=(1.0, 1.0))) for t in range(T)]
    return model.test_step(dict(inputs=inputs, data_samples=samples)), cfg.test_evaluator[0]


def _process_without_sync(metric, samples, instances, monkeypatch):
    """process() must neither wait for the device nor copy to the host."""
    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f'CocoMetric.process called {name}')
        return f
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, 'synchronize', refuse('torch.cuda.synchronize'))
        for name in ('cpu', 'item', 'tolist', 'numpy'):
            mp.setattr(torch.Tensor, name, refuse(f'Tensor.{name}'))
        for s, ins in zip(samples, instances):
            metric.process(s, ins)


def _host_rows(samples, index):
    db = np.concatenate([s.pred_det_instances.bboxes.cpu().numpy().reshape(-1, 4) for s in samples]).astype(np.float32)
    sc = np.concatenate([s.pred_det_instances.scores.cpu().numpy().reshape(-1) for s in samples]).astype(np.float32)
    lb = np.concatenate([s.pred_det_instances.labels.cpu().numpy().reshape(-1) for s in samples])
    di = np.concatenate([np.full(len(s.pred_det_instances.scores), index[s.metainfo['img_id']]) for s in samples])
    return db, sc, lb, di


def _check_metric(metric, want):
    for k in ('precision', 'recall', 'scores', 'stats'):
        assert np.array_equal(getattr(metric, k), want[k]), k


def test_product_instances_mode(airdrone, cuda, monkeypatch):
    from stereotracking_amd.registry import METRICS
    outs, entry = _detect(airdrone, cuda)
    infos = airdrone[2]
    metric = METRICS.build(dict(entry, ann_file=None))
    _process_without_sync(metric, outs, [i['instances'] for i in infos], monkeypatch)
    got = metric.evaluate()
    ids = sorted(i['img_id'] for i in infos)
    index = {v: n for n, v in enumerate(ids)}
    db, sc, lb, di = _host_rows(outs, index)
    assert len(sc) > 0, 'the scenario produced no detections'
    gb, gc, gi = [], [], []
    for info in infos:
        for ins in info['instances']:
            x1, y1, x2, y2 = ins['bbox']
            gb.append([x1, y1, x2 - x1, y2 - y1])
            gc.append(ins['ignore_flag'])
            gi.append(index[info['img_id']])
    gb = np.array(gb, dtype=np.float64).reshape(-1, 4)
    assert len(gb) > 0
    want = ref.evaluate(db, sc, lb, di, gb, gb[:, 2] * gb[:, 3], gc, np.zeros(len(gb), dtype=int), gi, len(ids), 1)
    _check_metric(metric, want)
    print(got, want['stats'].tolist())
    assert got == ref.mmdet_results(want['stats'], want['precision'])
    # The seeded weights detect nothing real, so the figures above are zeros.  Second pass over the same device
    # detections with ground truth made from them (every third box of a frame, corners rounded to half pixels, every
    # fifth of those crowd): hits, misses and ignored rows all occur.
    made = []
    for s in outs:
        b = s.pred_det_instances.bboxes.cpu().numpy().reshape(-1, 4)[::3]
        made.append([dict(bbox=(np.round(bb.astype(np.float64) * 2) / 2).tolist(), ignore_flag=int(j % 5 == 4), bbox_label=0)
                     for j, bb in enumerate(b) if np.round(bb[2] * 2) > np.round(bb[0] * 2) and np.round(bb[3] * 2) > np.round(bb[1] * 2)])
    metric = METRICS.build(dict(entry, ann_file=None))
    _process_without_sync(metric, outs, made, monkeypatch)
    got = metric.evaluate()
    gb, gc, gi = [], [], []
    for s, inst in zip(outs, made):
        for ins in inst:
            x1, y1, x2, y2 = ins['bbox']
            gb.append([x1, y1, x2 - x1, y2 - y1])
            gc.append(ins['ignore_flag'])
            gi.append(index[s.metainfo['img_id']])
    gb = np.array(gb, dtype=np.float64).reshape(-1, 4)
    want = ref.evaluate(db, sc, lb, di, gb, gb[:, 2] * gb[:, 3], gc, np.zeros(len(gb), dtype=int), gi, len(ids), 1)
    _check_metric(metric, want)
    print(got, want['stats'].tolist())
    assert got == ref.mmdet_results(want['stats'], want['precision'])
    assert want['stats'][0] > 0 and want['matched'].any() and not want['matched'].all()


def test_product_ann_file_mode_counts_unprocessed_frames_as_misses(airdrone, cuda, monkeypatch):
    from stereotracking_amd.registry import METRICS
    outs, entry = _detect(airdrone, cuda)
    infos, ann = airdrone[2], airdrone[3]
    metric = METRICS.build(dict(entry, ann_file=ann))
    seen = outs[:T - 2]                                           # the last two frames are never processed
    _process_without_sync(metric, seen, [None] * len(seen), monkeypatch)
    got = metric.evaluate()
    coco = json.load(open(ann))
    ids = sorted(im['id'] for im in coco['images'])
    assert len(ids) == T
    index = {v: n for n, v in enumerate(ids)}
    db, sc, lb, di = _host_rows(seen, index)
    anns = [a for a in coco['annotations'] if a['category_id'] == 1]
    gb = np.array([a['bbox'] for a in anns], dtype=np.float64).reshape(-1, 4)
    want = ref.evaluate(db, sc, lb, di, gb, [a['area'] for a in anns], [a.get('iscrowd', 0) for a in anns],
                        np.zeros(len(anns), dtype=int), [index[a['image_id']] for a in anns], len(ids), 1)
    _check_metric(metric, want)
    assert got == ref.mmdet_results(want['stats'], want['precision'])
    in_last = sum(1 for a in anns if index[a['image_id']] >= T - 2)
    assert in_last > 0 and int(metric.npig[0, 0]) == sum(1 for a in anns if not a.get('iscrowd', 0))
