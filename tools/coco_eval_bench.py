#!/usr/bin/env python
"""Time the device COCO bbox evaluation (csrc/coco_eval.hip) on one synthetic split, per stage, and the numpy
restatement tests/coco_eval_ref.py on a stated fraction of the same split (it is Python loops: the whole split would
take many minutes).  Record-only: writes profiles/coco_eval_bench.json, asserts no speed.

    python tools/coco_eval_bench.py [--images 65536 --max-det 100 --runs 7 --ref-images 1024 --out profiles/coco_eval_bench.json]

Device times are HIP events around the three stage calls, warm, median of --runs; 'evaluate_ms' is the host clock
around the whole call including the uploads of the ground truth and the copy of the results back."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def synthetic_split(images, max_det, seed=0):
    """One category; 1-4 ground-truth boxes and 0..max_det detections per image; four fifths of the detections are
    jittered copies of a box of their image; scores with three decimals."""
    rng = np.random.RandomState(seed)
    ng = rng.randint(1, 5, images)
    nd = rng.randint(0, max_det + 1, images)
    gi = np.repeat(np.arange(images, dtype=np.int32), ng)
    G = len(gi)
    gwh = np.exp(rng.uniform(np.log(4), np.log(250), (G, 2)))
    gxy = rng.uniform(0, 1000, (G, 2))
    gb = np.concatenate([gxy, gwh], axis=1)
    di = np.repeat(np.arange(images, dtype=np.int32), nd)
    D = len(di)
    first = np.concatenate([[0], np.cumsum(ng)[:-1]])
    pick = first[di] + (rng.randint(0, 4, D) % ng[di])
    src = gb[pick]
    xy = src[:, :2] + rng.uniform(-.25, .25, (D, 2)) * src[:, 2:]
    wh = src[:, 2:] * rng.uniform(.8, 1.25, (D, 2))
    rand = rng.rand(D) >= 0.8
    xy[rand] = rng.uniform(0, 1000, (int(rand.sum()), 2))
    wh[rand] = np.exp(rng.uniform(np.log(4), np.log(250), (int(rand.sum()), 2)))
    db = np.concatenate([xy, xy + wh], axis=1).astype(np.float32)
    return dict(det_boxes=db, det_scores=np.round(rng.rand(D), 3).astype(np.float32),
                det_labels=np.zeros(D, dtype=np.int32), det_img=di, gt_boxes=gb, gt_area=gb[:, 2] * gb[:, 3],
                gt_crowd=(rng.rand(G) < 0.1).astype(np.int32), gt_cat=np.zeros(G, dtype=np.int32), gt_img=gi,
                num_images=images, num_cats=1)


def head(s, images):
    d, g = s['det_img'] < images, s['gt_img'] < images
    out = {k: (v[d] if k.startswith('det_') else v[g] if k.startswith('gt_') else v) for k, v in s.items()}
    out['num_images'] = images
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=65536)
    ap.add_argument('--max-det', type=int, default=100)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--ref-images', type=int, default=1024)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'coco_eval_bench.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('coco_eval_bench needs a GPU: a CPU run says nothing about device time')
    import coco_eval_ref as ref
    from stereotracking_amd.coco_metric import coco_eval_device
    dev = torch.device('cuda:0')
    s = synthetic_split(args.images, args.max_det)
    det = [torch.from_numpy(s[k]).to(dev) for k in ('det_boxes', 'det_scores', 'det_labels', 'det_img')]
    gt = [s[k] for k in ('gt_boxes', 'gt_area', 'gt_crowd', 'gt_cat', 'gt_img')]

    def once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = coco_eval_device(*det, *gt, s['num_images'], 1, timing=True)
        host = {k: out[k].cpu().numpy() for k in ('precision', 'recall', 'scores', 'status')}
        wall = (time.perf_counter() - t0) * 1e3
        assert host['status'][0] == 0, host['status']
        ev = out['events']
        return dict(prepare_ms=ev[0].elapsed_time(ev[1]), match_ms=ev[1].elapsed_time(ev[2]),
                    accumulate_ms=ev[2].elapsed_time(ev[3]), evaluate_ms=wall), host
    for _ in range(args.warmup):
        once()
    runs = [once()[0] for _ in range(args.runs)]
    med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    spread = {k: [float(min(r[k] for r in runs)), float(max(r[k] for r in runs))] for k in runs[0]}

    sub = head(s, min(args.ref_images, args.images))
    t0 = time.perf_counter()
    want = ref.evaluate(*[sub[k] for k in ('det_boxes', 'det_scores', 'det_labels', 'det_img', 'gt_boxes', 'gt_area',
                                           'gt_crowd', 'gt_cat', 'gt_img')], sub['num_images'], 1)
    ref_ms = (time.perf_counter() - t0) * 1e3
    sub_det = [torch.from_numpy(sub[k]).to(dev) for k in ('det_boxes', 'det_scores', 'det_labels', 'det_img')]
    out = coco_eval_device(*sub_det, *[sub[k] for k in ('gt_boxes', 'gt_area', 'gt_crowd', 'gt_cat', 'gt_img')],
                           sub['num_images'], 1)
    same = all(np.array_equal(out[k].cpu().numpy(), want[k]) for k in ('precision', 'recall', 'scores'))
    rec = dict(tool='tools/coco_eval_bench.py', device=torch.cuda.get_device_name(0),
               split=dict(images=args.images, categories=1, detections=int(len(s['det_scores'])),
                          ground_truth=int(len(s['gt_area'])), max_det_per_image=args.max_det, gt_per_image='1-4',
                          iou_thrs=10, area_ranges=4, max_dets=[100, 300, 1000]),
               device_ms_median=med, device_ms_min_max=spread, runs=args.runs, warmup=args.warmup,
               restatement=dict(images=sub['num_images'], detections=int(len(sub['det_scores'])), ms=ref_ms,
                                fraction_of_split=sub['num_images'] / args.images,
                                extrapolated_whole_split_ms=ref_ms * args.images / sub['num_images'],
                                device_equals_restatement_on_fraction=bool(same)),
               note='record-only; restatement = tests/coco_eval_ref.py (Python loops), timed on the stated fraction')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
