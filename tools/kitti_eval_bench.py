#!/usr/bin/env python
"""Time MOTKittiMetrics' device backend (st_mot_kitti_preprocess and the four scoring stages of csrc/mot_eval.hip) per
stage, and the host backend on the same rows.  Record-only: writes profiles/kitti_eval_bench.json, asserts no speed.

    python tools/kitti_eval_bench.py [--runs 7 --sequences 21 --frames 380 --objects 12 --out profiles/kitti_eval_bench.json]

The shape is KITTI Tracking's own: 21 sequences of about 380 frames with about 12 annotated objects per frame, classes
car and pedestrian evaluated (vans, sitting persons, cyclists and DontCare regions among the rows).  The rows are
synthetic: objects on a grid drifting with constant velocity, occlusion / truncation drawn per frame, predictions =
80 % of the ground truth jittered by up to 3 px plus spurious boxes, two DontCare boxes per frame.  Device times are HIP
events around the stage calls, warm, median of --runs with the spread; 'call' is the host clock around the whole device
path (row tables, upload, the preprocessing stage, masks applied in numpy, pack_sequences, the scoring stages, the copy
back, Identity's assignment and the divisions), with the host's shares listed.  The host backend (kitti_preprocess +
clear_identity + hota per video and class) is timed once."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAR, VAN, PED, PERSON, CYCLIST = 1, 2, 4, 5, 6
CLASSES = [(CAR, [VAN]), (PED, [PERSON])]


def kitti_like_sequence(seed, frames, nobj):
    """(gt_rows (n, 9), pred_rows (m, 8), ignore_boxes (k, 5)) in metrics.kitti_preprocess's layouts."""
    rng = np.random.RandomState(seed)
    k = np.arange(nobj)
    cls = rng.choice([CAR, CAR, CAR, VAN, PED, PED, PERSON, CYCLIST], nobj)
    pos = np.stack([40.0 + 150.0 * (k % 8), 60.0 + 160.0 * (k // 8)], 1) + rng.uniform(-5, 5, (nobj, 2))
    vel = rng.uniform(-0.3, 0.3, (nobj, 2))
    size = np.where(np.isin(cls, (CAR, VAN))[:, None], rng.uniform([50, 18], [90, 60], (nobj, 2)),
                    rng.uniform([14, 18], [30, 70], (nobj, 2)))
    gt, pred, ign = [], [], []
    for t in range(frames):
        present = rng.uniform(size=nobj) < 0.9
        n = int(present.sum())
        b = np.concatenate([pos + vel * t, pos + vel * t + size], 1)[present].astype(np.float32).astype(np.float64)
        gt.append(np.column_stack([np.full(n, t), 10 + k[present], cls[present], rng.choice([0, 0, 0, 0, 1], n),
                                   rng.choice([0, 0, 0, 1, 2, 3], n), b]))
        det = rng.uniform(size=n) < 0.8
        pc = np.where(np.isin(cls[present], (CAR, VAN)), CAR, np.where(np.isin(cls[present], (PED, PERSON)), PED, rng.choice([CAR, PED], n)))
        pb = (b + rng.uniform(-3, 3, (n, 4))).astype(np.float32).astype(np.float64)
        pid = 110 + k[present] + np.where((t >= frames // 2) & (k[present] % 3 == 0), 1000, 0)
        pred.append(np.column_stack([np.full(n, t), pid, pc, pb, rng.uniform(0.3, 1.0, n)])[det])
        ns = rng.randint(0, 4)
        xy, wh = rng.uniform([0, 400], [1100, 520], (ns, 2)), rng.uniform([20, 10], [60, 60], (ns, 2))
        pred.append(np.column_stack([np.full(ns, t), 9000 + 10 * (t % 5) + np.arange(ns), rng.choice([CAR, PED], ns), xy, xy + wh,
                                     rng.uniform(0.3, 1.0, ns)]))
        dxy = rng.uniform([0, 380], [1000, 440], (2, 2))
        ign.append(np.column_stack([np.full(2, t), dxy, dxy + rng.uniform([120, 80], [200, 120], (2, 2))]))
    return np.concatenate(gt), np.concatenate(pred), np.concatenate(ign)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def xywh(rows, b):
    return np.column_stack([rows[:, 0], rows[:, 1], rows[:, b], rows[:, b + 1], rows[:, b + 2] - rows[:, b], rows[:, b + 3] - rows[:, b + 1]])


def device_call(sequences, mot_eval):
    """The device path of MOTKittiMetrics._evaluate_local on prepared rows, with the clock of its parts."""
    t0 = time.perf_counter()
    masks, tk = mot_eval.kitti_keep_masks(sequences, CLASSES, timing=True)
    t1 = time.perf_counter()
    gts = {(s, c): xywh(sequences[s][0][gk[c]], 5) for s, (gk, pk) in enumerate(masks) for c in range(len(CLASSES))}
    preds = {(s, c): xywh(sequences[s][1][pk[c]], 3) for s, (gk, pk) in enumerate(masks) for c in range(len(CLASSES))}
    t2 = time.perf_counter()
    packed = mot_eval.pack_sequences(gts, preds)
    t3 = time.perf_counter()
    res, te = mot_eval.evaluate_packed(packed, 0.5, timing=True)
    t4 = time.perf_counter()
    stages = dict(tk['stages_ms'], **te['stages_ms'])
    host = tk['host_prepare_s'] + tk['host_finish_s'] + (t2 - t1) + (t3 - t2) + te['host_prepare_s'] + te['host_finish_s']
    parts = dict(kitti_keep_masks_s=t1 - t0, kitti_keep_masks_host_prepare_s=tk['host_prepare_s'], apply_masks_s=t2 - t1,
                 pack_sequences_s=t3 - t2, evaluate_packed_s=t4 - t3, evaluate_packed_host_finish_s=te['host_finish_s'],
                 call_s=t4 - t0, host_share_of_call=host / (t4 - t0))
    return dict(zip(packed['videos'], res)), masks, stages, parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--sequences', type=int, default=21)
    ap.add_argument('--frames', type=int, default=380)
    ap.add_argument('--objects', type=int, default=12)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kitti_eval_bench.json'))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'kitti_eval_bench needs a GPU'
    from stereotracking_amd import metrics as M
    from stereotracking_amd import mot_eval
    sequences = [kitti_like_sequence(300 + s, a.frames, a.objects) for s in range(a.sequences)]
    device_call(sequences, mot_eval)          # warm: library load, allocator, the kernels' first launch
    stages, parts = {}, {}
    for _ in range(a.runs):
        torch.cuda.synchronize()
        res, masks, st, pt = device_call(sequences, mot_eval)
        for k, v in st.items():
            stages.setdefault(k, []).append(v)
        for k, v in pt.items():
            parts.setdefault(k, []).append(v)
    t0 = time.perf_counter()
    host_masks = [[M.kitti_preprocess(s[0], s[1], s[2], cid, dis) for cid, dis in CLASSES] for s in sequences]
    t1 = time.perf_counter()
    ref = {}
    for s, seq in enumerate(sequences):
        for c in range(len(CLASSES)):
            g, p = xywh(seq[0][host_masks[s][c][0]], 5), xywh(seq[1][host_masks[s][c][1]], 3)
            ref[(s, c)] = (M.clear_identity(g, p, 0.5), M.hota(g, p))
    t2 = time.perf_counter()
    masks_equal = all(np.array_equal(masks[s][0][c], host_masks[s][c][0]) and np.array_equal(masks[s][1][c], host_masks[s][c][1])
                      for s in range(len(sequences)) for c in range(len(CLASSES)))
    counts_equal = all(res[k]['clear_identity']['TP'] == c['TP'] and res[k]['clear_identity']['IDSW'] == c['IDSW'] and
                       np.array_equal(res[k]['hota']['HOTA_TP'], h['HOTA_TP']) for k, (c, h) in ref.items())
    removed = int(sum((seq[1][:, 2] == cid).sum() - host_masks[s][c][1].sum() for s, seq in enumerate(sequences)
                      for c, (cid, _) in enumerate(CLASSES)))
    out = dict(tool='tools/kitti_eval_bench.py', device=torch.cuda.get_device_name(0), runs=a.runs,
               shape=f'{a.sequences} sequences x {a.frames} frames x {a.objects} objects, classes car and pedestrian',
               gt_rows=int(sum(len(s[0]) for s in sequences)), pred_rows=int(sum(len(s[1]) for s in sequences)),
               ignore_rows=int(sum(len(s[2]) for s in sequences)), predictions_removed_by_the_rules=removed,
               device_stage_ms={k: spread(v) for k, v in stages.items()},
               device_stages_total_ms=spread(np.sum([stages[k] for k in stages], axis=0)),
               device_call={k: spread(v) for k, v in parts.items()},
               host_backend_s=dict(kitti_preprocess=t1 - t0, clear_identity_and_hota=t2 - t1, total=t2 - t0, runs=1),
               host_backend='kitti_preprocess + clear_identity + hota (numpy, scipy), one Python iteration per frame',
               host_over_device_call=(t2 - t0) / float(np.median(parts['call_s'])),
               masks_equal_host=bool(masks_equal), counts_equal_host=bool(counts_equal))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
