"""COCO bbox evaluation, restated in plain numpy: the yardstick of tests/test_coco_metric_gpu.py.

pycocotools and mmdet are not installed and not part of the reference tree (which only holds the thin CocoVideoMetric
subclass), so the rules below are COCOeval.evaluateImg / accumulate / summarize and mmdet 3.0.0rc4's CocoMetric written
down from memory [upstream-memory], the way tests/sgbm_ref.py restates OpenCV.  Parity with pycocotools itself is
unpinned.  Python loops on purpose: this file is meant to be read next to the rules, not to be fast.

Inputs are the flat rows the device takes (stereotracking_amd/coco_metric.py):
  det_boxes (D, 4) float32 xyxy, det_scores (D,) float32, det_labels (D,) int in [0, K), det_img (D,) int image index
  gt_boxes (G, 4) float64 xywh, gt_area (G,) float64, gt_crowd (G,), gt_cat (G,) in [0, K), gt_img (G,) image index
Image index = position of the image id in the ascending list of evaluated image ids; rows of one image keep their
arrival order.

Rules (U = uncertain, restated from memory and marked so in DESIGN.md):
  R1 (U) xyxy -> xywh: the four float32 values are widened to float64 first, then w = x2 - x1, h = y2 - y1
         (mmdet's xyxy2xywh works on bbox.tolist()); detection area = w * h (COCO.loadRes).
  R2     per (image, category): detections ordered by score descending with a STABLE sort
         (np.argsort(-score, kind='mergesort')), cut to max_dets[-1].
  R3 (U) max_dets = list(proposal_nums) = [100, 300, 1000] in mmdet, so AP is read at 1000 detections per image.
  R4 (U) a ground-truth box is ignored for an area range if it is crowd or its area lies outside [lo, hi]; an
         annotation's own `ignore` key is overwritten with `iscrowd` by COCOeval._prepare and does not count.
  R5     ground truth ordered non-ignored first (stable); IoU on xywh in float64:
         iw = min(dx + dw, gx + gw) - max(dx, gx), ih likewise, 0 if iw <= 0 or ih <= 0, else
         inter / (dw * dh + gw * gh - inter), or inter / (dw * dh) against a crowd box.
  R6     greedy match per IoU threshold t, detections in score order: best = min(t, 1 - 1e-10), m = none; walk the
         ground truth in order: skip a box already matched at t unless it is crowd; stop when m is set and not ignored
         and the box is ignored; skip if iou < best; else best = iou, m = box (equal IoU moves on to the later box).
         A matched detection inherits m's ignore flag.  An unmatched detection whose area lies outside [lo, hi] is
         ignored.
  R7     per (category, area range, max_dets entry m): the first m detections of every image's group, all images
         concatenated in image order, sorted by score descending, stable; tp = matched & ~ignored, fp = ~matched &
         ~ignored, running sums; rc = tp / npig, pr = tp / (fp + tp + np.spacing(1)); pr made non-increasing from the
         right; at each recall point the first index with rc >= r gives precision and score (0 past the end);
         recall = rc[-1] (0 without detections).  npig == 0 leaves -1.
  R8     the 12 summary numbers: mean of the entries > -1 of a slice (-1 if none); AP slices at max_dets[-1]; an IoU
         threshold is selected by equality with .5 / .75.
  R9 (U) mmdet rounds with float(f'{round(v, 3)}') and names the keys bbox_mAP, bbox_mAP_50, ... ; classwise adds
         '<class>_precision' = round(mean of precision[:, :, k, 0, -1] > -1, 3).
"""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNGS = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
METRIC_ITEMS = {'mAP': 0, 'mAP_50': 1, 'mAP_75': 2, 'mAP_s': 3, 'mAP_m': 4, 'mAP_l': 5, 'AR@100': 6, 'AR@300': 7,
                'AR@1000': 8, 'AR_s@1000': 9, 'AR_m@1000': 10, 'AR_l@1000': 11}


def xyxy_to_xywh(boxes_f32):
    b = np.asarray(boxes_f32, dtype=np.float32).reshape(-1, 4).astype(np.float64)      # R1: widen, then subtract
    return np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], axis=1)


def iou_xywh(d, g, crowd):
    iw = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    if iw <= 0:
        return 0.0
    ih = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if ih <= 0:
        return 0.0
    inter = iw * ih
    da = d[2] * d[3]
    union = da if crowd else da + g[2] * g[3] - inter
    return inter / union


def match_group(dbox, dscore, gbox, garea, gcrowd, iou_thrs, area_rngs, max_det):
    """One (image, category) group.  dbox (n, 4) xywh float64 in arrival order.  Returns (order, matched, ignored,
    gt_ignored): order = arrival indices of the kept detections in score order; matched / ignored (len(order), T, A)
    bool; gt_ignored (G, A) bool."""
    T, A = len(iou_thrs), len(area_rngs)
    order = np.argsort(-np.asarray(dscore, dtype=np.float32), kind='mergesort')[:max_det]          # R2
    G = len(gbox)
    gt_ignored = np.zeros((G, A), dtype=bool)
    for a, (lo, hi) in enumerate(area_rngs):
        for g in range(G):
            gt_ignored[g, a] = bool(gcrowd[g]) or garea[g] < lo or garea[g] > hi                   # R4
    iou = np.zeros((len(order), G))
    for i, d in enumerate(order):
        for g in range(G):
            iou[i, g] = iou_xywh(dbox[d], gbox[g], bool(gcrowd[g]))                                # R5
    matched = np.zeros((len(order), T, A), dtype=bool)
    ignored = np.zeros((len(order), T, A), dtype=bool)
    for a, (lo, hi) in enumerate(area_rngs):
        gorder = [g for g in range(G) if not gt_ignored[g, a]] + [g for g in range(G) if gt_ignored[g, a]]
        for t, thr in enumerate(iou_thrs):
            taken = np.zeros(G, dtype=bool)
            for i, d in enumerate(order):                                                          # R6
                best = min(thr, 1 - 1e-10)
                m = -1
                for g in gorder:
                    if taken[g] and not gcrowd[g]:
                        continue
                    if m > -1 and not gt_ignored[m, a] and gt_ignored[g, a]:
                        break
                    if iou[i, g] < best:
                        continue
                    best = iou[i, g]
                    m = g
                if m > -1:
                    matched[i, t, a] = True
                    ignored[i, t, a] = gt_ignored[m, a]
                    taken[m] = True
                else:
                    area = dbox[d][2] * dbox[d][3]
                    ignored[i, t, a] = area < lo or area > hi
    return order, matched, ignored, gt_ignored


def evaluate(det_boxes, det_scores, det_labels, det_img, gt_boxes, gt_area, gt_crowd, gt_cat, gt_img, num_images,
             num_cats, iou_thrs=None, max_dets=(100, 300, 1000), area_rngs=None, rec_thrs=None):
    """-> dict(rank (D,), matched (D, T, A), ignored (D, T, A), npig (K, A), precision (T, R, K, A, M),
    recall (T, K, A, M), scores (T, R, K, A, M), stats (12,))."""
    iou_thrs = IOU_THRS if iou_thrs is None else np.asarray(iou_thrs, dtype=np.float64)
    rec_thrs = REC_THRS if rec_thrs is None else np.asarray(rec_thrs, dtype=np.float64)
    area_rngs = AREA_RNGS if area_rngs is None else np.asarray(area_rngs, dtype=np.float64)
    max_dets = list(max_dets)                                                                      # R3
    det_scores = np.asarray(det_scores, dtype=np.float32).reshape(-1)
    det_labels = np.asarray(det_labels).reshape(-1).astype(np.int64)
    det_img = np.asarray(det_img).reshape(-1).astype(np.int64)
    gt_boxes = np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 4)
    gt_area = np.asarray(gt_area, dtype=np.float64).reshape(-1)
    gt_crowd = np.asarray(gt_crowd).reshape(-1).astype(bool)
    gt_cat = np.asarray(gt_cat).reshape(-1).astype(np.int64)
    gt_img = np.asarray(gt_img).reshape(-1).astype(np.int64)
    dxywh = xyxy_to_xywh(det_boxes)
    D, T, A, M, R, K = len(det_scores), len(iou_thrs), len(area_rngs), len(max_dets), len(rec_thrs), num_cats
    rank = np.full(D, -1, dtype=np.int64)
    matched = np.zeros((D, T, A), dtype=bool)
    ignored = np.zeros((D, T, A), dtype=bool)
    det_rows = [[[] for _ in range(K)] for _ in range(num_images)]
    gt_rows = [[[] for _ in range(K)] for _ in range(num_images)]
    for i in range(D):
        det_rows[det_img[i]][det_labels[i]].append(i)
    for g in range(len(gt_area)):
        gt_rows[gt_img[g]][gt_cat[g]].append(g)
    npig = np.zeros((K, A), dtype=np.int64)
    groups = {}       # (k, img) -> (rows in score order, gt_ignored)
    for img in range(num_images):
        for k in range(K):
            dr, gr = np.array(det_rows[img][k], dtype=np.int64), np.array(gt_rows[img][k], dtype=np.int64)
            if len(dr) == 0 and len(gr) == 0:
                continue
            order, mt, ig, gt_ig = match_group(dxywh[dr], det_scores[dr], gt_boxes[gr], gt_area[gr], gt_crowd[gr],
                                               iou_thrs, area_rngs, max_dets[-1])
            rows = dr[order]
            rank[rows] = np.arange(len(rows))
            matched[rows] = mt
            ignored[rows] = ig
            npig[k] += (~gt_ig).sum(axis=0)
            groups[(k, img)] = rows
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k in range(K):                                                                             # R7
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                rows = [groups[(k, img)][:max_det] for img in range(num_images) if (k, img) in groups]
                if len(rows) == 0:
                    continue
                rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
                rows = rows[np.argsort(-det_scores[rows], kind='mergesort')]
                if npig[k, a] == 0:
                    continue
                tps = matched[rows, :, a] & ~ignored[rows, :, a]          # (nd, T)
                fps = ~matched[rows, :, a] & ~ignored[rows, :, a]
                tp_sum = np.cumsum(tps, axis=0).astype(np.float64)
                fp_sum = np.cumsum(fps, axis=0).astype(np.float64)
                nd = len(rows)
                for t in range(T):
                    tp, fp = tp_sum[:, t], fp_sum[:, t]
                    rc = tp / npig[k, a]
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q, ss = np.zeros(R), np.zeros(R)
                    for ri, pi in enumerate(np.searchsorted(rc, rec_thrs, side='left')):
                        if pi >= nd:
                            break
                        q[ri] = pr[pi]
                        ss[ri] = det_scores[rows[pi]]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    return dict(rank=rank, matched=matched, ignored=ignored, npig=npig, precision=precision, recall=recall,
                scores=scores, stats=summarize(precision, recall, iou_thrs, max_dets))


def _mean_valid(s):
    s = s[s > -1]
    return -1.0 if s.size == 0 else float(np.mean(s))


def summarize(precision, recall, iou_thrs, max_dets):
    """R8: pycocotools' 12 numbers (AP, AP50, AP75, APs, APm, APl at max_dets[2]; AR at max_dets[0..2]; ARs, ARm, ARl)."""
    if len(max_dets) != 3:
        raise ValueError('the 12-number summary is defined for three max_dets entries')

    def ap(thr=None, a=0):
        s = precision if thr is None else precision[np.where(thr == iou_thrs)[0]]
        return _mean_valid(s[:, :, :, a, 2])

    def ar(a=0, m=2):
        return _mean_valid(recall[:, :, a, m])

    return np.array([ap(), ap(.5), ap(.75), ap(a=1), ap(a=2), ap(a=3), ar(m=0), ar(m=1), ar(m=2), ar(a=1), ar(a=2),
                     ar(a=3)], dtype=np.float64)


def mmdet_results(stats, precision, class_names=None, metric_items=None, classwise=False, prefix='coco'):
    """R9: the dict mmdet's CocoMetric.compute_metrics returns for metric='bbox'."""
    names = dict(METRIC_ITEMS)
    out = {}
    for item in (metric_items or ['mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l']):
        out[f'{prefix}/bbox_{item}'] = float(f'{round(float(stats[names[item]]), 3)}')
    if classwise:
        for k, name in enumerate(class_names):
            p = precision[:, :, k, 0, -1]
            p = p[p > -1]
            out[f'{prefix}/{name}_precision'] = round(float(np.mean(p)) if p.size else float('nan'), 3)
    return out
