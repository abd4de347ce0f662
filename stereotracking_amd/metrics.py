"""MOTChallenge writer + CLEAR-MOT / Identity metrics for the AirDrone evaluation.

Behavioural spec: reference mmtrack/evaluation/metrics/mot_drone_metrics.py
  process()                 :155-221  per-frame rows, depth-range filters
                                      (pred kept iff depth_thr >= depth > 0, gt iff location[-1] <= depth_thr)
  _save_one_video_gts_preds :223-253  MOTChallenge txt formats
  compute_metrics           :255-333  the metric list (default ['HOTA', 'CLEAR', 'Identity'], :83-88) and the keys reported:
                                      HOTA / AssA / DetA; MOTA MOTP IDSW TP FP FN Frag MT ML; IDF1 IDTP IDFN IDFP IDP IDR
The reference delegates the scores to TrackEval (un-vendored, absent here): CLEAR (MOTA, MOTP, IDSW, Frag, MT, ML),
Identity (IDF1, IDP, IDR) and HOTA (HOTA, DetA, AssA over the localisation thresholds 0.05 .. 0.95) are restated from
their published definitions (Bernardin & Stiefelhagen 2008; Ristani et al. 2016; Luiten et al., IJCV 2021) the way
TrackEval computes them [upstream-memory]: CLEAR - per-frame Hungarian matching on IoU >= 0.5 with priority for the
previous frame's match; Identity - one global bipartite matching; HOTA - per-frame Hungarian matching that maximises
(global alignment score x IoU), thresholded per alpha, association accuracy per matched pair from the id-pair counts.
Parity is UNPINNED against TrackEval itself (absent); the known-answer tests are hand-derived from the definitions.

What is scored, MOTDroneMetrics(protocol=...): 'rows' (the default) scores the in-memory float rows as they were
collected; 'trackeval' scores what the reference scores - the values a reader of the written MOTChallenge files gets
(motchallenge_file_rows: ground truth '%d', predictions '%.3f', :223-253) after the preprocessing TrackEval's
MotChallenge2DBox applies with CLASSES_TO_EVAL=['pedestrian'] and DO_PREPROC=True except for MOT15 (:273-289, :364-417;
motchallenge_preprocess, restated [upstream-memory], parity UNPINNED).

KITTI Tracking (stereotracking_amd/kitti_metrics.py, MOTKittiMetrics): kitti_box_ious and kitti_preprocess restate the
preprocessing TrackEval applies to KITTI's 2-D boxes before these scorers see a sequence [upstream-memory].
"""
import os
from collections import defaultdict

import numpy as np
from scipy.optimize import linear_sum_assignment


def box_iou_xywh(a, b):
    """IoU of (n,4) and (m,4) boxes in MOTChallenge x,y,w,h form."""
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)))
    ax2, ay2 = a[:, 0] + a[:, 2], a[:, 1] + a[:, 3]
    bx2, by2 = b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]
    iw = np.clip(np.minimum(ax2[:, None], bx2[None]) - np.maximum(a[:, None, 0], b[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(ay2[:, None], by2[None]) - np.maximum(a[:, None, 1], b[None, :, 1]), 0, None)
    inter = iw * ih
    union = (a[:, 2] * a[:, 3])[:, None] + (b[:, 2] * b[:, 3])[None] - inter
    return np.where(union > 0, inter / np.maximum(union, 1e-12), 0.0)


BACKENDS = ('host', 'device')


def _check_backend(backend):
    if backend not in BACKENDS:
        raise ValueError(f'backend must be one of {BACKENDS}, got {backend!r}')


def _device_single(gt_rows, pred_rows, iou_thr, metrics):
    """One sequence through the device backend (stereotracking_amd/mot_eval.py)."""
    from . import mot_eval
    return mot_eval.evaluate_packed(mot_eval.pack_sequences([gt_rows], [pred_rows]), iou_thr, metrics)[0]


def clear_identity(gt_rows, pred_rows, iou_thr=0.5, backend='host'):
    """gt_rows / pred_rows: arrays of (frame, id, x, y, w, h, ...).  Returns a dict with the CLEAR counts
    (TP, FN, FP, IDSW, MOTA, MOTP) and Identity scores (IDTP, IDFN, IDFP, IDF1, IDP, IDR).
    backend='device': the same dict from the HIP path (mot_eval.py); raises without the library or a device."""
    _check_backend(backend)
    if backend == 'device':
        return _device_single(gt_rows, pred_rows, iou_thr, ('CLEAR', 'Identity'))['clear_identity']
    gt_rows = np.asarray(gt_rows, dtype=np.float64)
    pred_rows = np.asarray(pred_rows, dtype=np.float64)
    if gt_rows.size == 0:
        gt_rows = np.zeros((0, 6))
    if pred_rows.size == 0:
        pred_rows = np.zeros((0, 6))
    gt_ids = {v: i for i, v in enumerate(sorted(set(gt_rows[:, 1].astype(int).tolist())))}
    tr_ids = {v: i for i, v in enumerate(sorted(set(pred_rows[:, 1].astype(int).tolist())))}
    frames = sorted(set(gt_rows[:, 0].astype(int).tolist()) | set(pred_rows[:, 0].astype(int).tolist()))
    ng, nt = len(gt_ids), len(tr_ids)
    tp = fn = fp = idsw = 0
    motp_sum = 0.0
    prev_tracker = np.full(ng, np.nan)       # last tracker id matched to each gt (ever)
    prev_step_tracker = np.full(ng, np.nan)  # tracker id matched in the previous frame
    potential = np.zeros((ng, nt))
    gt_count, tr_count = np.zeros(ng), np.zeros(nt)
    gt_frames, gt_matched, gt_frag = np.zeros(ng), np.zeros(ng), np.zeros(ng)   # MT / PT / ML and Frag bookkeeping
    eps = np.finfo(float).eps
    for f in frames:
        g = gt_rows[gt_rows[:, 0].astype(int) == f]
        p = pred_rows[pred_rows[:, 0].astype(int) == f]
        gi = np.array([gt_ids[int(v)] for v in g[:, 1]], dtype=int)
        ti = np.array([tr_ids[int(v)] for v in p[:, 1]], dtype=int)
        gt_count[gi] += 1
        tr_count[ti] += 1
        if len(g) == 0:
            fp += len(p)
            continue
        if len(p) == 0:        # (no reset of the previous-frame match here: the frame is skipped, as TrackEval does)
            fn += len(g)
            gt_frames[gi] += 1
            continue
        sim = box_iou_xywh(g[:, 2:6], p[:, 2:6])
        rr, cc = np.nonzero(sim >= iou_thr - eps)
        potential[gi[rr], ti[cc]] += 1
        score = (ti[None, :] == prev_step_tracker[gi][:, None]) * 1000.0 + sim
        score[sim < iou_thr - eps] = 0
        rows, cols = linear_sum_assignment(-score)
        ok = score[rows, cols] > eps
        rows, cols = rows[ok], cols[ok]
        mg, mt = gi[rows], ti[cols]
        prev = prev_tracker[mg]
        idsw += int(np.sum(~np.isnan(prev) & (prev != mt)))
        prev_tracker[mg] = mt
        not_tracked_before = np.isnan(prev_step_tracker)
        prev_step_tracker[:] = np.nan
        prev_step_tracker[mg] = mt
        tracked_now = ~np.isnan(prev_step_tracker)
        gt_matched += tracked_now
        gt_frag += not_tracked_before & tracked_now         # a new tracked segment of this gt starts
        gt_frames[gi] += 1
        tp += len(rows)
        fn += len(g) - len(rows)
        fp += len(p) - len(rows)
        motp_sum += float(sim[rows, cols].sum())
    return _clear_identity_result(tp, fn, fp, idsw, motp_sum, potential, gt_count, tr_count, gt_frames, gt_matched, gt_frag)


def _clear_identity_result(tp, fn, fp, idsw, motp_sum, potential, gt_count, tr_count, gt_frames, gt_matched, gt_frag):
    """The result dict from a sequence's accumulated counts (either backend's): Identity's global assignment, the
    MT / PT / ML / Frag bookkeeping and the ratios."""
    ng, nt = len(gt_count), len(tr_count)
    # identity: one global assignment minimising IDFN + IDFP
    fn_mat = np.zeros((ng + nt, ng + nt))
    fp_mat = np.zeros((ng + nt, ng + nt))
    fp_mat[ng:, :nt] = 1e10
    fn_mat[:ng, nt:] = 1e10
    for i in range(ng):
        fn_mat[i, :nt] = gt_count[i]
        fn_mat[i, nt + i] = gt_count[i]
    for j in range(nt):
        fp_mat[:ng, j] = tr_count[j]
        fp_mat[j + ng, j] = tr_count[j]
    fn_mat[:ng, :nt] -= potential
    fp_mat[:ng, :nt] -= potential
    r, c = linear_sum_assignment(fn_mat + fp_mat)
    idfn, idfp = float(fn_mat[r, c].sum()), float(fp_mat[r, c].sum())
    idtp = float(gt_count.sum() - idfn)
    seen = gt_frames > 0
    ratio = gt_matched[seen] / gt_frames[seen]
    mt_n = int(np.sum(ratio > 0.8))
    pt_n = int(np.sum(ratio >= 0.2)) - mt_n
    return dict(TP=tp, FN=fn, FP=fp, IDSW=idsw, Frag=int(np.sum(gt_frag[gt_frag > 0] - 1)), MT=mt_n, PT=pt_n,
                ML=ng - mt_n - pt_n,
                MOTA=(tp - fp - idsw) / max(1.0, tp + fn), MOTP=motp_sum / max(1.0, tp),
                IDTP=idtp, IDFN=idfn, IDFP=idfp,
                IDF1=idtp / max(1.0, idtp + 0.5 * idfp + 0.5 * idfn),
                IDP=idtp / max(1.0, idtp + idfp), IDR=idtp / max(1.0, idtp + idfn))


HOTA_ALPHAS = np.arange(0.05, 0.99, 0.05)     # 19 localisation thresholds 0.05 .. 0.95


def hota(gt_rows, pred_rows, backend='host'):
    """HOTA of ONE sequence (Luiten et al., "HOTA: A Higher Order Metric for Evaluating Multi-Object Tracking", IJCV 2021;
    reference mot_drone_metrics.py:291-295 reports the averages over alpha of HOTA / AssA / DetA).  gt_rows / pred_rows:
    arrays of (frame, id, x, y, w, h, ...); similarity = box IoU.  Returns per-alpha arrays HOTA_TP / HOTA_FN / HOTA_FP,
    AssA, AssRe, AssPr, LocA, DetA, DetRe, DetPr, HOTA (each of length 19).

    Per alpha: a TP is a (gt, prediction) pair of one frame matched by the Hungarian assignment that maximises
    global_alignment(gt id, pred id) x IoU, kept if IoU >= alpha; DetA = TP / (TP + FN + FP);
    A(c) = TPA / (TPA + FNA + FPA) for a TP c with ids (g, p): TPA = TPs carrying the same id pair, FNA / FPA = the
    other detections of g / p; AssA = mean of A over the TPs; HOTA = sqrt(DetA x AssA).
    backend='device': the same dict from the HIP path (mot_eval.py); raises without the library or a device."""
    _check_backend(backend)
    if backend == 'device':
        return _device_single(gt_rows, pred_rows, 0.5, ('HOTA',))['hota']
    gt_rows = np.asarray(gt_rows, dtype=np.float64).reshape(-1, np.shape(gt_rows)[-1] if np.size(gt_rows) else 6)
    pred_rows = np.asarray(pred_rows, dtype=np.float64).reshape(-1, np.shape(pred_rows)[-1] if np.size(pred_rows) else 6)
    A = len(HOTA_ALPHAS)
    res = {k: np.zeros(A) for k in ('HOTA_TP', 'HOTA_FN', 'HOTA_FP', 'AssA', 'AssRe', 'AssPr', 'LocA')}
    eps = np.finfo(float).eps
    if len(pred_rows) == 0 or len(gt_rows) == 0:
        res['HOTA_FN'] += len(gt_rows)
        res['HOTA_FP'] += len(pred_rows)
        res['LocA'] += 1.0
        return _hota_final(res)
    gt_ids = {v: i for i, v in enumerate(sorted(set(gt_rows[:, 1].astype(int).tolist())))}
    tr_ids = {v: i for i, v in enumerate(sorted(set(pred_rows[:, 1].astype(int).tolist())))}
    ng, nt = len(gt_ids), len(tr_ids)
    frames = sorted(set(gt_rows[:, 0].astype(int).tolist()) | set(pred_rows[:, 0].astype(int).tolist()))
    per_frame = []
    potential = np.zeros((ng, nt))
    gt_count, tr_count = np.zeros((ng, 1)), np.zeros((1, nt))
    for f in frames:          # pass 1: how well could each id pair be aligned over the whole sequence
        g = gt_rows[gt_rows[:, 0].astype(int) == f]
        p = pred_rows[pred_rows[:, 0].astype(int) == f]
        gi = np.array([gt_ids[int(v)] for v in g[:, 1]], dtype=int)
        ti = np.array([tr_ids[int(v)] for v in p[:, 1]], dtype=int)
        sim = box_iou_xywh(g[:, 2:6], p[:, 2:6])
        per_frame.append((gi, ti, sim))
        if len(gi) and len(ti):
            den = sim.sum(0)[None, :] + sim.sum(1)[:, None] - sim
            siou = np.zeros_like(sim)
            m = den > eps
            siou[m] = sim[m] / den[m]
            potential[gi[:, None], ti[None, :]] += siou
        gt_count[gi] += 1
        tr_count[0, ti] += 1
    align = potential / (gt_count + tr_count - potential)
    matches = [np.zeros((ng, nt)) for _ in range(A)]
    for gi, ti, sim in per_frame:      # pass 2: one assignment per frame, thresholded per alpha
        if len(gi) == 0:
            res['HOTA_FP'] += len(ti)
            continue
        if len(ti) == 0:
            res['HOTA_FN'] += len(gi)
            continue
        rows, cols = linear_sum_assignment(-(align[gi[:, None], ti[None, :]] * sim))
        for a, alpha in enumerate(HOTA_ALPHAS):
            ok = sim[rows, cols] >= alpha - eps
            r, c = rows[ok], cols[ok]
            res['HOTA_TP'][a] += len(r)
            res['HOTA_FN'][a] += len(gi) - len(r)
            res['HOTA_FP'][a] += len(ti) - len(r)
            if len(r):
                res['LocA'][a] += sim[r, c].sum()
                matches[a][gi[r], ti[c]] += 1
    for a in range(A):
        mc = matches[a]
        tp = max(1.0, res['HOTA_TP'][a])
        res['AssA'][a] = np.sum(mc * (mc / np.maximum(1, gt_count + tr_count - mc))) / tp
        res['AssRe'][a] = np.sum(mc * (mc / np.maximum(1, gt_count))) / tp
        res['AssPr'][a] = np.sum(mc * (mc / np.maximum(1, tr_count))) / tp
    res['LocA'] = np.maximum(1e-10, res['LocA']) / np.maximum(1e-10, res['HOTA_TP'])
    return _hota_final(res)


def _hota_final(res):
    tp, fn, fp = res['HOTA_TP'], res['HOTA_FN'], res['HOTA_FP']
    res['DetRe'] = tp / np.maximum(1, tp + fn)
    res['DetPr'] = tp / np.maximum(1, tp + fp)
    res['DetA'] = tp / np.maximum(1, tp + fn + fp)
    res['HOTA'] = np.sqrt(res['DetA'] * res['AssA'])
    return res


def hota_combine(per_sequence):
    """Sequences -> the combined result the way TrackEval's COMBINED_SEQ does: detection counts summed, the association
    and localisation scores averaged with the sequences' TP counts as weights, then DetA / HOTA from the combined values."""
    seqs = list(per_sequence)
    A = len(HOTA_ALPHAS)
    res = {k: sum((s[k] for s in seqs), np.zeros(A)) for k in ('HOTA_TP', 'HOTA_FN', 'HOTA_FP')}
    for k in ('AssA', 'AssRe', 'AssPr', 'LocA'):
        num = sum((s[k] * s['HOTA_TP'] for s in seqs), np.zeros(A))
        res[k] = np.maximum(1e-10, num) / np.maximum(1e-10, res['HOTA_TP']) if k == 'LocA' else num / np.maximum(1.0, res['HOTA_TP'])
    return _hota_final(res)


def kitti_box_ious(a, b, do_ioa=False):
    """IoU of (n, 4) and (m, 4) boxes in x1, y1, x2, y2 form with the rules of TrackEval's _calculate_box_ious
    [upstream-memory]: intersection clipped at 0, union = a1 + a2 - inter, intersection 0 where an area or the union is
    <= eps, union 1 where it is <= eps.  do_ioa: the intersection over the area of `a` instead (0 where that area is
    <= eps)."""
    eps = np.finfo(float).eps
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 4), np.asarray(b, dtype=np.float64).reshape(-1, 4)
    lo = np.maximum(a[:, None, :2], b[None, :, :2])
    hi = np.minimum(a[:, None, 2:], b[None, :, 2:])
    inter = np.maximum(hi[..., 0] - lo[..., 0], 0) * np.maximum(hi[..., 1] - lo[..., 1], 0)
    area1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    if do_ioa:
        inter[area1 <= eps, :] = 0
        return inter / np.where(area1 <= eps, 1.0, area1)[:, None]
    area2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    union = area1[:, None] + area2[None, :] - inter
    inter[area1 <= eps, :] = 0
    inter[:, area2 <= eps] = 0
    inter[union <= eps] = 0
    union[union <= eps] = 1
    return inter / union


def kitti_preprocess(gt_rows, pred_rows, ignore_boxes, cls_id, distractor_ids, max_occlusion=2, max_truncation=0,
                     min_height=25, match_thr=0.5, ignore_thr=0.5):
    """KITTI's per-frame preprocessing of ONE sequence for ONE evaluated class: what TrackEval's
    Kitti2DBox.get_preprocessed_seq_data does before a sequence is scored, restated from memory of that package
    [upstream-memory] (the reference's Kitti2DBox_MOT, mmtrack/evaluation/functional/kitti_2d_box.py, inherits it and
    fixes the constants, :56-58).  The executable specification of st_mot_kitti_preprocess.

    gt_rows (frame, id, class, truncation, occlusion, x1, y1, x2, y2) without the DontCare rows, pred_rows (frame, id,
    class, x1, y1, x2, y2, score), ignore_boxes (frame, x1, y1, x2, y2): the DontCare regions.  Per frame: one
    assignment between the ground truth of class cls_id or a distractor and the predictions of class cls_id on the IoU
    thresholded at match_thr; a matched prediction is removed when its partner is a distractor, occluded or truncated
    beyond the limits; an unmatched one when it is not higher than min_height or lies more than ignore_thr inside an
    ignore region.  Returns (gt_keep, pred_keep), boolean masks over the input rows: the rows scored for the class."""
    eps = np.finfo(float).eps
    gt_rows = np.asarray(gt_rows, dtype=np.float64).reshape(-1, 9)
    pred_rows = np.asarray(pred_rows, dtype=np.float64).reshape(-1, 8)
    ignore_boxes = np.asarray(ignore_boxes, dtype=np.float64).reshape(-1, 5)
    distractor_ids = list(distractor_ids)
    gt_keep = (gt_rows[:, 2] == cls_id) & (gt_rows[:, 4] <= max_occlusion) & (gt_rows[:, 3] <= max_truncation)
    pred_keep = np.zeros(len(pred_rows), dtype=bool)
    g_in = np.isin(gt_rows[:, 2], [cls_id] + distractor_ids)
    p_in = pred_rows[:, 2] == cls_id
    gf, pf, nf = gt_rows[:, 0].astype(np.int64), pred_rows[:, 0].astype(np.int64), ignore_boxes[:, 0].astype(np.int64)
    for f in np.unique(pf[p_in]):
        gi, pi = np.nonzero(g_in & (gf == f))[0], np.nonzero(p_in & (pf == f))[0]
        g, p = gt_rows[gi], pred_rows[pi]
        unmatched = np.ones(len(pi), dtype=bool)
        removed = np.zeros(len(pi), dtype=bool)
        if len(gi) and len(pi):
            score = kitti_box_ious(g[:, 5:9], p[:, 3:7])
            score[score < match_thr - eps] = 0
            rows, cols = linear_sum_assignment(-score)
            ok = score[rows, cols] > 0 + eps
            rows, cols = rows[ok], cols[ok]
            removed[cols] = np.isin(g[rows, 2], distractor_ids) | (g[rows, 4] > max_occlusion + eps) | \
                (g[rows, 3] > max_truncation + eps)
            unmatched[cols] = False
        too_small = p[:, 6] - p[:, 4] <= min_height + eps
        in_ignore = np.any(kitti_box_ious(p[:, 3:7], ignore_boxes[nf == f, 1:5], do_ioa=True) > ignore_thr + eps, axis=1)
        removed |= unmatched & (too_small | in_ignore)
        pred_keep[pi] = ~removed
    return gt_keep, pred_keep


PROTOCOLS = ('rows', 'trackeval')
MOTCHALLENGE_BENCHMARKS = ('MOT15', 'MOT16', 'MOT17', 'MOT20', 'DanceTrack')      # mot_drone_metrics.py:84
MOTCHALLENGE_NUM_CLASSES = 13         # MOTChallenge's class ids 1 .. 13; 1 = pedestrian, the one class evaluated
_MOTCHALLENGE_DISTRACTORS = (2, 7, 8, 12)     # person_on_vehicle, static_person, distractor, reflection


def motchallenge_distractors(benchmark):
    """The distractor class ids of a benchmark; () where TrackEval does not preprocess (MOT15).  MOT20 adds 6
    (non_mot_vehicle) [upstream-memory]."""
    if benchmark not in MOTCHALLENGE_BENCHMARKS:
        raise ValueError(f'benchmark must be one of {MOTCHALLENGE_BENCHMARKS}, got {benchmark!r}')
    if benchmark == 'MOT15':
        return ()
    return _MOTCHALLENGE_DISTRACTORS + ((6,) if benchmark == 'MOT20' else ())


def motchallenge_gt8(gt_rows):
    """Ground-truth rows as (n, 8) fp64 (frame, id, x, y, w, h, conf, class): rows without the conf / class columns
    (a sweep's 6-column ground truth) get conf 1, class 1; visibility is not scored and is dropped."""
    rows = np.asarray(gt_rows, dtype=np.float64)
    rows = rows.reshape(-1, rows.shape[-1]) if rows.size else np.zeros((0, 8))
    if rows.shape[1] < 6:
        raise ValueError(f'ground-truth rows need at least 6 columns, got {rows.shape[1]}')
    if rows.shape[1] < 8:
        rows = np.column_stack([rows, np.ones((len(rows), 8 - rows.shape[1]))])
    return np.ascontiguousarray(rows[:, :8])


def motchallenge_pred7(pred_rows):
    """Prediction rows as (m, 7) fp64 (frame, id, x, y, w, h, score): 6-column rows get the score 1."""
    rows = np.asarray(pred_rows, dtype=np.float64)
    rows = rows.reshape(-1, rows.shape[-1]) if rows.size else np.zeros((0, 7))
    if rows.shape[1] < 6:
        raise ValueError(f'prediction rows need at least 6 columns, got {rows.shape[1]}')
    if rows.shape[1] < 7:
        rows = np.column_stack([rows, np.ones(len(rows))])
    return np.ascontiguousarray(rows[:, :7])


def _require_finite(rows, kind, video):
    bad = np.nonzero(~np.isfinite(rows).all(axis=1))[0]
    if len(bad):
        where = '' if video is None else f'video {video!r}, '
        raise ValueError(f'MOTChallenge files: a non-finite value: {where}{kind} row {int(bad[0])}')


def motchallenge_file_rows(gt_rows, pred_rows, video=None):
    """The values a reader of the files of write_motchallenge gets back (reference :223-253), without writing them.
    Ground truth (frame, id, x, y, w, h, conf, class) is written with '%d': int(v), which truncates toward zero.
    Predictions: frame and id with '%d', x, y, w, h and the score with '%.3f': float('%.3f' % v) - the EXACT binary
    value to 3 decimals, ties to even, then the nearest double to that decimal.  np.rint(v * 1000) / 1000 is not that
    (v * 1000 is rounded before rint sees it), so the predictions go through Python's own formatting, value by value:
    the executable specification of st_mot_file_round.
    A non-finite value raises ValueError naming `video` and the row ('%d' % nan raises in the reference).
    Returns (gt (n, 8), pred (m, 7)) fp64 in the row order given (motchallenge_gt8 / motchallenge_pred7 widths)."""
    gt, pred = motchallenge_gt8(gt_rows), motchallenge_pred7(pred_rows)
    _require_finite(gt, 'ground-truth', video)
    _require_finite(pred, 'prediction', video)
    gt = np.trunc(gt) + 0.0                      # + 0.0: int(-0.5) is 0, not -0
    out = np.empty_like(pred)
    out[:, :2] = np.trunc(pred[:, :2]) + 0.0
    out[:, 2:] = np.array([float('%.3f' % v) for v in pred[:, 2:].ravel().tolist()], dtype=np.float64).reshape(-1, 5)
    return gt, out


def motchallenge_preprocess(gt_rows, pred_rows, benchmark='MOT17'):
    """The preprocessing of ONE sequence that TrackEval's MotChallenge2DBox.get_preprocessed_seq_data applies for the
    class 'pedestrian' before a sequence is scored, restated from memory of that package [upstream-memory]; parity with
    TrackEval itself (absent here) is UNPINNED.  The executable specification of st_mot_challenge_preprocess
    (DESIGN.md section 21).

    gt_rows (frame, id, x, y, w, h, conf, class, ...), pred_rows (frame, id, x, y, w, h, ...): what the files hold
    (motchallenge_file_rows).  A ground-truth class outside 1 .. 13 raises ValueError.  Every benchmark but MOT15: per
    frame with ground truth (of any class) and predictions, one assignment that maximises the sum of the IoU with
    entries < 0.5 - eps zeroed (TrackEval's constant, not the scorers' iou_thr); a prediction matched (weight > eps) to
    ground truth of a distractor class (motchallenge_distractors) is removed; ground truth is kept iff conf != 0 and
    class == 1.  MOT15: no prediction is removed, ground truth is kept iff conf != 0.
    Returns (gt_keep, pred_keep), boolean masks over the input rows.  The removed set is defined up to ties among the
    optimal assignments that carry positive weight ("Ties")."""
    eps = np.finfo(float).eps
    distractors = list(motchallenge_distractors(benchmark))
    gt, pred = motchallenge_gt8(gt_rows), motchallenge_pred7(pred_rows)
    cls = gt[:, 7]
    bad = np.nonzero(~((cls >= 1) & (cls <= MOTCHALLENGE_NUM_CLASSES) & (cls == np.floor(cls))))[0]
    if len(bad):
        raise ValueError(f'MOTChallenge preprocessing: ground-truth row {int(bad[0])} has class {cls[bad[0]]:g}, outside '
                         f'1..{MOTCHALLENGE_NUM_CLASSES}')
    pred_keep = np.ones(len(pred), dtype=bool)
    if benchmark == 'MOT15':
        return gt[:, 6] != 0, pred_keep
    gf, pf = gt[:, 0].astype(np.int64), pred[:, 0].astype(np.int64)
    for f in np.intersect1d(gf, pf):
        gi, pi = np.nonzero(gf == f)[0], np.nonzero(pf == f)[0]
        score = box_iou_xywh(gt[gi, 2:6], pred[pi, 2:6])
        score[score < 0.5 - eps] = 0
        rows, cols = linear_sum_assignment(-score)
        ok = score[rows, cols] > 0 + eps
        rows, cols = rows[ok], cols[ok]
        pred_keep[pi[cols[np.isin(cls[gi[rows]], distractors)]]] = False
    return (gt[:, 6] != 0) & (cls == 1), pred_keep


def motchallenge_scored_rows(gt_by_video, pred_by_video, videos, benchmark='MOT17'):
    """protocol='trackeval' on the host: video -> the file rows (motchallenge_file_rows) that motchallenge_preprocess
    keeps, for both sides; what clear_identity / hota then score."""
    gt, pred = {}, {}
    for v in videos:
        g, p = motchallenge_file_rows(gt_by_video.get(v, ()), pred_by_video.get(v, ()), video=v)
        gk, pk = motchallenge_preprocess(g, p, benchmark)
        gt[v], pred[v] = g[gk], p[pk]
    return gt, pred


def combine_videos(per_video, hota_by_video=None):
    """The combined result over videos (count-summed, like TrackEval's COMBINED_SEQ) of per-video clear_identity
    dicts.  hota_by_video: the videos' hota() dicts when HOTA is asked for (None: not asked); every video's dict then
    gains its HOTA / DetA / AssA means over the 19 thresholds and the combined one those of hota_combine, with LocA."""
    tot = defaultdict(float)
    for r in per_video.values():
        for k in ('TP', 'FN', 'FP', 'IDSW', 'IDTP', 'IDFN', 'IDFP'):
            tot[k] += r[k]
        tot['motp_sum'] += r['MOTP'] * r['TP']
    combined = dict(tot)
    combined['MOTA'] = (tot['TP'] - tot['FP'] - tot['IDSW']) / max(1.0, tot['TP'] + tot['FN'])
    combined['MOTP'] = tot['motp_sum'] / max(1.0, tot['TP'])
    combined['IDF1'] = tot['IDTP'] / max(1.0, tot['IDTP'] + 0.5 * tot['IDFP'] + 0.5 * tot['IDFN'])
    combined['IDP'] = tot['IDTP'] / max(1.0, tot['IDTP'] + tot['IDFP'])
    combined['IDR'] = tot['IDTP'] / max(1.0, tot['IDTP'] + tot['IDFN'])
    for k in ('Frag', 'MT', 'PT', 'ML'):
        combined[k] = float(sum(r[k] for r in per_video.values()))
    if hota_by_video is not None:      # mot_drone_metrics.py:291-295: the averages over the 19 thresholds
        hs = hota_by_video
        for v, h in hs.items():
            per_video[v].update(HOTA=float(h['HOTA'].mean()), DetA=float(h['DetA'].mean()), AssA=float(h['AssA'].mean()))
        hc = hota_combine(hs.values()) if hs else _hota_final({k: np.zeros(len(HOTA_ALPHAS)) for k in
                                                               ('HOTA_TP', 'HOTA_FN', 'HOTA_FP', 'AssA', 'AssRe', 'AssPr', 'LocA')})
        combined.update(HOTA=float(hc['HOTA'].mean()), DetA=float(hc['DetA'].mean()), AssA=float(hc['AssA'].mean()),
                        LocA=float(hc['LocA'].mean()))
    return combined


class GatheredVideoMetric:
    """What the video metrics share: per-video row lists in self.pred / self.gt, merged over the ranks by gather(), and
    evaluate() that lets rank 0 compute _evaluate_local() and broadcasts the result."""

    def gather(self):
        """Multi-rank evaluation, the reference's way (mot_drone_metrics.py:336-358: barrier, all_gather_object of the
        per-video `seq_info`, rank 0 evaluates, broadcast_object_list of the result): ranks hold DISJOINT whole videos
        (video_sampler.py:62-70 / dist.shard_videos), so the per-video row lists are merged by key.  Afterwards every
        rank holds every video's rows.  No-op without an initialised process group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return self
        dist.barrier()                                   # wait for all processes to complete prediction (:336)
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, dict(pred=dict(self.pred), gt=dict(self.gt)))   # KBs of pickled rows (:340)
        pred, gt = defaultdict(list), defaultdict(list)
        for part in parts:                               # rank order = video order of shard_videos
            for v, rows in part['pred'].items():
                if v in pred:
                    raise RuntimeError(f'video {v!r} was evaluated on more than one rank: videos shard whole')
                pred[v] = rows
            for v, rows in part['gt'].items():
                gt[v] = rows
        self.pred, self.gt = pred, gt
        return self

    def evaluate(self, distributed=True):
        """Per-video and combined (count-summed, like TrackEval's COMBINED_SEQ) scores.  With a process group (and
        `distributed`): gather first, rank 0 computes, every rank returns the broadcast result (:344-358)."""
        import torch.distributed as dist
        multi = distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        if multi:
            self.gather()
            box = [self._evaluate_local() if dist.get_rank() == 0 else None]
            dist.broadcast_object_list(box, src=0)
            return box[0]
        return self._evaluate_local()


class MOTDroneMetrics(GatheredVideoMetric):
    """Collects per-frame tracks, writes MOTChallenge files, scores them (depth-range filtered)."""

    allowed_metrics = ('HOTA', 'CLEAR', 'Identity')

    def __init__(self, depth_thr=80, ignore_depth=False, iou_thr=0.5, metric=('HOTA', 'CLEAR', 'Identity'),
                 backend='host', postprocess_tracklet_cfg=(), protocol='rows', benchmark='MOT17'):
        _check_backend(backend)       # 'device': all videos in one mot_eval.evaluate_packed call, at evaluate()
        self.backend = backend
        # 'rows': the collected float rows are scored; 'trackeval': what the reference's TrackEval run scores - the
        # written files' values (motchallenge_file_rows) after motchallenge_preprocess for `benchmark` (:84, :273-289)
        if protocol not in PROTOCOLS:
            raise ValueError(f'protocol must be one of {PROTOCOLS}, got {protocol!r}')
        motchallenge_distractors(benchmark)               # refuses a benchmark outside the reference's list
        self.protocol, self.benchmark = protocol, benchmark
        # mot_drone_metrics.py:95, 110-113: TASK_UTILS entries applied to every video's prediction rows.  The reference
        # applies them in process() when a video's last frame arrives (:210-219); process() here has no video length,
        # so they run once per video at evaluation time (postprocessed_pred), after gather(), on the evaluating rank.
        self.postprocess_tracklet_methods = [self._build_postprocess(c) for c in (postprocess_tracklet_cfg or ())]
        self._postprocessed = None
        self.depth_thr, self.ignore_depth, self.iou_thr = depth_thr, ignore_depth, iou_thr
        self.metrics = [metric] if isinstance(metric, str) else list(metric)      # mot_drone_metrics.py:83-103
        for m in self.metrics:
            if m not in self.allowed_metrics:
                raise KeyError(f'metric {m} is not supported.')
        self.pred = defaultdict(list)
        self.gt = defaultdict(list)

    def _build_postprocess(self, cfg):
        from .registry import TASK_UTILS
        from . import tracklets  # noqa: F401  (registers InterpolateTracklets)
        if not isinstance(cfg, dict):
            return cfg                                    # an instance, used as it is
        if str(cfg.get('type', '')).split('.')[-1] == 'AppearanceFreeLink':
            raise NotImplementedError('postprocess_tracklet_cfg: AppearanceFreeLink needs a trained link network and its '
                                      'checkpoint, which are not available; InterpolateTracklets is supported')
        cfg = dict(cfg)
        cfg.setdefault('backend', self.backend)           # an entry without a backend inherits the metric's
        return TASK_UTILS.build(cfg)

    def postprocessed_pred(self):
        """video -> prediction rows after the post-processing entries (the collected rows without any): what is scored
        and written.  Every entry sees all videos in one forward_many call; the result is kept until rows are added, so
        write_motchallenge and evaluate share one pass."""
        if not self.postprocess_tracklet_methods:
            return self.pred
        videos = sorted(self.pred)
        key = (id(self.pred), tuple((v, len(self.pred[v])) for v in videos))   # process() appends, gather() replaces
        if self._postprocessed is None or self._postprocessed[0] != key:
            rows = [np.asarray(self.pred[v], dtype=np.float64).reshape(-1, 7) for v in videos]
            for method in self.postprocess_tracklet_methods:
                rows = method.forward_many(rows)
            self._postprocessed = (key, dict(zip(videos, rows)))
        return self._postprocessed[1]

    def process(self, video, data_sample, gt_instances=None):
        """data_sample: TrackDataSample with pred_track_instances (+ metainfo frame_id);
        gt_instances: list of dicts with instance_id, bbox (xyxy), mot_conf, category_id, visibility, location."""
        frame_id = data_sample.metainfo['frame_id']
        if gt_instances is not None:
            for ins in gt_instances:
                if self.ignore_depth or ins['location'][-1] <= self.depth_thr:
                    x1, y1, x2, y2 = ins['bbox']
                    self.gt[video].append([frame_id + 1, ins['instance_id'], x1, y1, x2 - x1, y2 - y1,
                                           ins.get('mot_conf', 1), ins.get('category_id', 1),
                                           ins.get('visibility', 1.0)])
        trk = data_sample.pred_track_instances
        ids = trk['instances_id'].cpu().numpy()
        boxes = trk['bboxes'].cpu().numpy()
        scores = trk['scores'].cpu().numpy()
        depth = trk['depth'].cpu().numpy() if 'depth' in trk else np.ones(len(ids))
        for i in range(len(ids)):
            if self.ignore_depth or self.depth_thr >= depth[i] > 0:
                b = boxes[i]
                self.pred[video].append([frame_id + 1, int(ids[i]), b[0], b[1], b[2] - b[0], b[3] - b[1], scores[i]])

    def write_motchallenge(self, out_dir):
        """pred: frame,id,x,y,w,h,score,-1,-1,-1   gt: frame,id,x,y,w,h,conf,class,visibility (reference :223-253)."""
        os.makedirs(os.path.join(out_dir, 'pred'), exist_ok=True)
        os.makedirs(os.path.join(out_dir, 'gt'), exist_ok=True)
        for video, rows in self.postprocessed_pred().items():
            with open(os.path.join(out_dir, 'pred', video + '.txt'), 'wt') as f:
                for t in rows:
                    f.write('%d,%d,%.3f,%.3f,%.3f,%.3f,%.3f,-1,-1,-1\n' % tuple(t[:7]))
        for video, rows in self.gt.items():
            with open(os.path.join(out_dir, 'gt', video + '.txt'), 'wt') as f:
                for t in rows:
                    f.write('%d,%d,%d,%d,%d,%d,%d,%d,%.5f\n' % tuple(t[:9]))

    @classmethod
    def read_motchallenge(cls, out_dir, **kwargs):
        """A metric (built with `kwargs`) whose gt / pred hold what out_dir/gt/*.txt and out_dir/pred/*.txt, as
        write_motchallenge wrote them, read back: every field through float(); the predictions' three trailing -1
        fields are dropped.  The rows are final (tracklet post-processing ran before they were written)."""
        m = cls(**kwargs)
        for kind, store, width in (('gt', m.gt, 9), ('pred', m.pred, 7)):
            folder = os.path.join(out_dir, kind)
            for name in sorted(os.listdir(folder)) if os.path.isdir(folder) else ():
                if not name.endswith('.txt'):
                    continue
                with open(os.path.join(folder, name), 'rt') as f:
                    store[name[:-4]] = [[float(v) for v in line.split(',')[:width]] for line in f if line.strip()]
        return m

    def _evaluate_local(self):
        videos = sorted(set(self.gt) | set(self.pred))
        pred = self.postprocessed_pred()
        gt = self.gt
        wanted = ['CLEAR', 'Identity'] + (['HOTA'] if 'HOTA' in self.metrics else [])
        if self.protocol == 'trackeval' and self.backend == 'device':
            from . import mot_eval
            scored = dict(zip(videos, mot_eval.evaluate_motchallenge(
                [gt.get(v, []) for v in videos], [pred.get(v, []) for v in videos], self.benchmark, self.iou_thr, wanted,
                videos=videos)))
            per_video = {v: scored[v]['clear_identity'] for v in videos}
        elif self.backend == 'device':
            from . import mot_eval
            packed = mot_eval.pack_sequences({v: gt.get(v, []) for v in videos}, {v: pred.get(v, []) for v in videos})
            scored = dict(zip(packed['videos'], mot_eval.evaluate_packed(packed, self.iou_thr, wanted)))
            per_video = {v: scored[v]['clear_identity'] for v in videos}
        else:
            if self.protocol == 'trackeval':
                gt, pred = motchallenge_scored_rows(gt, pred, videos, self.benchmark)
            per_video = {v: clear_identity(gt.get(v, []), pred.get(v, []), self.iou_thr) for v in videos}
        hs = None
        if 'HOTA' in self.metrics:
            hs = {v: scored[v]['hota'] for v in per_video} if self.backend == 'device' else \
                {v: hota(gt.get(v, []), pred.get(v, [])) for v in per_video}
        return dict(per_video=per_video, combined=combine_videos(per_video, hs))


from .registry import METRICS  # noqa: E402
METRICS.register_module(name=['MOTDroneMetrics', 'mmtrack.MOTDroneMetrics'], module=MOTDroneMetrics)
