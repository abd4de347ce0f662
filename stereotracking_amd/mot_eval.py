"""MOT evaluation on the device: CLEAR, Identity and HOTA of many sequences in one call (csrc/mot_eval.hip behind
st_mot_similarity / st_mot_walk / st_mot_hota_match / st_mot_hota_accumulate; include/stereotrack.h section 15).

The rules are those of stereotracking_amd/metrics.py (clear_identity, hota), the executable specification; this module
returns the same dictionaries.  The host keeps what is small or does not suit a wave: the sort
and id compaction of the rows (pack_sequences, numpy), Identity's one global assignment per sequence (scipy, fed with
the device's integer arrays), the final divisions and the combination over videos.

    packed = pack_sequences(gt_by_video, pred_by_video)        # numpy only, no GPU needed
    results = evaluate_packed(packed, iou_thr=0.5)             # one upload, one wait, one copy back
    results[i]['clear_identity'], results[i]['hota']           # what metrics.clear_identity / metrics.hota return

KITTI's 2-D box preprocessing (metrics.kitti_preprocess, the specification; st_mot_kitti_preprocess, include/stereotrack.h
section 16) runs ahead of them for MOTKittiMetrics(backend='device'):

    masks = kitti_keep_masks(sequences, classes)               # one upload, one launch, one wait and copy back

The MOTChallenge protocol of MOTDroneMetrics(protocol='trackeval') (metrics.motchallenge_file_rows / motchallenge_preprocess,
the specification; st_mot_file_round / st_mot_challenge_preprocess, include/stereotrack.h section 21):

    masks = motchallenge_keep_masks(gts, preds, 'MOT17')       # one upload, two roundings, one launch, one copy back
    results = evaluate_motchallenge(gts, preds, 'MOT17')       # the same, then the kept rows through evaluate_packed

Both backends are defined up to ties of the assignment optimum ("Ties").
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import StMotArgs, check, current_stream
from ._packed import PackedCall

ST_MOT_CLEAR, ST_MOT_HOTA = 1, 2
STATUS_KINDS = ((1, 'a non-finite box'), (2, 'an id that occurs twice in one frame'), (4, 'rows that are not sorted by frame'),
                (8, 'more objects in one frame than a launch holds'), (16, 'an id index outside its sequence'))
LAUNCHES = collections.Counter()     # calls of every st_mot_* stage entry (tests read it)
_TABLES = ('seq_frame_off', 'frame_seq', 'frame_no', 'frame_gt_off', 'frame_pred_off', 'frame_pair_off', 'seq_ng',
           'seq_nt', 'seq_gid_off', 'seq_tid_off', 'seq_mat_off')


def max_frame_objects():
    """Largest number of ground-truth (or prediction) rows in one frame that a launch supports."""
    return int(_lib.load().st_mot_max_objects())


def _rows6(rows):
    rows = np.asarray(rows, dtype=np.float64)
    if rows.size == 0:
        return np.zeros((0, 6))
    return rows.reshape(-1, rows.shape[-1])[:, :6]


def _sort_and_compact(rows, video, kind):
    """rows sorted by frame (stable), ids replaced by their index in sorted(set(ids)); the frame numbers and the ids."""
    frames = rows[:, 0].astype(np.int64)
    order = np.argsort(frames, kind='stable')
    rows, frames = rows[order], frames[order]
    ids = rows[:, 1].astype(np.int64)
    uniq = np.unique(ids)
    dense = np.searchsorted(uniq, ids)
    if len(rows) > 1:
        o = np.lexsort((dense, frames))
        same = (frames[o][1:] == frames[o][:-1]) & (dense[o][1:] == dense[o][:-1])
        if same.any():
            k = o[1:][np.argmax(same)]
            raise ValueError(f'video {video!r}: {kind} id {int(ids[k])} occurs twice in frame {int(frames[k])}')
    out = np.empty((len(rows), 6))
    out[:, 0], out[:, 1], out[:, 2:] = frames, dense, rows[:, 2:6]
    return out, frames, uniq


def pack_sequences(gt_by_video, pred_by_video):
    """The host preparation (pure numpy).  gt_by_video / pred_by_video: dicts video -> rows (frame, id, x, y, w, h, ...),
    or two lists of equal length; a video missing on one side has no rows there.  Per video: rows sorted by frame, the
    frames = the ascending union of both sides' frame numbers, ids compacted to their index in sorted(set(ids)) as the
    host scorer does, and the ragged offset tables of include/stereotrack.h section 15.  An id twice in one frame
    raises ValueError naming the video and the frame.  Returns a dict of arrays ('videos': the order)."""
    if not isinstance(gt_by_video, dict):
        gt_by_video = dict(enumerate(gt_by_video))
    if not isinstance(pred_by_video, dict):
        pred_by_video = dict(enumerate(pred_by_video))
    videos = sorted(set(gt_by_video) | set(pred_by_video))
    srt, seq_ng, seq_nt, gt_ids, tr_ids = [], [], [], [], []
    for v in videos:
        g, gfr, gu = _sort_and_compact(_rows6(gt_by_video.get(v, ())), v, 'ground-truth')
        p, pfr, pu = _sort_and_compact(_rows6(pred_by_video.get(v, ())), v, 'prediction')
        srt.append([(g, gfr, None), (p, pfr, None)])
        seq_ng.append(len(gu))
        seq_nt.append(len(pu))
        gt_ids.append(gu)
        tr_ids.append(pu)
    t = _frame_tables(srt, (6, 6), lambda totals, F: f'pack_sequences: {totals[0]} ground-truth rows, {totals[1]} prediction '
                                                     f'rows, {F} frames: the offset tables are 32-bit')
    out = dict(videos=videos, gt_ids=gt_ids, tr_ids=tr_ids, frame_seq=t['frame_seq'], frame_no=t['frame_no'])
    (out['gt_rows'], out['pred_rows']), (out['frame_gt_off'], out['frame_pred_off']) = t['rows'], t['offs']
    out['seq_frame_off'] = np.searchsorted(t['frame_seq'], np.arange(len(videos) + 1)).astype(np.int32)
    G, P = np.diff(out['frame_gt_off']).astype(np.int64), np.diff(out['frame_pred_off']).astype(np.int64)
    out['frame_pair_off'] = np.concatenate([[0], np.cumsum(G * P)]).astype(np.int64)
    out['seq_ng'], out['seq_nt'] = np.asarray(seq_ng, np.int32), np.asarray(seq_nt, np.int32)
    ng, nt = out['seq_ng'].astype(np.int64), out['seq_nt'].astype(np.int64)
    out['seq_gid_off'] = np.concatenate([[0], np.cumsum(ng)]).astype(np.int64)
    out['seq_tid_off'] = np.concatenate([[0], np.cumsum(nt)]).astype(np.int64)
    out['seq_mat_off'] = np.concatenate([[0], np.cumsum(ng * nt)]).astype(np.int64)
    out['max_frame_objects'] = t['max_frame_objects']
    return out


def _raise_status(prefix, kinds, status, videos, frame_seq, frame_no, limit=''):
    """A non-zero device status word as an exception.  kinds: (bit, text) of every condition the entry reports, the first
    set one is raised; the status holds, in word 1 + the bit's position, the number of frames minus the first frame
    that has it.  limit: the note of bit 8, '{n}' = max_frame_objects()."""
    bits = int(status[0])
    for bit, what in kinds:
        if bits & bit:
            f = len(frame_no) - int(status[bit.bit_length()])
            msg = f'{prefix}: {what}: video {videos[int(frame_seq[f])]!r}, frame {int(frame_no[f])}'
            if bit == 8:
                msg += limit.format(n=max_frame_objects())
            raise ValueError(msg) if bit in (1, 2, 8) else _lib.StError(msg)
    raise _lib.StError(f'{prefix} failed on the device: status {bits}')


def evaluate_packed(packed, iou_thr=0.5, metrics=('HOTA', 'CLEAR', 'Identity'), device=None, alphas=None, timing=False,
                    return_arrays=False, device_boxes=None):
    """Scores every sequence of `packed` (pack_sequences) on the device.  Returns one dict per sequence, in the order of
    packed['videos']: 'clear_identity' = what metrics.clear_identity returns ('CLEAR' or 'Identity' in `metrics`, else
    None), 'hota' = what metrics.hota returns, per-alpha arrays included ('HOTA' in `metrics`, else None: the HOTA
    stages are then not launched).  One upload, one wait and one copy back per call, however many sequences.
    `timing`: returns (results, timing dict) - HIP events around every stage and the host clock of the parts of the
    call.  `return_arrays`: every dict also carries 'arrays' with the
    device's intermediates of that sequence (sim: the IoU matrix of every frame, hota_potential, id_potential,
    gt_count, tr_count) - one extra copy of the workspace, for tests.
    `device_boxes`: (gt (num_gt, 4), pred (num_pred, 4)) fp64 tensors on the device that replace the x, y, w, h columns
    of the packed rows after the upload (evaluate_motchallenge: boxes that never left the device)."""
    from . import metrics as M
    metrics = [metrics] if isinstance(metrics, str) else list(metrics)
    do_hota = 'HOTA' in metrics
    do_clear = 'CLEAR' in metrics or 'Identity' in metrics
    if not (do_hota or do_clear):
        raise ValueError(f'evaluate_packed: nothing to compute for metrics {metrics}')
    call = PackedCall('the MOT evaluation', 'csrc/mot_eval.hip', device, timing, LAUNCHES)
    dev = call.dev
    alphas = np.ascontiguousarray(M.HOTA_ALPHAS if alphas is None else alphas, dtype=np.float64)
    B, F, A = len(packed['videos']), len(packed['frame_no']), len(alphas)
    if B == 0:
        return []
    NG, NP_ = len(packed['gt_rows']), len(packed['pred_rows'])
    ids_g, ids_t, cells = int(packed['seq_gid_off'][-1]), int(packed['seq_tid_off'][-1]), int(packed['seq_mat_off'][-1])

    call.upload(dict(gt_rows=packed['gt_rows'], pred_rows=packed['pred_rows'], alphas=alphas, **{k: packed[k] for k in _TABLES}))
    if device_boxes is not None:
        for name, boxes in zip(('gt_rows', 'pred_rows'), device_boxes):
            n = len(packed[name])
            if tuple(boxes.shape) != (n, 4) or boxes.dtype != torch.float64 or boxes.device != dev:
                raise ValueError(f'evaluate_packed: device_boxes for {name} must be ({n}, 4) float64 on {dev}')
            if n:
                call.device_in(name)[:, 2:6] = boxes
    call.outputs((('status', (8,), np.int32), ('gt_count', (ids_g,), np.int32), ('tr_count', (ids_t,), np.int32),
                  ('id_potential', (cells,), np.int32), ('hota_potential', (cells,), np.float64),
                  ('gt_frames', (ids_g,), np.int32), ('gt_matched', (ids_g,), np.int32), ('gt_frag', (ids_g,), np.int32),
                  ('clear_counts', (B, 4), np.int32), ('motp_sum', (B,), np.float64), ('hota_counts', (B, A, 3), np.int32),
                  ('hota_sums', (B, A, 4), np.float64)), zero=True)

    args = StMotArgs()
    args.struct_size = C.sizeof(StMotArgs)
    args.num_seqs, args.num_frames, args.num_gt, args.num_pred, args.num_alphas = B, F, NG, NP_, A
    args.max_frame_objects = int(packed['max_frame_objects'])
    args.flags = (ST_MOT_CLEAR if do_clear else 0) | (ST_MOT_HOTA if do_hota else 0)
    args.num_pairs, args.num_cells, args.num_gids, args.num_tids = int(packed['frame_pair_off'][-1]), cells, ids_g, ids_t
    args.iou_thr = float(iou_thr)
    call.bind(args)
    call.workspace(args, call.workspace_bytes('st_mot_workspace_bytes', args))

    # over the limit st_mot_similarity launches its checks and returns -1: the status word names the frame
    over = args.max_frame_objects > max_frame_objects()
    with call.stages():
        over_limit = call.launch('st_mot_similarity', C.byref(args), ok=(0, -1) if over else (0,)) == -1
        if not over_limit:
            call.launch('st_mot_walk', C.byref(args))
            if do_hota:
                call.launch('st_mot_hota_match', C.byref(args))
                call.launch('st_mot_hota_accumulate', C.byref(args))
    o = call.fetch()
    if o['status'][0] or over_limit:
        _raise_status('MOT evaluation', STATUS_KINDS, o['status'], packed['videos'], packed['frame_seq'], packed['frame_no'],
                      ' (at most {n} ground-truth and {n} prediction rows per frame)')
    sim = None
    if return_arrays:
        off = int(call.lib.st_mot_workspace_sim_offset(C.byref(args)))
        sim = call.ws[off:off + 8 * args.num_pairs].cpu().numpy().view(np.float64)

    results = []
    for s in range(B):
        ng, nt = int(packed['seq_ng'][s]), int(packed['seq_nt'][s])
        g0, t0, m0 = int(packed['seq_gid_off'][s]), int(packed['seq_tid_off'][s]), int(packed['seq_mat_off'][s])
        f0, f1 = int(packed['seq_frame_off'][s]), int(packed['seq_frame_off'][s + 1])
        n_gt = int(packed['frame_gt_off'][f1] - packed['frame_gt_off'][f0])
        n_pr = int(packed['frame_pred_off'][f1] - packed['frame_pred_off'][f0])
        gt_count = o['gt_count'][g0:g0 + ng].astype(np.float64)
        tr_count = o['tr_count'][t0:t0 + nt].astype(np.float64)
        res = dict(clear_identity=None, hota=None)
        if do_clear:
            tp, fn, fp, idsw = (int(v) for v in o['clear_counts'][s])
            res['clear_identity'] = M._clear_identity_result(
                tp, fn, fp, idsw, float(o['motp_sum'][s]), o['id_potential'][m0:m0 + ng * nt].reshape(ng, nt).astype(np.float64),
                gt_count, tr_count, *(o[k][g0:g0 + ng].astype(np.float64) for k in ('gt_frames', 'gt_matched', 'gt_frag')))
        if do_hota:
            h = {k: np.zeros(A) for k in ('HOTA_TP', 'HOTA_FN', 'HOTA_FP', 'AssA', 'AssRe', 'AssPr', 'LocA')}
            if n_gt == 0 or n_pr == 0:        # metrics.hota's early return
                h['HOTA_FN'] += n_gt
                h['HOTA_FP'] += n_pr
                h['LocA'] += 1.0
            else:
                cnt, sums = o['hota_counts'][s], o['hota_sums'][s]
                h['HOTA_TP'] += cnt[:, 0]
                h['HOTA_FN'] += cnt[:, 1]
                h['HOTA_FP'] += cnt[:, 2]
                tp = np.maximum(1.0, h['HOTA_TP'])
                h['AssA'], h['AssRe'], h['AssPr'] = sums[:, 1] / tp, sums[:, 2] / tp, sums[:, 3] / tp
                h['LocA'] = np.maximum(1e-10, sums[:, 0]) / np.maximum(1e-10, h['HOTA_TP'])
            res['hota'] = M._hota_final(h)
        if return_arrays:
            po = packed['frame_pair_off']
            G, P = np.diff(packed['frame_gt_off']), np.diff(packed['frame_pred_off'])
            res['arrays'] = dict(sim=[sim[po[f]:po[f + 1]].reshape(G[f], P[f]).copy() for f in range(f0, f1)],
                                 hota_potential=o['hota_potential'][m0:m0 + ng * nt].reshape(ng, nt).copy(),
                                 id_potential=o['id_potential'][m0:m0 + ng * nt].reshape(ng, nt).copy(),
                                 gt_count=o['gt_count'][g0:g0 + ng].copy(), tr_count=o['tr_count'][t0:t0 + nt].copy())
        results.append(res)
    return (results, call.timing_dict()) if timing else results


KITTI_STATUS_KINDS = ((1, 'a non-finite box'), (8, 'more rows of one class in one frame than a launch holds'),
                      (32, 'a workspace slot that is too small'))
_KITTI_LDS_CELLS = 64 * 64      # frames with more cells than this (rows of all classes) get a workspace slot (section 16)
_KITTI_MAX_DISTRACTORS = 4


def _sorted_by_frame(rows, frames):
    """(rows, frames, order) in a stable sort by the integer frame numbers `frames`."""
    order = np.argsort(frames, kind='stable')
    return rows[order], frames[order], order


def _frame_tables(sorted_seqs, widths, too_many, cells_per_frame=1):
    """The per-frame tables of the scoring and preprocessing stages (include/stereotrack.h sections 15, 16 and 21).
    sorted_seqs: per sequence one (rows, frames, order) triple per row kind, sorted by frame (_sorted_by_frame), widths:
    the kinds' row widths (ground truth and predictions first).  The frames of a sequence are the union of its kinds'
    frame numbers.  Returns dict(rows: per kind the rows of all sequences, offs: per kind the (F + 1) int32 row offsets
    of the frames, frame_ws_off: the workspace cells in front of every frame, orders: per sequence the kinds' sort
    orders, frame_no, frame_seq, totals, max_frame_objects).  too_many(totals, F): the message when a table does not
    fit 32 bits."""
    kinds = range(len(widths))
    parts, offs, totals = [[np.zeros((0, w))] for w in widths], [[[0]] for _ in kinds], [0 for _ in kinds]
    orders, frame_no, frame_seq = [], [np.zeros(0, np.int64)], [np.zeros(0, np.int32)]
    for s, srt in enumerate(sorted_seqs):
        frames = np.unique(np.concatenate([fr for _, fr, _ in srt]))
        for k, (rows, fr, _) in enumerate(srt):
            parts[k].append(rows)
            offs[k].append(totals[k] + np.searchsorted(fr, frames, 'right'))
            totals[k] += len(rows)
        orders.append([o for _, _, o in srt])
        frame_no.append(frames)
        frame_seq.append(np.full(len(frames), s, np.int32))
    t = dict(rows=[np.concatenate(p) for p in parts], offs=[np.concatenate(o).astype(np.int32) for o in offs], orders=orders,
             frame_no=np.concatenate(frame_no), frame_seq=np.concatenate(frame_seq), totals=totals)
    F = len(t['frame_no'])
    if max(totals + [F * cells_per_frame]) >= 2 ** 31 - 1:
        raise ValueError(too_many(totals, F))
    G, P = np.diff(t['offs'][0]).astype(np.int64), np.diff(t['offs'][1]).astype(np.int64)
    t['frame_ws_off'] = np.concatenate([[0], np.cumsum(np.where(G * P > _KITTI_LDS_CELLS, G * P, 0))]).astype(np.int64)
    t['max_frame_objects'] = int(max(G.max(initial=0), P.max(initial=0)))
    return t


def _keep_masks(orders, keeps):
    """The keep bytes of the packed rows (per kind, rows on the last axis) as boolean arrays over the rows as they were
    passed: one tuple per sequence, one array per kind of `keeps`."""
    out, first = [], [0 for _ in keeps]
    for seq_orders in orders:
        masks = []
        for k, (keep, order) in enumerate(zip(keeps, seq_orders)):
            m = np.zeros(keep.shape[:-1] + (len(order),), bool)
            m[..., order] = keep[..., first[k]:first[k] + len(order)] != 0
            first[k] += len(order)
            masks.append(m)
        out.append(tuple(masks))
    return out


def kitti_keep_masks(sequences, classes, max_occlusion=2, max_truncation=0, min_height=25, match_thr=0.5, ignore_thr=0.5,
                     device=None, videos=None, timing=False):
    """KITTI's preprocessing (metrics.kitti_preprocess, the specification) of every sequence and class in ONE launch of
    st_mot_kitti_preprocess: one upload, one launch, one wait and copy back.
    sequences: a list of (gt_rows (n, 9), pred_rows (m, 8), ignore_boxes (k, 5)) in kitti_preprocess's layouts, rows in
    any order; classes: a list of (class id, distractor ids).  Returns one (gt_keep (C, n), pred_keep (C, m)) pair of
    boolean arrays per sequence, over the rows as they were passed.  videos: the sequences' names for error messages.
    timing: returns (masks, dict) with the stage's device time (HIP events) and the host clock of the call's parts."""
    call = PackedCall('the KITTI preprocessing', 'csrc/mot_eval.hip', device, timing, LAUNCHES)
    sequences = list(sequences)
    videos = list(range(len(sequences))) if videos is None else list(videos)
    table = np.full((len(classes), 1 + _KITTI_MAX_DISTRACTORS), -1, np.int32)
    for c, (cid, distractors) in enumerate(classes):
        distractors = list(distractors)
        if len(distractors) > _KITTI_MAX_DISTRACTORS or int(cid) < 0 or any(int(d) < 0 for d in distractors):
            raise ValueError(f'kitti_keep_masks: class {cid} with distractors {distractors}: ids must be >= 0, at most '
                             f'{_KITTI_MAX_DISTRACTORS} distractors')
        table[c, 0] = int(cid)
        table[c, 1:1 + len(distractors)] = [int(d) for d in distractors]
    C_ = len(classes)
    if C_ == 0 or not sequences:
        return ([], {}) if timing else []

    seqs = [[np.asarray(r, dtype=np.float64).reshape(-1, w) for r, w in zip(seq, (9, 8, 5))] for seq in sequences]
    t = _frame_tables(
        [[_sorted_by_frame(r, r[:, 0].astype(np.int64)) for r in seq] for seq in seqs], (9, 8, 5),
        lambda totals, F: f'kitti_keep_masks: {totals} rows, {F} frames x {C_} classes: the offset tables are 32-bit', C_)
    NG, NP_, NI = t['totals']
    call.upload(dict(zip(('gt_rows', 'pred_rows', 'ignore_rows', 'class_table', 'frame_gt_off', 'frame_pred_off',
                          'frame_ignore_off', 'frame_ws_off'), t['rows'] + [table] + t['offs'] + [t['frame_ws_off']])))
    call.outputs((('status', (8,), np.int32), ('gt_keep', (C_, NG), np.uint8), ('pred_keep', (C_, NP_), np.uint8)))

    args = _lib.StMotKittiArgs()
    args.struct_size = C.sizeof(_lib.StMotKittiArgs)
    args.num_frames, args.num_classes, args.num_gt, args.num_pred, args.num_ignore = len(t['frame_no']), C_, NG, NP_, NI
    args.max_frame_objects = t['max_frame_objects']
    args.num_ws_cells = int(t['frame_ws_off'][-1])
    args.max_occlusion, args.max_truncation, args.min_height = float(max_occlusion), float(max_truncation), float(min_height)
    args.match_thr, args.ignore_thr = float(match_thr), float(ignore_thr)
    call.bind(args)
    call.workspace(args, call.workspace_bytes('st_mot_kitti_workspace_bytes', args))
    with call.stages():
        call.launch('st_mot_kitti_preprocess', C.byref(args))
    host = call.fetch()
    if host['status'][0]:
        _raise_status('KITTI preprocessing', KITTI_STATUS_KINDS, host['status'], videos, t['frame_seq'], t['frame_no'],
                      ' (at most {n} ground-truth rows of a class and its distractors and {n} prediction rows of the class '
                      'per frame)')
    out = _keep_masks(t['orders'], (host['gt_keep'], host['pred_keep']))
    return (out, call.timing_dict()) if timing else out


CHALLENGE_STATUS_KINDS = ((1, 'a non-finite box'), (8, 'more rows in one frame than a launch holds'),
                          (32, 'a workspace slot that is too small'))
FILE_COPY, FILE_TRUNCATE, FILE_ROUND3 = 0, 1, 2          # ST_MOT_FILE_* of include/stereotrack.h section 21
_FILE_MODES = dict(gt=(FILE_TRUNCATE,) * 8, pred=(FILE_TRUNCATE,) * 2 + (FILE_ROUND3,) * 5)
_FILE_STATUS_KINDS = ((1, 'a non-finite value'), (2, 'a value of 2^43 or more in a column written with %.3f'))


def file_round(rows_dev, modes, out_dev, status_dev):
    """Enqueues st_mot_file_round on the current stream: rows_dev (n, len(modes)) fp64 on the device -> out_dev (the
    same shape; may be rows_dev), status_dev = 8 int32 on the device.  No wait: the caller reads the status."""
    n, cols = rows_dev.shape
    if len(modes) != cols or rows_dev.dtype != torch.float64 or not rows_dev.is_contiguous() or not out_dev.is_contiguous():
        raise ValueError(f'file_round: {tuple(rows_dev.shape)} {rows_dev.dtype} rows for {len(modes)} column modes')
    LAUNCHES['st_mot_file_round'] += 1
    check(_lib.load().st_mot_file_round(C.c_void_p(rows_dev.data_ptr()), C.c_void_p(out_dev.data_ptr()), n, cols,
                                        (C.c_int * cols)(*modes), C.c_void_p(status_dev.data_ptr()), current_stream()),
          'st_mot_file_round')


def _challenge_device(gts, preds, benchmark, device, videos, timing):
    """The device flow shared by motchallenge_keep_masks and evaluate_motchallenge: one upload, the two roundings, the
    preprocessing, one wait and one copy back of the status words and the keep bytes."""
    from . import metrics as M
    distractors = M.motchallenge_distractors(benchmark)
    call = PackedCall('the MOTChallenge protocol', 'csrc/mot_eval.hip', device, timing, LAUNCHES)
    dev = call.dev
    gts, preds = list(gts), list(preds)
    if len(gts) != len(preds):
        raise ValueError(f'MOTChallenge protocol: {len(gts)} ground-truth sets against {len(preds)} prediction sets')
    videos = list(range(len(gts))) if videos is None else list(videos)

    # ---- host tables, from the truncated frame column only; the class check needs the class column's integer part
    srt = []
    for s, (g, p) in enumerate(zip(gts, preds)):
        g, p = M.motchallenge_gt8(g), M.motchallenge_pred7(p)
        M._require_finite(g, 'ground-truth', videos[s])
        M._require_finite(p, 'prediction', videos[s])
        cls = np.trunc(g[:, 7])
        bad = np.nonzero((cls < 1) | (cls > M.MOTCHALLENGE_NUM_CLASSES))[0]
        if len(bad):
            raise ValueError(f'MOTChallenge preprocessing: video {videos[s]!r}: ground-truth row {int(bad[0])} has class '
                             f'{cls[bad[0]]:g}, outside 1..{M.MOTCHALLENGE_NUM_CLASSES}')
        srt.append([_sorted_by_frame(rows, np.trunc(rows[:, 0]).astype(np.int64)) for rows in (g, p)])
    t = _frame_tables(srt, (8, 7), lambda totals, F: f'MOTChallenge protocol: {totals[0]} ground-truth rows, {totals[1]} '
                                                     f'prediction rows, {F} frames: the offset tables are 32-bit')
    NG, NP_ = t['totals']
    call.upload(dict(zip(('gt_rows', 'pred_rows', 'frame_gt_off', 'frame_pred_off', 'frame_ws_off'),
                         t['rows'] + t['offs'] + [t['frame_ws_off']])))
    call.outputs((('status_gt', (8,), np.int32), ('status_pred', (8,), np.int32), ('status', (8,), np.int32),
                  ('gt_keep', (NG,), np.uint8), ('pred_keep', (NP_,), np.uint8)))
    gt_file = torch.empty((NG, 8), dtype=torch.float64, device=dev)    # the rows a reader of the files gets
    pred_file = torch.empty((NP_, 7), dtype=torch.float64, device=dev)

    args = _lib.StMotChallengeArgs()
    args.struct_size = C.sizeof(_lib.StMotChallengeArgs)
    args.num_frames, args.num_gt, args.num_pred = len(t['frame_no']), NG, NP_
    args.max_frame_objects = t['max_frame_objects']
    args.do_preproc = int(benchmark != 'MOT15')
    args.num_distractors = len(distractors)
    for k, d in enumerate(distractors):
        args.distractors[k] = int(d)
    args.num_ws_cells = int(t['frame_ws_off'][-1])
    call.bind(args, ('frame_gt_off', 'frame_pred_off', 'frame_ws_off'), ('gt_keep', 'pred_keep', 'status'))
    args.gt_rows, args.pred_rows = C.c_void_p(gt_file.data_ptr()), C.c_void_p(pred_file.data_ptr())
    call.workspace(args, call.workspace_bytes('st_mot_challenge_workspace_bytes', args))
    with call.stages():
        call.begin('st_mot_file_round')
        file_round(call.device_in('gt_rows'), _FILE_MODES['gt'], gt_file, call.device_out('status_gt'))
        file_round(call.device_in('pred_rows'), _FILE_MODES['pred'], pred_file, call.device_out('status_pred'))
        call.launch('st_mot_challenge_preprocess', C.byref(args))
    host = call.fetch()

    def row_of(kind, packed_row):      # (video, index among the rows as they were passed) of a packed row
        bounds = np.cumsum([0] + [len(o[kind]) for o in t['orders']])
        s = int(np.searchsorted(bounds, packed_row, 'right')) - 1
        return videos[s], int(t['orders'][s][kind][packed_row - bounds[s]])
    for kind, (name, total) in enumerate((('status_gt', NG), ('status_pred', NP_))):
        st = host[name]
        for bit, what in _FILE_STATUS_KINDS:
            if int(st[0]) & bit:
                video, row = row_of(kind, total - int(st[bit.bit_length()]))
                raise ValueError(f'MOTChallenge files: {what}: video {video!r}, {("ground-truth", "prediction")[kind]} row {row}')
        if st[0]:
            raise _lib.StError(f'st_mot_file_round failed on the device: status {int(st[0])}')
    if host['status'][0]:
        _raise_status('MOTChallenge preprocessing', CHALLENGE_STATUS_KINDS, host['status'], videos, t['frame_seq'],
                      t['frame_no'], ' (at most {n} ground-truth and {n} prediction rows per frame)')
    return dict(gt_file=gt_file, pred_file=pred_file, gt_keep=host['gt_keep'], pred_keep=host['pred_keep'],
                orders=t['orders'], sorted=srt, videos=videos, call=call)


def motchallenge_keep_masks(gts, preds, benchmark='MOT17', device=None, videos=None, timing=False):
    """protocol='trackeval' ahead of the scorers, for every sequence (or sweep member) in ONE call: the rows are
    uploaded once, st_mot_file_round turns them into what a reader of the MOTChallenge files gets
    (metrics.motchallenge_file_rows, the specification), st_mot_challenge_preprocess applies TrackEval's preprocessing
    to those (metrics.motchallenge_preprocess), and the keep bytes come back with one wait and one copy.
    gts / preds: lists of row arrays, gt (n, 6 .. 9) = (frame, id, x, y, w, h[, conf, class, visibility]; conf 1 and
    class 1 where absent), pred (m, 6 .. 7), rows in any order.  Returns one (gt_keep (n,), pred_keep (m,)) pair of
    boolean arrays per sequence, over the rows as they were passed.  videos: the names for error messages.
    timing: returns (masks, dict) with the stages' device time (HIP events) and the host clock of the call's parts."""
    r = _challenge_device(gts, preds, benchmark, device, videos, timing)
    out = _keep_masks(r['orders'], (r['gt_keep'], r['pred_keep']))
    return (out, r['call'].timing_dict()) if timing else out


def evaluate_motchallenge(gts, preds, benchmark='MOT17', iou_thr=0.5, metrics=('HOTA', 'CLEAR', 'Identity'), device=None,
                          videos=None, timing=False):
    """MOTDroneMetrics(protocol='trackeval', backend='device'): the sequences through _challenge_device, then the rows
    it keeps through the four scoring stages (evaluate_packed).  The scorers' tables come from the frame and id columns,
    truncated on the host; the rounded boxes are gathered on the device and never visit the host.  Returns one dict per
    sequence as evaluate_packed does; timing: (results, dict) with both parts' figures."""
    r = _challenge_device(gts, preds, benchmark, device, videos, timing)
    names = r['videos']
    keys = names if sorted(set(names)) == names else list(range(len(names)))      # pack_sequences sorts its videos
    kept, by_video = [], ({}, {})
    for kind, keep in enumerate((r['gt_keep'], r['pred_keep'])):
        kept.append(np.nonzero(keep)[0])
        r0 = 0
        for s, seq in enumerate(r['sorted']):
            rows, frames, _ = seq[kind]
            m = keep[r0:r0 + len(rows)] != 0
            head = np.zeros((int(m.sum()), 6))
            head[:, 0], head[:, 1] = frames[m], np.trunc(rows[m, 1])
            by_video[kind][keys[s]] = head
            r0 += len(rows)
    packed = pack_sequences(*by_video)
    dev = r['call'].dev
    boxes = [src[torch.from_numpy(idx).to(dev)][:, 2:6].contiguous() for src, idx in zip((r['gt_file'], r['pred_file']), kept)]
    res = evaluate_packed(packed, iou_thr, metrics, dev, timing=timing, device_boxes=boxes)
    if timing:
        res, t = res
        challenge = r['call'].timing_dict()
        t['challenge'] = {k: challenge[k] for k in ('stages_ms', 'host_prepare_s', 'device_and_copies_s')}
        return res, t
    return res


def image_space_rows(frames, rows, ids, n):
    """Tracker outputs on the host - frames (T, B), rows (T, B, M, row floats), ids (T, B, M), n (T, B), views allowed -
    -> one (R, 6) fp64 array per sequence: (frame, id, x, y, w, h) of every output row, in step order, in IMAGE
    space: the tracker's rows carry depth-scaled boxes, which are scaled back about their centres by 1 / scale
    (the row's scale column) with the fp32 operations of mot.scale_bbox, as every product path does before a box is
    reported or scored.  The ground truth they are scored against is the image-space one MOTDroneMetrics uses.
    Shared by TrackCollector.prediction_rows and sweep.SweepResult.prediction_rows."""
    from .records import TRACK_ROW
    two = np.float32(2.0)
    T, B = n.shape
    out = []
    for b in range(B):
        parts = []
        for t in range(T):
            k = int(n[t, b])
            if k <= 0:
                continue
            r = rows[t, b, :k]
            inv = np.float32(1.0) / r[:, TRACK_ROW.scale]
            cx, cy = (r[:, 0] + r[:, 2]) / two, (r[:, 1] + r[:, 3]) / two
            w, h = (r[:, 2] - r[:, 0]) * inv, (r[:, 3] - r[:, 1]) * inv
            box = np.stack([cx - w / two, cy - h / two, cx + w / two, cy + h / two], 1).astype(np.float64)
            parts.append(np.column_stack([np.full(k, frames[t, b], np.float64), ids[t, b, :k].astype(np.float64),
                                          box[:, 0], box[:, 1], box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]]))
        out.append(np.concatenate(parts) if parts else np.zeros((0, 6)))
    return out


class TrackCollector:
    """Collects the per-step outputs of a BatchedGpuTracker run on the device and brings them to the host with ONE
    device-to-host copy per run (to_host), not one per step."""

    def __init__(self):
        self.frames, self._rows, self._ids, self._n = [], [], [], []

    def add(self, frame_ids, rows, ids, n):
        """frame_ids: the step's frame number of every sequence (host ints); rows / ids / n: what step() returned
        (the tracker reuses these buffers, so they are copied, device to device)."""
        self.frames.append(np.asarray(frame_ids, dtype=np.int64).reshape(-1))
        self._rows.append(rows.detach().clone())
        self._ids.append(ids.detach().clone())
        self._n.append(n.detach().clone())

    def to_host(self):
        """-> frames (T, B), rows (T, B, M, row floats) float32, ids (T, B, M) int64, n (T, B) int32."""
        rows, ids, n = torch.stack(self._rows), torch.stack(self._ids), torch.stack(self._n)
        parts = [t.contiguous().view(torch.uint8).reshape(-1) for t in (ids, rows, n)]
        flat = torch.cat(parts).cpu().numpy()          # the run's one device-to-host copy
        a, b = parts[0].numel(), parts[0].numel() + parts[1].numel()
        return (np.stack(self.frames), flat[a:b].view(np.float32).reshape(tuple(rows.shape)),
                flat[:a].view(np.int64).reshape(tuple(ids.shape)), flat[b:].view(np.int32).reshape(tuple(n.shape)))

    def prediction_rows(self):
        """One (R, 6) fp64 array per sequence: image_space_rows of the run (to_host)."""
        return image_space_rows(*self.to_host())


def evaluate_sweep(predictions, gt, iou_thr=0.5, metrics=('HOTA', 'CLEAR', 'Identity'), device=None, backend='device',
                   postprocess=None, protocol='rows', benchmark='MOT17'):
    """Scores the B prediction sets of a batched tracker run (a TrackCollector, or a list of B row arrays) against one
    ground-truth row array (shared) or a list of B of them.  Returns B dicts as evaluate_packed does.  A collector's
    rows are scaled back to image space (TrackCollector.prediction_rows), so the ground truth is the image-space one;
    row arrays passed directly are scored as they are.
    backend='host' scores the same rows with metrics.clear_identity / metrics.hota (the reference of the tests).
    postprocess: any entry with forward_many(list of row arrays) -> list - a tracklets.InterpolateTracklets, an
    aflink.AppearanceFreeLink - or a list of them, applied in order over the B prediction sets before they are scored,
    each through one forward_many call on its own backend; 6-column rows (a collector's) get the score 1.0 first.
    protocol='trackeval': what MOTDroneMetrics(protocol='trackeval', benchmark=...) scores - the MOTChallenge files'
    values after TrackEval's preprocessing (metrics.motchallenge_file_rows / motchallenge_preprocess; on the device
    evaluate_motchallenge, one call for all B members).  The ground truth may then carry 9 columns (conf, class,
    visibility); without them every row has conf 1, class 1."""
    from . import metrics as M
    if protocol not in M.PROTOCOLS:
        raise ValueError(f'evaluate_sweep: protocol must be one of {M.PROTOCOLS}, got {protocol!r}')
    M.motchallenge_distractors(benchmark)
    preds = predictions.prediction_rows() if isinstance(predictions, TrackCollector) else list(predictions)
    if postprocess is not None:
        preds = [np.asarray(p, dtype=np.float64).reshape(-1, np.shape(p)[-1] if np.size(p) else 7) for p in preds]
        preds = [np.column_stack([p, np.ones(len(p))]) if p.shape[1] == 6 else p for p in preds]
        for method in (postprocess if isinstance(postprocess, (list, tuple)) else [postprocess]):
            preds = method.forward_many(preds)
    gts = list(gt) if isinstance(gt, (list, tuple)) else [gt] * len(preds)
    if len(gts) != len(preds):
        raise ValueError(f'evaluate_sweep: {len(preds)} prediction sets against {len(gts)} ground-truth sets')
    if backend == 'host':
        if protocol == 'trackeval':
            ks = list(range(len(preds)))
            g_, p_ = M.motchallenge_scored_rows(dict(zip(ks, gts)), dict(zip(ks, preds)), ks, benchmark)
            gts, preds = [g_[k] for k in ks], [p_[k] for k in ks]
        return [dict(clear_identity=M.clear_identity(g, p, iou_thr), hota=M.hota(g, p) if 'HOTA' in metrics else None)
                for g, p in zip(gts, preds)]
    if backend != 'device':
        raise ValueError(f"evaluate_sweep: backend must be 'host' or 'device', got {backend!r}")
    if protocol == 'trackeval':
        return evaluate_motchallenge(gts, preds, benchmark, iou_thr, metrics, device)
    return evaluate_packed(pack_sequences(gts, preds), iou_thr, metrics, device)
