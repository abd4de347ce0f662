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
import time

import numpy as np
import torch

from . import _lib
from ._lib import StMotArgs, check, current_stream

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
    gt_parts, pr_parts, frame_no, frame_seq, fg, fp_ = [], [], [], [], [0], [0]
    seq_frame_off, seq_ng, seq_nt, gt_ids, tr_ids = [0], [], [], [], []
    ngt = npr = 0
    for s, v in enumerate(videos):
        g, gfr, gu = _sort_and_compact(_rows6(gt_by_video.get(v, ())), v, 'ground-truth')
        p, pfr, pu = _sort_and_compact(_rows6(pred_by_video.get(v, ())), v, 'prediction')
        frames = np.union1d(gfr, pfr)
        gt_parts.append(g)
        pr_parts.append(p)
        frame_no.append(frames)
        frame_seq.append(np.full(len(frames), s, np.int32))
        fg.append(ngt + np.searchsorted(gfr, frames, 'right'))
        fp_.append(npr + np.searchsorted(pfr, frames, 'right'))
        ngt, npr = ngt + len(g), npr + len(p)
        seq_frame_off.append(seq_frame_off[-1] + len(frames))
        seq_ng.append(len(gu))
        seq_nt.append(len(pu))
        gt_ids.append(gu)
        tr_ids.append(pu)
    if max(ngt, npr, seq_frame_off[-1]) >= 2 ** 31 - 1:
        raise ValueError(f'pack_sequences: {ngt} ground-truth rows, {npr} prediction rows, {seq_frame_off[-1]} frames: the '
                         f'offset tables are 32-bit')
    out = dict(videos=videos, gt_ids=gt_ids, tr_ids=tr_ids)
    out['gt_rows'] = np.ascontiguousarray(np.concatenate(gt_parts)) if videos else np.zeros((0, 6))
    out['pred_rows'] = np.ascontiguousarray(np.concatenate(pr_parts)) if videos else np.zeros((0, 6))
    out['seq_frame_off'] = np.asarray(seq_frame_off, np.int32)
    out['frame_seq'] = np.concatenate(frame_seq + [np.zeros(0, np.int32)]).astype(np.int32)
    out['frame_no'] = np.concatenate(frame_no + [np.zeros(0, np.int64)]).astype(np.int64)
    out['frame_gt_off'] = np.concatenate([np.atleast_1d(a) for a in fg]).astype(np.int32)
    out['frame_pred_off'] = np.concatenate([np.atleast_1d(a) for a in fp_]).astype(np.int32)
    G, P = np.diff(out['frame_gt_off']).astype(np.int64), np.diff(out['frame_pred_off']).astype(np.int64)
    out['frame_pair_off'] = np.concatenate([[0], np.cumsum(G * P)]).astype(np.int64)
    out['seq_ng'], out['seq_nt'] = np.asarray(seq_ng, np.int32), np.asarray(seq_nt, np.int32)
    ng, nt = out['seq_ng'].astype(np.int64), out['seq_nt'].astype(np.int64)
    out['seq_gid_off'] = np.concatenate([[0], np.cumsum(ng)]).astype(np.int64)
    out['seq_tid_off'] = np.concatenate([[0], np.cumsum(nt)]).astype(np.int64)
    out['seq_mat_off'] = np.concatenate([[0], np.cumsum(ng * nt)]).astype(np.int64)
    out['max_frame_objects'] = int(max(G.max(initial=0), P.max(initial=0)))
    return out


class _Layout:
    """Arrays side by side in one byte buffer, every one at a multiple of 256 bytes."""

    def __init__(self):
        self.items, self.size = {}, 0

    def add(self, name, shape, dtype):
        dtype = np.dtype(dtype)
        n = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        self.items[name] = (self.size, tuple(int(v) for v in shape), dtype)
        self.size += (n + 255) // 256 * 256 + 256

    def view(self, buf, name):
        off, shape, dtype = self.items[name]
        n = int(np.prod(shape, dtype=np.int64))
        return buf[off:off + n * dtype.itemsize].view(dtype).reshape(shape)


def _device_view(layout, buf, name):
    """_Layout.view for the device copy of the buffer (a uint8 tensor)."""
    off, shape, dtype = layout.items[name]
    n = int(np.prod(shape, dtype=np.int64))
    return buf[off:off + n * dtype.itemsize].view(getattr(torch, dtype.name)).view(shape)


def _where(packed, status, kind):
    f = int(packed['frame_no'].shape[0]) - int(status[1 + kind])
    return packed['videos'][int(packed['frame_seq'][f])], int(packed['frame_no'][f])


def _raise_status(packed, status):
    bits = int(status[0])
    for kind, (bit, what) in enumerate(STATUS_KINDS):
        if bits & bit:
            video, frame = _where(packed, status, kind)
            msg = f'MOT evaluation: {what}: video {video!r}, frame {frame}'
            if bit == 8:
                msg += f' (at most {max_frame_objects()} ground-truth and {max_frame_objects()} prediction rows per frame)'
            raise ValueError(msg) if bit in (1, 2, 8) else _lib.StError(msg)
    raise _lib.StError(f'MOT evaluation failed on the device: status {bits}')


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
    t_start = time.perf_counter()
    metrics = [metrics] if isinstance(metrics, str) else list(metrics)
    do_hota = 'HOTA' in metrics
    do_clear = 'CLEAR' in metrics or 'Identity' in metrics
    if not (do_hota or do_clear):
        raise ValueError(f'evaluate_packed: nothing to compute for metrics {metrics}')
    if not torch.cuda.is_available():
        raise RuntimeError('the device backend of the MOT evaluation runs on the HIP path only (csrc/mot_eval.hip) and '
                           'no CUDA (ROCm) device is available; use backend=\'host\'')
    lib = _lib.load()
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.type != 'cuda':
        raise RuntimeError(f'the device backend of the MOT evaluation needs a CUDA (ROCm) device, got {dev}')
    alphas = np.ascontiguousarray(M.HOTA_ALPHAS if alphas is None else alphas, dtype=np.float64)
    B, F, A = len(packed['videos']), len(packed['frame_no']), len(alphas)
    if B == 0:
        return []
    NG, NP_ = len(packed['gt_rows']), len(packed['pred_rows'])
    ids_g, ids_t, cells = int(packed['seq_gid_off'][-1]), int(packed['seq_tid_off'][-1]), int(packed['seq_mat_off'][-1])

    # ---- one upload
    lin = _Layout()
    host_in = dict(gt_rows=packed['gt_rows'], pred_rows=packed['pred_rows'], alphas=alphas, **{k: packed[k] for k in _TABLES})
    for k, v in host_in.items():
        lin.add(k, v.shape, v.dtype)
    hbuf = np.zeros(lin.size, np.uint8)
    for k, v in host_in.items():
        lin.view(hbuf, k)[...] = v
    t_prep = time.perf_counter()
    dbuf = torch.from_numpy(hbuf).to(dev)
    if device_boxes is not None:
        for name, boxes in zip(('gt_rows', 'pred_rows'), device_boxes):
            off, (n, _), _ = lin.items[name]
            if tuple(boxes.shape) != (n, 4) or boxes.dtype != torch.float64 or boxes.device != dev:
                raise ValueError(f'evaluate_packed: device_boxes for {name} must be ({n}, 4) float64 on {dev}')
            if n:
                dbuf[off:off + n * 48].view(torch.float64).view(n, 6)[:, 2:6] = boxes

    lout = _Layout()
    for name, shape, dt in (('status', (8,), np.int32), ('gt_count', (ids_g,), np.int32), ('tr_count', (ids_t,), np.int32),
                            ('id_potential', (cells,), np.int32), ('hota_potential', (cells,), np.float64),
                            ('gt_frames', (ids_g,), np.int32), ('gt_matched', (ids_g,), np.int32),
                            ('gt_frag', (ids_g,), np.int32), ('clear_counts', (B, 4), np.int32),
                            ('motp_sum', (B,), np.float64), ('hota_counts', (B, A, 3), np.int32),
                            ('hota_sums', (B, A, 4), np.float64)):
        lout.add(name, shape, dt)
    obuf = torch.zeros(lout.size, dtype=torch.uint8, device=dev)

    args = StMotArgs()
    args.struct_size = C.sizeof(StMotArgs)
    args.num_seqs, args.num_frames, args.num_gt, args.num_pred, args.num_alphas = B, F, NG, NP_, A
    args.max_frame_objects = int(packed['max_frame_objects'])
    args.flags = (ST_MOT_CLEAR if do_clear else 0) | (ST_MOT_HOTA if do_hota else 0)
    args.num_pairs, args.num_cells, args.num_gids, args.num_tids = int(packed['frame_pair_off'][-1]), cells, ids_g, ids_t
    args.iou_thr = float(iou_thr)
    for k in host_in:
        setattr(args, k, C.c_void_p(dbuf.data_ptr() + lin.items[k][0]))
    for k in lout.items:
        setattr(args, k, C.c_void_p(obuf.data_ptr() + lout.items[k][0]))
    args.ws, args.ws_bytes = None, 0
    nbytes = int(lib.st_mot_workspace_bytes(C.byref(args)))
    if nbytes == 0:
        raise _lib.StError('st_mot_workspace_bytes: invalid sizes')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    args.ws, args.ws_bytes = C.c_void_p(ws.data_ptr()), nbytes

    stages = [('st_mot_similarity', lib.st_mot_similarity), ('st_mot_walk', lib.st_mot_walk)]
    if do_hota:
        stages += [('st_mot_hota_match', lib.st_mot_hota_match), ('st_mot_hota_accumulate', lib.st_mot_hota_accumulate)]
    over_limit = False
    with torch.cuda.device(dev):
        stream = current_stream()
        events = [torch.cuda.Event(enable_timing=True) for _ in range(len(stages) + 1)] if timing else None
        for i, (name, fn) in enumerate(stages):
            if timing:
                events[i].record()
            LAUNCHES[name] += 1
            rc = fn(C.byref(args), stream)
            if name == 'st_mot_similarity' and rc == -1 and args.max_frame_objects > max_frame_objects():
                over_limit = True      # the checks were launched: the status word names the frame
                break
            check(rc, name)
        if timing and not over_limit:
            events[-1].record()
    host = obuf.cpu().numpy()          # the one wait and the one copy back
    t_back = time.perf_counter()
    status = lout.view(host, 'status')
    if status[0] or over_limit:
        _raise_status(packed, status)
    o = {k: lout.view(host, k) for k in lout.items}
    sim = None
    if return_arrays:
        off = int(lib.st_mot_workspace_sim_offset(C.byref(args)))
        sim = ws[off:off + 8 * args.num_pairs].cpu().numpy().view(np.float64)

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
    if timing:
        t_end = time.perf_counter()
        return results, dict(stages_ms={name: events[i].elapsed_time(events[i + 1]) for i, (name, _) in enumerate(stages)},
                             host_prepare_s=t_prep - t_start, device_and_copies_s=t_back - t_prep,
                             host_finish_s=t_end - t_back, total_s=t_end - t_start)
    return results


KITTI_STATUS_KINDS = ((1, 0, 'a non-finite box'), (8, 3, 'more rows of one class in one frame than a launch holds'),
                      (32, 5, 'a workspace slot that is too small'))
_KITTI_LDS_CELLS = 64 * 64      # frames with more cells than this (rows of all classes) get a workspace slot (section 16)
_KITTI_MAX_DISTRACTORS = 4


def _sorted_by_frame(rows, width):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, width)
    frames = rows[:, 0].astype(np.int64)
    order = np.argsort(frames, kind='stable')
    return rows[order], frames[order], order


def kitti_keep_masks(sequences, classes, max_occlusion=2, max_truncation=0, min_height=25, match_thr=0.5, ignore_thr=0.5,
                     device=None, videos=None, timing=False):
    """KITTI's preprocessing (metrics.kitti_preprocess, the specification) of every sequence and class in ONE launch of
    st_mot_kitti_preprocess: one upload, one launch, one wait and copy back.
    sequences: a list of (gt_rows (n, 9), pred_rows (m, 8), ignore_boxes (k, 5)) in kitti_preprocess's layouts, rows in
    any order; classes: a list of (class id, distractor ids).  Returns one (gt_keep (C, n), pred_keep (C, m)) pair of
    boolean arrays per sequence, over the rows as they were passed.  videos: the sequences' names for error messages.
    timing: returns (masks, dict) with the stage's device time (HIP events) and the host clock of the call's parts."""
    t_start = time.perf_counter()
    if not torch.cuda.is_available():
        raise RuntimeError('the device backend of the KITTI preprocessing runs on the HIP path only (csrc/mot_eval.hip) '
                           'and no CUDA (ROCm) device is available; use backend=\'host\'')
    lib = _lib.load()
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.type != 'cuda':
        raise RuntimeError(f'the device backend of the KITTI preprocessing needs a CUDA (ROCm) device, got {dev}')
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

    # ---- host tables: the frames of a sequence are the union of its three row kinds' frame numbers
    parts, orders, frame_no, frame_seq = ([], [], []), [], [], []
    offs = ([0], [0], [0])
    totals = [0, 0, 0]
    for s, seq in enumerate(sequences):
        srt = [_sorted_by_frame(rows, w) for rows, w in zip(seq, (9, 8, 5))]
        frames = np.unique(np.concatenate([fr for _, fr, _ in srt]))
        for k, (rows, fr, _) in enumerate(srt):
            parts[k].append(rows)
            offs[k].append(totals[k] + np.searchsorted(fr, frames, 'right'))
            totals[k] += len(rows)
        orders.append([o for _, _, o in srt])
        frame_no.append(frames)
        frame_seq.append(np.full(len(frames), s, np.int32))
    frame_no, frame_seq = np.concatenate(frame_no), np.concatenate(frame_seq)
    F = len(frame_no)
    if max(totals + [F * C_]) >= 2 ** 31 - 1:
        raise ValueError(f'kitti_keep_masks: {totals} rows, {F} frames x {C_} classes: the offset tables are 32-bit')
    host_in = dict(gt_rows=np.concatenate(parts[0]), pred_rows=np.concatenate(parts[1]), ignore_rows=np.concatenate(parts[2]),
                   class_table=table)
    for k, name in enumerate(('frame_gt_off', 'frame_pred_off', 'frame_ignore_off')):
        host_in[name] = np.concatenate([np.atleast_1d(a) for a in offs[k]]).astype(np.int32)
    G, P = np.diff(host_in['frame_gt_off']).astype(np.int64), np.diff(host_in['frame_pred_off']).astype(np.int64)
    host_in['frame_ws_off'] = np.concatenate([[0], np.cumsum(np.where(G * P > _KITTI_LDS_CELLS, G * P, 0))]).astype(np.int64)
    NG, NP_, NI = totals

    # ---- one upload
    lin = _Layout()
    for k, v in host_in.items():
        lin.add(k, v.shape, v.dtype)
    hbuf = np.zeros(lin.size, np.uint8)
    for k, v in host_in.items():
        lin.view(hbuf, k)[...] = v
    t_prep = time.perf_counter()
    dbuf = torch.from_numpy(hbuf).to(dev)
    lout = _Layout()
    for name, shape, dt in (('status', (8,), np.int32), ('gt_keep', (C_, NG), np.uint8), ('pred_keep', (C_, NP_), np.uint8)):
        lout.add(name, shape, dt)
    obuf = torch.empty(lout.size, dtype=torch.uint8, device=dev)       # the stage zeroes what it does not write

    args = _lib.StMotKittiArgs()
    args.struct_size = C.sizeof(_lib.StMotKittiArgs)
    args.num_frames, args.num_classes, args.num_gt, args.num_pred, args.num_ignore = F, C_, NG, NP_, NI
    args.max_frame_objects = int(max(G.max(initial=0), P.max(initial=0)))
    args.num_ws_cells = int(host_in['frame_ws_off'][-1])
    args.max_occlusion, args.max_truncation, args.min_height = float(max_occlusion), float(max_truncation), float(min_height)
    args.match_thr, args.ignore_thr = float(match_thr), float(ignore_thr)
    for k in host_in:
        setattr(args, k, C.c_void_p(dbuf.data_ptr() + lin.items[k][0]))
    for k in lout.items:
        setattr(args, k, C.c_void_p(obuf.data_ptr() + lout.items[k][0]))
    nbytes = int(lib.st_mot_kitti_workspace_bytes(C.byref(args)))
    if nbytes == 0:
        raise _lib.StError('st_mot_kitti_workspace_bytes: invalid sizes')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    args.ws, args.ws_bytes = C.c_void_p(ws.data_ptr()), nbytes
    with torch.cuda.device(dev):
        events = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if timing else None
        if timing:
            events[0].record()
        LAUNCHES['st_mot_kitti_preprocess'] += 1
        check(lib.st_mot_kitti_preprocess(C.byref(args), current_stream()), 'st_mot_kitti_preprocess')
        if timing:
            events[1].record()
    host = obuf.cpu().numpy()          # the one wait and the one copy back
    t_back = time.perf_counter()
    status = lout.view(host, 'status')
    if status[0]:
        for bit, kind, what in KITTI_STATUS_KINDS:
            if int(status[0]) & bit:
                f = F - int(status[1 + kind])
                msg = f'KITTI preprocessing: {what}: video {videos[int(frame_seq[f])]!r}, frame {int(frame_no[f])}'
                if bit == 8:
                    msg += (f' (at most {max_frame_objects()} ground-truth rows of a class and its distractors and '
                            f'{max_frame_objects()} prediction rows of the class per frame)')
                raise ValueError(msg) if bit in (1, 8) else _lib.StError(msg)
        raise _lib.StError(f'KITTI preprocessing failed on the device: status {int(status[0])}')
    gk, pk = lout.view(host, 'gt_keep'), lout.view(host, 'pred_keep')
    out, g0, p0 = [], 0, 0
    for s, seq in enumerate(sequences):
        og, op_, _ = orders[s]
        a, b = np.zeros((C_, len(og)), bool), np.zeros((C_, len(op_)), bool)
        a[:, og] = gk[:, g0:g0 + len(og)] != 0
        b[:, op_] = pk[:, p0:p0 + len(op_)] != 0
        g0, p0 = g0 + len(og), p0 + len(op_)
        out.append((a, b))
    if timing:
        t_end = time.perf_counter()
        return out, dict(stages_ms={'st_mot_kitti_preprocess': events[0].elapsed_time(events[1])},
                         host_prepare_s=t_prep - t_start, device_and_copies_s=t_back - t_prep,
                         host_finish_s=t_end - t_back, total_s=t_end - t_start)
    return out


CHALLENGE_STATUS_KINDS = ((1, 0, 'a non-finite box'), (8, 3, 'more rows in one frame than a launch holds'),
                          (32, 5, 'a workspace slot that is too small'))
FILE_COPY, FILE_TRUNCATE, FILE_ROUND3 = 0, 1, 2          # ST_MOT_FILE_* of include/stereotrack.h section 21
_FILE_MODES = dict(gt=(FILE_TRUNCATE,) * 8, pred=(FILE_TRUNCATE,) * 2 + (FILE_ROUND3,) * 5)
_FILE_STATUS_KINDS = ((1, 0, 'a non-finite value'), (2, 1, 'a value of 2^43 or more in a column written with %.3f'))


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
    t_start = time.perf_counter()
    distractors = M.motchallenge_distractors(benchmark)
    if not torch.cuda.is_available():
        raise RuntimeError('the device backend of the MOTChallenge protocol runs on the HIP path only (csrc/mot_eval.hip) '
                           'and no CUDA (ROCm) device is available; use backend=\'host\'')
    lib = _lib.load()
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.type != 'cuda':
        raise RuntimeError(f'the device backend of the MOTChallenge protocol needs a CUDA (ROCm) device, got {dev}')
    gts, preds = list(gts), list(preds)
    if len(gts) != len(preds):
        raise ValueError(f'MOTChallenge protocol: {len(gts)} ground-truth sets against {len(preds)} prediction sets')
    videos = list(range(len(gts))) if videos is None else list(videos)

    # ---- host tables, from the truncated frame column only; the class check needs the class column's integer part
    parts, orders, frames_of, frame_no, frame_seq = ([], []), [], [], [], []
    offs, totals = ([0], [0]), [0, 0]
    for s, (g, p) in enumerate(zip(gts, preds)):
        g, p = M.motchallenge_gt8(g), M.motchallenge_pred7(p)
        M._require_finite(g, 'ground-truth', videos[s])
        M._require_finite(p, 'prediction', videos[s])
        cls = np.trunc(g[:, 7])
        bad = np.nonzero((cls < 1) | (cls > M.MOTCHALLENGE_NUM_CLASSES))[0]
        if len(bad):
            raise ValueError(f'MOTChallenge preprocessing: video {videos[s]!r}: ground-truth row {int(bad[0])} has class '
                             f'{cls[bad[0]]:g}, outside 1..{M.MOTCHALLENGE_NUM_CLASSES}')
        srt = []
        for rows in (g, p):
            fr = np.trunc(rows[:, 0]).astype(np.int64)
            order = np.argsort(fr, kind='stable')
            srt.append((rows[order], fr[order], order))
        frames = np.union1d(srt[0][1], srt[1][1])
        for k, (rows, fr, _) in enumerate(srt):
            parts[k].append(rows)
            offs[k].append(totals[k] + np.searchsorted(fr, frames, 'right'))
            totals[k] += len(rows)
        orders.append((srt[0][2], srt[1][2]))
        frames_of.append((srt[0][1], srt[1][1]))
        frame_no.append(frames)
        frame_seq.append(np.full(len(frames), s, np.int32))
    frame_no = np.concatenate(frame_no + [np.zeros(0, np.int64)])
    frame_seq = np.concatenate(frame_seq + [np.zeros(0, np.int32)])
    F, (NG, NP_) = len(frame_no), totals
    if max(NG, NP_, F) >= 2 ** 31 - 1:
        raise ValueError(f'MOTChallenge protocol: {NG} ground-truth rows, {NP_} prediction rows, {F} frames: the offset tables '
                         f'are 32-bit')
    host_in = dict(gt_rows=np.concatenate(parts[0] + [np.zeros((0, 8))]), pred_rows=np.concatenate(parts[1] + [np.zeros((0, 7))]))
    for k, name in enumerate(('frame_gt_off', 'frame_pred_off')):
        host_in[name] = np.concatenate([np.atleast_1d(a) for a in offs[k]]).astype(np.int32)
    G, P = np.diff(host_in['frame_gt_off']).astype(np.int64), np.diff(host_in['frame_pred_off']).astype(np.int64)
    host_in['frame_ws_off'] = np.concatenate([[0], np.cumsum(np.where(G * P > _KITTI_LDS_CELLS, G * P, 0))]).astype(np.int64)

    # ---- one upload
    lin = _Layout()
    for k, v in host_in.items():
        lin.add(k, v.shape, v.dtype)
    hbuf = np.zeros(lin.size, np.uint8)
    for k, v in host_in.items():
        lin.view(hbuf, k)[...] = v
    t_prep = time.perf_counter()
    dbuf = torch.from_numpy(hbuf).to(dev)
    lout = _Layout()
    for name, shape, dt in (('status_gt', (8,), np.int32), ('status_pred', (8,), np.int32), ('status', (8,), np.int32),
                            ('gt_keep', (NG,), np.uint8), ('pred_keep', (NP_,), np.uint8)):
        lout.add(name, shape, dt)
    obuf = torch.empty(lout.size, dtype=torch.uint8, device=dev)       # the stages zero what they do not write
    dview = lambda name: _device_view(lin, dbuf, name)
    oview = lambda name: _device_view(lout, obuf, name)
    gt_file = torch.empty((NG, 8), dtype=torch.float64, device=dev)    # the rows a reader of the files gets
    pred_file = torch.empty((NP_, 7), dtype=torch.float64, device=dev)

    args = _lib.StMotChallengeArgs()
    args.struct_size = C.sizeof(_lib.StMotChallengeArgs)
    args.num_frames, args.num_gt, args.num_pred = F, NG, NP_
    args.max_frame_objects = int(max(G.max(initial=0), P.max(initial=0)))
    args.do_preproc = int(benchmark != 'MOT15')
    args.num_distractors = len(distractors)
    for k, d in enumerate(distractors):
        args.distractors[k] = int(d)
    args.num_ws_cells = int(host_in['frame_ws_off'][-1])
    args.gt_rows, args.pred_rows = C.c_void_p(gt_file.data_ptr()), C.c_void_p(pred_file.data_ptr())
    for k in ('frame_gt_off', 'frame_pred_off', 'frame_ws_off'):
        setattr(args, k, C.c_void_p(dbuf.data_ptr() + lin.items[k][0]))
    for k in ('gt_keep', 'pred_keep', 'status'):
        setattr(args, k, C.c_void_p(obuf.data_ptr() + lout.items[k][0]))
    nbytes = int(lib.st_mot_challenge_workspace_bytes(C.byref(args)))
    if nbytes == 0:
        raise _lib.StError('st_mot_challenge_workspace_bytes: invalid sizes')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    args.ws, args.ws_bytes = C.c_void_p(ws.data_ptr()), nbytes
    with torch.cuda.device(dev):
        events = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timing else None
        if timing:
            events[0].record()
        file_round(dview('gt_rows'), _FILE_MODES['gt'], gt_file, oview('status_gt'))
        file_round(dview('pred_rows'), _FILE_MODES['pred'], pred_file, oview('status_pred'))
        if timing:
            events[1].record()
        LAUNCHES['st_mot_challenge_preprocess'] += 1
        check(lib.st_mot_challenge_preprocess(C.byref(args), current_stream()), 'st_mot_challenge_preprocess')
        if timing:
            events[2].record()
    host = obuf.cpu().numpy()          # the one wait and the one copy back
    t_back = time.perf_counter()

    def row_of(kind, packed_row):      # (video, index among the rows as they were passed) of a packed row
        bounds = np.cumsum([0] + [len(o[kind]) for o in orders])
        s = int(np.searchsorted(bounds, packed_row, 'right')) - 1
        return videos[s], int(orders[s][kind][packed_row - bounds[s]])
    for kind, (name, total) in enumerate((('status_gt', NG), ('status_pred', NP_))):
        st = lout.view(host, name)
        for bit, k, what in _FILE_STATUS_KINDS:
            if int(st[0]) & bit:
                video, row = row_of(kind, total - int(st[1 + k]))
                raise ValueError(f'MOTChallenge files: {what}: video {video!r}, {("ground-truth", "prediction")[kind]} row {row}')
        if st[0]:
            raise _lib.StError(f'st_mot_file_round failed on the device: status {int(st[0])}')
    status = lout.view(host, 'status')
    if status[0]:
        for bit, kind, what in CHALLENGE_STATUS_KINDS:
            if int(status[0]) & bit:
                f = F - int(status[1 + kind])
                msg = f'MOTChallenge preprocessing: {what}: video {videos[int(frame_seq[f])]!r}, frame {int(frame_no[f])}'
                if bit == 8:
                    msg += f' (at most {max_frame_objects()} ground-truth and {max_frame_objects()} prediction rows per frame)'
                raise ValueError(msg) if bit in (1, 8) else _lib.StError(msg)
        raise _lib.StError(f'MOTChallenge preprocessing failed on the device: status {int(status[0])}')
    out = dict(gt_file=gt_file, pred_file=pred_file, gt_keep=lout.view(host, 'gt_keep'), pred_keep=lout.view(host, 'pred_keep'),
               orders=orders, frames_of=frames_of, sorted_rows=parts, videos=videos, device=dev)
    if timing:
        out['timing'] = dict(events=events, host_prepare_s=t_prep - t_start, device_and_copies_s=t_back - t_prep, t_back=t_back)
    return out


def _challenge_stage_ms(r):
    ev = r['timing']['events']
    return {'st_mot_file_round': ev[0].elapsed_time(ev[1]), 'st_mot_challenge_preprocess': ev[1].elapsed_time(ev[2])}


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
    out, g0, p0 = [], 0, 0
    for og, op_ in r['orders']:
        a, b = np.zeros(len(og), bool), np.zeros(len(op_), bool)
        a[og] = r['gt_keep'][g0:g0 + len(og)] != 0
        b[op_] = r['pred_keep'][p0:p0 + len(op_)] != 0
        g0, p0 = g0 + len(og), p0 + len(op_)
        out.append((a, b))
    if timing:
        t = r['timing']
        t_end = time.perf_counter()
        return out, dict(stages_ms=_challenge_stage_ms(r), host_prepare_s=t['host_prepare_s'],
                         device_and_copies_s=t['device_and_copies_s'], host_finish_s=t_end - t['t_back'])
    return out


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
        for s, rows in enumerate(r['sorted_rows'][kind]):
            m = keep[r0:r0 + len(rows)] != 0
            head = np.zeros((int(m.sum()), 6))
            head[:, 0], head[:, 1] = r['frames_of'][s][kind][m], np.trunc(rows[m, 1])
            by_video[kind][keys[s]] = head
            r0 += len(rows)
    packed = pack_sequences(*by_video)
    dev = r['device']
    boxes = [src[torch.from_numpy(idx).to(dev)][:, 2:6].contiguous() for src, idx in zip((r['gt_file'], r['pred_file']), kept)]
    res = evaluate_packed(packed, iou_thr, metrics, dev, timing=timing, device_boxes=boxes)
    if timing:
        res, t = res
        t['challenge'] = dict(stages_ms=_challenge_stage_ms(r), host_prepare_s=r['timing']['host_prepare_s'],
                              device_and_copies_s=r['timing']['device_and_copies_s'])
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
