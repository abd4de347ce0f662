"""Tracker-option sweeps: K option sets of OCSORTTracker_Disparity x V recorded videos tracked as K * V independent
sequences of ONE batched device tracker (batched_assoc.BatchedGpuTracker(options=...)), each video's whole detection
stream in one launch (BatchedGpuTracker.run), and scored by the device evaluator (mot_eval.evaluate_sweep).

    sweep = TrackerSweep(grid(match_iou_thr=[0.1, 0.3], num_tentatives=[1, 3]))
    for records in videos:                       # frame records of sequence.detect_shard / gather_shard_records
        sweep.add_video(records)
    result = sweep.run()
    scores = result.scores(gt_by_video)          # one dict per option set, combined over the videos
    k, options, best = result.best('HOTA')

Member order everywhere: (option set k, video v) -> k * V + v."""
import itertools
import warnings

import numpy as np
import torch

from . import _lib
from .records import (BOX, LABEL, REC_CAP, REC_COUNT, REC_DEPTH, REC_FLOATS, REC_HEADER, REC_SCALE, REC_SCALED_BOX,
                      REC_VALID, SCORE)


def _check_options(options, what):
    unknown = sorted(set(options) - set(_lib.TRACKER_OPTIONS))
    if unknown:
        raise ValueError(f'{what}: unknown tracker options {unknown} (known: {list(_lib.TRACKER_OPTIONS)})')


def grid(base=None, **lists):
    """The option dicts of the cartesian product of `lists` (option name -> list of values), each on top of `base`.
    Order: itertools.product over the keywords in the order they are given - the LAST keyword varies fastest.  Names
    outside _lib.TRACKER_OPTIONS raise ValueError."""
    base = dict(base or {})
    _check_options(base, 'grid: base')
    _check_options(lists, 'grid')
    names = list(lists)
    return [dict(base, **dict(zip(names, values))) for values in itertools.product(*(list(lists[k]) for k in names))]


def records_to_detections(records):
    """Frame records (F, max_det + 1, C >= 12; sequence.detect_shard / gather_shard_records, a tensor on any device or
    an array) -> (dets (F, max_det, 8) float32, counts (F,) int32) with the column rule of st_tracker_track_records:
    [depth-scaled box, score, label, depth, scale], the count from the header row, -1 for a record that is batch
    padding (valid flag 0)."""
    rec = records.detach().cpu().numpy() if torch.is_tensor(records) else np.asarray(records)
    if rec.ndim != 3 or rec.shape[1] < 2 or rec.shape[2] < REC_SCALED_BOX.stop:
        raise ValueError(f'frame records: expected (F, max_det + 1, >= {REC_SCALED_BOX.stop}) (the records must carry the '
                         f'scaled box), got {rec.shape}')
    rec = rec.astype(np.float32, copy=False)
    hdr, body = rec[:, REC_HEADER], rec[:, REC_HEADER + 1:]
    valid = hdr[:, REC_VALID] != 0
    if np.any(hdr[valid, REC_CAP].astype(np.int64) != body.shape[1]):
        raise ValueError(f'frame records: a record capacity differs from the {body.shape[1]} rows of the records')
    counts = np.where(valid, hdr[:, REC_COUNT].astype(np.int64), -1)
    if counts.max(initial=-1) > body.shape[1]:
        f = int(np.argmax(counts))
        raise ValueError(f'frame {f}: {counts[f]} detections kept but the detection buffer has {body.shape[1]} rows')
    dets = np.zeros(body.shape[:2] + (REC_FLOATS,), np.float32)
    dets[..., BOX] = body[..., REC_SCALED_BOX]
    for col in (SCORE, LABEL, REC_DEPTH, REC_SCALE):
        dets[..., col] = body[..., col]
    return dets, counts.astype(np.int32)


class TrackerSweep:
    """option_sets: the K option dicts (over _lib.TRACKER_OPTIONS; missing keys take BatchedGpuTracker's defaults).
    max_dets: detection rows per frame (None: the largest count of the videos added).  max_output_bytes: members are
    tracked in groups whose device output (members * F * max_dets * 40 bytes) stays under it."""

    def __init__(self, option_sets, max_tracks=128, max_dets=None, device=None, max_output_bytes=1 << 30):
        self.option_sets = [dict(o) for o in option_sets]
        if not self.option_sets:
            raise ValueError('TrackerSweep: no option sets')
        for k, o in enumerate(self.option_sets):
            _check_options(o, f'option_sets[{k}]')
        self.max_tracks, self.max_dets, self.device = int(max_tracks), None if max_dets is None else int(max_dets), device
        self.max_output_bytes = int(max_output_bytes)
        self.videos = []          # (frame_ids (F,) int32, dets (F, m, 8) float32, counts (F,) int32) on the host

    def add_video(self, records=None, *, frame_ids=None, dets=None, counts=None):
        """One video: its frame records (frame_ids: the frame ids, default 0 .. F-1), or explicit arrays frame_ids (F,),
        dets (F, m, 8) = rows [depth-scaled box, score, label, depth, scale], counts (F,) (-1: no such frame).  Returns
        the video's index."""
        if (records is None) == (dets is None):
            raise ValueError('add_video: give the frame records, or frame_ids / dets / counts')
        if records is not None:
            if counts is not None:
                raise ValueError('add_video: frame records carry their own counts')
            dets, counts = records_to_detections(records)
        else:
            if frame_ids is None or counts is None:
                raise ValueError('add_video: explicit arrays need frame_ids, dets and counts')
            dets = np.ascontiguousarray(dets.detach().cpu().numpy() if torch.is_tensor(dets) else dets, dtype=np.float32)
            counts = np.asarray(counts.detach().cpu().numpy() if torch.is_tensor(counts) else counts).astype(np.int32)
        F = len(counts)
        if frame_ids is None:
            frame_ids = np.arange(F)
        frame_ids = np.asarray(frame_ids.detach().cpu().numpy() if torch.is_tensor(frame_ids) else frame_ids).astype(np.int32)
        if dets.ndim != 3 or dets.shape[2] != REC_FLOATS or F == 0 or dets.shape[0] != F or frame_ids.shape != (F,) or \
                counts.shape != (F,):
            raise ValueError(f'add_video: expected frame_ids (F,), dets (F, m, {REC_FLOATS}), counts (F,) with F >= 1, got '
                             f'{frame_ids.shape}, {dets.shape}, {counts.shape}')
        most = int(counts.max())
        if most > dets.shape[1]:
            raise ValueError(f'add_video: a frame counts {most} detections, dets has {dets.shape[1]} rows per frame')
        if self.max_dets is not None and most > self.max_dets:
            raise ValueError(f'add_video: video {len(self.videos)} has a frame with {most} detections > max_dets = '
                             f'{self.max_dets}')
        self.videos.append((frame_ids, dets, counts))
        return len(self.videos) - 1

    def members(self):
        """[(option set k, video v)] in member order: member k * V + v."""
        V = len(self.videos)
        return [(k, v) for k in range(len(self.option_sets)) for v in range(V)]

    def _stacked(self):
        """The videos as one (V, F, M, 8) stream, ragged lengths padded with count -1."""
        V, F = len(self.videos), max(len(c) for _, _, c in self.videos)
        M = self.max_dets if self.max_dets is not None else max(1, max(int(c.max()) for _, _, c in self.videos))
        fids, dets, counts = np.zeros((V, F), np.int32), np.zeros((V, F, M, REC_FLOATS), np.float32), np.full((V, F), -1, np.int32)
        for v, (f, d, c) in enumerate(self.videos):
            m = min(M, d.shape[1])
            fids[v, :len(c)], counts[v, :len(c)], dets[v, :len(c), :m] = f, c, d[:, :m]
        return fids, dets, counts, M

    def run(self):
        """Tracks every member; one launch and one device-to-host copy per group of members.  -> SweepResult."""
        from .batched_assoc import BatchedGpuTracker
        if not self.videos:
            raise ValueError('TrackerSweep.run: no videos (add_video first)')
        fids, dets, counts, M = self._stacked()
        V, F = counts.shape
        members = self.members()
        B = len(members)
        per_member = F * M * (REC_FLOATS * 4 + 8) + F * 4
        if per_member > self.max_output_bytes:
            raise ValueError(f'TrackerSweep.run: one member\'s output takes {per_member} bytes > max_output_bytes = '
                             f'{self.max_output_bytes}')
        group = max(1, min(B, self.max_output_bytes // per_member))
        device = torch.device(self.device) if self.device is not None else torch.device('cuda', torch.cuda.current_device())
        rows, ids = np.empty((B, F, M, REC_FLOATS), np.float32), np.empty((B, F, M), np.int64)
        n, status = np.empty((B, F), np.int32), np.empty(B, np.int32)
        with torch.cuda.device(device):
            d_fids, d_dets, d_counts = (torch.from_numpy(a).to(device) for a in (fids, dets, counts))   # once, shared
            for m0 in range(0, B, group):
                part = members[m0:m0 + group]
                trk = BatchedGpuTracker(len(part), max_tracks=self.max_tracks, max_dets=M, device=device,
                                        options=[self.option_sets[k] for k, _ in part])
                video_of = torch.tensor([v for _, v in part], dtype=torch.int32, device=device)
                out = trk.run(d_fids, d_dets, d_counts, video_of)
                parts = [t.view(torch.uint8).reshape(-1) for t in (out[1], out[0], out[2], trk.status)]
                flat = torch.cat(parts).cpu().numpy()          # the group's one device-to-host copy
                o = 0
                for dst, p in zip((ids, rows, n, status), parts):
                    dst[m0:m0 + len(part)] = flat[o:o + p.numel()].view(dst.dtype).reshape(dst[m0:m0 + len(part)].shape)
                    o += p.numel()
        return SweepResult(self.option_sets, fids, rows, ids, n, status, groups=-(-B // group), device=device)


class SweepResult:
    """What TrackerSweep.run tracked, on the host: frame_ids (V, F), rows (B, F, M, 8), ids (B, F, M), n (B, F),
    status (B,) = the members' overflow codes (0 ok, 1 = more than max_tracks live tracks, 2 = more than max_dets
    detections), B = K * V in member order k * V + v."""

    def __init__(self, option_sets, frame_ids, rows, ids, n, status, groups=1, device=None):
        self.option_sets, self.frame_ids, self.rows, self.ids, self.n, self.status = option_sets, frame_ids, rows, ids, n, status
        self.groups, self.device = groups, device
        self.V, self.K = frame_ids.shape[0], len(option_sets)
        self._scores = None

    def overflowed(self):
        """Indices of the members with a non-zero status: their outputs stop at the overflowing frame."""
        return np.nonzero(self.status)[0].tolist()

    def prediction_rows(self):
        """One (R, 6) fp64 array per member: (frame, track id, x, y, w, h) in image space
        (mot_eval.image_space_rows, the conversion of TrackCollector.prediction_rows).  frame = the frame's INDEX in
        the video as it was added: its frame id, unless the video has gaps in its ids or starts over at frame id 0, where
        frame ids repeat and could not key a ground truth."""
        from .mot_eval import image_space_rows
        F, B = self.n.shape[1], self.n.shape[0]
        frames = np.tile(np.arange(F)[:, None], (1, B))                                   # (F, B)
        return image_space_rows(frames, self.rows.transpose(1, 0, 2, 3), self.ids.transpose(1, 0, 2), self.n.T)

    def scores(self, gt_by_video, iou_thr=0.5, metrics=('HOTA', 'CLEAR', 'Identity'), backend='device', postprocess=None,
               protocol='rows', benchmark='MOT17'):
        """gt_by_video: the V ground-truth row arrays (frame, id, x, y, w, h, ...), image space, frame = the frame's
        index in the video (prediction_rows).  -> one dict per option set: its V videos' results combined by metrics.combine_videos (the
        rule of MOTDroneMetrics), plus 'status' = the set's V member codes.  An option set with an overflowed member is
        NOT scored: its dict holds only 'status' and 'overflowed' = True, and a warning names the members.
        protocol / benchmark: as MOTDroneMetrics' (mot_eval.evaluate_sweep); with 'trackeval' the ground truth may carry
        the conf, class and visibility columns."""
        from . import metrics as M
        from .mot_eval import evaluate_sweep
        gts = list(gt_by_video)
        if len(gts) != self.V:
            raise ValueError(f'scores: {len(gts)} ground-truth sets for {self.V} videos')
        bad = self.overflowed()
        if bad:
            warnings.warn(f'tracker sweep: members {bad} (option sets {sorted({m // self.V for m in bad})}) exceeded a '
                          f'capacity (status {self.status[bad].tolist()}) and are not scored')
        good = [k for k in range(self.K) if not self.status[k * self.V:(k + 1) * self.V].any()]
        preds = self.prediction_rows()
        res = evaluate_sweep([preds[k * self.V + v] for k in good for v in range(self.V)], gts * len(good), iou_thr,
                             metrics, self.device, backend, postprocess, protocol, benchmark) if good else []
        out = [dict(status=self.status[k * self.V:(k + 1) * self.V].tolist(), overflowed=True) for k in range(self.K)]
        for i, k in enumerate(good):
            r = res[i * self.V:(i + 1) * self.V]
            per_video = {v: r[v]['clear_identity'] for v in range(self.V)}
            hs = {v: r[v]['hota'] for v in range(self.V)} if 'HOTA' in metrics else None
            out[k] = dict(M.combine_videos(per_video, hs), status=out[k]['status'], overflowed=False)
        self._scores = out
        return out

    def best(self, key='HOTA'):
        """(index, option dict, scores) of the option set with the largest `key` of the last scores() call; ties go to
        the lowest index; option sets that overflowed do not take part."""
        if self._scores is None:
            raise ValueError('best: call scores() first')
        cand = [k for k, s in enumerate(self._scores) if not s['overflowed']]
        if not cand:
            raise ValueError('best: every option set overflowed a capacity')
        k = max(cand, key=lambda i: (self._scores[i][key], -i))
        return k, self.option_sets[k], self._scores[k]
