"""KITTI Tracking evaluation (2-D boxes): MOTKittiMetrics, the reference's second benchmark metric.

Behavioural spec: reference mmtrack/evaluation/metrics/mot_kitti_metrics.py
  process()                 :169-232  per-frame rows (0-based frame_id, xyxy boxes, class = label2cat[label])
  _save_one_video_gts_preds :247-284  the 18-column prediction and 17-column ground-truth lines
  collect_results           :331-359  the reported keys, suffixed _{cls}
and mmtrack/evaluation/functional/kitti_2d_box.py (Kitti2DBox_MOT): the classes, the distractors (:186-201) and the
constants max_occlusion 2 / max_truncation 0 / min_height 25 (:56-58).  The preprocessing itself is TrackEval's
(un-vendored): metrics.kitti_preprocess restates it [upstream-memory]; the rows it keeps are scored by the scorers
MOTDroneMetrics uses (metrics.clear_identity / metrics.hota, or mot_eval.evaluate_packed on the device), handed over as
(frame, id, x1, y1, x2 - x1, y2 - y1).  DESIGN.md section 16.

Not part of this class: tracklet post-processing (AppearanceFreeLink, InterpolateTracklets): a non-empty
postprocess_tracklet_cfg raises NotImplementedError.
"""
import os
from collections import defaultdict

import numpy as np

from . import metrics as M
from .registry import METRICS

CLASS_NAME_TO_CLASS_ID = {'car': 1, 'van': 2, 'truck': 3, 'pedestrian': 4, 'person': 5, 'cyclist': 6, 'tram': 7,
                          'misc': 8, 'dontcare': 9}       # mot_kitti_metrics.py:87-88 ('person' = person sitting)
DISTRACTORS = {'car': ('van',), 'pedestrian': ('person',)}        # kitti_2d_box.py:194-198
SUMMARY_KEYS = dict(HOTA=('HOTA', 'AssA', 'DetA'), CLEAR=('MOTA', 'MOTP', 'IDSW', 'TP', 'FP', 'FN', 'Frag', 'MT', 'ML'),
                    Identity=('IDF1', 'IDTP', 'IDFN', 'IDFP', 'IDP', 'IDR'))      # collect_results, in its order


def _file_float(v):
    """A value as the reference's files carry it: through '%.6f'."""
    return float('%.6f' % float(v))


@METRICS.register_module(name=['MOTKittiMetrics', 'mmtrack.MOTKittiMetrics'])
class MOTKittiMetrics(M.GatheredVideoMetric):
    """Collects per-frame KITTI rows, writes the reference's files, scores car and pedestrian with KITTI's rules.
    backend='device': the preprocessing of all videos and classes in one mot_eval.kitti_keep_masks call and the scores of
    all (video, class) pairs in one mot_eval.evaluate_packed call, at evaluate()."""

    allowed_metrics = ('HOTA', 'CLEAR', 'Identity')
    allowed_benchmarks = ('KITTI',)
    max_occlusion, max_truncation, min_height = 2, 0, 25          # kitti_2d_box.py:56-58

    def __init__(self, metric=('HOTA', 'CLEAR', 'Identity'), classes_eval=('car', 'pedestrian'), track_iou_thr=0.5,
                 benchmark='KITTI', format_only=False, postprocess_tracklet_cfg=(), backend='host', outfile_prefix=None,
                 collect_device='cpu', prefix=None):
        # outfile_prefix / collect_device / prefix: the reference's keywords, accepted so that its configs build; files
        # are written by write_kitti(out_dir) only, and the rows are gathered as MOTDroneMetrics gathers them.
        M._check_backend(backend)
        self.backend = backend
        self.metrics = [metric] if isinstance(metric, str) else list(metric)
        for m in self.metrics:
            if m not in self.allowed_metrics:
                raise KeyError(f'metric {m} is not supported.')
        self.classes_eval = [str(c).lower() for c in classes_eval]
        for c in self.classes_eval:
            if c not in DISTRACTORS:
                raise ValueError(f'Attempted to evaluate an invalid class {c!r}. Only classes {sorted(DISTRACTORS)} are valid.')
        if benchmark not in self.allowed_benchmarks:
            raise ValueError(f'benchmark must be one of {self.allowed_benchmarks}, got {benchmark!r}')
        if postprocess_tracklet_cfg:
            raise NotImplementedError('MOTKittiMetrics: tracklet post-processing (postprocess_tracklet_cfg) is not implemented')
        self.benchmark, self.track_iou_thr, self.format_only = benchmark, track_iou_thr, format_only
        self.pred = defaultdict(list)       # video -> the reference's 18-value prediction rows
        self.gt = defaultdict(list)         # video -> the reference's 19-value ground-truth rows

    def process(self, video, data_sample, gt_instances=None, cat2label=None):
        """data_sample: TrackDataSample with pred_track_instances (instances_id, labels, bboxes xyxy, scores) and
        metainfo frame_id; gt_instances: MOTKittiDataset's instance dicts; cat2label: the dataset's category id ->
        label map (also read from the sample's metainfo).  Rows as mot_kitti_metrics.py:169-232 builds them."""
        frame_id = data_sample.metainfo['frame_id']
        for ins in gt_instances or ():
            self.gt[video].append([frame_id, ins['instance_id'], ins['category_id'], ins['truncated'], ins['occluded'],
                                   ins['alpha'], *ins['bbox'], *ins['dim'], *ins['location'], ins['rotation_y'],
                                   ins['mot_conf'], ins['visibility']])
        if cat2label is None:
            cat2label = data_sample.metainfo.get('cat2label')
        if cat2label is None:
            raise KeyError('MOTKittiMetrics.process needs cat2label (the dataset puts it into every data info)')
        label2cat = {v: k for k, v in cat2label.items()}
        trk = data_sample.pred_track_instances
        ids, labels = trk['instances_id'].cpu().numpy(), trk['labels'].cpu().numpy()
        boxes, scores = trk['bboxes'].cpu().numpy(), trk['scores'].cpu().numpy()
        for i in range(len(ids)):
            self.pred[video].append([frame_id, int(ids[i]), label2cat[int(labels[i])], -1, -1, -1, *boxes[i][:4].tolist(),
                                     -1, -1, -1, -1, -1, -1, -1, float(scores[i])])

    def write_kitti(self, out_dir):
        """pred/<video>.txt: 18 columns, gt/<video>.txt: 17 columns (reference :261-279): frame, id, class name,
        truncated, occluded as integers, the rest with six decimals."""
        names = {v: k for k, v in CLASS_NAME_TO_CLASS_ID.items()}
        for kind, by_video, cols in (('pred', self.pred, 18), ('gt', self.gt, 17)):
            os.makedirs(os.path.join(out_dir, kind), exist_ok=True)
            for video, rows in by_video.items():
                with open(os.path.join(out_dir, kind, video + '.txt'), 'wt') as f:
                    for t in rows:
                        head = f'{int(t[0])},{int(t[1])},{names[int(t[2])]},{int(t[3])},{int(t[4])}'
                        f.write(head + ''.join(f',{float(v):.6f}' for v in t[5:cols]) + '\n')

    def rows(self, video):
        """The video's rows as the reference's files carry them to the scorer: ground truth (frame, id, class,
        truncation, occlusion, x1, y1, x2, y2) and predictions (frame, id, class, x1, y1, x2, y2, score); ids,
        truncation and occlusion through int(), boxes and score through '%.6f'.  A class id outside the benchmark's
        table raises KeyError, as writing the file would."""
        names = {v: k for k, v in CLASS_NAME_TO_CLASS_ID.items()}
        gt = [[int(t[0]), int(t[1]), CLASS_NAME_TO_CLASS_ID[names[int(t[2])]], int(t[3]), int(t[4])] +
              [_file_float(v) for v in t[6:10]] for t in self.gt.get(video, ())]
        pred = [[int(t[0]), int(t[1]), CLASS_NAME_TO_CLASS_ID[names[int(t[2])]]] + [_file_float(v) for v in t[6:10]] +
                [_file_float(t[17])] for t in self.pred.get(video, ())]
        return np.asarray(gt, dtype=np.float64).reshape(-1, 9), np.asarray(pred, dtype=np.float64).reshape(-1, 8)

    @staticmethod
    def split_ground_truth(gt_rows):
        """DontCare rows -> ignore regions (frame, x1, y1, x2, y2) first, then the other rows with a negative id are
        dropped (the class filter follows in kitti_preprocess)."""
        dc = gt_rows[:, 2] == CLASS_NAME_TO_CLASS_ID['dontcare']
        return gt_rows[~dc & (gt_rows[:, 1] >= 0)], gt_rows[dc][:, [0, 5, 6, 7, 8]]

    def _evaluate_local(self):
        if self.format_only:
            return dict(per_class={}, summary={})
        videos = sorted(set(self.gt) | set(self.pred))
        data = {}
        for v in videos:
            gt, pred = self.rows(v)
            data[v] = (*self.split_ground_truth(gt), pred)                   # (gt, ignore, pred)
        classes = [(CLASS_NAME_TO_CLASS_ID[c], [CLASS_NAME_TO_CLASS_ID[d] for d in DISTRACTORS[c]]) for c in self.classes_eval]
        consts = dict(max_occlusion=self.max_occlusion, max_truncation=self.max_truncation, min_height=self.min_height)
        if self.backend == 'device':
            from . import mot_eval
            masks = mot_eval.kitti_keep_masks([(data[v][0], data[v][2], data[v][1]) for v in videos], classes,
                                              videos=videos, **consts)
            masks = {(v, c): (gk[k], pk[k]) for v, (gk, pk) in zip(videos, masks) for k, c in enumerate(self.classes_eval)}
        else:
            masks = {(v, c): M.kitti_preprocess(data[v][0], data[v][2], data[v][1], cid, dis, **consts)
                     for v in videos for c, (cid, dis) in zip(self.classes_eval, classes)}

        def xywh(rows, box):        # (frame, id, x1, y1, x2 - x1, y2 - y1): the scorers' layout
            return np.column_stack([rows[:, 0], rows[:, 1], rows[:, box], rows[:, box + 1], rows[:, box + 2] - rows[:, box],
                                    rows[:, box + 3] - rows[:, box + 1]]).reshape(-1, 6)
        gts = {k: xywh(data[k[0]][0][gk], 5) for k, (gk, pk) in masks.items()}
        preds = {k: xywh(data[k[0]][2][pk], 3) for k, (gk, pk) in masks.items()}
        want_hota = 'HOTA' in self.metrics
        if self.backend == 'device' and masks:
            packed = mot_eval.pack_sequences(gts, preds)
            wanted = ['CLEAR', 'Identity'] + (['HOTA'] if want_hota else [])
            scored = dict(zip(packed['videos'], mot_eval.evaluate_packed(packed, self.track_iou_thr, wanted)))
        else:
            scored = {k: dict(clear_identity=M.clear_identity(gts[k], preds[k], self.track_iou_thr),
                              hota=M.hota(gts[k], preds[k]) if want_hota else None) for k in masks}
        per_class, summary = {}, {}
        for c in self.classes_eval:
            per_video = {v: scored[(v, c)]['clear_identity'] for v in videos}
            combined = M.combine_videos(per_video, {v: scored[(v, c)]['hota'] for v in videos} if want_hota else None)
            per_class[c] = dict(per_video=per_video, combined=combined)
            for m in self.metrics:
                for k in SUMMARY_KEYS[m]:
                    summary[f'{k}_{c}'] = combined[k]
        return dict(per_class=per_class, summary=summary)
