"""CocoMetric - the evaluator the reference's stereo-tracking configs switch on (`val_evaluator` / `test_evaluator` =
[dict(type='mmdet.CocoMetric', ann_file=..., metric='bbox', format_only=False)], reference config
yolox_s_mmyolo_mot_airdrone_disp.py:214-231; mmtrack/evaluation/metrics/coco_video_metric.py maps the fields): COCO
bbox mAP / AR of the detector's boxes (`pred_det_instances`), matched and accumulated on the device
(csrc/coco_eval.hip behind st_coco_prepare / st_coco_match / st_coco_accumulate).

pycocotools and mmdet are absent: the rules are COCOeval.evaluateImg / accumulate / summarize and mmdet 3.0.0rc4's
CocoMetric restated from memory [upstream-memory]; they are listed in tests/coco_eval_ref.py (the numpy restatement,
the executable spec) and DESIGN.md "COCO bbox evaluation", the uncertain ones marked.  Parity with pycocotools itself
is unpinned.  There is no host implementation in the product: without a CUDA (ROCm) device evaluate() raises.
"""
import ctypes as C
import json
import os

import numpy as np
import torch

from . import _lib
from ._lib import StCocoArgs, check, current_stream
from .registry import METRICS

SUPPORTED_METRICS = ('bbox',)
METRIC_ITEMS = {'mAP': 0, 'mAP_50': 1, 'mAP_75': 2, 'mAP_s': 3, 'mAP_m': 4, 'mAP_l': 5, 'AR@100': 6, 'AR@300': 7,
                'AR@1000': 8, 'AR_s@1000': 9, 'AR_m@1000': 10, 'AR_l@1000': 11}
DEFAULT_ITEMS = ('mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l')
STATUS_BITS = {1: 'det_img is not non-decreasing inside [0, num_images)', 2: 'gt_img is not non-decreasing inside '
               '[0, num_images)', 4: 'non-finite detection', 8: 'detection label outside the categories',
               16: 'more ground-truth boxes in one (image, category) group than a launch holds',
               32: 'ground-truth category outside the categories'}


def default_params():
    """pycocotools Params(iouType='bbox'): the host's fp64 tables, passed to the device as they are."""
    return dict(iou_thrs=np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
                rec_thrs=np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True),
                area_rngs=np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]],
                                   dtype=np.float64))


def max_gt_per_group():
    """Largest number of ground-truth boxes of one category in one image that a launch supports."""
    return int(_lib.load().st_coco_max_gt())


def _mean_valid(s):
    s = s[s > -1]
    return -1.0 if s.size == 0 else float(np.mean(s))


def summarize(precision, recall, iou_thrs, max_dets):
    """pycocotools' 12 summary numbers from the arrays the device wrote (numpy on the host: 12 means of slices)."""
    if len(max_dets) != 3:
        raise ValueError(f'the 12-number COCO summary needs three max_dets / proposal_nums entries, got {list(max_dets)}')

    def ap(thr=None, a=0):
        s = precision if thr is None else precision[np.where(thr == iou_thrs)[0]]
        return _mean_valid(s[:, :, :, a, 2])

    def ar(a=0, m=2):
        return _mean_valid(recall[:, :, a, m])

    return np.array([ap(), ap(.5), ap(.75), ap(a=1), ap(a=2), ap(a=3), ar(m=0), ar(m=1), ar(m=2), ar(a=1), ar(a=2),
                     ar(a=3)], dtype=np.float64)


def coco_eval_device(det_boxes, det_scores, det_labels, det_img, gt_boxes, gt_area, gt_crowd, gt_cat, gt_img,
                     num_images, num_cats, iou_thrs=None, max_dets=(100, 300, 1000), area_rngs=None, rec_thrs=None,
                     timing=False, out=None):
    """The three device stages on flat rows (layout: include/stereotrack.h section 12).

    det_*: CUDA tensors (float32 (D, 4) xyxy, float32 (D,), int (D,), int (D,) non-decreasing image index); gt_*: host
    arrays (float64 xywh, area, crowd, category, image index - sorted here by image, stable).  Enqueues on the current
    stream and returns device tensors without waiting: dict(rank, matched, ignored (int64 bit tables, bit t * A + a),
    npig, precision, recall, scores, status).  `timing` adds HIP events around the stages ('events').  `out`: a dict
    of preallocated output tensors to write into (tests poison them)."""
    if not torch.cuda.is_available():
        raise RuntimeError('CocoMetric evaluates on the HIP path only (csrc/coco_eval.hip) and no CUDA (ROCm) device is '
                           'available; stereotracking_amd has no host implementation of the evaluation')
    lib = _lib.load()
    p = default_params()
    iou_thrs = p['iou_thrs'] if iou_thrs is None else np.asarray(iou_thrs, dtype=np.float64).reshape(-1)
    rec_thrs = p['rec_thrs'] if rec_thrs is None else np.asarray(rec_thrs, dtype=np.float64).reshape(-1)
    area_rngs = p['area_rngs'] if area_rngs is None else np.asarray(area_rngs, dtype=np.float64).reshape(-1, 2)
    max_dets = [int(m) for m in max_dets]
    dev = det_boxes.device
    if dev.type != 'cuda':
        raise RuntimeError(f'detections must be CUDA (ROCm) tensors, got {dev}')
    D, K = int(det_scores.shape[0]), int(num_cats)
    T, A, M, R = len(iou_thrs), len(area_rngs), len(max_dets), len(rec_thrs)
    det_boxes = det_boxes.reshape(-1, 4).to(torch.float32).contiguous()
    det_scores = det_scores.reshape(-1).to(torch.float32).contiguous()
    det_labels = det_labels.reshape(-1).to(torch.int32).contiguous()
    det_img = det_img.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()

    gt_img_h = np.asarray(gt_img, dtype=np.int32).reshape(-1)
    perm = np.argsort(gt_img_h, kind='stable')
    gt_img_h = np.ascontiguousarray(gt_img_h[perm])
    gt_cat_h = np.ascontiguousarray(np.asarray(gt_cat, dtype=np.int32).reshape(-1)[perm])
    gt_boxes_h = np.ascontiguousarray(np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 4)[perm])
    gt_area_h = np.ascontiguousarray(np.asarray(gt_area, dtype=np.float64).reshape(-1)[perm])
    gt_crowd_h = np.ascontiguousarray(np.asarray(gt_crowd).reshape(-1)[perm].astype(np.int32))
    G = len(gt_img_h)

    def up(a):
        return torch.from_numpy(a).to(dev)
    g_boxes, g_area, g_crowd, g_cat, g_img = up(gt_boxes_h), up(gt_area_h), up(gt_crowd_h), up(gt_cat_h), up(gt_img_h)
    d_iou, d_area, d_rec = up(np.ascontiguousarray(iou_thrs)), up(np.ascontiguousarray(area_rngs)), up(np.ascontiguousarray(rec_thrs))
    max_dets_h = (C.c_int * M)(*max_dets)

    out = dict(out or {})

    def buf(name, shape, dtype):
        t = out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        assert tuple(t.shape) == tuple(shape) and t.dtype == dtype and t.is_contiguous() and t.device == dev, name
        out[name] = t
        return t
    rank = buf('rank', (D,), torch.int32)
    matched = buf('matched', (D,), torch.int64)
    ignored = buf('ignored', (D,), torch.int64)
    npig = buf('npig', (K, A), torch.int32)
    precision = buf('precision', (T, R, K, A, M), torch.float64)
    recall = buf('recall', (T, K, A, M), torch.float64)
    scores = buf('scores', (T, R, K, A, M), torch.float64)
    status = buf('status', (4,), torch.int32)

    def dp(t):
        return C.c_void_p(t.data_ptr()) if t.numel() else None
    args = StCocoArgs()
    args.struct_size = C.sizeof(StCocoArgs)
    args.num_images, args.num_cats, args.num_dets, args.num_gts = int(num_images), K, D, G
    args.T, args.A, args.M, args.R = T, A, M, R
    args.det_boxes, args.det_scores, args.det_labels, args.det_img = dp(det_boxes), dp(det_scores), dp(det_labels), dp(det_img)
    args.gt_boxes, args.gt_area, args.gt_crowd, args.gt_cat, args.gt_img = dp(g_boxes), dp(g_area), dp(g_crowd), dp(g_cat), dp(g_img)
    args.gt_img_host = gt_img_h.ctypes.data_as(C.c_void_p) if G else None
    args.gt_cat_host = gt_cat_h.ctypes.data_as(C.c_void_p) if G else None
    args.iou_thrs, args.area_rng, args.rec_thrs = dp(d_iou), dp(d_area), dp(d_rec)
    args.max_dets = C.cast(max_dets_h, C.c_void_p)
    args.det_rank, args.det_matched, args.det_ignored = dp(rank), dp(matched), dp(ignored)
    args.npig, args.precision, args.recall, args.scores, args.status = dp(npig), dp(precision), dp(recall), dp(scores), dp(status)
    args.ws, args.ws_bytes = None, 0
    nbytes = int(lib.st_coco_workspace_bytes(C.byref(args)))
    if nbytes == 0:
        raise _lib.StError(f'st_coco_workspace_bytes: invalid sizes (images {num_images}, categories {K}, '
                           f'detections {D}, max_dets {max_dets})')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    args.ws, args.ws_bytes = C.c_void_p(ws.data_ptr()), nbytes
    stream = current_stream()
    events = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if timing else None
    for i, (name, fn) in enumerate((('st_coco_prepare', lib.st_coco_prepare), ('st_coco_match', lib.st_coco_match),
                                    ('st_coco_accumulate', lib.st_coco_accumulate))):
        if timing:
            events[i].record()
        check(fn(C.byref(args), stream), name)
    if timing:
        events[3].record()
        out['events'] = events
    # keep what the enqueued kernels read alive until the caller has synchronised on the results
    out['_keep'] = (det_boxes, det_scores, det_labels, det_img, g_boxes, g_area, g_crowd, g_cat, g_img, d_iou, d_area,
                    d_rec, ws, max_dets_h, gt_img_h, gt_cat_h)
    return out


def status_message(status):
    bits = int(status[0])
    return '; '.join(msg for b, msg in STATUS_BITS.items() if bits & b)


@METRICS.register_module(name=['CocoMetric', 'CocoVideoMetric'])
class CocoMetric:
    """mmdet.CocoMetric (and mmtrack's CocoVideoMetric, the same evaluation fed from `pred_det_instances`) for
    metric='bbox'.  process() keeps device references, evaluate() runs the device stages once over everything."""

    default_prefix = 'coco'

    def __init__(self, ann_file=None, metric='bbox', classwise=False, proposal_nums=(100, 300, 1000), iou_thrs=None,
                 metric_items=None, format_only=False, outfile_prefix=None, prefix='coco', classes=('drone',),
                 **kwargs):
        metrics = [metric] if isinstance(metric, str) else list(metric)
        for m in metrics:
            if m in ('segm', 'proposal', 'proposal_fast'):
                raise NotImplementedError(f"CocoMetric: metric {m!r} is not implemented; supported: "
                                          f"{list(SUPPORTED_METRICS)} (the configs evaluate metric='bbox')")
            if m not in SUPPORTED_METRICS:
                raise KeyError(f"CocoMetric: metric {m!r} is not supported; supported: {list(SUPPORTED_METRICS)}")
        self.metrics = metrics
        self.ann_file, self.classwise = ann_file, bool(classwise)
        self.proposal_nums = [int(v) for v in proposal_nums]
        if len(self.proposal_nums) != 3 or sorted(self.proposal_nums) != self.proposal_nums or self.proposal_nums[0] < 1:
            raise ValueError(f'CocoMetric: proposal_nums must be three increasing positive ints (they are the max_dets '
                             f'of the evaluation), got {list(proposal_nums)}')
        self.iou_thrs = default_params()['iou_thrs'] if iou_thrs is None else \
            np.asarray([iou_thrs] if np.isscalar(iou_thrs) else iou_thrs, dtype=np.float64)
        if metric_items is not None:
            for it in metric_items:
                if it not in METRIC_ITEMS:
                    raise KeyError(f'CocoMetric: metric item {it!r} is not supported; supported: {list(METRIC_ITEMS)}')
        self.metric_items = list(metric_items) if metric_items is not None else None
        self.format_only = bool(format_only)
        if self.format_only and outfile_prefix is None:
            raise ValueError('CocoMetric: outfile_prefix must be given when format_only=True')
        self.outfile_prefix, self.prefix = outfile_prefix, prefix
        self.unused_kwargs = dict(kwargs)       # collect_device, backend_args, file_client_args: accepted, unused
        self.classes = tuple(classes)
        self.cat_ids = list(range(1, len(self.classes) + 1))      # without ann_file: mmdet numbers the categories itself
        self._ann = None          # read on first use: building the metric from a config does not need the file
        self.records = []        # per image: dict(img_id, ori_shape, bboxes, scores, labels, gt (rows or None))
        self.stats = self.precision = self.recall = self.scores = self.npig = None
        self.last_events = None

    @property
    def dataset_meta(self):
        """mmengine's evaluator hands the dataset's metainfo over through this attribute (classes -> categories)."""
        return dict(classes=self.classes)

    @dataset_meta.setter
    def dataset_meta(self, meta):
        self.classes = tuple(meta.get('classes', meta.get('CLASSES', self.classes)))
        self.cat_ids = list(range(1, len(self.classes) + 1))
        self._ann = None

    # ---- ground truth ---------------------------------------------------------------------------------------
    def _load_ann(self, ann_file):
        with open(ann_file) as f:
            coco = json.load(f)
        by_name = {c['name']: c['id'] for c in coco.get('categories', [])}
        missing = [n for n in self.classes if n not in by_name]
        if missing:
            raise KeyError(f'CocoMetric: classes {missing} are not categories of {ann_file}')
        self.cat_ids = [by_name[n] for n in self.classes]
        label_of = {cid: i for i, cid in enumerate(self.cat_ids)}
        img_ids = sorted(im['id'] for im in coco['images'])
        rows = {i: [] for i in img_ids}
        for ann in coco.get('annotations', []):
            if ann['category_id'] not in label_of or ann['image_id'] not in rows:
                continue
            x, y, w, h = (float(v) for v in ann['bbox'])
            rows[ann['image_id']].append((x, y, w, h, float(ann['area']), int(bool(ann.get('iscrowd', 0))),
                                          label_of[ann['category_id']]))
        self._ann = dict(img_ids=img_ids, rows=rows)

    @staticmethod
    def _gt_rows_from_instances(instances):
        rows = []
        for ins in instances:
            x1, y1, x2, y2 = (float(v) for v in ins['bbox'])
            w, h = x2 - x1, y2 - y1
            rows.append((x1, y1, w, h, w * h, int(bool(ins.get('ignore_flag', 0))), int(ins.get('bbox_label', 0))))
        return rows

    # ---- collection -----------------------------------------------------------------------------------------
    def process(self, data_sample, instances=None):
        """One frame (or a list of frames, with a list of `instances`): keeps references to the detector's boxes
        `pred_det_instances.bboxes / scores / labels` where they are - no copy to the host, no synchronisation."""
        if isinstance(data_sample, (list, tuple)):
            ins = instances if instances is not None else [None] * len(data_sample)
            if len(ins) != len(data_sample):
                raise ValueError('process: one `instances` list per data sample')
            for s, g in zip(data_sample, ins):
                self.process(s, g)
            return
        meta = data_sample.metainfo
        if 'img_id' not in meta:
            raise KeyError('CocoMetric.process: the data sample carries no img_id')
        det = data_sample.pred_det_instances
        gt = None
        if self.ann_file is None and not self.format_only:
            if instances is None:
                instances = meta.get('instances')
            if instances is None:
                raise ValueError(f"CocoMetric without ann_file needs the frame's ground-truth `instances` "
                                 f"(image {meta['img_id']})")
            gt = self._gt_rows_from_instances(instances)
        self.records.append(dict(img_id=meta['img_id'], ori_shape=tuple(meta.get('ori_shape', ())[:2]),
                                 bboxes=det['bboxes'], scores=det['scores'], labels=det['labels'], gt=gt))

    # ---- several ranks --------------------------------------------------------------------------------------
    @staticmethod
    def _host_record(r):
        return dict(r, bboxes=r['bboxes'].detach().cpu().numpy() if isinstance(r['bboxes'], torch.Tensor) else r['bboxes'],
                    scores=r['scores'].detach().cpu().numpy() if isinstance(r['scores'], torch.Tensor) else r['scores'],
                    labels=r['labels'].detach().cpu().numpy() if isinstance(r['labels'], torch.Tensor) else r['labels'])

    def gather(self):
        """MOTDroneMetrics.gather's scheme: barrier, all_gather_object of the per-image host records, merged in rank
        order; an image id held by two ranks is an error.  No-op without an initialised process group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return self
        dist.barrier()
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, [self._host_record(r) for r in self.records])
        seen, merged = {}, []
        for rank, part in enumerate(parts):
            for r in part:
                if r['img_id'] in seen:
                    raise RuntimeError(f"image {r['img_id']!r} was processed on more than one rank "
                                       f"({seen[r['img_id']]} and {rank}): videos shard whole")
                seen[r['img_id']] = rank
                merged.append(r)
        self.records = merged
        return self

    def evaluate(self, distributed=True):
        import torch.distributed as dist
        multi = distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        if multi:
            self.gather()
            box = [self._evaluate_local() if dist.get_rank() == 0 else None]
            dist.broadcast_object_list(box, src=0)
            return box[0]
        return self._evaluate_local()

    # ---- evaluation -----------------------------------------------------------------------------------------
    def _unique_records(self):
        seen = set()
        for r in self.records:
            if r['img_id'] in seen:
                raise RuntimeError(f"image {r['img_id']!r} was processed twice")
            seen.add(r['img_id'])
        return sorted(self.records, key=lambda r: r['img_id'])

    def results_json(self):
        """The detections in COCO result form (image_id, bbox xywh, score, category_id), as mmdet's results2json."""
        out = []
        for r in self._unique_records():
            h = self._host_record(r)
            b = np.asarray(h['bboxes'], dtype=np.float32).reshape(-1, 4).astype(np.float64)
            for i in range(len(b)):
                out.append(dict(image_id=r['img_id'], bbox=[b[i, 0], b[i, 1], b[i, 2] - b[i, 0], b[i, 3] - b[i, 1]],
                                score=float(h['scores'][i]), category_id=self.cat_ids[int(h['labels'][i])]))
        return out

    def _evaluate_local(self):
        if self.format_only:
            path = f'{self.outfile_prefix}.bbox.json'
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, 'w') as f:
                json.dump(self.results_json(), f)
            return {}
        if not torch.cuda.is_available():
            raise RuntimeError('CocoMetric.evaluate runs on the HIP path only (csrc/coco_eval.hip) and no CUDA (ROCm) '
                               'device is available; stereotracking_amd has no host implementation of the evaluation')
        recs = self._unique_records()
        if self.ann_file is not None:
            if self._ann is None:
                self._load_ann(self.ann_file)
            img_ids = self._ann['img_ids']            # every image of the file, as mmdet sets imgIds to the file's
            index = {i: n for n, i in enumerate(img_ids)}
            for r in recs:
                if r['img_id'] not in index:
                    raise KeyError(f"image {r['img_id']!r} is not in {self.ann_file}")
            gt_rows = [(index[i], row) for i in img_ids for row in self._ann['rows'][i]]
        else:
            img_ids = [r['img_id'] for r in recs]
            index = {i: n for n, i in enumerate(img_ids)}
            gt_rows = [(index[r['img_id']], row) for r in recs for row in r['gt']]
        if not img_ids:
            raise ValueError('CocoMetric.evaluate: nothing to evaluate (no image was processed)')
        dev = next((r['bboxes'].device for r in recs if isinstance(r['bboxes'], torch.Tensor) and r['bboxes'].is_cuda),
                   torch.device('cuda', torch.cuda.current_device()))

        def dev_t(v, dtype):
            t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))
            return t.to(device=dev, dtype=dtype)
        counts = [int(r['scores'].shape[0]) for r in recs]          # shapes: known on the host without a sync
        if recs:
            boxes = torch.cat([dev_t(r['bboxes'], torch.float32).reshape(-1, 4) for r in recs])
            scores = torch.cat([dev_t(r['scores'], torch.float32).reshape(-1) for r in recs])
            labels = torch.cat([dev_t(r['labels'], torch.int32).reshape(-1) for r in recs])
        else:
            boxes = torch.zeros((0, 4), dtype=torch.float32, device=dev)
            scores = torch.zeros((0,), dtype=torch.float32, device=dev)
            labels = torch.zeros((0,), dtype=torch.int32, device=dev)
        det_img_h = np.repeat(np.array([index[r['img_id']] for r in recs], dtype=np.int32), counts)
        det_img = torch.from_numpy(det_img_h)
        gt = np.array([row for _, row in gt_rows], dtype=np.float64).reshape(-1, 7)
        gt_img = np.array([i for i, _ in gt_rows], dtype=np.int32)
        res = coco_eval_device(boxes, scores, labels, det_img, gt[:, :4], gt[:, 4], gt[:, 5].astype(np.int32),
                               gt[:, 6].astype(np.int32), gt_img, len(img_ids), len(self.classes),
                               iou_thrs=self.iou_thrs, max_dets=self.proposal_nums, timing=True)
        status = res['status'].cpu().numpy()         # the one wait: everything before it was only enqueued
        if status[0]:
            D = len(det_img_h)
            if status[0] & 4:
                row = D - int(status[1])
                raise ValueError(f'CocoMetric: non-finite box or score among the detections of image '
                                 f'{img_ids[int(det_img_h[row])]!r}')
            if status[0] & 8:
                row = D - int(status[2])
                raise ValueError(f'CocoMetric: a detection label of image {img_ids[int(det_img_h[row])]!r} is outside '
                                 f'the {len(self.classes)} classes')
            raise _lib.StError(f'coco evaluation failed on the device: {status_message(status)}')
        self.precision, self.recall = res['precision'].cpu().numpy(), res['recall'].cpu().numpy()
        self.scores, self.npig = res['scores'].cpu().numpy(), res['npig'].cpu().numpy()
        ev = res['events']
        self.last_events = dict(prepare_ms=ev[0].elapsed_time(ev[1]), match_ms=ev[1].elapsed_time(ev[2]),
                                accumulate_ms=ev[2].elapsed_time(ev[3]))
        self.stats = summarize(self.precision, self.recall, self.iou_thrs, self.proposal_nums)
        out = {}
        for item in (self.metric_items or DEFAULT_ITEMS):
            out[f'{self.prefix}/bbox_{item}'] = float(f'{round(float(self.stats[METRIC_ITEMS[item]]), 3)}')
        if self.classwise:
            for k, name in enumerate(self.classes):
                p = self.precision[:, :, k, 0, -1]
                p = p[p > -1]
                out[f'{self.prefix}/{name}_precision'] = round(float(np.mean(p)) if p.size else float('nan'), 3)
        return out


METRICS.register_module(name='mmdet.CocoMetric', module=CocoMetric)
