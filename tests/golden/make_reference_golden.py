#!/usr/bin/env python
"""Records tests/golden/reference/: outputs of the REFERENCE PROJECT'S OWN CODE, executed unmodified, on the CPU.

Every other fixture in tests/golden/ comes from oracle/ (make_golden.py), i.e. from our restatement of the reference.
These come from the reference's text itself, so that a transcription slip in the oracle - which the kernel and its test
would both reproduce - shows up as a difference.  tests/test_cpu_reference_fixtures.py holds the oracles, the host
backends and the test-side restatements to these files; tests/test_reference_fixtures_gpu.py holds the kernels to them.

Run on a development machine that has the reference tree:
    python tests/golden/make_reference_golden.py /path/to/reference [family ...]
The GPU machine and a clean checkout never need the tree: only the recorded arrays and manifest.json are committed.

HOW THE REFERENCE RUNS WITHOUT ITS DEPENDENCIES (mmengine, mmcv, mmdet, cv2, lap, addict, trackeval are absent):
  * a sys.meta_path finder serves stand-in modules for those roots.  A stand-in holds the shims of SHIMS below and, for
    any other name a reference module merely IMPORTS (type annotations, base classes of classes that are never
    instantiated, functions of branches that are never taken), an inert placeholder class: calling or instantiating a
    placeholder raises, and the manifest lists every placeholder that was handed out, so no placeholder can have
    contributed to a recorded number;
  * bare namespace shells (a module object with __path__ set to the real directory) stand in for the mmtrack.* packages,
    so that no __init__.py chain runs and every submodule is loaded from its own file, unmodified, by the ordinary path
    finder;
  * no function or method defined in the reference tree is replaced or patched.  This file names reference modules and
    attributes as strings and calls them; it contains no statement of the reference.

The shim list is CLOSED (things the reference does not define):
    registry register_module()            identity decorator
    addict.Dict                           oracle.tracker.Dict
    mmengine.structures.InstanceData      oracle.tracker.Instances
    mmengine.model.BaseModule             a torch.nn.Module subclass that swallows init_cfg
    lap.lapjv                             oracle/lapjv.py (and, to reject solver-dependent streams, a second one on
                                          scipy.optimize.linear_sum_assignment with the same cost extension)
    mmdet...bbox_overlaps                 oracle.tracker.bbox_overlaps
    save_prediction_results               decorator factory returning identity
    np.int                                int, for the duration of the run (numpy >= 1.24 has no np.int)
    names imported from mmtrack.utils / mmtrack.structures   object (type aliases; imrenormalize and TrackDataSample are
                                          imported by the tracker and never used with cmc=None; calling `object` raises)

numpy: the reference pins numpy 1.x (value-based casting): `python_float * np.float32_scalar` is float64 there and
float32 under NEP 50 (numpy >= 2).  Only KalmanFilter.initiate is touched by this (its measurement arrives as float32
from the tracker).  The recordings named `*_np1` pass the measurement through a CALLER-SIDE adapter that widens it to
float64 before the reference's initiate sees it, which reproduces the numpy-1 value exactly (float32 -> float64 is
exact, and every later operation on the mean is float64 under either numpy); the recordings named `*_raw` call the
reference as is under the running numpy.  Both are stored."""
import contextlib
import hashlib
import importlib
import importlib.abc
import importlib.machinery
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'reference')
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import lapjv as olap, tracker as otr  # noqa: E402  (the shims of the closed list live in oracle/)
from stereotracking_amd.synthetic import synthetic_detection_stream  # noqa: E402  (seeded INPUT generator)

THIRD_PARTY = ('mmengine', 'mmcv', 'mmdet', 'cv2', 'lap', 'addict', 'trackeval')
SHELLS = ('mmtrack', 'mmtrack.models', 'mmtrack.models.mot', 'mmtrack.models.trackers', 'mmtrack.models.motion',
          'mmtrack.models.task_modules', 'mmtrack.models.task_modules.track', 'mmtrack.structures',
          'mmtrack.structures.bbox', 'mmtrack.datasets', 'mmtrack.datasets.transforms')
MAX_NPZ_BYTES = 512 * 1024
MAX_DIR_BYTES = 2 * 1024 * 1024


# ------------------------------------------------------------------------------------------------------------- shims
class _BaseModule(torch.nn.Module):
    """mmengine.model.BaseModule as the reference's classes need it: nn.Module that swallows init_cfg."""

    def __init__(self, init_cfg=None, **kwargs):
        super().__init__()


class _Registry:
    """mmengine Registry as the reference's modules use it at import: register_module() is an identity decorator."""

    def register_module(self, *args, **kwargs):
        return lambda cls: cls


def _save_prediction_results(*args, **kwargs):
    return lambda fn: fn


def lapjv_scipy(cost, extend_cost=True, cost_limit=np.inf):
    """A second lap.lapjv stand-in: the same NaN rule and the same (rows + cols)^2 cost extension as oracle/lapjv.py,
    solved by scipy.optimize.linear_sum_assignment.  Used only to REJECT streams whose rows depend on how a restated
    third-party solver breaks ties; nothing recorded comes from it."""
    from scipy.optimize import linear_sum_assignment
    assert extend_cost and np.isfinite(cost_limit)
    cost = np.asarray(cost, dtype=np.float64)
    cost = np.where(np.isnan(cost), 1e6, cost)
    n_rows, n_cols = cost.shape
    r, c = linear_sum_assignment(olap.extend(cost, cost_limit))
    x = np.full(n_rows + n_cols, -1, np.int32)
    y = np.full(n_rows + n_cols, -1, np.int32)
    x[r], y[c] = c, r
    x[x >= n_cols] = -1
    y[y >= n_rows] = -1
    x, y = x[:n_rows], y[:n_cols]
    return cost[np.nonzero(x != -1)[0], x[x != -1]].sum(), x, y


SHIMS = {
    'addict': dict(Dict=otr.Dict),
    'lap': dict(lapjv=olap.lapjv),
    'mmengine.structures': dict(InstanceData=otr.Instances),
    'mmengine.model': dict(BaseModule=_BaseModule),
    'mmdet.structures.bbox': dict(bbox_overlaps=otr.bbox_overlaps),
}
SHIM_NOTES = {
    'registry register_module()': 'identity decorator (mmtrack.registry shell: every registry name)',
    'addict.Dict': 'oracle.tracker.Dict',
    'mmengine.structures.InstanceData': 'oracle.tracker.Instances',
    'mmengine.model.BaseModule': 'torch.nn.Module subclass that swallows init_cfg',
    'lap.lapjv': 'oracle/lapjv.py; every committed tracker stream also reproduced under a second shim on '
                 'scipy.optimize.linear_sum_assignment with the same cost extension',
    'mmdet.structures.bbox.bbox_overlaps': 'oracle.tracker.bbox_overlaps',
    'mmtrack.utils.collect_results.save_prediction_results': 'decorator factory returning identity',
    'np.int': 'int for the duration of the run',
    'names imported from mmtrack.utils, mmtrack.structures': 'object (type aliases; imrenormalize, TrackDataSample: '
                                                             'imported, never used)',
}


class _Loader(importlib.abc.Loader):
    def __init__(self, handed_out):
        self.handed_out = handed_out

    def create_module(self, spec):
        mod = types.ModuleType(spec.name)
        mod.__path__ = []                                     # a package, so that `import a.b.c` resolves through us
        shims, handed_out = SHIMS.get(spec.name, {}), self.handed_out

        def placeholder(name):
            if name.startswith('__'):
                raise AttributeError(name)
            if name in shims:
                return shims[name]
            full = f'{spec.name}.{name}'
            if full in sys.modules:
                return sys.modules[full]

            def refuse(self, *a, **k):
                raise RuntimeError(f'{full} is an inert placeholder of an absent third-party name; the recorder must '
                                   'not reach code that uses it')
            handed_out.add(full)
            return type(name, (), {'__init__': refuse, '__call__': refuse})
        mod.__getattr__ = placeholder
        return mod

    def exec_module(self, module):
        pass


class _Finder(importlib.abc.MetaPathFinder):
    def __init__(self):
        self.handed_out = set()

    def find_spec(self, name, path=None, target=None):
        if name.split('.')[0] in THIRD_PARTY:
            return importlib.machinery.ModuleSpec(name, _Loader(self.handed_out), is_package=True)
        return None


def _ours(name):
    return name.split('.')[0] in THIRD_PARTY + ('mmtrack',)


@contextlib.contextmanager
def reference_modules(ref_root):
    """Inside: `load(name)` imports a reference module from its own file.  On exit every stand-in, shell and reference
    module is dropped from sys.modules again, np.int is removed and the finder is gone."""
    pkg = os.path.join(ref_root, 'mmtrack')
    if not os.path.isdir(pkg):
        raise FileNotFoundError(f'no reference tree at {ref_root!r} (expected {pkg}/)')
    assert not any(_ours(m) for m in sys.modules), 'a real mmtrack / mm* package is already imported'
    finder = _Finder()
    used_files = set()
    had_np_int = hasattr(np, 'int')
    try:
        sys.meta_path.insert(0, finder)
        if not had_np_int:
            np.int = int
        for name in SHELLS:
            shell = types.ModuleType(name)
            shell.__path__ = [os.path.join(ref_root, *name.split('.'))]
            sys.modules[name] = shell
        registry = types.ModuleType('mmtrack.registry')
        registry.__getattr__ = lambda name: _Registry() if name.isupper() else _raise_attr(name)
        utils = types.ModuleType('mmtrack.utils')
        utils.__path__ = []
        utils.__getattr__ = lambda name: object if not name.startswith('__') else _raise_attr(name)
        collect = types.ModuleType('mmtrack.utils.collect_results')
        collect.save_prediction_results = _save_prediction_results
        sys.modules.update({'mmtrack.registry': registry, 'mmtrack.utils': utils,
                            'mmtrack.utils.collect_results': collect})
        sys.modules['mmtrack.structures'].__getattr__ = \
            lambda name: object if not name.startswith('__') else _raise_attr(name)

        def load(name):
            mod = importlib.import_module(name)
            for m in list(sys.modules.values()):
                f = getattr(m, '__file__', None)
                if f and os.path.abspath(f).startswith(os.path.abspath(ref_root) + os.sep):
                    used_files.add(os.path.relpath(f, ref_root))
            return mod

        # `from mmtrack.structures.bbox import bbox_xyxy_to_cxcyah`: the shell re-exports its own transforms.py
        tf = load('mmtrack.structures.bbox.transforms')
        for k, v in vars(tf).items():
            if k.startswith('bbox_') or k.startswith('quad'):
                setattr(sys.modules['mmtrack.structures.bbox'], k, v)
        load.used_files, load.finder = used_files, finder
        yield load
    finally:
        sys.meta_path.remove(finder)
        if not had_np_int and hasattr(np, 'int'):
            del np.int
        for m in [m for m in sys.modules if _ours(m)]:
            del sys.modules[m]


def _raise_attr(name):
    raise AttributeError(name)


def sha256_of(path):
    with open(path, 'rb') as f:
        return hashlib.sha256(f.read()).hexdigest()


# ------------------------------------------------------------------------------------------------------------ kalman
KALMAN_STEPS = 20


def kalman_measurements(seed):
    """20 + 1 cxcyah measurements of a drifting box with heights that are not round numbers: (float64 rows, the same
    rows rounded to float32 and widened back, scores for the NSA variant)."""
    rng = np.random.RandomState(seed)
    t = np.arange(KALMAN_STEPS + 1)[:, None]
    base = np.array([[412.37, 233.91, 0.4713, 57.318]]) + t * np.array([[3.1, -1.7, 0.0021, 0.37]])
    m64 = base + rng.normal(0, [0.8, 0.8, 0.004, 0.6], base.shape)
    m32 = m64.astype(np.float32).astype(np.float64)
    return m64, m32, rng.uniform(0.3, 0.97, KALMAN_STEPS + 1)


def record_kalman(load):
    KF = load('mmtrack.models.motion.kalman_filter').KalmanFilter
    out = {}
    for nsa in (False, True):
        for kind_i, kind in enumerate(('f64', 'f32_widened')):
            kf = KF(use_nsa=nsa)
            m64, m32, score = kalman_measurements(11 + kind_i)
            meas = m64 if kind == 'f64' else m32
            key = f'nsa{int(nsa)}/{kind}'
            mean, cov = kf.initiate(meas[0])
            rec = dict(init_mean=mean, init_cov=cov, pred_mean=[], pred_cov=[], proj_mean=[], proj_cov=[], upd_mean=[],
                       upd_cov=[], gate=[], gate_pos=[])
            for s in range(1, KALMAN_STEPS + 1):
                mean, cov = kf.predict(mean, cov)
                rec['pred_mean'].append(mean), rec['pred_cov'].append(cov)
                pm, pc = kf.project(mean, cov, score[s]) if nsa else kf.project(mean, cov)
                rec['proj_mean'].append(pm), rec['proj_cov'].append(pc)
                if hasattr(kf, 'gating_distance'):
                    near = meas[[(s - 2) % len(meas), s - 1, s, (s + 1) % len(meas)]]
                    rec['gate'].append(kf.gating_distance(mean, cov, near.copy()))
                    rec['gate_pos'].append(kf.gating_distance(mean, cov, near.copy(), only_position=True))
                mean, cov = kf.update(mean, cov, meas[s], score[s]) if nsa else kf.update(mean, cov, meas[s])
                rec['upd_mean'].append(mean), rec['upd_cov'].append(cov)
            out[f'{key}/measurements'], out[f'{key}/scores'] = meas, score
            for k, v in rec.items():
                if len(v):
                    out[f'{key}/{k}'] = np.asarray(v)
    # the float32 measurement AS the tracker hands it over (no widening): what the running numpy makes of it
    kf = KF()
    m32 = kalman_measurements(12)[1][0].astype(np.float32)
    mean, cov = kf.initiate(m32)
    out['raw_float32/measurement'], out['raw_float32/init_mean'], out['raw_float32/init_cov'] = m32, mean, cov
    return out, dict(cases=['use_nsa off/on x (float64 measurements, float32-valued measurements widened to float64 by '
                            'the caller = the value-based casting of the reference\'s pinned numpy 1.x)'],
                     raw_float32='KalmanFilter.initiate on a float32 array under the running numpy (NEP 50 for '
                                 'numpy >= 2): stored for the record, not the reference environment\'s value')


# ----------------------------------------------------------------------------------------------------------- tracker
REFERENCE_DEFAULTS = dict(obj_score_thr=0.3, init_track_thr=0.7, weight_iou_with_det_scores=True, match_iou_thr=0.3,
                          num_tentatives=3, vel_consist_weight=0.2, vel_delta_t=3, num_frames_retain=10)
TRACKER_OPTION_SETS = {
    'defaults': REFERENCE_DEFAULTS,
    'thresholds': dict(REFERENCE_DEFAULTS, match_iou_thr=0.1, init_track_thr=0.5),
    'unweighted_iou': dict(REFERENCE_DEFAULTS, weight_iou_with_det_scores=False),
    'no_direction_term': dict(REFERENCE_DEFAULTS, vel_consist_weight=0.0),
    'tentatives_1': dict(REFERENCE_DEFAULTS, num_tentatives=1),
    'retain_30_delta_1': dict(REFERENCE_DEFAULTS, num_frames_retain=30, vel_delta_t=1, weight_iou_with_det_scores=False,
                              match_iou_thr=0.1),
}


def tracker_streams():
    """name -> (rows [step, x1,y1,x2,y2, score, depth, scale] float32, frame_ids (S,) int32).  T <= 40, K <= 8."""
    T = 40
    steps = np.arange(T, dtype=np.int32)
    out = {'occlusion': (synthetic_detection_stream(seed=51, T=T, K=8, occlusion=(3, 20, 28)), steps.copy())}
    # empty frames (steps 7, 8, 19) and a frame-id restart at 0 (step 22), then a second, EMPTY frame 0 (step 34)
    det = synthetic_detection_stream(seed=52, T=T, K=5, occlusion=(1, 11, 16))
    det = det[~np.isin(det[:, 0], [7, 8, 19, 34])]
    out['empty_restart'] = (det, np.concatenate([np.arange(22), np.arange(12), np.arange(6)]).astype(np.int32))
    # detections below obj_score_thr (0.3) / between it and init_track_thr, and boxes of area <= 100 (10 x 10 exactly,
    # 9 x 11, and a zero-width box), next to three ordinary objects
    det = synthetic_detection_stream(seed=53, T=T, K=3, occlusion=(2, 14, 21))      # 3 + at most 5 extras: K <= 8
    extra = []
    for t in range(T):
        extra.append([t, 900 + 2 * t, 100, 930 + 2 * t, 140, 0.2 + 0.05 * (t % 5), 20.0, 1.0])      # 0.2 .. 0.4
        extra.append([t, 300 + t, 650, 310 + t, 660, 0.85, 30.0, 1.0])                              # area 100 exactly
        if t % 3 == 0:
            extra.append([t, 40 + t, 40, 49 + t, 51, 0.9, 30.0, 1.0])                               # area 99
        if t % 4 == 1:
            extra.append([t, 500 + t, 400, 500 + t, 430, 0.8, 25.0, 1.0])                           # zero width
        extra.append([t, 1000, 300 + 3 * t, 1030, 340 + 3 * t, 0.5 + 0.01 * (t % 7), 12.0, 1.0])    # 0.5: below init thr
    det = np.concatenate([det, np.asarray(extra, np.float32)])
    out['low_score_small_area'] = (det[np.argsort(det[:, 0], kind='stable')], steps.copy())
    # further candidates
    out['short_gaps'] = (synthetic_detection_stream(seed=54, T=32, K=4, occlusion=(0, 6, 9)),
                         np.arange(32, dtype=np.int32))
    out['crossing'] = (synthetic_detection_stream(seed=55, T=T, K=7, occlusion=(5, 25, 33)), steps.copy())
    return out


TRACKER_PAIRS = (('occlusion', 'defaults'), ('occlusion', 'unweighted_iou'), ('occlusion', 'no_direction_term'),
                 ('occlusion', 'retain_30_delta_1'), ('empty_restart', 'defaults'), ('empty_restart', 'tentatives_1'),
                 ('low_score_small_area', 'defaults'), ('low_score_small_area', 'thresholds'),
                 ('short_gaps', 'tentatives_1'), ('crossing', 'thresholds'), ('crossing', 'defaults'))


class _WidenInitiate:
    """The caller-side adapter of the `*_np1` recordings: the reference KalmanFilter, its initiate() given the
    measurement widened to float64 (module docstring)."""

    def __init__(self, kf):
        self._kf = kf

    def initiate(self, measurement):
        return self._kf.initiate(np.asarray(measurement, np.float64))

    def __getattr__(self, name):
        return getattr(self._kf, name)


def run_reference_tracker(load, det, fids, cfg, widen, solver):
    """-> (rows [step, id, box (4), score, depth, scale] float64, live ids (n,), means (n, 8), covariances (n, 8, 8),
    tentative (n,))."""
    Tracker = load('mmtrack.models.trackers.ocsort_tracker_disparity').OCSORTTracker_Disparity
    KF = load('mmtrack.models.motion.kalman_filter').KalmanFilter
    sys.modules['lap'].lapjv = solver          # the stand-in module's attribute: the reference calls lap.lapjv(...)

    class _Model:
        motion = _WidenInitiate(KF()) if widen else KF()

    trk = Tracker(**cfg)
    rows = []
    for s, fid in enumerate(fids):
        d = det[det[:, 0] == s]
        inst = otr.Instances(bboxes=torch.from_numpy(d[:, 1:5].copy()), scores=torch.from_numpy(d[:, 5].copy()),
                             labels=torch.zeros(len(d), dtype=torch.long), scales=torch.from_numpy(d[:, 7].copy()),
                             depth=torch.from_numpy(d[:, 6].copy()))
        r = trk.track(_Model(), None, None, otr.Sample(int(fid), inst))
        for i in range(len(r.instances_id)):
            rows.append([s, int(r.instances_id[i]), *r.bboxes[i].tolist(), float(r.scores[i]), float(r.depth[i]),
                         float(r.scales[i])])
    ids = np.asarray(list(trk.tracks), np.int64)
    means = np.asarray([np.asarray(trk.tracks[i].mean, np.float64) for i in ids]).reshape(-1, 8)
    covs = np.asarray([np.asarray(trk.tracks[i].covariance, np.float64) for i in ids]).reshape(-1, 8, 8)
    tent = np.asarray([bool(trk.tracks[i].tentative) for i in ids], bool)
    return np.asarray(rows, np.float64).reshape(-1, 9), ids, means, covs, tent


def record_tracker(load):
    streams = tracker_streams()
    out = dict(configs=np.asarray(json.dumps(TRACKER_OPTION_SETS, sort_keys=True)))
    committed, rejected = [], []
    for sname, cname in TRACKER_PAIRS:
        det, fids = streams[sname]
        cfg = TRACKER_OPTION_SETS[cname]
        a = run_reference_tracker(load, det, fids, cfg, True, olap.lapjv)
        b = run_reference_tracker(load, det, fids, cfg, True, lapjv_scipy)
        if not all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:2], b[:2])):
            rejected.append(dict(stream=sname, options=cname,
                                 reason='rows differ between oracle/lapjv.py and the linear_sum_assignment shim'))
            continue
        raw = run_reference_tracker(load, det, fids, cfg, False, olap.lapjv)
        key = f'{sname}/{cname}'
        committed.append(key)
        out[f'{sname}/detections'], out[f'{sname}/frame_ids'] = det, fids
        for tag, rec in (('np1', a), ('raw', raw)):
            for k, v in zip(('rows', 'ids', 'means', 'covs', 'tentative'), rec):
                out[f'{key}/{tag}/{k}'] = v
        print(f'  tracker {key:42s} {len(a[0]):4d} rows {len(set(a[0][:, 1].tolist())):3d} ids {len(a[1]):2d} live')
    sys.modules['lap'].lapjv = olap.lapjv
    out['pairs'] = np.asarray(committed)
    return out, dict(candidates=[f'{s}/{c}' for s, c in TRACKER_PAIRS], committed=committed, rejected=rejected,
                     recordings=dict(np1='model.motion = reference KalmanFilter behind a caller-side adapter whose '
                                         'initiate widens the float32 measurement to float64 (numpy 1.x value)',
                                     raw='model.motion = reference KalmanFilter as is, under the running numpy'),
                     solver_condition='a (stream, option set) pair is committed only if ids and rows are identical '
                                      'under oracle/lapjv.py and under scipy.optimize.linear_sum_assignment on the '
                                      'same extended cost matrix')


# --------------------------------------------------------------------------------------------------------------- gmc
def record_gmc(load):
    """apply_gmc_to_tracks_cxcyah on the live track states of a recorded run, for several 2x3 warps."""
    gmc = load('mmtrack.models.trackers.gmc')
    streams = tracker_streams()
    det, fids = streams['occlusion']
    _, ids, means, covs, _ = run_reference_tracker(load, det, fids[:25], TRACKER_OPTION_SETS['defaults'], True,
                                                   olap.lapjv)
    c, s = np.cos(np.deg2rad(3.0)), np.sin(np.deg2rad(3.0))
    warps = np.asarray([
        [[1, 0, 0], [0, 1, 0]],                                              # identity
        [[1, 0, 7.25], [0, 1, -3.5]],                                        # translation
        [[1.04 * c, -1.04 * s, 11.0], [1.04 * s, 1.04 * c, -6.0]],           # similarity: 3 degrees, scale 1.04
        [[0.93, 0.02, -4.0], [-0.01, 1.05, 2.0]],                            # general affine
        [[1, 2, 0], [2, 4, 1]],                                              # singular: det 0 -> the 1e-12 floor
        [[-1, 0, 640], [0, 1, 0]],                                           # reflection: det < 0 -> the floor
    ], np.float32)                                                           # float32, as GLME_affine returns it
    out = dict(ids=ids, means=means, covs=covs, warps=warps)
    for w, warp in enumerate(warps):
        tracks = {int(i): otr.Dict(mean=means[k].copy(), covariance=covs[k].copy()) for k, i in enumerate(ids)}
        tracks[10 ** 6] = otr.Dict(mean=None, covariance=None)               # skipped by the function
        use = [int(i) for i in ids[::-1]] + [10 ** 6]
        gmc.apply_gmc_to_tracks_cxcyah(tracks, use, warp)
        out[f'warp{w}/means'] = np.asarray([tracks[int(i)].mean for i in ids])
        out[f'warp{w}/covs'] = np.asarray([tracks[int(i)].covariance for i in ids])
    return out, dict(note='GLME_affine (cv2) stays unpinned; the warps are given')


# ------------------------------------------------------------------------------------------------------------- depth
DEPTH_METHODS = ('truncated_mean', 'mean', 'median', 'center')


def depth_inputs():
    """(disp (160, 256) float32 with holes, boxes (48, 4) float32) and (disp (736, 1280), the two w > 800 boxes + 2)."""
    rng = np.random.RandomState(131)
    H, W = 160, 256
    disp = np.full((H, W), 2.0, np.float32) + rng.uniform(0, 0.5, (H, W)).astype(np.float32)
    for _ in range(10):
        y, x = rng.randint(0, H - 40), rng.randint(0, W - 60)
        h, w = rng.randint(5, 40), rng.randint(5, 60)
        disp[y:y + h, x:x + w] = rng.uniform(3, 40) + rng.uniform(0, 0.3, (h, w))
    disp[rng.uniform(size=(H, W)) < 0.05] = 0.0
    disp[130:145, 180:210] = 0.0                                                       # an all-invalid window
    disp[20:60, 30:100] = 120.0 + rng.uniform(0, 8.0, (40, 70)).astype(np.float32)     # near: 1 < depth^2 < 3
    boxes = [(32.0, 22.0, 98.0, 58.0), (26.5, 15.0, 110.0, 66.0)]
    for _ in range(36):
        x1, y1 = rng.uniform(0, W - 6), rng.uniform(0, H - 6)
        boxes.append((x1, y1, min(W, x1 + rng.uniform(1, 110)), min(H, y1 + rng.uniform(1, 80))))
    boxes += [(10.2, 10.7, 10.9, 30.0),        # zero width after truncation
              (0.0, 0.0, 1.9, 40.0),           # x2 - 2 < 0: the corner slice starts at a negative index
              (-3.5, 20.0, 40.0, 50.0),        # a negative coordinate
              (50.0, 50.0, 51.5, 51.5),        # 1 x 1
              (180.0, 130.0, 210.0, 145.0),    # all-invalid window
              (0.0, 0.0, 256.0, 160.0),        # touches every border
              (200.0, 100.0, 256.0, 160.0),    # touches the right / bottom border
              (15.0, 8.0, 31.0, 22.0),
              (120.3, 0.0, 121.9, 1.7),        # 1 x 1 at the top border
              (244.6, 150.2, 255.9, 159.9)]    # one pixel short of the corner (a box past the map makes the reference's
                                               # `center` variant raise IndexError, so none is recorded)
    assert len(boxes) == 48
    rng2 = np.random.RandomState(132)
    Hb, Wb = 736, 1280
    big = (4.0 + rng2.uniform(0, 30.0, (Hb // 16, Wb // 16))).astype(np.float32).repeat(16, 0).repeat(16, 1)
    yy, xx = np.mgrid[:Hb, :Wb]              # 16 x 16 blocks and a regular hole pattern: the file has to compress
    big[(yy * 7 + xx * 13) % 31 == 0] = 0.0
    big_boxes = [(100.0, 200.0, 901.5, 420.0), (0.0, 0.0, 1280.0, 736.0), (100.0, 200.0, 900.9, 420.0),
                 (300.7, 100.2, 520.1, 330.8)]                                          # w 801, 1280, 800, 220
    return disp, np.asarray(boxes, np.float32), big, np.asarray(big_boxes, np.float32)


def record_depth(load):
    mod = load('mmtrack.models.mot.ocsort_disparity')
    cmp_mod = load('mmtrack.models.mot.depth_extraction_comparison')
    cls = mod.OCSORT_Disparity

    class _Self:
        """Stand-in `self` for the unbound calls: the two numbers of the constructor defaults and the class's own
        (unmodified) functions as methods."""
        baseline, focal_length = 0.25, 640
    for name in ('disp2depth', 'extract_depth', 'bbox_postp_depth'):
        setattr(_Self, name, getattr(cls, name))
    me = _Self()
    disp, boxes, big, big_boxes = depth_inputs()
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')      # np.mean of an empty slice -> NaN: the reference's own behaviour
        for tag, d, b in (('small', disp, boxes), ('big', big, big_boxes)):
            disp3 = torch.from_numpy(np.repeat(d[None, None], 3, 1))
            bx = torch.from_numpy(b)
            depth = cls.disp2depth(me, disp3[:, 0:1])
            values, scales = cls.extract_depth(me, depth, bx)
            inst, dv = cls.bbox_postp_depth(me, dict(bboxes=bx.clone()), disp3)
            assert [float(v) for v in dv['d_values']] == [float(v) for v in values] or \
                np.array_equal(np.asarray(dv['d_values'], np.float64), np.asarray(values, np.float64), equal_nan=True)
            out[f'{tag}/disp'], out[f'{tag}/boxes'] = d, b
            out[f'{tag}/depth_map'] = depth[0, 0].numpy() if tag == 'small' else depth[0, 0, ::16, ::16].numpy()
            out[f'{tag}/values'] = np.asarray([float(v) for v in values], np.float64)     # float32 values, -1 and NaN
            out[f'{tag}/scales'] = np.asarray([float(v) for v in scales], np.float64)
            out[f'{tag}/postp_scaled_boxes'] = inst['bboxes'].numpy()
            out[f'{tag}/postp_scales'] = inst['scales'].numpy()
            out[f'{tag}/postp_depth'] = inst['depth'].numpy()
            out[f'{tag}/scale_bbox'] = load('mmtrack.models.trackers.utils').scale_bbox(
                bx, torch.Tensor(scales).to(bx)).numpy()
            for m in DEPTH_METHODS:
                wrapped = getattr(cmp_mod, m + '_decorator')(cls.extract_depth)
                v, s = wrapped(me, depth, bx)
                out[f'{tag}/{m}/values'] = np.asarray([float(x) for x in v], np.float64)
                out[f'{tag}/{m}/scales'] = np.asarray([float(x) for x in s], np.float64)
    out['baseline'], out['focal_length'] = np.float64(0.25), np.float64(640)
    return out, dict(note='bbox_postp_depth / extract_depth / disp2depth called unbound on a stand-in self holding '
                          'baseline=0.25, focal_length=640 (the constructor defaults); big/depth_map keeps every 16th '
                          'pixel')


# --------------------------------------------------------------------------------------------------------- tracklets
def record_tracklets(load):
    import tracklets_ref as tr
    Interp = load('mmtrack.models.task_modules.track.interpolation').InterpolateTracklets
    out, names = {}, []
    for mn, mx in ((5, 20), (2, 4)):
        for name, rows in tr.linear_scenarios(mn, mx).items():
            key = f'linear/{mn}_{mx}/{name}'
            names.append(key)
            out[key + '/rows'] = rows
            out[key + '/out'] = Interp(min_num_frames=mn, max_num_frames=mx).forward(rows[:, :7].copy())
    gsi = []
    for name, case in tr.gsi_cases().items():
        rows = tr.gsi_rows(case)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res = Interp(min_num_frames=5, max_num_frames=20, use_gsi=True, smooth_tau=int(case['tau'])).forward(rows)
        gsi.append(name)
        out[f'gsi/{name}/rows'], out[f'gsi/{name}/out'] = rows, np.asarray(res, np.float64)
    out['linear_names'], out['gsi_names'] = np.asarray(names), np.asarray(gsi)
    return out, dict(note='forward() output order is an unstable argsort on the frame: tests compare after ordering by '
                          '(frame, id) and check the multiset separately')


# ------------------------------------------------------------------------------------------------------------ aflink
AFLINK_SEED = 7
AFLINK_SETS = ((41, 12, dict(frames=60, max_len=15, extent=60.0)), (35, 8, dict(frames=40, max_len=12, extent=50.0)),
               (33, 5, dict(frames=60)))        # (seed, tracks <= 12, options) of aflink_cases.video


def canonical_ids(rows):
    """The rows with the ids renumbered 0 .. N-1 in the order of the tracks' first frames, which must be distinct: the
    one input form on which the reference's relabelling (matrix indices used as ids) is well defined."""
    ids = np.unique(rows[:, 1])
    first = {i: rows[rows[:, 1] == i, 0].min() for i in ids}
    assert len(set(first.values())) == len(ids), 'two tracks start in the same frame: pick another seed'
    rank = {i: k for k, i in enumerate(sorted(ids, key=lambda i: first[i]))}
    out = rows.copy()
    out[:, 1] = [rank[i] for i in rows[:, 1]]
    return out


def record_aflink(load):
    """AFLinkModel and AppearanceFreeLink.forward with the seeded weights of aflink_cases.recipe_state_dict: the
    network's inputs and outputs for every pair the reference scores (read by a torch forward hook on the module, in the
    order of the reference's own loop) and the relabelled rows."""
    import aflink_cases
    import aflink_ref
    mod = load('mmtrack.models.task_modules.track.aflink')
    sd = aflink_cases.recipe_state_dict(AFLINK_SEED)
    sets = [canonical_ids(aflink_cases.video(s, n, **kw)) for s, n, kw in AFLINK_SETS]
    sets.append(aflink_cases.video(*AFLINK_SETS[0][:2], **AFLINK_SETS[0][2]))     # set 0 under its own, unordered ids
    # INPUT construction only: fc2 rescaled so that the confidences of these sets' candidates spread over (0, 1), and
    # the threshold put into the widest gap between the quartiles (as aflink_cases.case does).  The rescaled fc2 is
    # stored in the fixture; everything else is the recipe.
    xs = []
    for rows in sets:
        _, _, infos = aflink_ref.tracks(rows)
        xs.append(aflink_ref.inputs(infos, np.argwhere(aflink_ref.gate_flags(infos))))
    x = np.concatenate(xs)
    _, lg = aflink_ref.scores(sd, x, torch.float64)
    d = lg[:, 1] - lg[:, 0]
    scale = 2.5 / max(float(d.std()), 1e-12)
    shift = float(np.median(d)) * scale
    w, b = sd['classifier.fc2.weight'].double(), sd['classifier.fc2.bias'].double()
    sd['classifier.fc2.weight'] = (w * scale).float()
    sd['classifier.fc2.bias'] = (b * scale - torch.tensor([-shift / 2, shift / 2], dtype=torch.float64)).float()
    conf64 = np.sort(aflink_ref.scores(sd, x, torch.float64)[0])
    q0, q1 = len(conf64) // 4, 3 * len(conf64) // 4
    k = q0 + int(np.argmax(np.diff(conf64[q0:q1 + 1])))
    threshold = float((conf64[k] + conf64[k + 1]) / 2)

    link = mod.AppearanceFreeLink(checkpoint='', confidence_threshold=threshold)
    link.model.load_state_dict(sd)
    link.model.eval()
    seen = []
    hook = link.model.register_forward_hook(
        lambda m, args, res: seen.append((args[0].detach().numpy().copy(), args[1].detach().numpy().copy(),
                                          res.detach().numpy().copy())))
    out = dict(seed=np.int64(AFLINK_SEED), state_dict_sha256=np.asarray(aflink_cases.state_dict_sha256(sd)),
               fc2_weight=sd['classifier.fc2.weight'].numpy(), fc2_bias=sd['classifier.fc2.bias'].numpy(),
               threshold=np.float64(threshold), num_sets=np.int64(len(sets)))
    with torch.no_grad():
        for s, rows in enumerate(sets):
            del seen[:]
            res = link.forward(rows.copy())
            out[f'set{s}/rows'], out[f'set{s}/linked'] = rows, res
            out[f'set{s}/x1'] = np.asarray([a[0, 0] for a, _, _ in seen], np.float32).reshape(-1, 30, 5)
            out[f'set{s}/x2'] = np.asarray([b[0, 0] for _, b, _ in seen], np.float32).reshape(-1, 30, 5)
            out[f'set{s}/conf'] = np.asarray([c for _, _, c in seen], np.float32).reshape(-1)
            print(f'  aflink set {s}: {len(np.unique(rows[:, 1]))} tracks, {len(seen)} scored pairs, '
                  f'{int((out[f"set{s}/conf"] >= threshold).sum())} above the threshold, '
                  f'{len(np.unique(res[:, 1]))} ids after linking')
    hook.remove()
    return out, dict(weights='aflink_cases.recipe_state_dict(seed) (numpy RandomState: frozen stream) with classifier.fc2 '
                             'rescaled; the full state dict is 4.2 MB, above the size condition, so the fixture stores '
                             'the seed, the rescaled fc2, and the sha256 of every tensor instead',
                     ids='sets 0-2: ids renumbered 0 .. N-1 by first frame (distinct first frames), where the reference\'s '
                         'relabelling by matrix index is well defined; set 3 = set 0 under its own ids: the reference '
                         'relabels by index there (DESIGN.md section 18, "Ids, not indices") and only its network '
                         'inputs and outputs are compared',
                     outputs='inputs and outputs of AFLinkModel.forward read by a torch forward hook, in the order of the '
                             'reference\'s loop over (i, j)')


# ----------------------------------------------------------------------------------------------------------- loading
def record_loading(load):
    """LoadDisparityFromFile._post_processing_v2, called unbound (it reads nothing from self), on uint16 code arrays
    with 65535 holes."""
    cls = load('mmtrack.datasets.transforms.loading_disparity').LoadDisparityFromFile
    out = {}
    for k, (h, w) in enumerate(((50, 70), (48, 72))):
        rng = np.random.RandomState(200 + k)
        codes = rng.randint(0, 4096, (h, w)).astype(np.uint16)
        codes[rng.uniform(size=(h, w)) < 0.1] = 65535
        codes[0, 0], codes[h - 1, w - 1], codes[1, 1], codes[2, 2] = 65535, 65534, 0, 1
        for ch in (1, 3):
            disp = np.repeat(codes[:, :, None], ch, axis=-1)
            given = disp.copy()
            out[f'{h}x{w}/c{ch}/postp'] = cls._post_processing_v2(None, dict(disp=given))
            out[f'{h}x{w}/c{ch}/disp_after'] = given          # the function zeroes the holes of its input in place
        out[f'{h}x{w}/codes'] = codes
    return out, dict(note='_post_processing_v2 called unbound with self=None; mmcv.transforms.BaseTransform is an inert '
                          'placeholder base class (the class is never instantiated)')


FAMILIES = dict(kalman=record_kalman, tracker=record_tracker, gmc=record_gmc, depth=record_depth,
                tracklets=record_tracklets, aflink=record_aflink, loading=record_loading)


def record(ref_root, families=None):
    """-> ({family: {array name: ndarray}}, manifest dict).  Pure: writes nothing."""
    import scipy
    import sklearn
    arrays, manifest = {}, dict(
        versions=dict(numpy=np.__version__, scipy=scipy.__version__, torch=torch.__version__.split('+')[0],
                      sklearn=sklearn.__version__),
        numpy_note='the reference pins numpy 1.x; *_np1 / f32_widened recordings reproduce its value-based casting by '
                   'widening the float32 Kalman measurement to float64 on the caller\'s side (see the recorder)',
        shims=SHIM_NOTES, families={})
    torch.set_num_threads(1)
    for fam in families or FAMILIES:
        with reference_modules(ref_root) as load:
            out, info = FAMILIES[fam](load)
            arrays[fam] = {k: np.asarray(v) for k, v in out.items()}
            info['files'] = {f: sha256_of(os.path.join(ref_root, f)) for f in sorted(load.used_files)}
            info['placeholders_handed_out'] = sorted(load.finder.handed_out)
            manifest['families'][fam] = info
    return arrays, manifest


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__.split('\n\n')[2])
    ref_root, wanted = argv[1], argv[2:]
    if not os.path.isdir(os.path.join(ref_root, 'mmtrack')):
        sys.exit(f'make_reference_golden.py: no reference tree at {ref_root!r} (expected {ref_root}/mmtrack/)')
    arrays, manifest = record(ref_root, wanted or None)
    os.makedirs(OUT, exist_ok=True)
    mpath = os.path.join(OUT, 'manifest.json')
    if wanted and os.path.exists(mpath):                      # a partial run keeps the other families' entries
        with open(mpath) as f:
            old = json.load(f)
        old['families'].update(manifest['families'])
        manifest = dict(manifest, families=old['families'])
    for fam, arrs in arrays.items():
        path = os.path.join(OUT, fam + '.npz')
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size < MAX_NPZ_BYTES, f'{path}: {size} bytes, the limit is {MAX_NPZ_BYTES}'
        print(f'wrote {fam}.npz  {size} bytes, {len(arrs)} arrays')
    with open(mpath, 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write('\n')
    total = sum(os.path.getsize(os.path.join(OUT, n)) for n in os.listdir(OUT))
    assert total < MAX_DIR_BYTES, f'{OUT}: {total} bytes, the limit is {MAX_DIR_BYTES}'
    print(f'{OUT}: {total} bytes')


if __name__ == '__main__':
    main(sys.argv)
