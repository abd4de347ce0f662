"""GPU: every cross-stream handoff of the package under forced adverse schedules (tests/stream_schedule.py; DESIGN.md 2,
"Stream contract").

A scenario is one product path driven entirely under a side stream: a warm call (streams and lazily allocated buffers
exist, the persistent buffers hold valid data of ANOTHER problem), a plain run (the reference, under the Recorder), then
one run per entry point the Recorder saw with a device-side delay in front of that entry point, and one run per stream
the package created (plus the caller's) with a delay at the head of that stream before every product call.  Every
delayed run must equal the plain run bit for bit: a missing ordering edge lets a consumer read the previous round's
data and the result changes.

Scenarios: P = InflightPipelines.submit (every form of the stereo module, SGBM, a depth estimator), H = the shell's
test_step over six configs at two (inflight, queue_depth) settings, M = MultiStreamTracker through step() and run(),
Q = a sequence.py run through the RawFrameUploader's copy stream, E = the single-stream users of the library.

The delay D = max(50 ms, 2 x t0) capped at 500 ms (t0: the longest host wall time of one plain product call) is a
strength parameter, not a pass bar; the planted race and the two sabotage checks at the end prove that D is long enough
to expose a missing edge in the real product.

$ST_STREAM_SCHEDULE_OUT=<file>: t0, D, the entry points and streams seen, the query() outcomes and the sabotage outcomes
are written there as JSON (how profiles/stream_schedule.json is produced)."""
import json
import os
import time

import numpy as np
import pytest
import torch

import stream_schedule as ss
from stereotracking_amd import _lib
from stereotracking_amd.pipeline import InflightPipelines
from stereotracking_amd.structures import InstanceData, TrackDataSample
from stereotracking_amd.synthetic import synthetic_batch, synthetic_state_dict
from test_cpu_stream_schedule import BLOCKING, COVER, EXEMPT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort')
ORI = (64, 96)
MAX_DISP = 32
REPORT = {}


def _report(key, **values):
    REPORT.setdefault(key, {}).update(values)
    path = os.environ.get('ST_STREAM_SCHEDULE_OUT')
    if path:
        with open(path, 'w') as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def _noop():
    pass


# ---- scenarios -----------------------------------------------------------------------------------------------------
class Scenario:
    """One product path.  drive(before_call) makes every product call of one run, calling before_call() in front of
    each, and returns everything the run produced; it is entered under the side stream and the stream is synchronised
    before the results are compared."""

    def __init__(self, name, cuda):
        self.name, self.cuda = name, cuda
        self.side = torch.cuda.Stream(device=cuda)
        self.lib = _lib.load()
        with torch.cuda.stream(self.side):
            ss.calibrate()
            with ss.recording_streams() as created:
                self.build()
                self.run(_noop)                          # the warm call
                self.warm_other()
            self.created = list(created)
            self.call_times = []
            with ss.Recorder(self.lib) as rec:
                self.plain = self.run(self._timed)
            self.recorder = rec
        self.t0 = max(self.call_times)
        self.D = ss.delay_length(self.t0)
        print(f'{name}: t0 = {self.t0 * 1e3:.2f} ms, D = {self.D:.0f} ms, {len(self.created)} streams created, '
              f'entries {rec.entries()}')
        _report(name, t0_ms=round(self.t0 * 1e3, 3), D_ms=round(self.D, 3), entries=rec.entries(),
                streams=dict(created=len(self.created), seen_by_entries=len(rec.streams())))

    def _timed(self):
        now = time.perf_counter()
        if getattr(self, '_t_last', None) is not None:
            self.call_times.append(now - self._t_last)
        self._t_last = now

    def build(self):
        raise NotImplementedError

    def warm_other(self):
        """Leave valid data of another problem in the persistent buffers (default: the warm call's own)."""

    def drive(self, before_call):
        raise NotImplementedError

    def run(self, before_call):
        self._t_last = None
        with torch.cuda.stream(self.side):
            out = self.drive(before_call)
            if before_call == self._timed:
                self.side.synchronize()
                self._timed()                            # closes the last call's interval
            self.side.synchronize()
        return out

    def streams(self):
        """[(label, stream)]: the caller's side stream and every stream the package created."""
        return [('caller', self.side)] + [(f'created{i}', s) for i, s in enumerate(self.created)]


def _pipe_inputs(mono, seeds, cuda):
    out = []
    for s in seeds:
        b = synthetic_batch([s, s + 100], ORI[0], ORI[1], MAX_DISP)
        if mono:
            out.append(dict(img=b['img'].to(cuda), disp_postp=b['disp_postp'].to(cuda)))
        else:
            out.append(dict(img=b['img'].to(cuda), right=b['right'].to(cuda)))
    return out


class PipesScenario(Scenario):
    """P: InflightPipelines.submit, five submits.  Every batch is copied into ONE preallocated input buffer on the
    caller's stream right before its submit (so the buffer holds the previous batch until that copy has run); the test
    is the consumer: it waits on the returned event on its own stream and clones `out`."""

    KINDS = {'mono': dict(n=2, stereo=False), 'costvolume_lrcheck': dict(n=2, stereo=True, lr_check=True, agg_layers=1),
             'sgbm': dict(n=1, stereo=False, sgbm=dict(num_disparities=32, block_size=3, speckle_window_size=20)),
             # the remaining forms of the stereo module (stereo.py): the plain volume, 3-D aggregation, and the
             # full-resolution mode in its two-kernel and its single-kernel form
             'costvolume': dict(n=2, stereo=True),
             'costvolume_agg3d': dict(n=2, stereo=True, agg3d_layers=1),
             'fullres_agg3d': dict(n=2, stereo=True, full_res=True, agg3d_layers=2, max_disp=48),
             'fullres_single_kernel': dict(n=2, stereo=True, full_res=True, agg3d_layers=1, max_disp=48,
                                           fuse_softargmin=True),
             'median_depth': dict(n=2, stereo=False, depth_method='median')}

    def __init__(self, kind, cuda):
        self.kind = kind
        super().__init__('P/' + kind, cuda)

    def build(self):
        opt = dict(self.KINDS[self.kind])
        n, fuse = opt.pop('n'), opt.pop('fuse_softargmin', False)
        opt.setdefault('max_disp', MAX_DISP)
        self.pipes = InflightPipelines(n, 2, ORI, 0.375, 0.33, 1, max_det=200, **opt)
        for p in self.pipes.pipes:
            p.stereo_module.fuse_softargmin = fuse      # opt-in form of the full-resolution mode (stereo.py)
        sd = synthetic_state_dict(self.pipes.param_table(), seed=21, prior_prob=0.2, logit_std=2.5)
        self.pipes.load_state_dict(sd, autotune=False)
        self.batches = _pipe_inputs(not self.pipes.takes_right, range(300, 305), self.cuda)
        self.staged = {k: torch.zeros_like(v) for k, v in self.batches[0].items()}
        torch.cuda.synchronize()

    def drive(self, before_call):
        self.pipes._next = 0        # submit i runs on the same context in every run (their never-written cells differ)
        outs = []
        for batch in self.batches:
            before_call()
            for k, v in batch.items():
                self.staged[k].copy_(v)
            out, ev = self.pipes.submit(**self.staged)
            torch.cuda.current_stream().wait_event(ev)
            outs.append({k: v.clone() for k, v in out.items()})
        return outs


def _shell_frames(kind, seeds, cuda):
    """Per-frame input dicts as a dataset yields them + per-frame gt boxes (numpy), at ORI."""
    import disp_fuse_inputs as fuse
    b = synthetic_batch(list(seeds), ORI[0], ORI[1], MAX_DISP)
    frames = []
    for i, s in enumerate(seeds):
        f = dict(img=b['img'][i:i + 1].to(torch.uint8).to(cuda))
        disp = b['disp_postp'][i:i + 1]
        if kind == 'mono':
            f['disp_postp'] = disp.to(cuda)
            f['disp_mask'] = b['disp_mask'][i:i + 1].to(torch.uint8).to(cuda)
            f['depth_postp'] = (disp * 0.75 + 2.0).to(cuda)
        elif kind == 'fused':      # the input disparity has holes over the gt boxes: the head's pixels are read there
            f['disp_postp'] = torch.from_numpy(fuse.punch(disp[0].numpy(), fuse.gt_boxes(s)))[None].to(cuda)
            f['depth_postp'] = (0.25 * 640 / disp[:, :1].clamp(min=1.0)).to(cuda)
        else:
            f['right'] = b['right'][i:i + 1].to(torch.uint8).to(cuda)
            f['depth_postp'] = (0.25 * 640 / disp[:, :1].clamp(min=1.0)).to(cuda)
        frames.append(f)
    return frames, [fuse.gt_boxes(s) for s in seeds]


def _shell_data(frames, boxes, first_id, extra=None):
    samples = []
    for t in range(len(frames)):
        s = TrackDataSample(dict(dict(frame_id=first_id + t, ori_shape=ORI, img_shape=ORI, scale_factor=(1.0, 1.0)),
                                 **(extra[t] if extra else {})))
        s.gt_instances = InstanceData(bboxes=torch.from_numpy(boxes[t]))
        samples.append(s)
    return dict(inputs={k: [f[k] for f in frames] for k in frames[0]}, data_samples=samples)


def _small_calibration():
    """Rotating and distorting cameras (different left and right) for ORI-sized raw frames."""
    fx, cx, cy = 90.0, 47.5, 31.5
    P = [[fx, 0.0, cx, 0.0], [0.0, fx, cy, 0.0], [0.0, 0.0, 1.0, 0.0]]

    def rot(v):
        v = np.asarray(v, np.float64)
        th = np.linalg.norm(v)
        k = v / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx).tolist()
    return dict(type='StereoRectify', size=ORI, border=0,
                left=dict(K=[[91.0, 0, 46.5], [0, 90.5, 32.0], [0, 0, 1]], D=[-0.12, 0.03, 0.001, -0.002, 0.01],
                          R=rot([0.02, -0.03, 0.015]), P=P),
                right=dict(K=[[89.5, 0, 48.5], [0, 90.0, 31.0], [0, 0, 1]], D=[-0.1, 0.02, -0.001, 0.001],
                           R=rot([-0.015, 0.02, -0.02]), P=[[fx, 0.0, cx, -18.0], P[1], P[2]]))


# config file -> (input kind, changes to the config's model dict at test size)
SHELL_CONFIGS = {
    'disp': ('yolox_s_mmyolo_mot_airdrone_disp.py', 'mono', None),
    'costvolume_lrcheck': ('stereo_yolox_s_mot_airdrone_costvolume_lrcheck.py', 'stereo', None),
    'sgbm_rectify': ('stereo_yolox_s_mot_airdrone_sgbm_rectify.py', 'stereo', 'rectify'),
    'completion_v2_fused': ('yolox_s_mmyolo_mot_airdrone_disp_completion_v2_fused.py', 'fused', None),
    'disp_ecc': ('yolox_s_mmyolo_mot_airdrone_disp_ecc.py', 'mono', None),
    'sgbm_dispeval': ('stereo_yolox_s_mot_airdrone_sgbm_dispeval.py', 'stereo', None),
}


def build_shell(config, **options):
    """The config's shell at test size, as tests/test_disp_head_gpu.py's _build makes it: the heuristic launch plan (the
    same kernels in every run), seeded synthetic weights, score gates that let random weights start tracks."""
    import disp_head_ref
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    path, kind, special = SHELL_CONFIGS[config]
    cfg = Config.fromfile(os.path.join(CFG_DIR, path))
    cfg.model.tracker['init_track_thr'] = 0.03
    cfg.model.tracker['obj_score_thr'] = 0.02
    extra = {}
    if cfg.model.get('stereo') is not None and cfg.model.stereo.get('type') == 'StereoCostVolume':
        cfg.model.stereo['max_disp'] = MAX_DISP
    if cfg.model.get('stereo') is not None and cfg.model.stereo.get('type') == 'StereoSGBM':
        cfg.model.stereo['num_disparities'] = 32
    if special == 'rectify':
        extra['rectify'] = _small_calibration()
    if kind == 'fused':
        cfg.model.detector.disparity_head['channels'] = 32
    model = MODELS.build(dict(cfg.model, **dict(dict(autotune=False, dense_batch=2), **extra, **options)))
    table = list(model.detector._table)
    has_agg = model.stereo is not None and hasattr(model.stereo, 'param_table')
    if has_agg:
        table += [('stereo.' + n, shp) for n, shp in model.stereo.param_table()]
    sd = synthetic_state_dict(table, seed=5, prior_prob=0.2, logit_std=2.5)
    if kind == 'fused':
        head = disp_head_ref.random_state_dict(128, 32, seed=31)
        head['reg.conv.weight'] = head['reg.conv.weight'] * 0.05
        head['reg.conv.bias'] = torch.tensor([8.0])
        sd.update({'disp_head.' + k: v for k, v in head.items()})
    missing = model.detector.load_state_dict(sd, strict=False)
    assert not [k for k in missing.missing_keys if not k.endswith('num_batches_tracked')]
    if has_agg:
        model.stereo.load_state_dict({k[len('stereo.'):]: v for k, v in sd.items() if k.startswith('stereo.')})
    return model, kind


class ShellScenario(Scenario):
    """H: the shell's test_step, two consecutive calls of 5 frames of one video at dense_batch 2 (chunks 2 + 2 + 1):
    contexts, disparity ring slots, track_slot_event slots and page-locked buffers are all reused."""

    def __init__(self, config, inflight, queue_depth, cuda):
        self.config, self.inflight, self.queue_depth = config, inflight, queue_depth
        super().__init__(f'H/{config}/inflight{inflight}_queue{queue_depth}', cuda)

    def build(self):
        self.model, kind = build_shell(self.config, inflight=self.inflight, queue_depth=self.queue_depth)
        self.frames, self.boxes = _shell_frames(kind, range(400, 410), self.cuda)
        self.other = _shell_frames(kind, range(450, 455), self.cuda)
        torch.cuda.synchronize()

    def warm_other(self):      # the persistent buffers end up holding a DIFFERENT video's data
        self.model.test_step(_shell_data(*self.other, 0))

    def drive(self, before_call):
        outs = []
        for lo in (0, 5):
            before_call()
            outs.append(self.model.test_step(_shell_data(self.frames[lo:lo + 5], self.boxes[lo:lo + 5], lo)))
        return outs


class MultiStreamScenario(Scenario):
    """M: MultiStreamTracker on the stereo cost-volume config: 3 streams at chunk 2 (two chunks per tick, more slots than
    streams), 4 ticks, with gt depth maps; through step(), or through run() with ahead = 2."""

    def __init__(self, use_run, cuda):
        self.use_run = use_run
        super().__init__('M/' + ('run_ahead2' if use_run else 'step'), cuda)

    def build(self):
        from stereotracking_amd.multistream import MultiStreamTracker
        self.model, kind = build_shell('costvolume_lrcheck', inflight=2)
        self.mst = MultiStreamTracker(self.model, streams=3, max_tracks=512)
        assert (self.mst.chunk, self.mst.max_chunks) == (2, 2)
        if self.use_run:
            self.mst.ahead = 2
        self.videos = [_shell_frames(kind, range(500 + 10 * s, 504 + 10 * s), self.cuda) for s in range(3)]
        torch.cuda.synchronize()

    def _tick(self, t):
        order = [(t + k) % 3 for k in range(3)]      # the slot of a stream changes from tick to tick
        frames = [self.videos[s][0][t] for s in order]
        boxes = [self.videos[s][1][t] for s in order]
        return _shell_data(frames, boxes, 0, extra=[dict(stream=s, frame_id=t) for s in order])

    def drive(self, before_call):
        if self.use_run:
            before_call()
            return list(self.mst.run(self._tick(t) for t in range(4)))
        outs = []
        for t in range(4):
            before_call()
            outs.append(self.mst.step(self._tick(t)))
        return outs


class SequenceScenario(Scenario):
    """Q: one short sequence.py run (6 frames, batches of 2 over 2 contexts) of the disparity-input configuration
    through a RawFrameUploader kept across runs: its copy stream, its alternating page-locked slots and device byte
    buffers are reused.  raw_stem: the image reaches the stem as uint8 (the codes still go through st_pack_raw_inputs),
    else both inputs are cast + padded by st_pack_raw_inputs."""

    def __init__(self, raw_stem, cuda):
        self.raw_stem = raw_stem
        super().__init__('Q/' + ('raw_stem' if raw_stem else 'packed'), cuda)

    def build(self):
        from stereotracking_amd.sequence import RawFrameUploader, synthetic_sequence
        self.pipes = InflightPipelines(2, 2, ORI, 0.375, 0.33, 1, stereo=False, max_det=200)
        sd = synthetic_state_dict(self.pipes.param_table(), seed=9, prior_prob=0.2, logit_std=2.5)
        self.pipes.load_state_dict(sd, autotune=False)
        self.frames = list(synthetic_sequence(6, 3, ORI[0], ORI[1], MAX_DISP, seed=8))
        self.other = list(synthetic_sequence(6, 3, ORI[0], ORI[1], MAX_DISP, seed=11))
        self.uploader = RawFrameUploader(2, ORI, self.cuda, use_right=False, raw_stem=self.raw_stem)

    def _detect(self, frames):
        from stereotracking_amd.sequence import detect_shard
        self.pipes._next = 0
        return detect_shard(self.pipes, frames, self.cuda, uploader=self.uploader)

    def warm_other(self):
        self._detect(self.other)

    def drive(self, before_call):
        before_call()
        return self._detect(self.frames)


def _to_host(obj):
    """The result tree with every device tensor copied to the host (waits for the current stream)."""
    if torch.is_tensor(obj):
        return obj.cpu()
    if isinstance(obj, dict):
        return {k: _to_host(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_host(v) for v in obj)
    return obj


class CallScenario(Scenario):
    """E: a single-stream user of the library on a side stream; make(cuda) -> call(v), which makes the call(s) on
    problem v (0 or 1: two seeded input sets of the same shapes, through the same modules and cached workspaces) and
    returns their results.  A run is problem 1, then problem 0, both returned (copied to the host call by call): the
    blocks the caching allocator hands back, and every persistent workspace, hold the OTHER problem's valid values
    when a call starts.  What this tier can see: an entry point, or a wrapper between two entry points, that works off the passed
    stream reads its predecessor's unwritten output - the other problem's - and the result changes.  An off-stream
    launch of the FIRST entry point of a call is not visible here (its inputs were complete long before)."""

    def __init__(self, name, make, cuda):
        self.make = make
        super().__init__('E/' + name, cuda)

    def build(self):
        self.call = self.make(self.cuda)
        torch.cuda.synchronize()

    def drive(self, before_call):
        before_call()
        # each problem's results move to the host before the next call: every device block of the call is free again,
        # and the allocator hands the next call (the same sizes in the same order) those very blocks, role by role
        return [_to_host(self.call(1)), _to_host(self.call(0))]


class GatherScenario(Scenario):
    """G: dist.DetectionGatherer under a process group of ONE rank on the 'nccl' backend (single_rank_collective: the
    all-gather of one shard is a device copy through the communicator, on the gatherer's communication stream).  Two
    problems per run through one pipeline and ONE preallocated gather buffer: the frame records are packed on the
    caller's stream, the collective waits for the `ready` event recorded there, the consumer waits for `done` and clones.
    Runs in tests/stream_schedule_worker.py (the process group needs a process of its own)."""

    def __init__(self, cuda):
        super().__init__('G/one_rank_gather', cuda)

    def build(self):
        from stereotracking_amd.dist import DetectionGatherer
        from stereotracking_amd.pipeline import StereoDensePipeline
        self.pipe = StereoDensePipeline(2, ORI, 0.375, 0.33, 1, stereo=False, max_det=200)
        sd = synthetic_state_dict(self.pipe.param_table(), seed=21, prior_prob=0.2, logit_std=2.5)
        self.pipe.load_state_dict(sd, autotune=False)
        self.batches = _pipe_inputs(True, (800, 801), self.cuda)
        self.gatherer = DetectionGatherer(self.cuda, single_rank_collective=True)
        assert self.gatherer.on_device and self.gatherer.world == 1
        self.out = torch.zeros(2, self.pipe.max_det + 1, 8, device=self.cuda)
        torch.cuda.synchronize()

    def drive(self, before_call):
        res = []
        for v in (1, 0):
            before_call()
            o = self.pipe.run(self.batches[v]['img'], disp_postp=self.batches[v]['disp_postp'])
            rec = self.pipe.pack_detections(o, scaled=True, n_real=2)
            out, done = self.gatherer.gather(rec, out=self.out)
            torch.cuda.current_stream().wait_event(done)
            res.append(dict(gathered=out.clone(), records=rec.clone()))
        return res


def all_delayed_runs_equal(sc):
    """The three sweeps of the tests below on one scenario (for a scenario that lives in a worker process)."""
    _assert_same(sc, sc.run(_noop), 'a second plain run')
    early = {}
    for entry in sc.recorder.entries():
        with ss.Delayed(sc.lib, [entry], sc.D) as d:
            got = sc.run(_noop)
        _assert_same(sc, got, f'a delay in front of {entry}')
        early[entry] = dict(calls=len(d.returned_early[entry]), returned_before_the_device=sum(d.returned_early[entry]))
        assert entry in BLOCKING or all(d.returned_early[entry]), f'{sc.name}: {entry} waited for the device'
    for label, stream in sc.streams():
        _assert_same(sc, sc.run(ss.StreamDelayed(stream, sc.D)), f'a delay at the head of stream {label}')
    return dict(query=early, streams_delayed=[label for label, _ in sc.streams()])


def _e_mot_eval(cuda):
    import mot_eval_cases as cases
    from stereotracking_amd import mot_eval

    def other():      # random_b3's three videos from other seeds: the same sizes, other boxes
        out = {}
        for name, (seed, T, n) in dict(a=(12, 12, 3), b=(13, 40, 20), c=(14, 5, 7)).items():
            out[name] = cases.jittered_sequence(seed, T, n, frame_step=2 if name != 'c' else 1,
                                                id_scale=1000003 if name == 'a' else 7, switch_at=T // 2)
        return {k: v[0] for k, v in out.items()}, {k: v[1] for k, v in out.items()}
    packed = [mot_eval.pack_sequences(*cases.scenario('random_b3')), mot_eval.pack_sequences(*other())]
    return lambda v: mot_eval.evaluate_packed(packed[v], 0.5, device=cuda, return_arrays=True)


def _e_kitti(cuda):
    import kitti_eval_cases as cases
    from stereotracking_amd import mot_eval
    sequences = [list(cases.random_sequences().values()), [cases.random_sequence(50 + s) for s in range(3)]]
    return lambda v: mot_eval.kitti_keep_masks(sequences[v], cases.BOTH, device=cuda)


def _e_motchallenge(cuda):
    import motchallenge_ref as ref
    from stereotracking_amd import mot_eval
    videos = [ref.videos()[k][:2] for k in ('v0', 'v1')]
    rows = [torch.from_numpy(np.random.RandomState(3 + v).uniform(-50, 50, (64, 5))).to(cuda) for v in range(2)]
    modes = (mot_eval.FILE_TRUNCATE, mot_eval.FILE_ROUND3, mot_eval.FILE_COPY, mot_eval.FILE_ROUND3, mot_eval.FILE_ROUND3)

    def call(v):
        out, status = torch.empty_like(rows[v]), torch.empty(8, dtype=torch.int32, device=cuda)
        mot_eval.file_round(rows[v], modes, out, status)
        gt, pred = videos[v]
        return mot_eval.motchallenge_keep_masks([gt], [pred], device=cuda), out, status
    return call


def _e_coco(cuda):
    from stereotracking_amd.coco_metric import coco_eval_device
    from test_coco_metric_gpu import random_set
    sets = [random_set(4, 30, 2), random_set(9, 30, 2)]
    dev = [[torch.from_numpy(s[k]).to(cuda) for k in ('det_boxes', 'det_scores', 'det_labels')] for s in sets]

    def call(v):
        s = sets[v]
        out = coco_eval_device(*dev[v], torch.from_numpy(s['det_img']), s['gt_boxes'], s['gt_area'], s['gt_crowd'],
                               s['gt_cat'], s['gt_img'], s['num_images'], s['num_cats'])
        return {k: t for k, t in out.items() if torch.is_tensor(t)}
    return call


def _e_tracklets(cuda):
    import tracklets_ref as ref
    from stereotracking_amd.tracklets import InterpolateTracklets
    gsi = ref.gsi_cases()
    names = sorted(gsi, key=lambda n: len(gsi[n]['frames']))[:2]      # the two shortest fixture cases
    sets = [[ref.gsi_rows(gsi[n], tid=i + 1) for i, n in enumerate(names)]]
    # the other problem: the same frames, the boxes moved and stretched
    sets.append([ref.gsi_rows(dict(gsi[n], y=gsi[n]['y'] * 1.25 + 17.0), tid=i + 1) for i, n in enumerate(names)])
    it = InterpolateTracklets(use_gsi=True, smooth_tau=int(gsi[names[0]]['tau']), backend='device')
    return lambda v: it.forward_many(sets[v], device=cuda)


def _e_aflink(cuda):
    """device_stages waits after every stage by design, so gate / transform / score can only show the non-blocking
    outcome there; the ordering case of this scenario is forward_many (st_aflink_run: all stages in one call)."""
    import aflink_cases
    from stereotracking_amd.aflink import AppearanceFreeLink
    c = aflink_cases.case(n_tracks=30)      # the smallest video at which the builder finds its 40 candidates
    rows = [c['rows'], aflink_cases.video(7, 30)]
    link = AppearanceFreeLink(c['state_dict'], confidence_threshold=c['threshold'], backend='device')

    def call(v):
        stages = link.device_stages([rows[v]], device=cuda)
        return link.forward_many([rows[v]], device=cuda), {k: a for k, a in stages.items() if isinstance(a, np.ndarray)}
    return call


def _e_stereo_eval(cuda):
    from stereotracking_amd import stereo_eval
    b = [synthetic_batch([700 + 2 * v, 701 + 2 * v], ORI[0], ORI[1], MAX_DISP) for v in range(2)]
    disp = [x['disp_postp'].to(cuda) for x in b]
    depth = [(0.25 * 640 / (x['disp_postp'][:, :1] * 1.1).clamp(min=1.0)).to(cuda) for x in b]
    ext = torch.tensor([ORI, (ORI[0] - 3, ORI[1] - 5)], dtype=torch.int32).to(cuda)
    edges, taus = stereo_eval.check_options((0, 20, 40, 80), (0.5, 1, 2, 3))
    bf = stereo_eval.bf_float32(0.25, 640)
    return lambda v: stereo_eval.launch_stereo_eval(disp[v], depth[v], 'depth', bf, ext, None, None, edges, taus)


def _detection_videos(cuda, first_seed, V=2, F=6, M=16):
    """(frame_ids (V, F), dets (V, F, M, 8), counts (V, F)) of seeded synthetic detection streams, on the device."""
    from stereotracking_amd.synthetic import synthetic_detection_stream
    fids = np.tile(np.arange(F, dtype=np.int32), (V, 1))
    dets, counts = np.zeros((V, F, M, 8), np.float32), np.zeros((V, F), np.int32)
    for v in range(V):
        det = synthetic_detection_stream(first_seed + v, T=F, K=5)
        for t in range(F):
            d = det[det[:, 0] == t][:M]
            dets[v, t, :len(d), 0:4] = d[:, 1:5]
            dets[v, t, :len(d), 4], dets[v, t, :len(d), 6], dets[v, t, :len(d), 7] = d[:, 5], d[:, 6], d[:, 7]
            counts[v, t] = len(d)
    return tuple(torch.from_numpy(a).to(cuda) for a in (fids, dets, counts))


TRACKER_OPTIONS = dict(obj_score_thr=0.3, init_track_thr=0.5, weight_iou_with_det_scores=True, match_iou_thr=0.3,
                       num_tentatives=3, vel_consist_weight=0.2, vel_delta_t=3, num_frames_retain=30)


def _e_batched_tracker(cuda):
    from stereotracking_amd.batched_assoc import BatchedGpuTracker
    from stereotracking_amd.sweep import TrackerSweep
    problems = [_detection_videos(cuda, 60), _detection_videos(cuda, 80)]
    trk = BatchedGpuTracker(2, max_tracks=32, max_dets=16, device=cuda, **TRACKER_OPTIONS)
    video_of = torch.arange(2, dtype=torch.int32, device=cuda)
    options = [TRACKER_OPTIONS, dict(TRACKER_OPTIONS, match_iou_thr=0.5)]

    def call(v):
        fids, dets, counts = problems[v]
        stepped = []
        for t in range(fids.shape[1]):       # frame_id 0 first: the state restarts in every call
            rows, ids, n = trk.step(fids[:, t].contiguous(), dets[:, t].contiguous(), counts[:, t].contiguous(),
                                    check_status=False)
            stepped.append((rows.clone(), ids.clone(), n.clone()))
        ran = [t.clone() for t in trk.run(fids, dets, counts, video_of)]
        sweep = TrackerSweep(options, max_tracks=32, max_dets=16, device=cuda)
        for k in range(2):
            sweep.add_video(frame_ids=fids[k].cpu().numpy(), dets=dets[k].cpu().numpy(), counts=counts[k].cpu().numpy())
        res = sweep.run()
        return stepped, ran, {k: t for k, t in vars(res).items() if torch.is_tensor(t)}
    return call


def _e_sgbm_stages(cuda):
    from stereotracking_amd.sgbm import StereoSGBM
    h, w = 48, 64
    b = [synthetic_batch([710 + 2 * v, 711 + 2 * v], h, w, 16) for v in range(2)]
    pairs = [(x['img'].to(cuda), x['right'].to(cuda)) for x in b]
    sgbm = StereoSGBM(num_disparities=32, block_size=3, speckle_window_size=20)      # ONE module: its workspace persists

    def call(v):
        left, right = pairs[v]
        out = torch.empty(2, 3, left.shape[-2], left.shape[-1], device=cuda)
        sgbm.compute(left, right, (h, w), out)
        cost, raw = sgbm.match(left, right, (h, w))
        med = sgbm.median(raw)
        spk = sgbm.speckle(med)
        return out, cost, raw, med, spk
    return call


def _e_cmc(cuda):
    from stereotracking_amd import cmc
    h, w = ORI
    f32 = [synthetic_batch([720 + 3 * v, 721 + 3 * v, 722 + 3 * v], h, w, MAX_DISP)['img'].to(cuda) for v in range(2)]
    u8 = [[x[i:i + 1].to(torch.uint8) for i in range(3)] for x in f32]
    pts = [torch.from_numpy(np.random.RandomState(5 + v).uniform(0, 90, (2, 64, 4)).astype(np.float32)).to(cuda)
           for v in range(2)]
    down = int(cmc.ecc_params()['downscale'])

    def call(v):
        p8, p32 = cmc.front(u8[v], h, w), cmc.front(f32[v], h, w)
        flow = cmc.flow(p8[:-1], p8[1:], 31)
        e8, e32 = cmc.ecc_front(u8[v], h, w, down), cmc.ecc_front(f32[v], h, w, down)
        return (p8, p32, flow, cmc.mesh_fit(flow, h, w), cmc.fit(pts[v]), cmc.estimate(p8[:-1], p8[1:], h, w),
                e8, e32, cmc.ecc_estimate(e8[:-1], e8[1:], h, w), cmc.ecc_prepare(e8[:-1], e8[1:], h, w),
                cmc.ecc_step(e8[:-1], e8[1:], h, w))
    return call


def _e_datasets(cuda):
    from stereotracking_amd import datasets as ds
    from stereotracking_amd.mot import pack_raw_inputs
    from stereotracking_amd.shell_inputs import RawFrames
    h, w = 48, 80
    resize = ds.Resize_Disparity(scale=(60, 36), keep_ratio=True)
    problems = []
    for v in range(2):
        rng = np.random.RandomState(5 + v)
        codes = rng.randint(0, 500, (h, w)).astype(np.uint16)
        res = dict(img=rng.randint(0, 256, (h, w, 3)).astype(np.uint8), right=rng.randint(0, 256, (h, w, 3)).astype(np.uint8),
                   disp_codes=codes, disp_postp=np.repeat((codes / 16.0).astype(np.float32)[:, :, None], 3, axis=2),
                   disp_mask=(codes < 400).astype(np.uint8), img_shape=(h, w), ori_shape=(h, w))
        img = torch.from_numpy(rng.randint(0, 256, (3, 3, 50, 76)).astype(np.uint8)).to(cuda)
        code = torch.from_numpy(rng.randint(0, 3000, (3, 50, 76)).astype(np.int16)).to(cuda)
        problems.append((res, img, code, RawFrames([img[i:i + 1] for i in range(3)], (64, 96), 114.0)))

    def call(v):
        res, img, code, frames = problems[v]
        out = resize(dict(res))
        return ({k: a for k, a in out.items() if isinstance(a, np.ndarray)}, pack_raw_inputs(img, code),
                frames.chunk(0, 3, 4))
    return call


E_CASES = dict(mot_eval=_e_mot_eval, kitti=_e_kitti, motchallenge=_e_motchallenge, coco=_e_coco, tracklets=_e_tracklets,
               aflink=_e_aflink, stereo_eval=_e_stereo_eval, batched_tracker=_e_batched_tracker,
               sgbm_stages=_e_sgbm_stages, cmc=_e_cmc, datasets=_e_datasets)


# ---- the module's scenarios: one model each, built on first use ----------------------------------------------------
SCENARIOS = {}
for _k in PipesScenario.KINDS:
    SCENARIOS['P/' + _k] = (PipesScenario, (_k,))
for _c in SHELL_CONFIGS:
    for _i, _q in ((2, 1), (1, 2)):
        SCENARIOS[f'H/{_c}/inflight{_i}_queue{_q}'] = (ShellScenario, (_c, _i, _q))
SCENARIOS['M/step'] = (MultiStreamScenario, (False,))
SCENARIOS['M/run_ahead2'] = (MultiStreamScenario, (True,))
SCENARIOS['Q/raw_stem'] = (SequenceScenario, (True,))
SCENARIOS['Q/packed'] = (SequenceScenario, (False,))
for _k, _make in E_CASES.items():
    SCENARIOS['E/' + _k] = (CallScenario, (_k, _make))


@pytest.fixture(scope='module')
def built(cuda):
    cache = {}

    def get(name):
        if name not in cache:
            cls, args = SCENARIOS[name]
            cache[name] = cls(*args, cuda)
        return cache[name]
    yield get
    cache.clear()


def _assert_same(sc, got, what):
    diff = ss.differences(sc.plain, got)
    assert not diff, f'{sc.name}: {what} (D = {sc.D:.0f} ms) changed the result at {diff[:8]} ({len(diff)} paths)'


@pytest.mark.parametrize('name', list(SCENARIOS))
def test_plain_run_is_reproducible_and_tracks(built, name):
    """The yardstick itself: a second plain run equals the first (otherwise nothing below means anything), and the shell
    scenarios associate tracks (inputs that track nothing prove nothing about the track-depth handoffs)."""
    sc = built(name)
    _assert_same(sc, sc.run(_noop), 'a second plain run')
    if name[0] in 'HM':
        flat = ss.flatten(sc.plain)
        assert sum(len(v) for k, v in flat.items() if k.endswith('pred_track_instances.instances_id')) > 0


@pytest.mark.parametrize('half', [0, 1])
@pytest.mark.parametrize('name', list(SCENARIOS))
def test_delay_in_front_of_each_entry_point(built, name, half):
    """One run per entry point the plain run called (every second one per case: the sweep is split, D is not shortened)
    with D of device-side delay in front of every call of it: same bits, and the entry point has returned while the
    delay was still running unless BLOCKING documents its wait."""
    sc = built(name)
    outcomes = {}
    for entry in sc.recorder.entries()[half::2]:
        with ss.Delayed(sc.lib, [entry], sc.D) as d:
            got = sc.run(_noop)
        _assert_same(sc, got, f'a delay in front of {entry}')
        early = d.returned_early[entry]
        outcomes[entry] = dict(calls=len(early), returned_before_the_device=sum(early))
        _report(name, **{'query_half%d' % half: outcomes})
        if entry not in BLOCKING:
            assert all(early), f'{sc.name}: {entry} waited for the device in {len(early) - sum(early)} of {len(early)} calls'


@pytest.mark.parametrize('name', list(SCENARIOS))
def test_delay_at_the_head_of_each_stream(built, name):
    """One run per stream the package created, plus the caller's, with D of delay at its head before every product
    call: same bits."""
    sc = built(name)
    for label, stream in sc.streams():
        _assert_same(sc, sc.run(ss.StreamDelayed(stream, sc.D)), f'a delay at the head of stream {label}')
    _report(name, streams_delayed=[label for label, _ in sc.streams()])


def test_recorder_saw_every_entry_point_cover_names(built):
    """COVER (tests/test_cpu_stream_schedule.py) is not a wish list: each entry point it assigns to a scenario of this
    file was really called there."""
    missing = {}
    for entry, where in COVER.items():
        if entry in EXEMPT:
            continue
        if where not in SCENARIOS or entry not in built(where).recorder.entries():
            missing[entry] = where
    assert not missing, f'COVER names scenarios that never call the entry point: {missing}'


def test_gatherer_stream_in_a_one_rank_group(cuda, tmp_path):
    """dist.DetectionGatherer's communication stream, as far as one GPU takes it: the G scenario in a process of its own
    with a one-rank 'nccl' group (a file store; the environment as tests/test_multirank_gpu.py sets it for RCCL).  The
    gathered records of every delayed run equal the plain run's, and equal the local records (one rank: a copy)."""
    import subprocess
    import sys
    report = tmp_path / 'report.json'
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'ST_STREAM_SCHEDULE_OUT'):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'stream_schedule_worker.py'), str(tmp_path / 'store'),
                        str(report)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with open(report) as f:
        rec = json.load(f)
    assert 'st_pack_records' in rec['entries'] and rec['streams']['created'] >= 1      # the communication stream
    assert len(rec['streams_delayed']) == 1 + rec['streams']['created']
    _report('G/one_rank_gather', **rec)


# ---- the harness proves its teeth ----------------------------------------------------------------------------------
def _producer_consumer(cuda, ordered, before_call, side, producer):
    """Round r: the producer stream fills ONE float buffer with r, the consumer (the caller's stream) copies it out -
    behind a wait on the producer (`ordered`) or not (the planted race)."""
    buf = torch.zeros(1 << 16, device=cuda)
    seen = []
    with torch.cuda.stream(side):
        torch.cuda.synchronize()
        for r in range(1, 4):
            before_call()
            with torch.cuda.stream(producer):
                buf.fill_(float(r))
            if ordered:
                side.wait_stream(producer)
            seen.append(buf.clone())
            producer.wait_stream(side)       # the next round's write follows this round's read either way
        side.synchronize()
        producer.synchronize()
    return seen


def test_planted_race_differs_and_its_correct_twin_does_not(cuda):
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        ss.calibrate()
    producer = ss.independent_stream([side], cuda)      # on another hardware queue than the consumer
    D = ss.delay_length(0.0)
    want = _producer_consumer(cuda, True, _noop, side, producer)
    assert [float(t[0]) for t in want] == [1.0, 2.0, 3.0]
    twin = _producer_consumer(cuda, True, ss.StreamDelayed(producer, D), side, producer)
    assert ss.same_results(want, twin), 'the ORDERED producer / consumer changed under a delayed producer'
    raced = _producer_consumer(cuda, False, ss.StreamDelayed(producer, D), side, producer)
    assert not ss.same_results(want, raced), 'the planted race (no wait on the producer) went unnoticed'
    # ... and what it read is an EARLIER round's fill, never anything else
    assert all(float(t.max()) < r for r, t in zip((1.0, 2.0, 3.0), raced))
    _report('teeth', planted_race=dict(D_ms=round(D, 3), ordered_equal=True, race_differs=True))


def test_planted_off_stream_wrapper_in_the_single_stream_tier_differs(cuda):
    """The E tier's teeth: StereoSGBM's match and median stages as an E case whose wrapper can be switched to launch
    the median under ANOTHER stream without a wait.  With a delay in front of st_sgbm_match_f32 the ordered wrapper
    equals the plain run; the off-stream one reads the recycled block behind `raw` before the match has written it -
    a previous call's valid values - and differs."""
    from stereotracking_amd.sgbm import StereoSGBM
    planted = dict(on=False)

    def make(cuda):
        h, w = 48, 64
        b = [synthetic_batch([730 + 2 * v, 731 + 2 * v], h, w, 16) for v in range(2)]
        pairs = [(x['img'].to(cuda), x['right'].to(cuda)) for x in b]
        sgbm = StereoSGBM(num_disparities=32, block_size=3, speckle_window_size=20)
        caller = torch.cuda.current_stream()
        rogue = ss.independent_stream([caller], cuda)

        def call(v):
            _, raw = sgbm.match(*pairs[v], (h, w), cost=False)
            if not planted['on']:
                return raw, sgbm.median(raw)
            with torch.cuda.stream(rogue):       # the planted defect: off the caller's stream, and no wait
                med = sgbm.median(raw)
            torch.cuda.current_stream().wait_stream(rogue)
            return raw, med
        return call
    sc = CallScenario('planted_off_stream_median', make, cuda)
    with ss.Delayed(sc.lib, ['st_sgbm_match_f32'], sc.D):
        ordered = sc.run(_noop)
        planted['on'] = True
        off_stream = sc.run(_noop)
    _assert_same(sc, ordered, 'a delay in front of st_sgbm_match_f32 (ordered wrapper)')
    diff = ss.differences(sc.plain, off_stream)
    _report('teeth', planted_off_stream_wrapper=dict(D_ms=round(sc.D, 3), differing_paths=len(diff)))
    assert diff, 'a median launched off the caller\'s stream, in front of a delayed match, went unnoticed'
    assert all(k.endswith('[1]') for k in diff), diff      # the medians; `raw` itself is written on the caller's stream


def test_sabotage_submit_without_wait_stream_differs(built, monkeypatch):
    """(a) InflightPipelines.submit with its wait_stream made a no-op: behind a delay on the caller's stream the context
    reads the staged input buffer before the batch's copy_ has run - the previous batch (valid float planes)."""
    sc = built('P/mono')
    # the delayed caller and the racing contexts on different hardware queues, or the race cannot show
    monkeypatch.setattr(sc, 'side', ss.independent_stream(sc.pipes.streams, sc.cuda))
    hook = ss.StreamDelayed(sc.side, sc.D)
    _assert_same(sc, sc.run(hook), 'a delay at the head of the caller (intact submit)')
    for s in sc.pipes.streams:
        monkeypatch.setattr(s, 'wait_stream', lambda other: None, raising=True)
    got = sc.run(hook)
    monkeypatch.undo()
    torch.cuda.synchronize()
    diff = ss.differences(sc.plain, got)
    _report('teeth', sabotage_submit_wait_stream=dict(D_ms=round(sc.D, 3), differing_paths=len(diff)))
    assert diff, f'submit() without its wait_stream still equals the plain run: D = {sc.D:.0f} ms is too short'
    _assert_same(sc, sc.run(ss.StreamDelayed(sc.side, sc.D)), 'the restored submit under a delayed caller')


def test_sabotage_disparity_without_its_guard_differs(cuda, monkeypatch):
    """(b) StereoDensePipeline.disparity with the wait on disp_guard[k] made a no-op (the guard is dropped before the
    call), inflight 1, two disparity buffers, 5 chunks in one call, and a delay at the head of the shell's side stream:
    the track-box depth of chunk k is read after chunk k + 2 has rewritten its slot (another frame's valid disparity)."""
    model, kind = build_shell('costvolume_lrcheck', inflight=1, queue_depth=1)
    frames, boxes = _shell_frames(kind, range(600, 610), cuda)
    side = torch.cuda.Stream(device=cuda)

    def run(hook):
        with torch.cuda.stream(side):
            hook()
            out = model.test_step(_shell_data(frames, boxes, 0))
            side.synchronize()
        torch.cuda.synchronize()
        return out
    with torch.cuda.stream(side):
        ss.calibrate()
    run(_noop)
    t = time.perf_counter()
    plain = run(_noop)
    D = ss.delay_length(time.perf_counter() - t)
    runner = next(iter(model._dense.values()))[0]
    assert len(runner) == 1 and runner.pipes[0].disp_buffers == 2
    # the shell's side stream: one that a delay can hold while the context keeps running (different hardware queues)
    key, = [k for k in model._staging if isinstance(k, tuple) and k[0] == 'side_stream']
    # ... and the caller's stream too: every submit records an event there for the context to wait on, and an event
    # in the delayed stream's queue would hold the contexts back until the delay is over
    shell_side = model._staging[key] = ss.independent_stream(list(runner.streams) + [side], cuda)
    assert ss.same_results(plain, run(_noop)), 'another side stream changed the result'
    hook = ss.StreamDelayed(shell_side, D)
    assert ss.same_results(plain, run(hook)), 'the intact shell changed under a delayed side stream'
    for p in runner.pipes:
        real = p.disparity

        def unguarded(img, right, p=p, real=real):
            p.disp_guard = [None] * len(p.disp_guard)
            return real(img, right)
        monkeypatch.setattr(p, 'disparity', unguarded, raising=True)
    got = run(hook)
    monkeypatch.undo()
    diff = ss.differences(plain, got)
    _report('teeth', sabotage_disp_guard=dict(D_ms=round(D, 3), differing_paths=len(diff)))
    assert diff, f'disparity() without its guard wait still equals the plain run: D = {D:.0f} ms is too short'
    assert all('depth' in k for k in diff), diff[:8]      # only the tracks' depth column reads the ring late
