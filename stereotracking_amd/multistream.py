"""MultiStreamTracker: many videos tracked in lockstep on the device (SURVEY.md §8 f-4 as a product path).

The batch a live user has is ONE frame from each of S cameras per tick.  A tick's frames go through the wrapped
OCSORT_Disparity's dense launch plan `dense_batch` at a time on its in-flight contexts (so the tuned plan is the one
that runs, without waiting for frames of the future), then ONE batched association step (BatchedGpuTracker,
csrc/batched_assoc.hip) advances all S sequences, and everything after it - unscaling the track boxes, their depth
column, the result records - stays on the device (csrc/stream_track.hip): per tick there is one device->host copy and
one event the host waits on.  What a stream receives over the ticks equals what `model.test_step` returns for that
stream's frames run alone (tests/test_multistream_gpu.py): reference mmtrack/models/mot/ocsort_disparity.py:60-111 per
stream, with the reference's parallelism over whole videos (datasets/samplers/video_sampler.py:25-70) turned into
parallelism inside one process.

  step(data)      one tick: `data` as test_step takes it, at most one frame per stream, metainfo `stream`, `frame_id`
  run(iterable)   generator over ticks; tick k+1's dense work is submitted while tick k associates

Camera-motion compensation is not part of the batched association: a tracker configured with `cmc` is refused here
(OCSORT_Disparity is the path that has it).  There is no host fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, records, shell_inputs
from ._lib import StStreamTick, check, current_stream, ptr
from .batched_assoc import BatchedGpuTracker
from .registry import MODELS

MAX_STREAMS = 128        # ST_STREAM_MAX_STREAMS: the tick's routing travels in the kernel arguments


class StreamOverflow(RuntimeError):
    """A stream exceeded `max_tracks` (status 1) or `max_dets` (status 2) of the batched association.  `.streams` /
    `.status` name the streams and their status words, `.results` holds the tick's completed samples of the healthy
    streams (in the order given).  An overflowed stream stays invalid until its next frame with frame_id 0; leave it
    out of the ticks until then - the other streams are not affected."""

    def __init__(self, message, streams, status, results):
        super().__init__(message)
        self.streams, self.status, self.results = list(streams), list(status), results


@MODELS.register_module(name=['MultiStreamTracker'])
class MultiStreamTracker:
    """dict(type='MultiStreamTracker', model=<OCSORT_Disparity config or built model>, streams=S, max_tracks=128,
    max_dets=None).  Owns no weights: detector, stereo module, thresholds, baseline / focal_length, depth_extraction,
    dense_batch, inflight, queue_depth, max_det, results_device, the `rectify` calibration (shared by all streams) and
    the tracker options are the wrapped model's.
    max_tracks / max_dets: capacities per stream of the device tracker (max_dets=None: the model's max_det; EVERY
    detection the detector keeps is a row of the tracker's input, as in the host shell)."""

    def __init__(self, model, streams, max_tracks=128, max_dets=None):
        if isinstance(getattr(model, 'get', lambda k: None)('rectify'), (list, tuple)):
            raise NotImplementedError('MultiStreamTracker: the streams share the wrapped model\'s ONE `rectify` calibration; '
                                      'a list of calibrations (one per stream) is not implemented')
        if isinstance(model, dict):
            model = MODELS.build(model)
        if not all(hasattr(model, a) for a in ('dense_runner', '_box_depth', 'tracker', 'max_det', 'dense_batch')):
            raise TypeError('MultiStreamTracker wraps an OCSORT_Disparity (config dict or built model)')
        self.model = model
        self.streams = int(streams)
        if not 1 <= self.streams <= MAX_STREAMS:
            raise ValueError(f'streams must be in [1, {MAX_STREAMS}], got {streams}')
        trk = model.tracker
        if trk is None:
            raise ValueError('the wrapped model has no tracker configured')
        if getattr(trk, 'with_cmc', False) or getattr(trk, 'cmc_cfg', None) is not None:
            raise NotImplementedError(
                'camera-motion compensation (cmc) is not supported by MultiStreamTracker: its state would live inside '
                'the batched GPU association; use OCSORT_Disparity (test_step / test_steps) for a tracker with cmc')
        if getattr(model, 'stereo_eval', None) is not None:
            raise NotImplementedError(
                'stereo_eval (the dense disparity evaluator) is not wired into MultiStreamTracker; use OCSORT_Disparity '
                '(test_step / test_steps) for a model with stereo_eval set')
        self.max_tracks = int(max_tracks)
        self.max_dets = int(model.max_det if max_dets is None else max_dets)
        if not 1 <= self.max_dets <= int(model.max_det):
            raise ValueError(f'max_dets must be in [1, max_det = {model.max_det}] of the wrapped model, got {max_dets}')
        if self.max_tracks < 1:
            raise ValueError(f'max_tracks must be positive, got {max_tracks}')
        self.tracker_options = {k: getattr(trk, k) for k in _lib.TRACKER_OPTIONS}
        self._check_tracker_options()
        self.chunk = max(1, min(int(model.dense_batch), self.streams))     # frames per dense launch plan
        self.max_chunks = -(-self.streams // self.chunk)
        self.lib = _lib.load()
        # run() submits this many ticks ahead of the one it hands back: enough chunks to occupy the in-flight contexts
        self.ahead = max(1, -(-max(1, int(model.inflight)) // self.max_chunks))
        self._dev = None          # device state: built on the first tick
        self._pending = 0         # ticks submitted and not yet collected (<= ahead + 1: the page-locked result ring)

    def _check_tracker_options(self):
        """The options the batched association refuses, refused here - on the host, before a device is touched."""
        cfg = _lib.tracker_config(**self.tracker_options)
        lib, h = _lib.load(), C.c_void_p()
        try:
            check(lib.st_batched_tracker_create(C.byref(cfg), self.streams, self.max_tracks, self.max_dets, C.byref(h)),
                  'st_batched_tracker_create')
        except _lib.StError as e:
            raise ValueError(f'tracker options / capacities the batched GPU association refuses: {e}') from None
        lib.st_batched_tracker_destroy(h)

    # ---- a tick, validated on the host -------------------------------------------------------------------------------
    def _routing(self, data):
        """-> (stream of every sample, frame id of every sample).  Raises before anything is launched."""
        samples = data.get('data_samples')
        if not samples:
            raise ValueError('empty tick: a tick carries at least one frame')
        if len(samples) > self.streams:
            raise ValueError(f'a tick carries at most one frame per stream: {len(samples)} frames, {self.streams} streams')
        streams, fids, seen, metas = [], [], set(), [sm.metainfo for sm in samples]
        for meta in metas:
            if 'stream' not in meta or 'frame_id' not in meta:
                raise KeyError("every sample's metainfo needs 'stream' and 'frame_id'")
            s, f = int(meta['stream']), int(meta['frame_id'])
            if not 0 <= s < self.streams:
                raise ValueError(f'stream index {s} outside [0, {self.streams})')
            if s in seen:
                raise ValueError(f'stream {s} appears twice in one tick')
            if f < 0:
                raise ValueError(f'stream {s}: frame_id must be >= 0, got {f}')
            seen.add(s)
            streams.append(s)
            fids.append(f)
        shell_inputs.uniform_ori_shape(metas)
        return streams, fids

    # ---- device state ------------------------------------------------------------------------------------------------
    def _device_state(self, dev):
        d = self._dev
        if d is not None and d['dev'] == dev:
            return d
        S, T, M = self.streams, self.max_dets, int(self.model.max_det)
        slots = self.max_chunks * self.chunk
        nbytes = int(self.lib.st_stream_record_bytes(S, T, M))
        off_hdr = 8 * S * T
        off_trk = off_hdr + 4 * S * records.STREAM_HDR_INTS
        off_det = off_trk + 4 * S * T * records.STREAM_ROW.floats
        assert nbytes == off_det + 4 * S * M * records.STREAM_DET_FLOATS, 'tick record layout differs from include/stereotrack.h'
        with torch.cuda.device(dev):
            d = dict(dev=dev, stream=torch.cuda.Stream(device=dev),
                     tracker=BatchedGpuTracker(S, self.max_tracks, T, device=dev, **self.tracker_options),
                     dets=torch.zeros(S, T, records.REC_FLOATS, dtype=torch.float32, device=dev),
                     counts=torch.full((S,), -1, dtype=torch.int32, device=dev),
                     fids=torch.full((S,), -1, dtype=torch.int32, device=dev),
                     boxes=torch.zeros(slots, T, 4, dtype=torch.float32, device=dev),
                     box_counts=torch.zeros(slots, dtype=torch.int32, device=dev),
                     record=torch.zeros(nbytes, dtype=torch.uint8, device=dev),
                     # page-locked result buffers, allocated ONCE (OCSORT_Disparity._pinned: a pinned allocation stalls
                     # the host until the device is idle): the tick being consumed + the ones submitted behind it
                     host=[torch.zeros(nbytes, dtype=torch.uint8).pin_memory() for _ in range(self.ahead + 1)], turn=0,
                     offsets=(off_hdr, off_trk, off_det))
        self._dev = d
        return d

    # ---- submit: everything of a tick enqueued, no host wait ---------------------------------------------------------
    def _submit(self, data):
        model = self.model
        streams, fids = self._routing(data)
        data = shell_inputs.preprocess(model, data)
        inputs, samples = data['inputs'], data['data_samples']
        if len(inputs['img']) != len(samples):
            raise ValueError(f"{len(inputs['img'])} frames for {len(samples)} samples")
        img, second, gt, stereo, ori = shell_inputs.plan_inputs(model, inputs, samples, 'MultiStreamTracker')
        if self._pending > self.ahead:
            raise RuntimeError(f'{self._pending} ticks are already in flight: collect one before submitting another')
        n, B, S = len(samples), self.chunk, self.streams
        nc = -(-n // B)
        dev = img.device
        runner = model.dense_runner(ori, stereo, B)
        # a context's disparity buffers must outlive the tick: the track boxes' depth is read from them after the ONE
        # association step that follows all of the tick's chunks (across ticks pipe.disp_guard orders the reuse)
        need = max(model.queue_depth + 1, -(-self.max_chunks // len(runner)))
        for p in runner.pipes:
            if p.disp_buffers < need:
                p.disp_buffers = need
        d = self._device_state(dev)
        A = d['stream']
        jobs = []
        # a model with depth_source other than 'input': the track boxes' depth is read from the chunk's disp_depth, as
        # the detections' was (a slot of the disparity ring in both input configurations)
        from_head = getattr(model, 'depth_source', 'input') != 'input'
        for ci in range(nc):
            s, e = ci * B, min(n, ci * B + B)
            a, b = shell_inputs.chunk_inputs(model, img, second, stereo, s, e, B, runner)
            job = dict(s=s, e=e)
            ext = None
            if from_head:
                h, w = model._chunk_img_shape(dict(data_samples=samples), s, e)
                ext = (min(h, runner.height), min(w, runner.width))

            def post(out, ctx, job=job):      # under the context's stream: the chunk's frame records, a tensor of their own
                job.update(ctx=ctx, rec=runner.pipes[ctx].pack_detections(out, scaled='both', n_real=job['e'] - job['s']),
                           disp=out['disp_depth'] if from_head else out['disp_postp'],
                           disp_slot=runner.pipes[ctx].disp_slot if stereo or from_head else None)
                return out
            job['ev'] = runner.submit(a, right=b if stereo else None, disp_postp=None if stereo else b, post=post,
                                      ext=ext)[1]
            jobs.append(job)

        slot_stream = np.full(nc * B, -1, np.int32)
        slot_stream[:n] = streams
        fid_of = np.full(S, -1, np.int32)
        fid_of[streams] = fids
        tick = StStreamTick(C.sizeof(StStreamTick), S, B, nc, self.max_dets, int(model.max_det),
                            slot_stream.ctypes.data, fid_of.ctypes.data)
        trk = d['tracker']
        A.wait_stream(torch.cuda.current_stream(dev))      # the gt depth maps were uploaded on the caller's stream
        with torch.cuda.stream(A):
            for job in jobs:
                A.wait_event(job['ev'])
                job['rec'].record_stream(A)
                job['disp'].record_stream(A)
            recs = (C.c_void_p * nc)(*[job['rec'].data_ptr() for job in jobs])
            check(self.lib.st_stream_gather(C.byref(tick), recs, ptr(d['dets']), ptr(d['counts']), ptr(d['fids']),
                                            ptr(d['record']), current_stream()), 'st_stream_gather')
            rows, ids, cnt = trk.step(d['fids'], d['dets'], d['counts'], check_status=False)
            check(self.lib.st_stream_unscale(C.byref(tick), ptr(rows), ptr(cnt), ptr(d['boxes']), ptr(d['box_counts']),
                                             current_stream()), 'st_stream_unscale')
            depth, gt_depth = [], []
            for ci, job in enumerate(jobs):       # the tracks' depth column (ocsort_disparity.py:99-104), chunk by chunk
                bx, bc = d['boxes'][ci * B:ci * B + B], d['box_counts'][ci * B:ci * B + B]
                depth.append(model._box_depth(job['disp'], bx, bc, model.baseline, model.focal_length)[0])
                if gt is not None:
                    gt.record_stream(A)
                    gt_depth.append(model._box_depth(shell_inputs.padded(gt, job['s'], job['e'], B), bx, bc, -1.0, 1.0)[0])
            read = torch.cuda.Event()
            read.record(A)
            for job in jobs:                      # the disparity buffers may be rewritten once their depth has been read
                if job['disp_slot'] is not None:
                    runner.pipes[job['ctx']].disp_guard[job['disp_slot']] = read
            dptr = (C.c_void_p * nc)(*[t.data_ptr() for t in depth])
            gptr = (C.c_void_p * nc)(*[t.data_ptr() for t in gt_depth]) if gt is not None else None
            check(self.lib.st_stream_record(C.byref(tick), ptr(rows), ptr(ids), ptr(cnt), ptr(trk.status), ptr(d['counts']),
                                            ptr(d['boxes']), dptr, gptr, ptr(d['record']), current_stream()),
                  'st_stream_record')
            host = d['host'][d['turn'] % len(d['host'])]
            d['turn'] += 1
            host.copy_(d['record'], non_blocking=True)      # the tick's ONE device->host copy ...
            ev = torch.cuda.Event()
            ev.record(A)                                    # ... and the ONE event the host waits on
        self._pending += 1
        return dict(samples=samples, streams=streams, host=host, ev=ev, dev=dev)

    # ---- collect: wait for the tick's record, complete its samples ---------------------------------------------------
    def _collect(self, st):
        from .dist import DetectionOverflow
        model, d = self.model, self._dev
        S, T, M = self.streams, self.max_dets, int(model.max_det)
        st['ev'].synchronize()
        self._pending -= 1
        off_hdr, off_trk, off_det = d['offsets']
        raw = st['host'].numpy()
        ids = raw[:off_hdr].view(np.int64).reshape(S, T)
        hdr = raw[off_hdr:off_trk].view(np.int32).reshape(S, records.STREAM_HDR_INTS)
        trk = raw[off_trk:off_det].view(np.float32).reshape(S, T, records.STREAM_ROW.floats)
        det = raw[off_det:].view(np.float32).reshape(S, M, records.STREAM_DET_FLOATS)
        outs, bad = [], []
        for sample, s in zip(st['samples'], st['streams']):
            m, k, status, _ = (int(v) for v in hdr[s])
            if status != 0:
                bad.append((s, status))
                continue
            if k > M:
                raise DetectionOverflow(f'stream {s}: {k} detections kept but the detection buffer has {M} rows; '
                                        f'build the model with a larger max_det')
            # copies: the page-locked buffer is reused a few ticks later
            dets = records.detections(torch.from_numpy(det[s, :k].copy()), records.int_column(det[s, :k], records.LABEL),
                                      records.int_column(det[s, :k], records.STREAM_DET_PRIOR))
            tracks = records.tracks(torch.from_numpy(trk[s, :m].copy()), records.int_column(trk[s, :m], records.LABEL),
                                    torch.from_numpy(ids[s, :m].copy()), records.STREAM_ROW)
            if model.results_device == 'input':
                dets, tracks = dets.to(st['dev']), tracks.to(st['dev'])
            sample.pred_det_instances = dets
            sample.pred_track_instances = tracks
            outs.append(sample)
        if model.results_csv is not None and outs:
            from .mot import append_prediction_results
            append_prediction_results(model.results_csv, outs)
        if bad:
            raise StreamOverflow(
                f'capacity exceeded in streams {[s for s, _ in bad]} (status {[c for _, c in bad]}: 1 = max_tracks='
                f'{self.max_tracks}, 2 = max_dets={self.max_dets}); such a stream is invalid until its next frame_id 0',
                [s for s, _ in bad], [c for _, c in bad], outs)
        return outs

    # ---- public ------------------------------------------------------------------------------------------------------
    def step(self, data):
        """One tick -> the samples in the order given, completed like test_step completes them.  Raises
        StreamOverflow (carrying the healthy streams' samples) when a stream of the tick exceeded a capacity."""
        return self._collect(self._submit(data))

    def run(self, ticks):
        """Generator over successive step() inputs; yields what step() returns, tick by tick.  The in-flight contexts
        are kept busy across ticks: up to `ahead` ticks (at least tick k+1) are submitted - dense chunks, association
        and result copy enqueued, no host wait - before tick k's record is waited for.  A StreamOverflow ends the
        generator at the tick it belongs to (the ticks submitted behind it have advanced the device state of the
        healthy streams; their results are dropped: restart run() after them)."""
        from collections import deque
        queue = deque()
        try:
            for data in ticks:
                queue.append(self._submit(data))
                if len(queue) > self.ahead:
                    yield self._collect(queue.popleft())
            while queue:
                yield self._collect(queue.popleft())
        finally:
            while queue:      # abandoned with ticks in flight: their page-locked buffers must not be reused early
                queue.popleft()['ev'].synchronize()
                self._pending -= 1

    def reset(self):
        """Forget every stream's tracks (a frame_id of 0 does the same for one stream)."""
        if self._dev is not None:
            with torch.cuda.stream(self._dev['stream']):      # ordered with the ticks already enqueued
                self._dev['tracker'].reset()
