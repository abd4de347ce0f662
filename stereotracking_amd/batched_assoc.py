"""Batched GPU association: OCSORTTracker_Disparity.track for MANY independent sequences per step.

One wave per sequence runs the whole association step on the device (csrc/batched_assoc.hip): Kalman prediction, the
tracks x detections cost matrix and the Kalman updates across the lanes, the Jonker-Volgenant assignment and the track
bookkeeping on lane 0; the per-sequence state (tracks, Kalman filters, observation windows) stays in device memory.
Ids / rows equal the host tracker's (st_tracker_track) on the same detections - reference
mmtrack/models/trackers/ocsort_tracker_disparity.py:345-618.  Use it when a step carries hundreds of short sequences
(multi-camera serving); for ONE video the native host tracker is faster (0.05 ms per frame) and is what
OCSORT_Disparity uses."""
import ctypes as C

import torch

from . import _lib
from ._lib import check, current_stream, ptr
from .records import REC_FLOATS, TRACK_ROW


class BatchedGpuTracker:
    """`batch` sequences in lockstep.  step(frame_ids, dets, counts) -> (rows, ids, n) device tensors:
    rows (batch, max_dets, 8) = pred_track_instances rows [depth-scaled box, score, label, depth, scale] in the
    reference's output order, ids (batch, max_dets) int64, n (batch,) int32 (-1 = the sequence had no frame).

    options: None (every sequence runs the constructor's tracker options), or a sequence of `batch` dicts over
    _lib.TRACKER_OPTIONS - the options of sequence b, missing keys taking the constructor's values
    (st_batched_tracker_create_multi: the option sets live in device memory owned by the tracker).  A refused member
    (vel_delta_t above the observation window, ...) raises before a device is touched and names its index.

    run(frame_ids, dets, counts, video_of) advances every sequence over a whole recorded detection stream in ONE
    launch (st_batched_tracker_run); sequences that share a video read the same detection rows."""

    def __init__(self, batch, max_tracks=128, max_dets=512, device=None, obj_score_thr=0.3, init_track_thr=0.7,
                 weight_iou_with_det_scores=True, match_iou_thr=0.3, num_tentatives=3, vel_consist_weight=0.2,
                 vel_delta_t=3, num_frames_retain=10, cmc=None, options=None):
        if cmc is not None:
            raise NotImplementedError('camera-motion compensation (cmc) is not supported by the batched GPU association; '
                                      'use OCSORTTracker_Disparity (host tracker) for a tracker with cmc')
        self.lib = _lib.load()
        self.batch, self.max_tracks, self.max_dets = int(batch), int(max_tracks), int(max_dets)
        base = dict(obj_score_thr=obj_score_thr, init_track_thr=init_track_thr,
                    weight_iou_with_det_scores=weight_iou_with_det_scores, match_iou_thr=match_iou_thr,
                    num_tentatives=num_tentatives, vel_consist_weight=vel_consist_weight, vel_delta_t=vel_delta_t,
                    num_frames_retain=num_frames_retain)
        h = C.c_void_p()
        if options is None:
            self.options = None
            cfg = _lib.tracker_config(**base)
            check(self.lib.st_batched_tracker_create(C.byref(cfg), self.batch, self.max_tracks, self.max_dets, C.byref(h)),
                  'st_batched_tracker_create')
        else:
            options = [dict(o) for o in options]
            if len(options) != self.batch:
                raise ValueError(f'options: {len(options)} option sets for a batch of {self.batch} sequences')
            for b, o in enumerate(options):
                unknown = sorted(set(o) - set(_lib.TRACKER_OPTIONS))
                if unknown:
                    raise ValueError(f'options[{b}]: unknown tracker options {unknown} (known: {list(_lib.TRACKER_OPTIONS)})')
            self.options = [dict(base, **o) for o in options]
            cfgs = (_lib.StTrackerConfig * self.batch)(*[_lib.tracker_config(**o) for o in self.options])
            check(self.lib.st_batched_tracker_create_multi(cfgs, self.batch, self.max_tracks, self.max_dets, C.byref(h)),
                  'st_batched_tracker_create_multi')
        self.handle = h
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.state = torch.zeros(self.lib.st_batched_tracker_state_bytes(h), dtype=torch.uint8, device=self.device)
        self.scratch = torch.empty(self.lib.st_batched_tracker_scratch_bytes(h), dtype=torch.uint8, device=self.device)
        B, M = self.batch, self.max_dets
        self.rows = torch.zeros(B, M, TRACK_ROW.floats, dtype=torch.float32, device=self.device)
        self.ids = torch.zeros(B, M, dtype=torch.int64, device=self.device)
        self.n = torch.zeros(B, dtype=torch.int32, device=self.device)
        self.status = torch.zeros(B, dtype=torch.int32, device=self.device)

    def __del__(self):
        h = getattr(self, 'handle', None)
        if h:
            try:
                self.lib.st_batched_tracker_destroy(h)
            except Exception:
                pass
            self.handle = None

    def reset(self):
        self.state.zero_()

    def sequence_state(self, b):
        """Read-back of sequence b (st_batched_tracker_get_states; tests): (header, tracks).  header = dict(n_tracks,
        next_id, status: the sequence's sticky status); tracks = the live tracks in creation order, the list of dicts
        of OCSORTTracker_Disparity.track_states().  Ordered after the steps already enqueued on the current stream; one
        host sync; the device state is only read.  A sequence with a non-zero status has no tracks to report."""
        buf = (_lib.StTrackState * self.max_tracks)()
        n, nxt, st = C.c_int(), C.c_longlong(), C.c_int()
        check(self.lib.st_batched_tracker_get_states(self.handle, ptr(self.state), int(b), C.cast(buf, C.c_void_p),
                                                     self.max_tracks, C.sizeof(_lib.StTrackState), C.byref(n),
                                                     C.byref(nxt), C.byref(st), current_stream()),
              'st_batched_tracker_get_states')
        return (dict(n_tracks=n.value, next_id=nxt.value, status=st.value), _lib.track_state_dicts(buf, n.value))

    def track_states(self, b):
        """The live tracks of sequence b: sequence_state(b)[1]."""
        return self.sequence_state(b)[1]

    def step(self, frame_ids, dets, counts, check_status=True):
        """frame_ids (batch,) int32, dets (batch, max_dets, 8) float32, counts (batch,) int32 - CUDA tensors.
        check_status: one host sync to raise on a capacity overflow (False: read `self.status` yourself).  A non-zero
        status is sticky per sequence: the device state of that sequence is invalid until a step with frame_id 0."""
        for t, dt, shape in ((frame_ids, torch.int32, (self.batch,)), (dets, torch.float32, (self.batch, self.max_dets, REC_FLOATS)),
                             (counts, torch.int32, (self.batch,))):
            if not (t.is_cuda and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous()):
                raise ValueError(f'expected a contiguous CUDA {dt} tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}')
        self.status.zero_()
        check(self.lib.st_batched_tracker_step(self.handle, ptr(frame_ids), ptr(dets), ptr(counts), ptr(self.state),
                                               ptr(self.scratch), ptr(self.rows), ptr(self.ids), ptr(self.n),
                                               ptr(self.status), current_stream()), 'st_batched_tracker_step')
        if check_status:
            st = self.status.cpu()
            if int(st.max()) != 0:
                bad = torch.nonzero(st).flatten().tolist()
                raise RuntimeError(f'batched association: capacity exceeded in sequences {bad} '
                                   f'(status {st[bad].tolist()}: 1 = max_tracks={self.max_tracks}, 2 = max_dets={self.max_dets})')
        return self.rows, self.ids, self.n

    def run(self, frame_ids, dets, counts, video_of, f_begin=0, f_end=None, out=None):
        """Frames [f_begin, f_end) of a recorded detection stream for every sequence, in ONE launch
        (st_batched_tracker_run): sequence b walks the frames of video video_of[b].  CUDA tensors: frame_ids (V, F) int32,
        dets (V, F, max_dets, 8) float32, counts (V, F) int32 (-1: the video has no such frame: ragged lengths, gaps; the
        state does not move), video_of (batch,) int32 in [0, V).  -> (rows (batch, F, max_dets, 8) float32,
        ids (batch, F, max_dets) int64, n (batch, F) int32), equal on the bits to f_end - f_begin step() calls whose
        inputs were gathered through video_of; the state stays in device memory, so [0, F) in one call equals [0, k) then
        [k, F).  The output takes batch * F * max_dets * 40 bytes (+ 4 per frame); `out` = the (rows, ids, n) of an
        earlier call is written in place (frames outside the range are left alone), else new buffers are allocated
        with n = -1 everywhere.  No host sync: `self.status` (zeroed first) holds a non-zero code for every sequence
        with a frame in the range that reported a capacity overflow (sticky per sequence, as in step; 3 = video_of[b]
        outside [0, V))."""
        if not (torch.is_tensor(frame_ids) and frame_ids.dim() == 2):
            raise ValueError('frame_ids: expected a (V, F) tensor')
        V, F = (int(v) for v in frame_ids.shape)
        B, M = self.batch, self.max_dets
        f_end = F if f_end is None else int(f_end)
        f_begin = int(f_begin)
        if V <= 0 or F <= 0 or not 0 <= f_begin < f_end <= F:
            raise ValueError(f'run: bad frame range [{f_begin}, {f_end}) of {V} videos x {F} frames')
        expect = [(frame_ids, torch.int32, (V, F)), (dets, torch.float32, (V, F, M, REC_FLOATS)),
                  (counts, torch.int32, (V, F)), (video_of, torch.int32, (B,))]
        if out is None:
            out = (torch.zeros(B, F, M, TRACK_ROW.floats, dtype=torch.float32, device=self.device),
                   torch.zeros(B, F, M, dtype=torch.int64, device=self.device),
                   torch.full((B, F), -1, dtype=torch.int32, device=self.device))
        else:
            expect += [(out[0], torch.float32, (B, F, M, TRACK_ROW.floats)), (out[1], torch.int64, (B, F, M)),
                       (out[2], torch.int32, (B, F))]
        for t, dt, shape in expect:
            if not (torch.is_tensor(t) and t.is_cuda and t.device == self.device and t.dtype == dt and
                    tuple(t.shape) == shape and t.is_contiguous()):
                raise ValueError(f'expected a contiguous {dt} tensor of shape {shape} on {self.device}, got '
                                 f'{getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))} on {getattr(t, "device", None)}')
        rows, ids, n = out
        self.status.zero_()
        check(self.lib.st_batched_tracker_run(self.handle, ptr(frame_ids), ptr(dets), ptr(counts), ptr(video_of), V, F,
                                              f_begin, f_end, ptr(self.state), ptr(self.scratch), ptr(rows), ptr(ids),
                                              ptr(n), ptr(self.status), current_stream()), 'st_batched_tracker_run')
        return rows, ids, n
