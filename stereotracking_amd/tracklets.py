"""Tracklet post-processing between "tracker rows" and "scores": InterpolateTracklets, linear gap filling (ByteTrack,
arXiv 2110.06864) and Gaussian-smoothed interpolation (GSI; StrongSORT, arXiv 2202.13514).

Behavioural spec: reference mmtrack/models/task_modules/track/interpolation.py:125-160, restated:
  * tracks are taken per id; a track of <= 2 rows is dropped;
  * a track of > min_num_frames rows gets every frame gap g with 1 < g < max_num_frames filled with the rows
    j / g * (right - left) + left, j = 1 .. g - 1 (fp64 operations in this order), score 1.0;
  * use_gsi: the four coordinates of every kept track (filled rows included) are replaced by the mean of a Gaussian
    process at the track's own frames: len_scale = clip(tau * log(tau**3 / n), 1 / tau, tau**2) with n the row count
    after filling, K_ij = exp(-0.5 * ((t_i - t_j) / len_scale)**2), prediction K @ solve(K + 1e-10 I, y): what
    scikit-learn's GaussianProcessRegressor(RBF(len_scale, 'fixed')) computes with its default alpha, normalize_y=False
    and nothing to optimise.  Ids and scores are kept.

Decided where the reference is undefined or raises ("parity unpinned"):
  * output order: ascending frame, then ascending id (the reference's argsort() is unstable within a frame);
  * empty input, or input whose tracks are all dropped, returns (0, 7) (the reference raises from np.max / np.concatenate);
  * frames and ids must be integral and the frames of one id strictly increasing in input order, else ValueError naming
    the id;
  * the smoother sees a track's rows in frame order (the reference appends the filled rows behind the track; the GP mean
    does not depend on the order, its rounding does);
  * a Cholesky pivot <= 0 raises numpy.linalg.LinAlgError on both backends, never a silent result.

backend='host' (numpy + scipy, one factorisation per track for the four right-hand sides) is the executable
specification.  backend='device' runs csrc/tracklet_post.hip (st_tracklet_interpolate, st_tracklet_gsi;
include/stereotrack.h section 17): the filled rows are bit-equal to the host's, the smoothed coordinates are another
correct fp64 evaluation of the same ill-conditioned system (both meet the tolerance of tests/golden/gsi_truth.npz).
There is no fallback from 'device' to 'host'.
"""
import collections
import ctypes as C
import time

import numpy as np
import torch

from . import _lib
from ._packed import PackedCall
from .metrics import _check_backend
from .registry import TASK_UTILS

GSI_ALPHA = 1e-10                    # scikit-learn's default GaussianProcessRegressor(alpha)
WORKSPACE_BUDGET_BYTES = 256 << 20   # st_tracklet_gsi's global workspace per launch (forward_many splits to keep it)
LAUNCHES = collections.Counter()     # calls of every st_tracklet_* stage entry (tests read it)


def max_track_rows():
    """Longest track (rows after filling) the device smoother supports."""
    return int(_lib.load().st_tracklet_max_rows())


def gsi_len_scale(tau, n):
    return np.clip(tau * np.log(tau ** 3 / n), tau ** -1, tau ** 2)


def _as_rows(rows):
    rows = np.asarray(rows, dtype=np.float64)
    if rows.size == 0:
        return np.zeros((0, 7))
    if rows.ndim != 2 or rows.shape[1] < 7:
        raise ValueError(f'InterpolateTracklets: rows must be (N, >= 7) (frame, id, c0, c1, c2, c3, score), got {rows.shape}')
    return rows[:, :7]


def _sorted_tracks(rows):
    """rows grouped by id (stable, so a track keeps its input order) after the input checks; the first row of every
    track and the ids."""
    frames, ids = rows[:, 0], rows[:, 1]
    if not np.all(np.isfinite(frames)) or np.any(frames != np.floor(frames)):
        bad = int(np.argmax(~(np.isfinite(frames) & (frames == np.floor(frames)))))
        raise ValueError(f'InterpolateTracklets: frame {frames[bad]:g} of id {ids[bad]:g} is not integral')
    if not np.all(np.isfinite(ids)) or np.any(ids != np.floor(ids)):
        bad = int(np.argmax(~(np.isfinite(ids) & (ids == np.floor(ids)))))
        raise ValueError(f'InterpolateTracklets: id {ids[bad]:g} (frame {frames[bad]:g}) is not integral')
    order = np.argsort(ids.astype(np.int64), kind='stable')
    rows = rows[order]
    key = rows[:, 1].astype(np.int64)
    new = np.ones(len(rows), bool)
    new[1:] = key[1:] != key[:-1]
    bad = ~new[1:] & (rows[1:, 0] <= rows[:-1, 0])
    if bad.any():
        raise ValueError(f'InterpolateTracklets: the frames of id {int(key[1:][np.argmax(bad)])} are not strictly increasing')
    return rows, np.flatnonzero(new), key


def _finish(rows):
    """Ascending frame, then ascending id."""
    if len(rows) == 0:
        return np.zeros((0, 7))
    return np.ascontiguousarray(rows[np.lexsort((rows[:, 1].astype(np.int64), rows[:, 0]))])


def _raise_status(status, plan):
    """The device's per-track status words (include/stereotrack.h section 17) as exceptions; nothing when all are 0."""
    if not np.any(status):
        return
    if np.any(np.asarray(status) & 2):       # st_tracklet_interpolate reports it in word 0, whichever track it is
        raise _lib.StError('InterpolateTracklets: a table entry out of range on the device: the host tables and the '
                           'buffers disagree')
    t = int(np.argmax(np.asarray(status) != 0))
    raise np.linalg.LinAlgError(f'InterpolateTracklets: id {int(plan["trk_id"][t])} of set {int(plan["trk_set"][t])}: a '
                                f'pivot of the Cholesky factorisation is not positive ({int(plan["n_out"][t])} rows)')


@TASK_UTILS.register_module(name=['InterpolateTracklets', 'mmtrack.InterpolateTracklets'])
class InterpolateTracklets:
    """See the module docstring.  forward(rows) -> (M, 7); forward_many(list of row arrays) -> list of (M, 7)."""

    def __init__(self, min_num_frames=5, max_num_frames=20, use_gsi=False, smooth_tau=10, backend='host'):
        _check_backend(backend)
        self.min_num_frames, self.max_num_frames = min_num_frames, max_num_frames
        self.use_gsi, self.smooth_tau, self.backend = use_gsi, smooth_tau, backend

    # ------------------------------------------------------------------ host: the executable specification
    def _fill(self, track):
        parts = []
        for i in range(len(track) - 1):
            parts.append(track[i:i + 1])
            g = int(track[i + 1, 0] - track[i, 0])
            if 1 < g < self.max_num_frames:
                left, right = track[i, 2:6], track[i + 1, 2:6]
                new = np.ones((g - 1, 7))
                for j in range(1, g):
                    new[j - 1, 0] = j + track[i, 0]
                    new[j - 1, 1] = track[i, 1]
                    new[j - 1, 2:6] = j / g * (right - left) + left
                parts.append(new)
        parts.append(track[-1:])
        return np.concatenate(parts)

    def _smooth(self, track):
        from scipy.linalg import cho_factor, cho_solve
        n = len(track)
        ls = gsi_len_scale(self.smooth_tau, n)
        t = track[:, 0]
        d = (t[:, None] - t[None, :]) / ls
        K = np.exp(-0.5 * d ** 2)
        try:
            alpha = cho_solve(cho_factor(K + GSI_ALPHA * np.eye(n), lower=True), track[:, 2:6])
        except np.linalg.LinAlgError as e:
            raise np.linalg.LinAlgError(f'InterpolateTracklets: id {int(track[0, 1])}: {e}') from None
        out = track.copy()
        out[:, 2:6] = K @ alpha
        return out

    def _forward_host(self, rows):
        rows, starts, _ = _sorted_tracks(_as_rows(rows))
        out = []
        for a, b in zip(starts, list(starts[1:]) + [len(rows)]):
            track = rows[a:b]
            if len(track) <= 2:
                continue
            if len(track) > self.min_num_frames:
                track = self._fill(track)
            if self.use_gsi:
                track = self._smooth(track)
            out.append(track)
        return _finish(np.concatenate(out) if out else np.zeros((0, 7)))

    def forward(self, pred_tracks):
        """(N, >= 7) fp64 rows (frame, id, c0, c1, c2, c3, score) -> (M, 7)."""
        if self.backend == 'device':
            return self.forward_many([pred_tracks])[0]
        return self._forward_host(pred_tracks)

    # ------------------------------------------------------------------ many videos / sweep members
    def forward_many(self, row_arrays, device=None, workspace_budget=None, timing=False):
        """forward() of every array of the list.  backend='device': ONE upload, the launches, ONE wait and ONE copy back
        for the whole list.  workspace_budget: bytes of global workspace one st_tracklet_gsi launch may use (default
        WORKSPACE_BUDGET_BYTES); the sorted track list is split into several launches to stay below it - the result
        does not depend on the split.  timing: returns (list, dict) with per-stage device times (HIP events) and the
        host clock of the call's parts."""
        row_arrays = list(row_arrays)
        if self.backend == 'host':
            t0 = time.perf_counter()
            out = [self._forward_host(r) for r in row_arrays]
            return (out, dict(total_s=time.perf_counter() - t0)) if timing else out
        return self._forward_many_device(row_arrays, device, workspace_budget, timing)

    def _plan(self, row_arrays):
        """The host preparation of the device path (numpy): the kept tracks of all sets sorted by (set, id, frame), the
        per-row and per-track tables of include/stereotrack.h section 17.  They follow from the frame numbers alone."""
        parts, sets = [], []
        for s, r in enumerate(row_arrays):
            rows, starts, _ = _sorted_tracks(_as_rows(r))
            n_in = np.diff(np.append(starts, len(rows)))
            keep = np.repeat(n_in > 2, n_in)
            parts.append(rows[keep])
            sets.append(np.full(int(keep.sum()), s, np.int64))
        rows = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 7))
        sets = np.concatenate(sets) if sets else np.zeros(0, np.int64)
        R = len(rows)
        ids = rows[:, 1].astype(np.int64)
        new = np.ones(R, bool)
        new[1:] = (ids[1:] != ids[:-1]) | (sets[1:] != sets[:-1])
        starts = np.flatnonzero(new)
        T = len(starts)
        n_in = np.diff(np.append(starts, R))
        fill_track = np.repeat(n_in > self.min_num_frames, n_in)
        gap = np.zeros(R, np.int64)
        gap[:-1] = np.where(new[1:], 0, rows[1:, 0] - rows[:-1, 0]).astype(np.int64)
        gap = np.where(fill_track & (gap > 1) & (gap < self.max_num_frames), gap, 0)
        per_row = 1 + np.maximum(gap - 1, 0)
        row_out_off = np.concatenate([[0], np.cumsum(per_row)])
        M = int(row_out_off[-1])
        if M >= 2 ** 31 - 1:
            raise ValueError(f'InterpolateTracklets: {M} output rows: the offset tables are 32-bit')
        trk_out_off = np.append(row_out_off[starts], M) if T else np.zeros(1, np.int64)
        n_out = np.diff(trk_out_off)
        return dict(rows=rows, R=R, T=T, M=M, row_out_off=row_out_off[:-1].astype(np.int32), row_gap=gap.astype(np.int32),
                    trk_out_off=trk_out_off.astype(np.int32), n_out=n_out, trk_set=sets[starts], trk_id=ids[starts],
                    trk_order=np.argsort(-n_out, kind='stable').astype(np.int32),
                    trk_len_scale=np.asarray(gsi_len_scale(self.smooth_tau, np.maximum(n_out, 1)), np.float64).reshape(-1))

    @staticmethod
    def _launch_ranges(n_sorted, lib, groups_wanted, budget):
        """(first, count, groups) of every st_tracklet_gsi launch over the tracks sorted by descending row count.  A
        launch's workspace is groups x the slot of its longest track; where the budget allows fewer workgroups than
        wanted, the launch ends where the slot has shrunk to half, so that shorter tracks run on more workgroups."""
        def slot(n):
            a = _lib.StTrackletArgs()
            a.struct_size, a.num_groups, a.max_rows = C.sizeof(_lib.StTrackletArgs), 1, int(n)
            return int(lib.st_tracklet_gsi_workspace_bytes(C.byref(a))) - 256
        uniq = np.unique(n_sorted)                                   # one query per distinct length
        slot_of = np.array([slot(n) for n in uniq], np.int64)[np.searchsorted(uniq, n_sorted)]      # non-increasing
        out, first, T = [], 0, len(n_sorted)
        while first < T:
            want = min(groups_wanted, T - first)
            s = int(slot_of[first])
            groups = want if s == 0 else min(want, (budget - 256) // s)       # a launch needs 256 + groups * slot bytes
            if groups < 1:
                raise ValueError(f'InterpolateTracklets: a track of {int(n_sorted[first])} rows needs {256 + s} bytes of '
                                 f'workspace, the budget is {budget}')
            end = T
            if groups < want:
                half = np.flatnonzero(slot_of[first:] * 2 <= s)
                if len(half):
                    end = first + int(half[0])
            out.append((first, end - first, min(groups, end - first)))
            first = end
        return out

    def _forward_many_device(self, row_arrays, device, budget, timing):
        call = PackedCall('InterpolateTracklets', 'csrc/tracklet_post.hip', device, timing, LAUNCHES)
        lib, dev = call.lib, call.dev
        budget = WORKSPACE_BUDGET_BYTES if budget is None else int(budget)
        p = self._plan(row_arrays)
        B, T, R, M = len(row_arrays), p['T'], p['R'], p['M']
        if T == 0:
            out = [np.zeros((0, 7)) for _ in range(B)]
            return (out, dict(stages_ms={}, host_prepare_s=time.perf_counter() - call.t_start)) if timing else out
        n_sorted = p['n_out'][p['trk_order']]
        ranges = []
        if self.use_gsi:
            if int(n_sorted[0]) > max_track_rows():
                t = int(p['trk_order'][0])
                raise ValueError(f'InterpolateTracklets: id {int(p["trk_id"][t])} of set {int(p["trk_set"][t])} has '
                                 f'{int(n_sorted[0])} rows after filling, the device smoother supports {max_track_rows()}')
            cus = torch.cuda.get_device_properties(dev).multi_processor_count
            ranges = self._launch_ranges(n_sorted, lib, cus, budget)

        args = _lib.StTrackletArgs()
        args.struct_size = C.sizeof(_lib.StTrackletArgs)
        args.num_rows, args.num_out_rows, args.num_tracks = R, M, T
        launches, ws_bytes = [], 256
        for first, count, groups in ranges:
            args.num_groups, args.max_rows = groups, int(n_sorted[first])
            launches.append((first, count, groups, int(n_sorted[first])))
            ws_bytes = max(ws_bytes, call.workspace_bytes('st_tracklet_gsi_workspace_bytes', args))

        call.upload({k: p[k] for k in ('rows', 'row_out_off', 'row_gap', 'trk_out_off', 'trk_order', 'trk_len_scale')})
        call.outputs((('status', (T,), np.int32), ('out_rows', (M, 7), np.float64)))    # the status: zeroed by the first stage
        call.workspace(args, ws_bytes)
        ticks = torch.zeros((max([g for _, _, g, _ in launches] + [1]), 4), dtype=torch.int64, device=dev) if timing else None
        args.phase_ticks = C.c_void_p(ticks.data_ptr()) if timing else None
        call.bind(args)
        with call.stages():
            args.first = args.count = 0
            args.num_groups = args.max_rows = 1
            call.launch('st_tracklet_interpolate', C.byref(args))
            call.begin('st_tracklet_gsi')
            for first, count, groups, nmax in launches:
                args.first, args.count, args.num_groups, args.max_rows = first, count, groups, nmax
                call.launch('st_tracklet_gsi', C.byref(args))
        host = call.fetch()
        _raise_status(host['status'], p)
        rows = host['out_rows']
        set_off = np.searchsorted(np.repeat(p['trk_set'], p['n_out']), np.arange(B + 1))
        out = [_finish(rows[set_off[s]:set_off[s + 1]]) for s in range(B)]
        if timing:
            tm = call.timing_dict(gsi_launches=len(launches), tracks=T, rows_in=R, rows_out=M)
            phase = ticks.sum(0).cpu().numpy().astype(np.float64)      # after the timed part: a second, small copy
            tm['gsi_phase_share'] = dict(zip(('build_k', 'factorisation', 'solves', 'product'),
                                             (phase / max(1.0, phase.sum())).tolist()))
            return out, tm
        return out
