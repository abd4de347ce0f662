#!/usr/bin/env python
"""Time a tracker-option sweep three ways.  Record-only: writes profiles/sweep_bench.json, asserts no speed.

    python tools/sweep_bench.py [--videos 8 --sets 128 --small-sets 8 --frames 512 --runs 5 --baseline-only
                                 --baseline-parent FILE --assoc-parent FILE --assoc-this FILE --out FILE]

Shape: --videos videos x --sets option sets (B = videos * sets sequences) x --frames frames x 8 objects, the detections
of tools/mot_eval_bench.py's generator (jittered boxes, a tenth missing, spurious ones), plus one small point of
--small-sets option sets.  Per shape, the host clock around the whole thing (uploads, launches, the copy back), warm,
median of --runs with the spread, and us per sequence-frame:
  (a) baseline     one BatchedGpuTracker per option set (`videos` sequences each), stepped frame by frame with a
                   TrackCollector each - what a sweep costs without per-sequence options
  (b) multi_step   ONE tracker with per-sequence options, B sequences, stepped the same way
  (c) run          TrackerSweep.run(): one launch and one copy back per group of members; `kernel_ms` = HIP events
                   around BatchedGpuTracker.run alone
and the time of SweepResult.scores() on the device backend (once).  (a) uses nothing newer than BatchedGpuTracker.step,
so --baseline-only also runs on a tree or a library from before the sweep entry points (ST_LIBRARY=<older build>).
--baseline-parent: the JSON a --baseline-only run on the parent commit wrote; --assoc-parent / --assoc-this: the printed
output of tools/assoc_bench.py on the parent commit and on this one (same box, same session, repeated runs
concatenated); all three are stored in the record as given."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from mot_eval_bench import jittered_sequence, spread  # noqa: E402

M, MAX_TRACKS, OBJECTS, SCALE = 16, 64, 8, 1.5
NEW_ENTRY_POINTS = ('st_batched_tracker_create_multi', 'st_batched_tracker_run')


def library_has_sweep():
    """False on a library from before the sweep entry points; their prototypes are then dropped so that it loads."""
    from stereotracking_amd import _lib
    raw = ctypes.CDLL(os.environ.get('ST_LIBRARY') or _lib.LIB_PATH)
    has = all(hasattr(raw, n) for n in NEW_ENTRY_POINTS) and all(n in _lib._PROTOS for n in NEW_ENTRY_POINTS)
    if not has:
        for n in NEW_ENTRY_POINTS:
            _lib._PROTOS.pop(n, None)
    return has


def video(seed, frames):
    """-> frame_ids (F,), dets (F, M, 8) [depth-scaled box, score, label, depth, scale], counts (F,), gt rows keyed by
    the frame's index."""
    gt, pred = jittered_sequence(seed, frames, OBJECTS)
    rng = np.random.RandomState(seed + 7)
    dets, counts = np.zeros((frames, M, 8), np.float32), np.zeros(frames, np.int32)
    for t in range(frames):
        p = pred[pred[:, 0] == 1.0 + t][:M]
        k = len(p)
        cx, cy, w, h = p[:, 2] + p[:, 4] / 2, p[:, 3] + p[:, 5] / 2, p[:, 4] * SCALE, p[:, 5] * SCALE
        dets[t, :k, 0:4] = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
        dets[t, :k, 4], dets[t, :k, 6], dets[t, :k, 7] = rng.uniform(0.4, 0.95, k), 20.0, SCALE
        counts[t] = k
    gt = gt.copy()
    gt[:, 0] -= 1.0
    return np.arange(frames, dtype=np.int32), dets, counts, gt


def option_sets(K):
    from itertools import product
    vals = product([0.6, 0.7], [0.1, 0.2, 0.3, 0.4], [1, 2, 3, 4], [0.0, 0.2], [1, 3])
    names = ('init_track_thr', 'match_iou_thr', 'num_tentatives', 'vel_consist_weight', 'vel_delta_t')
    sets = [dict(zip(names, v), obj_score_thr=0.3, weight_iou_with_det_scores=False, num_frames_retain=30) for v in vals]
    assert K <= len(sets)
    return sets[:K]


def timed(fn, runs):
    import torch
    fn()                                   # warm
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def stepped(trackers, dets_steps, counts_steps, fid_steps, frame_numbers):
    """Every tracker stepped over the frames with a TrackCollector of its own, then one copy back per tracker."""
    from stereotracking_amd.mot_eval import TrackCollector
    for trk, dets, counts in zip(trackers, dets_steps, counts_steps):
        trk.reset()
        col = TrackCollector()
        for t in range(len(fid_steps)):
            col.add(frame_numbers[t], *trk.step(fid_steps[t][:trk.batch], dets[t], counts[t], check_status=False))
        col.to_host()


def measure(videos, sets, runs, has_sweep, baseline_only, dev):
    import torch
    from stereotracking_amd.batched_assoc import BatchedGpuTracker
    V, K, F = len(videos), len(sets), len(videos[0][0])
    B = V * K
    rec = dict(shape=f'{V} videos x {K} option sets x {F} frames x {OBJECTS} objects', sequences=B, sequence_frames=B * F)
    per = lambda ts: dict(seconds=spread(ts), us_per_sequence_frame=spread(np.asarray(ts) / (B * F) * 1e6))
    dets = torch.from_numpy(np.stack([v[1] for v in videos], 1)).to(dev)           # (F, V, M, 8)
    counts = torch.from_numpy(np.stack([v[2] for v in videos], 1)).to(dev)         # (F, V)
    fid_steps = [torch.full((B,), t, dtype=torch.int32, device=dev) for t in range(F)]
    frame_numbers = [np.full(B, t) for t in range(F)]
    # (a) one tracker per option set
    trackers = [BatchedGpuTracker(V, max_tracks=MAX_TRACKS, max_dets=M, device=dev, **o) for o in sets]
    numbers_v = [f[:V] for f in frame_numbers]
    rec['a_baseline_one_tracker_per_option_set'] = per(timed(
        lambda: stepped(trackers, [dets] * K, [counts] * K, fid_steps, numbers_v), runs))
    del trackers
    if baseline_only or not has_sweep:
        return rec
    from stereotracking_amd.sweep import TrackerSweep
    # (b) one multi-option tracker, stepped
    video_of = torch.arange(B, device=dev) % V
    multi = BatchedGpuTracker(B, max_tracks=MAX_TRACKS, max_dets=M, device=dev, options=[sets[m // V] for m in range(B)])
    dets_b, counts_b = dets[:, video_of].contiguous(), counts[:, video_of].contiguous()
    rec['b_multi_option_tracker_stepped'] = per(timed(
        lambda: stepped([multi], [dets_b], [counts_b], fid_steps, frame_numbers), runs))
    del dets_b, counts_b
    # (c) TrackerSweep.run, and the launch alone
    sweep = TrackerSweep(sets, max_tracks=MAX_TRACKS, max_dets=M, device=dev)
    for f, d, c, _ in videos:
        sweep.add_video(frame_ids=f, dets=d, counts=c)
    result = [None]

    def run():
        result[0] = sweep.run()
    rec['c_tracker_sweep_run'] = per(timed(run, runs))
    rec['c_tracker_sweep_run']['groups'] = result[0].groups
    d_in = tuple(torch.from_numpy(np.stack([v[i] for v in videos])).to(dev) for i in (0, 1, 2))
    vo = video_of.to(torch.int32)
    out, kernel_ms = None, []
    for i in range(runs + 1):
        multi.reset()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = multi.run(*d_in, vo, out=out)
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            kernel_ms.append(ev[0].elapsed_time(ev[1]))
    rec['c_run_launch_alone'] = dict(kernel_ms=spread(kernel_ms),
                                     us_per_sequence_frame=spread(np.asarray(kernel_ms) * 1e3 / (B * F)))
    assert result[0].overflowed() == [] and int(multi.status.max()) == 0
    same = np.array_equal(out[2].cpu().numpy(), result[0].n) and np.array_equal(out[1].cpu().numpy(), result[0].ids)
    rec['run_equals_sweep_result'] = bool(same)
    t0 = time.perf_counter()
    scores = result[0].scores([v[3] for v in videos])
    rec['scores_device_backend_s'] = time.perf_counter() - t0
    k, opts, best = result[0].best('HOTA')
    rec['best'] = dict(index=k, options=opts, HOTA=best['HOTA'], IDSW=best['IDSW'],
                       distinct_HOTA=len({round(s['HOTA'], 9) for s in scores}))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--videos', type=int, default=8)
    ap.add_argument('--sets', type=int, default=128)
    ap.add_argument('--small-sets', type=int, default=8)
    ap.add_argument('--frames', type=int, default=512)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--baseline-only', action='store_true')
    ap.add_argument('--baseline-parent', default=None)
    ap.add_argument('--assoc-parent', default=None)
    ap.add_argument('--assoc-this', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sweep_bench.json'))
    a = ap.parse_args()
    has_sweep = library_has_sweep()
    import torch
    assert torch.cuda.is_available(), 'sweep_bench needs a GPU'
    dev = torch.device('cuda:0')
    videos = [video(1000 + v, a.frames) for v in range(a.videos)]
    out = dict(tool='tools/sweep_bench.py', device=torch.cuda.get_device_name(0), runs=a.runs,
               library_has_sweep_entry_points=has_sweep, baseline_only=bool(a.baseline_only or not has_sweep),
               max_dets=M, max_tracks=MAX_TRACKS,
               shapes=[measure(videos, option_sets(k), a.runs, has_sweep, a.baseline_only, dev)
                       for k in (a.sets, a.small_sets)])
    if a.baseline_parent:
        out['parent_commit_baseline'] = json.load(open(a.baseline_parent))
    for key, path in (('assoc_bench_parent_commit', a.assoc_parent), ('assoc_bench_this_commit', a.assoc_this)):
        if path:
            out[key] = [line for line in open(path).read().splitlines() if line.strip()]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
