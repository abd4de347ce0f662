#!/usr/bin/env python
"""MultiStreamTracker at the size users run, against the single-video shell, in ONE process -> profiles/multistream_bench.json.

Workload: the cost-volume stereo config at 1280x720, D = 192, full YOLOX-s, `sequence.synthetic_sequence` frames uploaded
as uint8 (padded with 114 as the dataset pipeline pads them), shipped tracker thresholds, S streams in {8, 32}: stream s
shows video s % videos from a start offset of its own, so the streams of a tick stand at different frames.

Legs, every shape warmed first, alternated, each repeated `--repeats` times (median and max - min are reported):
  tick_sync_ms       MultiStreamTracker.step() with a device synchronise per tick: the latency of one frame from each
                     of S cameras
  run_frames_per_s   MultiStreamTracker.run() over `--ticks` ticks
  A  test_step_S     model.test_step on S frames of one video per call, synchronised per call (same dense work, host
                     association)
  B  test_steps_64   model.test_steps with 64 frames per call (the single-video shell at its best)
  C  test_step_1     model.test_step with one frame per call, ms per frame (the reference's call shape)

`--leg run` runs the run() leg alone (for a kernel trace).  There is no CPU mode: without a device the tool stops."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--streams', type=int, nargs='+', default=[8, 32])
    ap.add_argument('--ticks', type=int, default=64, help='ticks per run() / step() leg (>= 64 for the record)')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--videos', type=int, default=8, help='distinct synthetic videos the streams show')
    ap.add_argument('--leg', choices=['all', 'run'], default='all')
    ap.add_argument('--max-disp', type=int, default=192)
    ap.add_argument('--max-det', type=int, default=1000)
    ap.add_argument('--objects', type=int, default=6)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multistream_bench.json'))
    return ap.parse_args(argv)


def spread(vals):
    return dict(median=statistics.median(vals), spread=max(vals) - min(vals), runs=[round(v, 4) for v in vals])


def main():
    a = parse()
    import torch
    if not torch.cuda.is_available():
        sys.exit('multistream_bench: no device - the tool measures the HIP path on a GPU and has no CPU mode')
    import stereotracking_amd  # noqa: F401  (before the first CUDA call: hardware queues)
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.multistream import MultiStreamTracker
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.sequence import synthetic_sequence
    from stereotracking_amd.structures import TrackDataSample
    from stereotracking_amd.synthetic import pad_to_divisor, synthetic_state_dict
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    H, W, T = 720, 1280, a.ticks
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort',
                                       'stereo_yolox_s_mot_airdrone_costvolume.py'))
    cfg.model.stereo['max_disp'] = a.max_disp
    model = MODELS.build(dict(cfg.model, dense_batch=8, inflight=3, max_det=a.max_det))
    table = list(model.detector._table) + [('stereo.' + n, shp) for n, shp in model.stereo.param_table()]
    # the weights of the configs[2] fixture: a few hundred detections and ~10 tracks per frame
    sd = synthetic_state_dict(table, seed=0, prior_prob=0.01, logit_std=0.6)
    model.detector.load_state_dict(sd, strict=False)
    model.stereo.load_state_dict({k[len('stereo.'):]: v for k, v in sd.items() if k.startswith('stereo.')})

    t0 = time.perf_counter()
    videos = []
    for v in range(a.videos):
        left, right = [], []
        for f in synthetic_sequence(T, a.objects, H, W, a.max_disp, seed=3 + v):
            left.append(torch.from_numpy(pad_to_divisor(f['left'], 32, 114))[None].to(dev))
            right.append(torch.from_numpy(pad_to_divisor(f['right'], 32, 114))[None].to(dev))
        videos.append((left, right))
    print(f'{a.videos} videos of {T} frames uploaded in {time.perf_counter() - t0:.1f} s', flush=True)

    def sample(fid, **more):
        return TrackDataSample(dict(frame_id=fid, ori_shape=(H, W), img_shape=(H, W), scale_factor=(1.0, 1.0), **more))

    def tick(S, k):      # stream s: video s % videos, `s // videos * 7 + s` frames ahead, wrapping; frame id = tick
        fr = [(s % a.videos, (k + s // a.videos * 7 + s) % T) for s in range(S)]
        return dict(inputs=dict(img=[videos[v][0][f] for v, f in fr], right=[videos[v][1][f] for v, f in fr]),
                    data_samples=[sample(k, stream=s) for s in range(S)])

    def call(v, lo, hi):
        return dict(inputs=dict(img=videos[v][0][lo:hi], right=videos[v][1][lo:hi]),
                    data_samples=[sample(t) for t in range(lo, hi)])

    stats = dict(frames=0, dets=0, tracks=0)

    def count(outs):
        stats['frames'] += len(outs)
        stats['dets'] += sum(len(o.pred_det_instances) for o in outs)
        stats['tracks'] += sum(len(o.pred_track_instances) for o in outs)

    def leg_tick_sync(mst, S):
        ms = []
        for k in range(T):
            d = tick(S, k)
            torch.cuda.synchronize()
            t = time.perf_counter()
            count(mst.step(d))
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t) * 1e3)
        return statistics.median(ms)

    def leg_run(mst, S):
        torch.cuda.synchronize()
        t = time.perf_counter()
        n = 0
        for outs in mst.run(tick(S, k) for k in range(T)):
            n += len(outs)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t)

    def leg_a(S):        # S frames of one video per call
        ms = []
        for v in range(a.videos):
            for lo in range(0, T - S + 1, S):
                d = call(v, lo, lo + S)
                torch.cuda.synchronize()
                t = time.perf_counter()
                model.test_step(d)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t) * 1e3)
        return statistics.median(ms)

    def leg_b():         # 64 frames per call through the primed loop
        per = min(64, T)
        torch.cuda.synchronize()
        t = time.perf_counter()
        n = sum(len(o) for o in model.test_steps(call(v, lo, lo + per) for v in range(a.videos)
                                                 for lo in range(0, T - per + 1, per)))
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t)

    def leg_c():         # one frame per call
        ms = []
        for t_ in range(T):
            d = call(0, t_, t_ + 1)
            torch.cuda.synchronize()
            t = time.perf_counter()
            model.test_step(d)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t) * 1e3)
        return statistics.median(ms)

    trackers = {S: MultiStreamTracker(model, streams=S) for S in a.streams}
    if a.leg == 'run':
        for S, mst in trackers.items():
            leg_run(mst, S)              # warm
            print(f'S={S}: run() {leg_run(mst, S):.1f} frames/s', flush=True)
        return
    # warm every shape: the plans (batch 8; batch 1 is measured on its first use), the device trackers, the pinned buffers
    for S, mst in trackers.items():
        for k in range(3):
            mst.step(tick(S, k))
        model.test_step(call(0, 0, S))
    model.test_step(call(0, 0, 1))
    list(model.test_steps([call(0, 0, min(64, T))]))
    torch.cuda.synchronize()
    stats.update(frames=0, dets=0, tracks=0)
    res = {S: dict(tick_sync_ms=[], run_frames_per_s=[], test_step_S_ms=[]) for S in a.streams}
    b, c = [], []
    for r in range(a.repeats):
        for S, mst in trackers.items():
            res[S]['tick_sync_ms'].append(leg_tick_sync(mst, S))
            res[S]['test_step_S_ms'].append(leg_a(S))
            res[S]['run_frames_per_s'].append(leg_run(mst, S))
        b.append(leg_b())
        c.append(leg_c())
        print(f'repeat {r}: ' + json.dumps({S: {k: round(v[-1], 3) for k, v in res[S].items()} for S in res})
              + f' test_steps_64 {b[-1]:.1f} frames/s, test_step_1 {c[-1]:.3f} ms', flush=True)
    rec = dict(
        what='MultiStreamTracker (one frame from each of S streams per tick) against the single-video shell, one process',
        workload=dict(config='stereo_yolox_s_mot_airdrone_costvolume.py', size=[H, W], max_disp=a.max_disp,
                      detector='YOLOX-s (widen 0.5, deepen 0.33)', frames='sequence.synthetic_sequence, uint8, padded with 114',
                      tracker='shipped thresholds', videos=a.videos, ticks=T, dense_batch=8, inflight=model.inflight,
                      queue_depth=model.queue_depth, max_det=a.max_det, max_tracks=128,
                      detections_per_frame=stats['dets'] / max(1, stats['frames']),
                      tracks_per_frame=stats['tracks'] / max(1, stats['frames'])),
        device=torch.cuda.get_device_name(0), repeats=a.repeats,
        hw_queues=stereotracking_amd.effective_hw_queues(),
        streams={str(S): {k: spread(v) for k, v in res[S].items()} for S in res},
        test_steps_64_frames_per_s=spread(b), test_step_1_ms_per_frame=spread(c))
    for S in res:
        s = rec['streams'][str(S)]
        s['tick_vs_test_step_S'] = s['tick_sync_ms']['median'] / s['test_step_S_ms']['median']
        s['tick_vs_S_one_frame_calls'] = s['tick_sync_ms']['median'] / (S * rec['test_step_1_ms_per_frame']['median'])
        s['run_vs_test_steps_64'] = s['run_frames_per_s']['median'] / rec['test_steps_64_frames_per_s']['median']
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
