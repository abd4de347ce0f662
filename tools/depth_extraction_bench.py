#!/usr/bin/env python
"""depth_extraction_bench.py - cost and accuracy of the per-box depth estimators (csrc/box_depth.hip) on MI355X.

Prints ONE JSON line with
  * kernel_us: device-event time of ONE per-box depth launch per method on the bench workload's boxes (bench.py's
    pipeline: 8 stereo pairs at 1280 x 720, seeded synthetic weights, its own disparity and kept boxes), measured as
    --launches back-to-back launches between two events, divided; median / min / max over --reps rounds, the methods
    alternated inside every round.  ratio = median / median of 'reference'.
  * depth_error: on a tools/make_tiny_airdrone.py dataset (depth PNGs = gt depth), the MOT shell (the _disp config,
    widen 0.375, seeded weights) per method; mean and median |depth - gt_depth| over the tracks where both are
    estimated (not -1, not NaN), how many tracks were left out, and how many kept a depth outside the valid range
    (0, 150) m ('center' reads the raw map: a centre pixel on an invalid disparity gives ~1.6e8 m).

  python tools/depth_extraction_bench.py [--reps 30] [--launches 20] [--out profiles/depth_extraction_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

METHODS = ('reference', 'truncated_mean', 'mean', 'median', 'center')


def kernel_times(dev, reps, launches):
    from stereotracking_amd._lib import check, current_stream, ptr
    from stereotracking_amd.pipeline import DEPTH_METHODS, StereoDensePipeline
    from stereotracking_amd.synthetic import synthetic_batch, synthetic_state_dict
    B = 8
    pipe = StereoDensePipeline(B, (720, 1280), 0.5, 0.33, 1, stereo=True, max_disp=192, max_det=1000, agg_layers=2)
    pipe.load_state_dict(synthetic_state_dict(pipe.param_table(), seed=0))
    batch = synthetic_batch(list(range(B)), 720, 1280, 192)
    out = pipe.run(batch['img'].to(dev), batch['right'].to(dev))
    torch.cuda.synchronize()
    disp, boxes, counts = out['disp_postp'], out['boxes'].clone(), out['counts'].clone()
    n_boxes = int(counts.clamp(max=pipe.max_det).sum().item())
    M = boxes.shape[1]
    res = [torch.empty(B, M, device=dev), torch.empty(B, M, device=dev), torch.empty(B, M, 4, device=dev)]
    lib = pipe.lib

    def launch(code):
        args = (ptr(disp), 3 * pipe.height * pipe.width, B, pipe.height, pipe.width, ptr(boxes), ptr(counts), M,
                pipe.baseline, pipe.focal_length, None, 0, current_stream(), ptr(res[0]), ptr(res[1]), ptr(res[2]))
        if code == 0:
            check(lib.st_box_depth(*args), 'st_box_depth')
        else:
            check(lib.st_box_depth_method(*args, code), 'st_box_depth_method')

    for m in METHODS:                       # warm-up: code objects loaded, caches in steady state
        for _ in range(5):
            launch(DEPTH_METHODS[m])
    torch.cuda.synchronize()
    times = {m: [] for m in METHODS}
    for _ in range(reps):
        for m in METHODS:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                launch(DEPTH_METHODS[m])
            b.record()
            b.synchronize()
            times[m].append(a.elapsed_time(b) * 1000.0 / launches)
    ref = statistics.median(times['reference'])
    out = {m: dict(median=round(statistics.median(t), 2), min=round(min(t), 2), max=round(max(t), 2),
                   ratio=round(statistics.median(t) / ref, 3)) for m, t in times.items()}
    return out, n_boxes


def depth_error(dev, videos, frames):
    from make_tiny_airdrone import make
    from stereotracking_amd import datasets as ds
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.structures import TrackDataSample
    from stereotracking_amd.synthetic import synthetic_state_dict
    h, w = 96, 160
    with tempfile.TemporaryDirectory() as tmp:
        base, _ = make(tmp, videos=videos, frames=frames, height=h, width=w, max_disp=32, objects=4)
        dataset = ds.MOTDispDataset(ann_file='annotations/val_cocoformat_80.json', data_root=base + os.sep,
                                    data_prefix=dict(img_path='val/'), depth_dir_name='depth')
        vids = []
        for _, idx in dataset.video_indices():
            seq, _, _, depth = ds.load_video(dataset, idx, False, with_depth=True, pin=False)
            codes = seq.codes.numpy().view(np.uint16)
            disp = np.where(codes == 65535, 0.0, codes / 16.0).astype(np.float32)
            vids.append((seq.left.numpy(), disp, depth.astype(np.float32)))
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone_disp.py'))
    for part in ('backbone', 'neck'):
        cfg.model.detector[part]['widen_factor'] = 0.375
    cfg.model.detector.bbox_head.head_module['widen_factor'] = 0.375
    cfg.model.tracker['init_track_thr'] = 0.03
    cfg.model.tracker['obj_score_thr'] = 0.02
    result = {}
    for m in METHODS:
        errs, left_out, outside = [], 0, 0
        for left, disp, depth in vids:
            model = MODELS.build(dict(cfg.model, autotune=False, dense_batch=4, inflight=2, depth_extraction=m))
            sd = synthetic_state_dict(list(model.detector._table), seed=5, prior_prob=0.2, logit_std=2.5)
            model.detector.load_state_dict(sd, strict=False)
            T = len(left)
            data = dict(inputs=dict(img=[torch.from_numpy(left[t:t + 1]).to(dev) for t in range(T)],
                                    disp_postp=[torch.from_numpy(np.repeat(disp[t:t + 1, None], 3, axis=1)).to(dev)
                                                for t in range(T)],
                                    depth_postp=[torch.from_numpy(depth[t:t + 1, None]).to(dev) for t in range(T)]),
                        data_samples=[TrackDataSample(dict(frame_id=t, ori_shape=(h, w), img_shape=(h, w),
                                                           scale_factor=(1.0, 1.0))) for t in range(T)])
            for s in model.test_step(data):
                d = s.pred_track_instances.depth.cpu().numpy()
                g = s.pred_track_instances.gt_depth.cpu().numpy()
                ok = np.isfinite(d) & np.isfinite(g) & (d != -1) & (g != -1)
                errs += np.abs(d[ok] - g[ok]).astype(np.float64).tolist()
                left_out += int((~ok).sum())
                outside += int((ok & ((d <= 0) | (d >= 150))).sum())
        result[m] = dict(mean_abs_err_m=round(float(np.mean(errs)), 4) if errs else None,
                         median_abs_err_m=round(float(np.median(errs)), 4) if errs else None, tracks=len(errs),
                         left_out=left_out, outside_0_150=outside)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--videos', type=int, default=3)
    ap.add_argument('--frames', type=int, default=24)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('depth_extraction_bench.py needs a GPU')
    dev = torch.device('cuda:0')
    kt, n_boxes = kernel_times(dev, args.reps, args.launches)
    rec = dict(device=torch.cuda.get_device_properties(0).name, workload='bench.py: 8 pairs 1280x720, seed 0',
               boxes=n_boxes, kernel_us=kt, launches_per_sample=args.launches, reps=args.reps,
               depth_error=depth_error(dev, args.videos, args.frames),
               depth_error_dataset=f'make_tiny_airdrone: {args.videos} videos x {args.frames} frames, 96x160')
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
