#!/usr/bin/env python
"""rectify_bench.py - cost of StereoRectify (csrc/rectify.hip) on MI355X.

Prints ONE JSON line (and writes it to --out) with
  * launch: device-event time of ONE chunk launch - --pairs left + right uint8 frames of --size x 3 through the two maps
    of configs/.../stereo_yolox_s_mot_airdrone_sgbm_rectify.py - median of --reps; the bytes the launch must move
    (sources + the maps once + outputs) and the fraction of the 8 TB/s HBM peak that time amounts to;
  * yardstick (recorded, not asserted): torch.nn.functional.grid_sample (bilinear, zeros padding, align_corners=True) on
    the same frames as fp32 with the float maps - alone, and with the uint8 -> fp32 -> uint8 casts a user would pay;
  * test_step: frame-pairs/s of model.test_step at --frames frames per call on the SGBM config and on the cost-volume
    config, with and without `rectify`, alternated in one process per config, --repeats times each;
  * with --parent-tree DIR (a checkout of the parent commit with its library built): the same rectify-off measurement
    run from that tree, in a process of its own between this tree's, beside the figures above.

  python tools/rectify_bench.py [--pairs 8] [--frames 64] [--repeats 3] [--parent-tree DIR] [--out profiles/rectify_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(os.environ.get('RECTIFY_BENCH_TREE') or HERE)      # the tree whose package a child process measures
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CFG_DIR = os.path.join('configs', 'stereo_tracking', 'ocsort')
CONFIGS = dict(sgbm='stereo_yolox_s_mot_airdrone_sgbm.py', costvolume='stereo_yolox_s_mot_airdrone_costvolume.py')
HBM_PEAK = 8e12


def _timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return dict(median=round(statistics.median(t), 4), min=round(min(t), 4), max=round(max(t), 4), reps=reps)


def calibration():
    from stereotracking_amd.config import Config
    cfg = Config.fromfile(os.path.join(HERE, CFG_DIR, 'stereo_yolox_s_mot_airdrone_sgbm_rectify.py'))
    return {k: v for k, v in cfg.model.rectify.items()}


def frames(n, h, w, dev):
    from stereotracking_amd.synthetic import synthetic_stereo_pair
    fr = [synthetic_stereo_pair(i, h, w, max_disp=48) for i in range(n)]
    return [torch.from_numpy(f['left'])[None].to(dev) for f in fr], [torch.from_numpy(f['right'])[None].to(dev) for f in fr]


def launch_cost(dev, args):
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd import rectify  # noqa: F401
    rect = MODELS.build(calibration())
    (h, w), B = rect.size, args.pairs
    left, right = frames(B, h, w, dev)
    srcs, idx = left + right, [0] * B + [1] * B
    out = torch.empty(2 * B, 3, h, w, dtype=torch.uint8, device=dev)
    rect.device_maps(dev)
    res = dict(pairs=B, size=[h, w], planes=3, time_ms=_timed(lambda: rect.remap(srcs, idx, out=out), args.reps))
    moved = 2 * (2 * B * 3 * h * w) + rect.maps.nbytes
    res['bytes_moved'] = int(moved)
    res['fraction_of_8TBps'] = round(moved / (res['time_ms']['median'] * 1e-3) / HBM_PEAK, 4)
    res['valid_fraction'] = [round(float(rect.valid_mask(c).mean()), 4) for c in ('left', 'right')]
    # yardstick: grid_sample with the float maps (pixel -> [-1, 1], align_corners=True)
    import torch.nn.functional as F
    g = np.stack(np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)), -1)
    grids = []
    for cam in ('left', 'right'):
        mx, my = rect.float_map(cam, g[..., 0], g[..., 1])
        grids.append(np.stack([2 * mx / (w - 1) - 1, 2 * my / (h - 1) - 1], -1).astype(np.float32))
    grid = torch.from_numpy(np.stack([grids[i] for i in idx])).to(dev)
    u8 = torch.cat(srcs)
    f32 = u8.float()
    res['grid_sample_ms'] = _timed(lambda: F.grid_sample(f32, grid, mode='bilinear', padding_mode='zeros', align_corners=True),
                                   args.reps)
    res['grid_sample_with_casts_ms'] = _timed(
        lambda: F.grid_sample(u8.float(), grid, mode='bilinear', padding_mode='zeros', align_corners=True)
        .add_(0.5).clamp_(0, 255).to(torch.uint8), args.reps)
    return res


def build(name, rectify, B, max_det):
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.synthetic import synthetic_state_dict
    cfg = Config.fromfile(os.path.join(ROOT, CFG_DIR, CONFIGS[name]))
    extra = dict(rectify=rectify) if rectify is not None else {}
    model = MODELS.build(dict(cfg.model, dense_batch=B, inflight=3, max_det=max_det,
                              tuning_cache=os.environ.get('ST_TUNE_CACHE'), **extra))
    table = list(model.detector._table)
    if hasattr(model.stereo, 'param_table'):
        table += [('stereo.' + n, shp) for n, shp in model.stereo.param_table()]
    sd = synthetic_state_dict(table, seed=0)
    model.detector.load_state_dict(sd, strict=False)
    if hasattr(model.stereo, 'param_table'):
        model.stereo.load_state_dict({k[len('stereo.'):]: v for k, v in sd.items() if k.startswith('stereo.')})
    return model


def test_step_rate(dev, args, name, with_rectify):
    """frame-pairs/s of test_step on config `name`: rectify off (and on, alternated, when with_rectify)."""
    from stereotracking_amd.structures import TrackDataSample
    cal = calibration() if with_rectify else None
    h, w = (720, 1280)
    B, F = 8, args.frames
    left, right = frames(B, h, w, dev)
    left, right = [left[i % B] for i in range(F)], [right[i % B] for i in range(F)]
    legs = [False, True] if with_rectify else [False]
    models = {on: build(name, cal if on else None, B, args.max_det) for on in legs}
    frame = dict.fromkeys(legs, 0)

    def call(on):
        samples = [TrackDataSample(dict(frame_id=frame[on] + i, ori_shape=(h, w), img_shape=(h, w), scale_factor=(1.0, 1.0)))
                   for i in range(F)]
        frame[on] += F
        return models[on].test_step(dict(inputs=dict(img=left, right=right), data_samples=samples))
    for on in legs:
        for _ in range(2):
            call(on)
    torch.cuda.synchronize()
    runs = {on: [] for on in legs}
    for _ in range(args.repeats):
        for on in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call(on)
            torch.cuda.synchronize()
            runs[on].append(round(args.calls * F / (time.perf_counter() - t0), 2))
    res = dict(frames_per_call=F, unit='frame-pairs/s', rectify_off=runs[False])
    if with_rectify:
        res['rectify_on'] = runs[True]
        res['ratio'] = round(statistics.median(runs[True]) / statistics.median(runs[False]), 4)
    return res


def child(tree, name, with_rectify, args):
    env = dict(os.environ, RECTIFY_BENCH_TREE=os.path.abspath(tree))
    cmd = [sys.executable, os.path.abspath(__file__), '--leg', name, '--frames', str(args.frames), '--repeats',
           str(args.repeats), '--calls', str(args.calls), '--max-det', str(args.max_det)] + ([] if with_rectify else ['--off-only'])
    out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=900).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=8)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=2, help='test_step calls per timed repeat')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--max-det', type=int, default=1000)
    ap.add_argument('--parent-tree', default=None, help='a checkout of the parent commit (library built): its rectify-off rate')
    ap.add_argument('--launch-only', action='store_true')
    ap.add_argument('--leg', default=None, help='(child process) measure one config of the tree $RECTIFY_BENCH_TREE names')
    ap.add_argument('--off-only', action='store_true', help='(child process) rectify off only')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(test_step_rate(torch.device('cuda:0'), args, args.leg, not args.off_only)))
        return
    res = dict(metric='rectify_cost')
    if not args.launch_only:       # the child processes first: this process has not opened the GPU yet
        res['test_step'] = {}
        for name in CONFIGS:
            rec = {}
            if args.parent_tree:
                rec['parent_commit'] = child(args.parent_tree, name, False, args)
            rec['this_tree'] = child(HERE, name, True, args)
            res['test_step'][name] = rec
            print(f'{name}: {json.dumps(rec)}', file=sys.stderr, flush=True)
    res['launch'] = launch_cost(torch.device('cuda:0'), args)
    res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
