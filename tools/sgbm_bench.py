#!/usr/bin/env python
"""sgbm_bench.py - cost of the StereoSGBM module (csrc/sgbm.hip) on MI355X.

Prints ONE JSON line with
  * stage_ms: device-event time of SGBM over --pairs stereo pairs at --size (1280 x 720) and --num-disparities (48: the
    reproducibility.md section 3 set), median of --reps: the whole call from fp32 batches and from uint8 frames, and
    its parts - prefilter + cost +
    top->bottom pass (st_sgbm_match_f32 without outputs), + the row pass (with the int16 map), median, speckle filter +
    pack;
  * test_step: frame-pairs/s of model.test_step at --frames frames per call, the SGBM config (left + right uint8
    frames) against the PNG-disparity config (left uint8 + the fp32 disparity), alternated in one process, --repeats
    times each; ratio = median(sgbm) / median(png).  Same detector, seeded random weights.

  * with --sweep: `runs`, one such record per (size, D) of the sweep, instead;
  * with --baseline-library: `baseline`, the stage cost at --size / --num-disparities of that build of the library (the
    parent commit's, say) against this tree's, each in --repeats fresh processes, the legs alternated: per stage both
    builds' per-process medians, the baseline's spread (max - min of them) and whether this tree's median stays within
    the baseline's median + spread.

  python tools/sgbm_bench.py [--pairs 8] [--frames 64] [--repeats 3] [--reps 20] [--out profiles/sgbm_bench.json]
  python tools/sgbm_bench.py --num-disparities 192 --size 576x1600
  python tools/sgbm_bench.py --sweep '720x1280:48,128,192,256;576x1600:128,192' --baseline-library OLD.so \
      --out profiles/sgbm_wide_bench.json
  rocprofv3 --kernel-trace --stats -d DIR -o sgbm -- python tools/sgbm_bench.py --stage-only   # per-kernel times
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

h, w, H, W, D = 720, 1280, 736, 1280, 48


def set_geometry(size, num_disparities):
    """--size HxW, --num-disparities: the frames of every function below (H, W: padded to the detector's 32)."""
    global h, w, H, W, D
    h, w = (int(v) for v in size.lower().split('x'))
    H, W, D = (h + 31) // 32 * 32, (w + 31) // 32 * 32, int(num_disparities)


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


def pairs(B, dev):
    from stereotracking_amd.synthetic import synthetic_stereo_pair
    fr = [synthetic_stereo_pair(i, h, w, max_disp=D) for i in range(B)]
    left = [torch.from_numpy(f['left']).to(dev) for f in fr]
    right = [torch.from_numpy(f['right']).to(dev) for f in fr]
    return left, right


def stage_ms(dev, reps, B):
    from stereotracking_amd import _lib
    from stereotracking_amd._lib import check, current_stream, ptr
    from stereotracking_amd.engine import RawChunk
    from stereotracking_amd.sgbm import StereoSGBM
    lib = _lib.load()
    m = StereoSGBM(num_disparities=D)
    left, right = pairs(B, dev)
    lb = torch.full((B, 3, H, W), 114.0, device=dev)
    rb = torch.full((B, 3, H, W), 114.0, device=dev)
    for i in range(B):
        lb[i, :, :h, :w] = left[i].float()
        rb[i, :, :h, :w] = right[i].float()
    lc, rc = RawChunk(left, 114.0), RawChunk(right, 114.0)
    out = torch.empty(B, 3, H, W, device=dev)
    ws, _ = m.workspace(dev, B, h, w)
    prm = m.params()
    raw = torch.empty(B, h, w, dtype=torch.int16, device=dev)

    def match(with_rows):
        check(lib.st_sgbm_match_f32(ptr(lb), ptr(rb), B, H, W, h, w, C.byref(prm), ptr(ws), ws.numel(), None,
                                    ptr(raw) if with_rows else None, current_stream()), 'st_sgbm_match_f32')
    match(True)
    med = m.median(raw)                  # the speckle filter's real input (its cost depends on the components)
    res = dict(pairs=B, size=[h, w], D=m.num_disparities,
               total_f32=_timed(lambda: m.compute(lb, rb, (h, w), out), reps),
               total_u8=_timed(lambda: m.compute(lc, rc, (h, w), out), reps),
               prefilter_cost_tb=_timed(lambda: match(False), reps),
               prefilter_cost_tb_rows=_timed(lambda: match(True), reps),
               median=_timed(lambda: m.median(raw), reps),
               speckle_pack=_timed(lambda: m.speckle(med), reps))
    res['rows'] = round(res['prefilter_cost_tb_rows']['median'] - res['prefilter_cost_tb']['median'], 4)
    torch.cuda.synchronize()
    res['status'] = int(m.last_status.item())
    res['valid_fraction'] = round(float((out[:, 0, :h, :w] > 0).float().mean()), 4)
    return res


def build(dev, B, sgbm, max_det):
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.synthetic import synthetic_state_dict
    name = 'stereo_yolox_s_mot_airdrone_sgbm.py' if sgbm else 'yolox_s_mmyolo_mot_airdrone_disp.py'
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', name))
    if sgbm:
        cfg.model.stereo['num_disparities'] = D
    model = MODELS.build(dict(cfg.model, dense_batch=B, inflight=3, max_det=max_det,
                              tuning_cache=os.environ.get('ST_TUNE_CACHE')))
    sd = synthetic_state_dict(list(model.detector._table), seed=0)
    model.detector.load_state_dict(sd, strict=False)
    return model


def test_step_rate(dev, args):
    from stereotracking_amd.structures import TrackDataSample
    from stereotracking_amd.synthetic import synthetic_stereo_pair
    B, F = 8, args.frames
    left, right = pairs(B, dev)
    left = [left[i % B][None] for i in range(F)]
    right = [right[i % B][None] for i in range(F)]
    disp = [torch.from_numpy(np.repeat(synthetic_stereo_pair(i, h, w, max_disp=D)['disp'][None].astype(np.float32),
                                       3, 0))[None].to(dev) for i in range(B)]
    disp = [disp[i % B] for i in range(F)]
    models = {False: build(dev, B, False, args.max_det), True: build(dev, B, True, args.max_det)}
    frame = {False: 0, True: 0}

    def call(sg):
        samples = [TrackDataSample(dict(frame_id=frame[sg] + i, ori_shape=(h, w), img_shape=(h, w),
                                        scale_factor=(1.0, 1.0))) for i in range(F)]
        frame[sg] += F
        inputs = dict(img=left, right=right) if sg else dict(img=left, disp_postp=disp)
        return models[sg].test_step(dict(inputs=inputs, data_samples=samples))
    for sg in (False, True):
        for _ in range(2):
            call(sg)
    torch.cuda.synchronize()
    runs = {False: [], True: []}
    for _ in range(args.repeats):
        for sg in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call(sg)
            torch.cuda.synchronize()
            runs[sg].append(args.calls * F / (time.perf_counter() - t0))
    png, sg = statistics.median(runs[False]), statistics.median(runs[True])
    return dict(frames_per_call=F, max_det=args.max_det, png=[round(v, 2) for v in runs[False]],
                sgbm=[round(v, 2) for v in runs[True]],
                unit='frame-pairs/s', ratio=round(sg / png, 4))


def baseline(args):
    """The stage cost of --baseline-library against this tree's library: --repeats fresh processes each, alternated."""
    cmd = [sys.executable, os.path.abspath(__file__), '--stage-only', '--pairs', str(args.pairs), '--reps', str(args.reps),
           '--size', args.size, '--num-disparities', str(args.num_disparities)]
    legs = {'baseline': [], 'this': []}
    if args.repeats < 3:
        raise SystemExit('--baseline-library needs --repeats >= 3 (the spread of three processes per build)')
    for _ in range(args.repeats):
        for leg in ('baseline', 'this'):
            env = dict(os.environ)
            env.pop('ST_LIBRARY', None)
            if leg == 'baseline':
                env['ST_LIBRARY'] = os.path.abspath(args.baseline_library)
            out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600).stdout
            legs[leg].append(json.loads(out.strip().splitlines()[-1])['stage_ms'])
            print(f"{leg}: total_f32 {legs[leg][-1]['total_f32']['median']} ms", file=sys.stderr, flush=True)
    res = dict(size=[h, w], D=D, pairs=args.pairs, processes_per_build=len(legs['this']), stages={})
    for st in [k for k, v in legs['this'][0].items() if isinstance(v, dict) and 'median' in v]:   # the timed stages
        old = [r[st]['median'] for r in legs['baseline']]
        new = [r[st]['median'] for r in legs['this']]
        spread = max(old) - min(old)
        res['stages'][st] = dict(baseline=old, this=new, baseline_median=round(statistics.median(old), 4),
                                 baseline_spread=round(spread, 4), this_median=round(statistics.median(new), 4),
                                 within=bool(statistics.median(new) <= statistics.median(old) + spread))
    res['within'] = all(v['within'] for v in res['stages'].values())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=8)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=3, help='timed test_step repeats; processes per build of '
                    '--baseline-library (at least 3)')
    ap.add_argument('--calls', type=int, default=2, help='test_step calls per timed repeat')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--num-disparities', type=int, default=48, help='16, 32, 48, 64, 128, 192 or 256')
    ap.add_argument('--size', default='720x1280', help='HxW of the frames')
    ap.add_argument('--max-det', type=int, default=1000,
                    help='rows of the detection buffer of both test_step models (a capacity; overflow raises)')
    ap.add_argument('--sweep', default=None, help="'HxW:D,D,..;HxW:D,..': one record per (size, D) in `runs`")
    ap.add_argument('--baseline-library', default=None,
                    help='another build of libstereotrack_hip.so to compare the stage cost with (alternated processes)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--stage-only', action='store_true', help='only the stage cost (e.g. under rocprofv3 --kernel-trace)')
    args = ap.parse_args()
    set_geometry(args.size, args.num_disparities)
    res = dict(metric='sgbm_cost')
    if args.baseline_library:          # first: its child processes start before this one opens the GPU
        res['baseline'] = baseline(args)
    dev = torch.device('cuda:0')

    def one():
        rec = dict(stage_ms=stage_ms(dev, args.reps, args.pairs))
        if not args.stage_only:
            rec['test_step'] = test_step_rate(dev, args)
        return rec
    if args.sweep:
        res['runs'] = []
        for part in args.sweep.split(';'):
            size, levels = part.split(':')
            for d in levels.split(','):
                set_geometry(size, d)
                res['runs'].append(one())
                print(f"{size} D={d}: total_f32 {res['runs'][-1]['stage_ms']['total_f32']['median']} ms", file=sys.stderr,
                      flush=True)
                torch.cuda.empty_cache()
        set_geometry(args.size, args.num_disparities)
    else:
        res.update(one())
    res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
