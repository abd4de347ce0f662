#!/usr/bin/env python
"""sgbm_bench.py - cost of the StereoSGBM module (csrc/sgbm.hip) on MI355X.

Prints ONE JSON line with
  * stage_ms: device-event time of SGBM over --pairs stereo pairs at 1280 x 720, D = 48 (the reproducibility.md section 3
    set), median of --reps: the whole call from fp32 batches and from uint8 frames, and its parts - prefilter + cost +
    top->bottom pass (st_sgbm_match_f32 without outputs), + the row pass (with the int16 map), median, speckle filter +
    pack;
  * test_step: frame-pairs/s of model.test_step at --frames frames per call, the SGBM config (left + right uint8
    frames) against the PNG-disparity config (left uint8 + the fp32 disparity), alternated in one process, --repeats
    times each; ratio = median(sgbm) / median(png).  Same detector, seeded random weights.

  python tools/sgbm_bench.py [--pairs 8] [--frames 64] [--repeats 3] [--reps 20] [--out profiles/sgbm_bench.json]
  rocprofv3 --kernel-trace --stats -d DIR -o sgbm -- python tools/sgbm_bench.py --stage-only   # per-kernel times
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

h, w, H, W = 720, 1280, 736, 1280


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
    fr = [synthetic_stereo_pair(i, h, w, max_disp=48) for i in range(B)]
    left = [torch.from_numpy(f['left']).to(dev) for f in fr]
    right = [torch.from_numpy(f['right']).to(dev) for f in fr]
    return left, right


def stage_ms(dev, reps, B):
    from stereotracking_amd import _lib
    from stereotracking_amd._lib import check, current_stream, ptr
    from stereotracking_amd.engine import RawChunk
    from stereotracking_amd.sgbm import StereoSGBM
    lib = _lib.load()
    m = StereoSGBM()
    left, right = pairs(B, dev)
    lb = torch.full((B, 3, H, W), 114.0, device=dev)
    rb = torch.full((B, 3, H, W), 114.0, device=dev)
    for i in range(B):
        lb[i, :, :h] = left[i].float()
        rb[i, :, :h] = right[i].float()
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


def build(dev, B, sgbm):
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.synthetic import synthetic_state_dict
    name = 'stereo_yolox_s_mot_airdrone_sgbm.py' if sgbm else 'yolox_s_mmyolo_mot_airdrone_disp.py'
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', name))
    model = MODELS.build(dict(cfg.model, dense_batch=B, inflight=3, tuning_cache=os.environ.get('ST_TUNE_CACHE')))
    sd = synthetic_state_dict(list(model.detector._table), seed=0)
    model.detector.load_state_dict(sd, strict=False)
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=8)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=2, help='test_step calls per timed repeat')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--stage-only', action='store_true', help='only the stage cost (e.g. under rocprofv3 --kernel-trace)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(metric='sgbm_cost', stage_ms=stage_ms(dev, args.reps, args.pairs))
    if not args.stage_only:
        from stereotracking_amd.structures import TrackDataSample
        B, F = 8, args.frames
        left, right = pairs(B, dev)
        left = [left[i % B][None] for i in range(F)]
        right = [right[i % B][None] for i in range(F)]
        from stereotracking_amd.synthetic import synthetic_stereo_pair
        disp = [torch.from_numpy(np.repeat(synthetic_stereo_pair(i, h, w, max_disp=48)['disp'][None].astype(np.float32),
                                           3, 0))[None].to(dev) for i in range(B)]
        disp = [disp[i % B] for i in range(F)]
        models = {False: build(dev, B, False), True: build(dev, B, True)}
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
        res['test_step'] = dict(frames_per_call=F, png=[round(v, 2) for v in runs[False]],
                                sgbm=[round(v, 2) for v in runs[True]], unit='frame-pairs/s', ratio=round(sg / png, 4))
    res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
