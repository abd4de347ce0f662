#!/usr/bin/env python
"""cmc_bench.py - cost of the tracker's Mesh-Affine camera-motion compensation (csrc/cmc_flow.hip) on MI355X.

Prints ONE JSON line with
  * chunk_ms: device-event time of the CMC work of one 8-frame chunk at 1280 x 720 (grey planes of the 8 frames + the
    8 speculative warps: the launches the MOT shell enqueues per chunk on its CMC stream), median of --reps, alone;
  * test_step: stereo frame-pairs/s of model.test_step at --frames frames per call (the bench.py test_step leg's model:
    the stereo config, seeded random weights) with the tracker's CMC off and on, alternated in one process on the
    same box, --repeats times each; ratio = median(on) / median(off).

  python tools/cmc_bench.py [--frames 64] [--repeats 3] [--reps 20] [--out profiles/cmc_bench.json]
  rocprofv3 --kernel-trace --stats -d DIR -o cmc -- python tools/cmc_bench.py --chunk-only   # per-kernel times
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def chunk_ms(dev, reps, B=8, h=720, w=1280):
    from stereotracking_amd import cmc
    g = torch.Generator().manual_seed(0)
    frames = [torch.randint(0, 256, (1, 3, h, w), generator=g, dtype=torch.uint8).to(dev) for _ in range(B)]
    prm = cmc.glme_params()
    planes = torch.empty(B + 1, cmc.SIDE, cmc.SIDE, dtype=torch.uint8, device=dev)
    ws = torch.empty(int(cmc._lib.load().st_cmc_workspace_bytes(B)), dtype=torch.uint8, device=dev)

    def once():
        cmc.front(frames, h, w, out=planes[1:])
        return cmc.estimate(planes[:-1], planes[1:], h, w, prm, ws=ws)
    for _ in range(3):
        once()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        once()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return dict(median=round(statistics.median(t), 4), min=round(min(t), 4), max=round(max(t), 4), reps=reps)


def build(dev, B, cmc_on):
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.synthetic import synthetic_state_dict
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort',
                                       'stereo_yolox_s_mot_airdrone_costvolume.py'))
    if cmc_on:
        cfg.model.tracker['cmc'] = dict(method='glme_affine')
    model = MODELS.build(dict(cfg.model, dense_batch=B, inflight=3, tuning_cache=os.environ.get('ST_TUNE_CACHE')))
    table = list(model.detector._table) + [('stereo.' + n, s) for n, s in model.stereo.param_table()]
    sd = synthetic_state_dict(table, seed=0)
    model.detector.load_state_dict(sd, strict=False)
    model.stereo.load_state_dict({k[len('stereo.'):]: v for k, v in sd.items() if k.startswith('stereo.')})
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=4, help='test_step calls per timed repeat')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--chunk-only', action='store_true', help='only the chunk cost (e.g. under rocprofv3 --kernel-trace)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    if args.chunk_only:
        print(json.dumps(dict(metric='cmc_cost', chunk_ms=chunk_ms(dev, args.reps))))
        return
    from stereotracking_amd.structures import TrackDataSample
    from stereotracking_amd.synthetic import synthetic_batch
    res = dict(metric='cmc_cost', chunk_ms=chunk_ms(dev, args.reps), frames_per_call=args.frames)
    B, F = 8, args.frames
    bc = synthetic_batch(list(range(B)), 736, 1280, 192)
    left = [bc['img'][i % B:i % B + 1, :, :720].to(torch.uint8).to(dev) for i in range(F)]
    right = [bc['right'][i % B:i % B + 1, :, :720].to(torch.uint8).to(dev) for i in range(F)]
    models = {False: build(dev, B, False), True: build(dev, B, True)}
    frame = {False: 0, True: 0}

    def call(on):
        m = models[on]
        samples = [TrackDataSample(dict(frame_id=frame[on] + i, ori_shape=(720, 1280), img_shape=(720, 1280),
                                        scale_factor=(1.0, 1.0))) for i in range(F)]
        frame[on] += F
        return m.test_step(dict(inputs=dict(img=left, right=right), data_samples=samples))
    for on in (False, True):
        for _ in range(2):
            call(on)
    torch.cuda.synchronize()
    runs = {False: [], True: []}
    for _ in range(args.repeats):
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call(on)
            torch.cuda.synchronize()
            runs[on].append(args.calls * F / (time.perf_counter() - t0))
    off, on = statistics.median(runs[False]), statistics.median(runs[True])
    res['test_step'] = dict(off=[round(v, 2) for v in runs[False]], on=[round(v, 2) for v in runs[True]],
                            unit='stereo frame-pairs/s', ratio=round(on / off, 4), target=0.90)
    res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
