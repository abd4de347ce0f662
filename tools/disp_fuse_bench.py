#!/usr/bin/env python
"""st_disp_fuse (csrc/disp_head.hip) at the product size, 8 x 736 x 1280 with a 3-plane disp_postp, on one MI355X, and what
depth_source='fused' costs the V2 shell.  Writes profiles/disp_fuse_bench.json (or --out):

  launch     modes 1 and 2: device ms of one call (hipEvents around it), median / min / max of --reps; the bytes the
             algorithm must move (one quarter-size read, one full read, one full write; mode 1 does not read disp, but
             the same 68 MB are charged to both so the two fractions compare) and the fraction of 8 TB/s
  bilinear   yardstick 1: st_disp_head_resize of the same head output to the same size in the same run (its bytes: the
             quarter-size read and the full write); profiles/disp_head_bench.json holds the figure at 720 x 1280
  torch      yardstick 2, record only: F.interpolate(bilinear, align_corners=False) + torch.where on the same tensors
  test_step  frame-pairs/s of model.test_steps on the V2 config, depth_source='fused' against 'input' (the parent's
             behaviour): one process, autotune off, alternated legs, --repeats each, 32 frames per call; the margin is
             the 'input' leg's own max - min plus the launch's share of a chunk

Seeded random weights and inputs: no trained completion weights exist, so nothing here says anything about the accuracy of
the filled depths."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

PEAK_HBM = 8.0e12
CFG = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone_disp_completion_v2.py')


def timed(fn, reps):
    """ms of fn() on the current stream, one event pair per call -> dict(median, min, max)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def bench_launch(a, dev):
    import torch.nn.functional as F
    from stereotracking_amd import _lib
    from stereotracking_amd._lib import check, current_stream, ptr
    lib = _lib.load()
    N, H, W, C = a.batch, 736, 1280, 3
    g = torch.Generator().manual_seed(0)
    dense = torch.relu(torch.randn(N, 1, H // 2, W // 2, generator=g) * 20 + 5).to(dev)
    disp = torch.rand(N, C, H, W, generator=g) * 60 + 0.5
    disp[:, 0][torch.rand(N, H, W, generator=g) < 0.3] = 0.0          # 30 % holes
    disp = disp.to(dev)
    out, filled = torch.empty(N, 1, H, W, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    up = torch.empty(N, 1, H, W, device=dev)
    quarter, full = 4.0 * N * (H // 2) * (W // 2), 4.0 * N * H * W
    res = dict(shape=dict(batch=N, height=H, width=W, disp_planes=C, holes=0.3))

    def fuse(mode, count=True):
        check(lib.st_disp_fuse(ptr(dense), ptr(disp), C * H * W, N, H, W, 720, 1280, mode, ptr(out),
                               ptr(filled) if count else None, current_stream()), 'st_disp_fuse')

    def bilinear():
        check(lib.st_disp_head_resize(ptr(dense), N, H // 2, W // 2, ptr(up), H, W, current_stream()), 'st_disp_head_resize')

    for name, fn, nbytes in (('mode1_completed', lambda: fuse(1), quarter + 2 * full),
                             ('mode2_fused', lambda: fuse(2), quarter + 2 * full),
                             ('mode2_fused_without_filled', lambda: fuse(2, False), quarter + 2 * full),
                             ('bilinear', bilinear, quarter + full)):
        t = timed(fn, a.reps)
        res[name] = dict(ms=t, mbytes=round(nbytes / 1e6, 2), fraction_of_8TBs=round(nbytes / (t['median'] * 1e-3) / PEAK_HBM, 4))
        print(name, res[name], flush=True)
    # the same map from torch ops (record only), and that it is the same map up to the interpolation's rounding
    def eager():
        u = F.interpolate(dense, size=(H, W), mode='bilinear', align_corners=False)
        return torch.where(disp[:, :1] > 0, disp[:, :1], u)
    t = timed(eager, a.reps)
    fuse(2)
    torch.cuda.synchronize()
    res['torch_interpolate_where'] = dict(ms=t, max_abs_diff_to_hip=float((eager() - out).abs().max()), note='record only')
    res['filled'] = filled.tolist()
    print('torch', res['torch_interpolate_where'], flush=True)
    return res


def bench_test_step(a, dev, launch_ms):
    import disp_head_ref as ref
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.structures import TrackDataSample
    from stereotracking_amd.synthetic import synthetic_batch, synthetic_state_dict
    Fc, ori = a.frames_per_call, (720, 1280)
    fr = synthetic_batch(list(range(8)), ori[0], ori[1], 192)
    imgs = [fr['img'][i % 8:i % 8 + 1, :, :ori[0]].to(torch.uint8).to(dev) for i in range(Fc)]
    disps = [fr['disp_postp'][i % 8:i % 8 + 1, :, :ori[0]].contiguous().to(dev) for i in range(Fc)]
    models = {}
    for src in ('input', 'fused'):
        cfg = Config.fromfile(CFG)
        cfg.model.detector.disparity_head['channels'] = a.channels
        model = MODELS.build(dict(cfg.model, dense_batch=a.batch, autotune=False, depth_source=src))
        sd = synthetic_state_dict(list(model.detector._table), seed=0)
        hs = ref.random_state_dict(128, a.channels, seed=1)
        hs['reg.conv.bias'] = torch.tensor([0.3])
        sd.update({'disp_head.' + k: v for k, v in hs.items()})
        model.detector.load_state_dict(sd, strict=False)
        models[src] = model

    def calls(n, t0):
        for c in range(n):
            samples = [TrackDataSample(dict(frame_id=t0 + c * Fc + t, ori_shape=ori, img_shape=ori, scale_factor=(1.0, 1.0)))
                       for t in range(Fc)]
            yield dict(inputs=dict(img=imgs, disp_postp=disps), data_samples=samples)

    rates = {k: [] for k in models}
    fill = None
    for k, m in models.items():           # warm: plans, buffers
        for outs in m.test_steps(calls(2, 0)):
            if k == 'fused':
                fill = outs[0].metainfo['disp_fill_ratio']
        torch.cuda.synchronize()
    for r in range(a.repeats):
        for k, m in models.items():       # alternated legs
            t0 = time.perf_counter()
            n = 0
            for outs in m.test_steps(calls(a.calls, 1000 * (r + 1))):
                n += len(outs)
            torch.cuda.synchronize()
            rates[k].append(n / (time.perf_counter() - t0))
            print(k, round(rates[k][-1], 1), flush=True)
    med = {k: statistics.median(v) for k, v in rates.items()}
    chunk_ms = a.batch / med['input'] * 1e3
    spread = (max(rates['input']) - min(rates['input'])) / med['input']
    share = launch_ms / chunk_ms
    gap = (med['input'] - med['fused']) / med['input']
    return dict(frames_per_call=Fc, calls=a.calls, dense_batch=a.batch, autotune=False, disp_fill_ratio_frame0=fill,
                pairs_per_s={k: dict(median=round(med[k], 1), min=round(min(v), 1), max=round(max(v), 1),
                                     runs=[round(x, 1) for x in v]) for k, v in rates.items()},
                chunk_ms_input=round(chunk_ms, 3), launch_share_of_chunk=round(share, 5),
                input_leg_spread=round(spread, 5), margin=round(spread + share, 5), gap_fused_below_input=round(gap, 5),
                within_margin=bool(gap <= spread + share))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=4)
    ap.add_argument('--frames-per-call', type=int, default=32)
    ap.add_argument('--no-test-step', dest='test_step', action='store_false')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'disp_fuse_bench.json'))
    a = ap.parse_args()
    import stereotracking_amd  # noqa: F401  (before the first torch.cuda call: the package sets up the HIP runtime's queues)
    if not torch.cuda.is_available():
        raise SystemExit('disp_fuse_bench needs a GPU: nothing here is measured on a CPU')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    p = torch.cuda.get_device_properties(0)
    res = dict(device=f'{p.name} ({getattr(p, "gcnArchName", "?")}, {p.multi_processor_count} CUs)',
               peaks=dict(hbm_tbs=PEAK_HBM / 1e12), launch=bench_launch(a, dev))
    if a.test_step:
        res['test_step'] = bench_test_step(a, dev, res['launch']['mode2_fused']['ms']['median'])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
