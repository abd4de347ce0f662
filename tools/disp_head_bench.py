#!/usr/bin/env python
"""The disparity-completion head (DispHeadV2, csrc/disp_head.hip) at the product size, 8 x 736 x 1280, on one MI355X.
Writes profiles/disp_head_bench.json (or --out):

  launches   per launch of st_disp_head_forward: median ms over --reps timed forwards (hipEvents around every launch);
             for the five convolutions the direct-convolution FLOPs and their share of the fp32 MFMA roof (157.3 TFLOP/s;
             a Winograd launch executes fewer multiplies than that count, so its share can exceed a direct kernel's);
             for the other kernels the bytes they must move (computed from the shapes) and their share of 8 TB/s
  head_ms    the whole forward (events around the call), and the rescale to 720 x 1280
  eager      the same modules (tests/disp_head_ref.py: torch.nn Conv2d / BatchNorm2d / ELU / Linear / interpolate) in eager
             torch on the same card, same weights and inputs - record only, no claim rests on it
  test_step  frame-pairs/s of model.test_steps with the disparity-completion config against the plain disparity config
             (64 frames per call, dense batch 8), alternating, median of --repeats

Random seeded weights and inputs: the head's speed does not depend on the values, its accuracy on trained weights is not
measured here (the reference publishes no weights for this family)."""
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

PEAK_FP32_MFMA = 157.3e12
PEAK_HBM = 8.0e12
CFG_DIR = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort')


def launch_costs(N, h, w, cin, C):
    """name -> dict(flops=...) for the convolutions (2 x MACs of the direct convolution), dict(bytes=...) for the
    bandwidth kernels (every float they must read and write, once)."""
    p8, p4, p2 = N * h * w, 4 * N * h * w, 16 * N * h * w
    conv = lambda px, ci, co: dict(flops=2.0 * px * 9 * ci * co)
    return {
        'dconv1_1': conv(p8, cin, C), 'dconv1_2': conv(p8, C, C), 'dconv2_1': conv(p4, C + 64, 256),
        'dconv2_2': conv(p4, 256, 256), 'dconv3_1': conv(p2, 256, 128),
        'elu_inplace(dconv1_1)': dict(bytes=4.0 * 2 * p8 * C),
        'elu_up2(dconv1_2)': dict(bytes=4.0 * (p8 * C + p4 * C)),
        'gate_pool': dict(bytes=4.0 * p4 * 64),
        'gate_mlp': dict(bytes=0.0),
        'gate_apply': dict(bytes=4.0 * 2 * p4 * 64),
        'elu_inplace(dconv2_1)': dict(bytes=4.0 * 2 * p4 * 256),
        'elu_up2(dconv2_2)': dict(bytes=4.0 * (p4 * 256 + p2 * 256)),
        'elu_reg_relu': dict(bytes=4.0 * (p2 * 128 + 2 * p2)),
    }


def bench_head(a, dev):
    import disp_head_ref as ref
    from stereotracking_amd.engine import HipDispHead
    N, H, W, cin, C = a.batch, 736, 1280, 128, a.channels
    h, w = H // 8, W // 8
    sd = ref.random_state_dict(cin, C, seed=1)
    sd['reg.conv.bias'] = torch.tensor([0.3])
    g = torch.Generator().manual_seed(0)
    p3 = torch.randn(N, h, w, cin, generator=g).to(dev)
    df = (torch.randn(N, 2 * h, 2 * w, 64, generator=g) * 1.5 + 0.2).to(dev)
    head = HipDispHead(N, h, w, cin, C)
    head.load_state_dict(sd)
    out = torch.empty(N, 1, 4 * h, 4 * w, device=dev)
    for _ in range(3):
        head.forward_views(p3, df, out)
    torch.cuda.synchronize()
    # whole forward, untimed launches
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    whole = []
    for _ in range(a.reps):
        e0.record()
        head.forward_views(p3, df, out)
        e1.record()
        e1.synchronize()
        whole.append(e0.elapsed_time(e1))
    full = torch.empty(N, 1, 720, 1280, device=dev)
    rs = []
    for _ in range(a.reps):
        e0.record()
        head.resize(out, (720, 1280), full)
        e1.record()
        e1.synchronize()
        rs.append(e0.elapsed_time(e1))
    head.set_timing(True)
    per = {}
    for _ in range(a.reps):
        head.forward_views(p3, df, out)
        for name, ms in head.launch_times():
            per.setdefault(name, []).append(ms)
    head.set_timing(False)
    costs = launch_costs(N, h, w, cin, C)
    launches = []
    for name, vals in per.items():
        ms = statistics.median(vals)
        row = dict(name=name, ms=round(ms, 4), ms_min=round(min(vals), 4), ms_max=round(max(vals), 4))
        c = costs[name]
        if 'flops' in c:
            row['gflop_direct'] = round(c['flops'] / 1e9, 2)
            row['share_of_fp32_mfma_roof'] = round(c['flops'] / (ms * 1e-3) / PEAK_FP32_MFMA, 4)
        else:
            row['mbytes'] = round(c['bytes'] / 1e6, 2)
            row['share_of_8TBs'] = round(c['bytes'] / (ms * 1e-3) / PEAK_HBM, 4) if c['bytes'] else None
        launches.append(row)
        print(row, flush=True)
    res = dict(shape=dict(batch=N, height=H, width=W, in_channels=cin, channels=C),
               workspace_gb=round(head.workspace_bytes() / 1e9, 3),
               head_ms=dict(median=round(statistics.median(whole), 3), min=round(min(whole), 3), max=round(max(whole), 3)),
               resize_to_720x1280_ms=dict(median=round(statistics.median(rs), 4), mbytes=round(4.0 * N * (h * w * 16 + 720 * 1280) / 1e6, 2)),
               sum_of_launches_ms=round(sum(r['ms'] for r in launches), 3),
               gflop_direct_per_frame=round(sum(c['flops'] for c in costs.values() if 'flops' in c) / N / 1e9, 2),
               launches=launches)
    print('head', res['head_ms'], flush=True)
    if a.eager:
        m = ref.RefDispHead(cin, C)
        m.load_state_dict(sd, strict=False)
        m = m.to(dev)
        x, d = p3.permute(0, 3, 1, 2).contiguous(), df.permute(0, 3, 1, 2).contiguous()
        with torch.no_grad():
            for _ in range(2):
                y = m(x, d)['pred']
            torch.cuda.synchronize()
            ev = []
            for _ in range(max(3, a.reps // 2)):
                e0.record()
                y = m(x, d)['pred']
                e1.record()
                e1.synchronize()
                ev.append(e0.elapsed_time(e1))
        res['eager'] = dict(ms_median=round(statistics.median(ev), 3), ms_min=round(min(ev), 3),
                            max_abs_diff_to_hip=float((y - out).abs().max()), note='record only')
        print('eager', res['eager'], flush=True)
        del m, x, d, y
    del head, p3, df, out
    torch.cuda.empty_cache()
    return res


def bench_test_step(a, dev):
    import disp_head_ref as ref
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.structures import TrackDataSample
    from stereotracking_amd.synthetic import synthetic_batch, synthetic_state_dict
    F, ori = a.frames_per_call, (720, 1280)
    fr = synthetic_batch(list(range(8)), ori[0], ori[1], 192)
    imgs = [fr['img'][i % 8:i % 8 + 1, :, :ori[0]].to(torch.uint8).to(dev) for i in range(F)]
    disps = [fr['disp_postp'][i % 8:i % 8 + 1, :, :ori[0]].contiguous().to(dev) for i in range(F)]
    models = {}
    for name, path in (('disp', 'yolox_s_mmyolo_mot_airdrone_disp.py'),
                       ('disp_completion_v2', 'yolox_s_mmyolo_mot_airdrone_disp_completion_v2.py')):
        cfg = Config.fromfile(os.path.join(CFG_DIR, path))
        if name != 'disp':
            cfg.model.detector.disparity_head['channels'] = a.channels
        model = MODELS.build(dict(cfg.model, dense_batch=a.batch))
        sd = synthetic_state_dict(list(model.detector._table), seed=0)
        if name != 'disp':
            hs = ref.random_state_dict(128, a.channels, seed=1)
            hs['reg.conv.bias'] = torch.tensor([0.3])
            sd.update({'disp_head.' + k: v for k, v in hs.items()})
        model.detector.load_state_dict(sd, strict=False)
        models[name] = model

    def calls(n, t0):
        for c in range(n):
            samples = [TrackDataSample(dict(frame_id=t0 + c * F + t, ori_shape=ori, img_shape=ori, scale_factor=(1.0, 1.0)))
                       for t in range(F)]
            yield dict(inputs=dict(img=imgs, disp_postp=disps), data_samples=samples)

    rates = {k: [] for k in models}
    for k, m in models.items():           # warm: plans, tuning, buffers
        for _ in m.test_steps(calls(2, 0)):
            pass
        torch.cuda.synchronize()
    for r in range(a.repeats):
        for k, m in models.items():
            t0 = time.perf_counter()
            n = 0
            for outs in m.test_steps(calls(a.calls, 1000 * (r + 1))):
                n += len(outs)
            torch.cuda.synchronize()
            rates[k].append(n / (time.perf_counter() - t0))
            print(k, round(rates[k][-1], 1), flush=True)
    return dict(frames_per_call=F, calls=a.calls, dense_batch=a.batch,
                pairs_per_s={k: dict(median=round(statistics.median(v), 1), runs=[round(x, 1) for x in v]) for k, v in rates.items()},
                tuning={k: [getattr(p, 'tuning_source', None) for ent in m._dense.values() for p in ent[0].pipes[:1]]
                        for k, m in models.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=4)
    ap.add_argument('--frames-per-call', type=int, default=64)
    ap.add_argument('--no-eager', dest='eager', action='store_false')
    ap.add_argument('--no-test-step', dest='test_step', action='store_false')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'disp_head_bench.json'))
    a = ap.parse_args()
    import stereotracking_amd  # noqa: F401  (before the first torch.cuda call: the package sets up the HIP runtime's queues)
    if not torch.cuda.is_available():
        raise SystemExit('disp_head_bench needs a GPU: nothing here is measured on a CPU')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    p = torch.cuda.get_device_properties(0)
    res = dict(device=f'{p.name} ({getattr(p, "gcnArchName", "?")}, {p.multi_processor_count} CUs)',
               peaks=dict(fp32_mfma_tflops=PEAK_FP32_MFMA / 1e12, hbm_tbs=PEAK_HBM / 1e12), head=bench_head(a, dev))
    if a.test_step:
        res['test_step'] = bench_test_step(a, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
