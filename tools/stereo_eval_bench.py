#!/usr/bin/env python
"""stereo_eval_bench.py - cost of the dense stereo evaluator (csrc/stereo_eval.hip) on MI355X, and the first accuracy
record of the stereo modules (on SYNTHETIC pairs with known truth).

Prints ONE JSON line (and writes it to --out) with
  * launch: device-event time of one stereo_eval launch (hist memset + the two kernels + the allocation of its buffers)
    over --pairs pairs at 1280 x 720 (padded 736 x 1280), with and without --boxes boxes per frame: median, min, max of
    --reps windows of --inner launches each; the bytes the launch must read (the two maps inside the extent) and the
    fraction of the 8 TB/s HBM peak that time amounts to;
  * yardstick (recorded, not asserted): the same accumulators (counts, sums, histogram per cell; no boxes) written with
    torch ops on the same tensors;
  * test_step: frame-pairs/s of model.test_step on the SGBM config with stereo_eval on and off, the two models alternated
    in this process (autotune off in both; recorded, no threshold);
  * accuracy: EPE, bad_1, bad_3, D1, density, A90 of StereoSGBM at 48 / 128 / 192 levels and of StereoCostVolume with
    and without lr_check on synthetic_stereo_pair truth.  The cost volume runs on SYNTHETIC (untrained) weights: its
    row records that the evaluator works on it, not what a trained module reaches.

  python tools/stereo_eval_bench.py [--pairs 8] [--frames 32] [--repeats 3] [--out profiles/stereo_eval_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CFG_DIR = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort')
HBM_PEAK = 8e12
H, W = 720, 1280
KEYS = ('EPE', 'bad_1', 'bad_3', 'D1', 'density', 'A90')


def _timed(fn, reps, inner):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) / inner)
    return dict(median=round(statistics.median(t), 4), min=round(min(t), 4), max=round(max(t), 4), reps=reps, inner=inner)


def maps(dev, pairs, seed=0):
    """Seeded disparity / depth maps of the padded size: depths 2..100 m, errors of a few pixels, 4 % holes each."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    z = torch.rand(pairs, 1, Hp, Wp, generator=g) * 98 + 2
    pred = (160.0 / z + torch.randn(pairs, 1, Hp, Wp, generator=g) * 1.5).repeat(1, 3, 1, 1)
    pred[torch.rand(pairs, 3, Hp, Wp, generator=g) < 0.04] = 0
    z[torch.rand(pairs, 1, Hp, Wp, generator=g) < 0.04] = 0
    return pred.to(dev), z.to(dev)


def torch_accumulate(pred, gt, bf, edges, taus):
    """The accumulators with torch ops (region 0 only): the yardstick."""
    N = pred.shape[0]
    p, g = pred[:, 0, :H, :W], gt[:, 0, :H, :W]
    K, T = len(edges) - 1, len(taus)
    gz, gd = g, bf / g
    gt_valid = torch.isfinite(g) & (g > 0) & (gz > edges[0]) & (gz <= edges[-1])
    b = sum((gz > e).long() for e in edges[1:-1]) if K > 1 else torch.zeros_like(g, dtype=torch.long)
    both = gt_valid & torch.isfinite(p) & (p > 0)
    pz, e = bf / p, (p - gd).abs()
    r = torch.maximum(pz / gz, gz / pz)
    flags = [gt_valid, both] + [both & (e > t) for t in taus] + [both & (e > 3) & (e > 0.05 * gd)] + \
        [both & (r < c) for c in (1.25, 1.5625, 1.953125)]
    cell = (torch.arange(N, device=p.device)[:, None, None] * K + b).reshape(-1)
    counts = torch.stack([torch.bincount(cell, weights=f.reshape(-1).double(), minlength=N * K) for f in flags], -1)
    ed, dz = e.double(), pz.double() - gz.double()
    bw = both.reshape(-1).double()
    terms = [ed, ed * ed, dz.abs() / gz.double(), dz * dz / gz.double(), dz * dz]
    sums = torch.stack([torch.bincount(cell, weights=torch.nan_to_num(t.reshape(-1)) * bw, minlength=N * K) for t in terms], -1)
    hb = torch.clamp(torch.nan_to_num(e * 16, posinf=511.0), max=511).long().reshape(-1)
    hist = torch.bincount((cell * 512 + hb)[both.reshape(-1)], minlength=N * K * 512)
    return counts, sums, hist


def launch_cost(dev, args):
    from stereotracking_amd import stereo_eval as S
    pred, gt = maps(dev, args.pairs)
    edges, taus = S.check_options()
    ext = torch.tensor([(H, W)] * args.pairs, dtype=torch.int32, device=dev)
    rng = np.random.RandomState(0)
    xy = rng.uniform(0, [W - 200, H - 200], (args.pairs, args.boxes, 2))
    wh = rng.uniform(20, 200, (args.pairs, args.boxes, 2))
    boxes = torch.from_numpy(np.concatenate([xy, xy + wh], -1).astype(np.float32)).to(dev)
    cnt = torch.full((args.pairs,), args.boxes, dtype=torch.int32, device=dev)
    res = dict(pairs=args.pairs, size=[H, W], padded=list(pred.shape[-2:]), boxes=args.boxes)
    res['no_boxes_ms'] = _timed(lambda: S.launch_stereo_eval(pred, gt, 'depth', 160.0, ext, None, None, edges, taus),
                                args.reps, args.inner)
    res['with_boxes_ms'] = _timed(lambda: S.launch_stereo_eval(pred, gt, 'depth', 160.0, ext, boxes, cnt, edges, taus),
                                  args.reps, args.inner)
    read = 2 * args.pairs * H * W * 4
    res['bytes_read'] = read
    for k in ('no_boxes', 'with_boxes'):
        res[k + '_fraction_of_8TBps'] = round(read / (res[k + '_ms']['median'] * 1e-3) / HBM_PEAK, 4)
    res['torch_ops_ms'] = _timed(lambda: torch_accumulate(pred, gt, 160.0, edges, taus), max(3, args.reps // 4), 1)
    st = S.stereo_error_stats(pred, gt, extent=[(H, W)] * args.pairs)
    c, s, h = torch_accumulate(pred, gt, 160.0, edges, taus)
    res['torch_ops_agree'] = dict(counts=bool(np.array_equal(st.counts[:, 0], c.reshape(args.pairs, 3, -1).long().cpu().numpy())),
                                  hist=bool(np.array_equal(st.hist[:, 0], h.reshape(args.pairs, 3, 512).cpu().numpy())))
    res['summary'] = {k: round(st.summary()[k], 5) for k in KEYS}
    return res


def build(stereo_eval, B):
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.synthetic import synthetic_state_dict
    cfg = Config.fromfile(os.path.join(CFG_DIR, 'stereo_yolox_s_mot_airdrone_sgbm.py'))
    extra = dict(stereo_eval=stereo_eval) if stereo_eval is not None else {}
    model = MODELS.build(dict(cfg.model, dense_batch=B, inflight=3, autotune=False, **extra))
    model.detector.load_state_dict(synthetic_state_dict(list(model.detector._table), seed=0), strict=False)
    return model


def test_step_rate(dev, args):
    from stereotracking_amd.structures import InstanceData, TrackDataSample
    from stereotracking_amd.synthetic import synthetic_stereo_pair
    B, F = args.pairs, args.frames
    fr = [synthetic_stereo_pair(i, H, W, max_disp=48) for i in range(B)]
    left = [torch.from_numpy(f['left'])[None].to(dev) for f in fr]
    right = [torch.from_numpy(f['right'])[None].to(dev) for f in fr]
    depth = [torch.from_numpy(np.where(f['disp'] > 0, 160.0 / np.maximum(f['disp'], 1), 0).astype(np.float32))[None, None].to(dev)
             for f in fr]
    inputs = dict(img=[left[i % B] for i in range(F)], right=[right[i % B] for i in range(F)],
                  depth_postp=[depth[i % B] for i in range(F)])
    gtb = torch.tensor([[100.0, 100, 300, 260], [600.0, 300, 760, 420]])
    models = {False: build(None, B), True: build(dict(boxes='gt'), B)}
    frame = {False: 0, True: 0}

    def call(on):
        samples = []
        for i in range(F):
            s = TrackDataSample(dict(frame_id=frame[on] + i, ori_shape=(H, W), img_shape=(H, W), scale_factor=(1.0, 1.0)))
            s.gt_instances = InstanceData(bboxes=gtb)
            samples.append(s)
        frame[on] += F
        return models[on].test_step(dict(inputs=inputs, data_samples=samples))
    for on in (False, True):
        for _ in range(2):
            out = call(on)
    torch.cuda.synchronize()
    assert 'stereo_stats' in out[0].metainfo
    runs = {False: [], True: []}
    for _ in range(args.repeats):
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call(on)
            torch.cuda.synchronize()
            runs[on].append(round(args.calls * F / (time.perf_counter() - t0), 2))
    return dict(config='stereo_yolox_s_mot_airdrone_sgbm.py', frames_per_call=F, dense_batch=B, autotune=False,
                unit='frame-pairs/s', stereo_eval_off=runs[False], stereo_eval_on=runs[True],
                ratio=round(statistics.median(runs[True]) / statistics.median(runs[False]), 4))


def accuracy(dev, args):
    """On synthetic_stereo_pair truth (piecewise-constant disparity, multiples of 4, in [4, 44]): gt_kind='disp'."""
    from stereotracking_amd import stereo_eval as S
    from stereotracking_amd.pipeline import StereoDensePipeline
    from stereotracking_amd.sgbm import StereoSGBM
    from stereotracking_amd.synthetic import synthetic_state_dict, synthetic_stereo_pair
    n = 4
    fr = [synthetic_stereo_pair(100 + i, H, W, max_disp=48, d_lo=4, d_hi=44) for i in range(n)]
    Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32

    def batch(key):
        out = torch.zeros(n, 3, Hp, Wp)
        out[:, :, :H, :W] = torch.from_numpy(np.stack([f[key] for f in fr])).float()
        return out.to(dev)
    left, right = batch('left'), batch('right')
    truth = torch.zeros(n, 1, Hp, Wp)
    truth[:, 0, :H, :W] = torch.from_numpy(np.stack([f['disp'] for f in fr]))
    truth = truth.to(dev)
    edges = (0, 5, 10, 20, 40)        # bf = 160: disparities 4 .. 44 px are depths 3.6 .. 40 m

    def score(disp):
        s = S.stereo_error_stats(disp, truth, gt_kind='disp', extent=[(H, W)] * n, depth_edges=edges).summary()
        return {k: round(s[k], 5) for k in KEYS}
    rows = {}
    for levels in (48, 128, 192):
        m = StereoSGBM(num_disparities=levels)
        rows[f'StereoSGBM_{levels}'] = score(m.compute(left, right, (H, W), torch.empty(n, 3, Hp, Wp, device=dev)))
    for lr in (False, True):
        pipe = StereoDensePipeline(n, (H, W), 0.375, 0.33, 1, stereo=True, max_disp=64, max_det=1000, lr_check=lr)
        pipe.load_state_dict(synthetic_state_dict(pipe.param_table(), seed=0), autotune=False)
        rows['StereoCostVolume_synthetic_weights' + ('_lr_check' if lr else '')] = score(pipe.disparity(left, right))
    return dict(data='synthetic_stereo_pair seeds 100..103, 1280 x 720, true disparity 4..44 px, gt_kind=disp', rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=8)
    ap.add_argument('--boxes', type=int, default=16)
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=2, help='test_step calls per timed repeat')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--inner', type=int, default=20, help='launches per timed window')
    ap.add_argument('--skip', default='', help='comma list of sections to leave out: launch, test_step, accuracy')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('stereo_eval_bench.py measures on the GPU; none is available')
    dev = torch.device('cuda:0')
    skip = set(filter(None, args.skip.split(',')))
    res = dict(metric='stereo_eval_cost', device=torch.cuda.get_device_name(0))
    for name, fn in (('launch', launch_cost), ('accuracy', accuracy), ('test_step', test_step_rate)):
        if name in skip:
            res[name] = 'not measured'
            continue
        res[name] = fn(dev, args)
        print(f'{name}: {json.dumps(res[name])}', file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
