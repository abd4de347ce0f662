#!/usr/bin/env python
"""ecc_bench.py - cost of the tracker's ECC camera-motion compensation (csrc/cmc_ecc.hip) on MI355X.

Prints ONE JSON line with
  * chunk: per downscale 1 / 2 / 4, the device-event time of the CMC work of one 8-frame chunk at 1280 x 720 (grey
    planes of the 8 frames + the 8 speculative ECC warps: what the MOT shell enqueues per chunk on its CMC stream),
    median of --reps, alone; the iterations the pairs ran; and the time per iteration, from the same chunk with
    stop_eps = 0 (every one of the 50 rounds then iterates).  The frames are a band-limited texture panned by
    (3, -2) px per frame, so the pairs converge as camera pans do; noise frames would fail in the first rounds.
  * numpy_ref_s: the numpy restatement (tests/ecc_ref.py, fp32 arithmetic) on ONE pair of the same frames at downscale 2,
    as a record of what the estimate costs on the CPU.
  * test_step: stereo frame-pairs/s of model.test_step at --frames frames per call (the bench.py test_step leg's model)
    with CMC off, Mesh-Affine and ECC, alternated in one process on the same box, --repeats times each.

  python tools/ecc_bench.py [--frames 64] [--repeats 3] [--reps 20] [--out profiles/ecc_bench.json]
  rocprofv3 --kernel-trace --stats -d DIR -o ecc -- python tools/ecc_bench.py --chunk-only   # per-kernel times
"""
import argparse
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


def panned_frames(n, h=720, w=1280, step=(3, -2), seed=0, cutoff=0.02):
    """n uint8 (1, 3, h, w) BGR frames: one periodic band-limited texture, rolled by `step` px per frame."""
    rng = np.random.default_rng(seed)
    F = np.fft.fft2(rng.standard_normal((h, w)))
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    t = np.real(np.fft.ifft2(F * np.exp(-(fx * fx + fy * fy) / (2 * cutoff * cutoff))))
    g = np.rint((t - t.min()) / (t.max() - t.min()) * 255).astype(np.uint8)
    out = []
    for i in range(n):
        r = np.roll(g, (i * step[1], i * step[0]), (0, 1))
        out.append(torch.from_numpy(np.stack([r, r, r])[None].copy()))
    return out


def chunk_cost(dev, reps, frames, downscale, h=720, w=1280):
    from stereotracking_amd import cmc
    B = len(frames) - 1
    fr = [f.to(dev) for f in frames]
    shape = cmc.ecc_plane_shape(h, w, downscale)
    planes = torch.empty(B + 1, *shape, device=dev)
    cmc.ecc_front(fr[:1], h, w, downscale, out=planes[:1])
    ws = cmc.ecc_workspace(B, shape, dev)
    res = {}
    for name, prm in (('chunk_ms', dict(downscale=downscale)), ('all_rounds_ms', dict(downscale=downscale, stop_eps=0.0))):
        def once():
            cmc.ecc_front(fr[1:], h, w, downscale, out=planes[1:])
            return cmc.ecc_estimate(planes[:-1], planes[1:], h, w, prm, with_iters=True, ws=ws)
        for _ in range(3):
            warps, iters = once()
        torch.cuda.synchronize()
        t = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            once()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b))
        res[name] = dict(median=round(statistics.median(t), 4), min=round(min(t), 4), max=round(max(t), 4), reps=reps)
        if name == 'chunk_ms':
            res['iterations'] = iters.cpu().tolist()
            res['valid'] = int(warps[:, 0].sum().item())
            res['shift_px'] = [round(float(v), 3) for v in warps[0, [4, 7]].cpu()]
        else:
            n = int(iters.max().item())
            res['per_iteration_ms'] = round(statistics.median(t) / n, 4)
    res['plane'] = list(shape)
    return res


def numpy_reference_s(frames, downscale=2, h=720, w=1280):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import ecc_ref as E
    T, I = (E.front(f[0].numpy(), h, w, downscale) for f in frames[:2])
    t0 = time.perf_counter()
    valid, rho, M, it = E.estimate(T, I, E.EUCLIDEAN, dt=np.float32)
    return dict(seconds=round(time.perf_counter() - t0, 3), iterations=it, valid=bool(valid), downscale=downscale,
                shift_px=[round(float(v), 3) for v in E.to_image(M, downscale)[:, 2]])


def build(dev, B, cmc_cfg):
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.synthetic import synthetic_state_dict
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort',
                                       'stereo_yolox_s_mot_airdrone_costvolume.py'))
    if cmc_cfg is not None:
        cfg.model.tracker['cmc'] = cmc_cfg
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
    frames = panned_frames(9)
    res = dict(metric='ecc_cost', chunk={f'downscale_{s}': chunk_cost(dev, args.reps, frames, s) for s in (1, 2, 4)})
    if not args.chunk_only:
        from stereotracking_amd.structures import TrackDataSample
        from stereotracking_amd.synthetic import synthetic_batch
        res['numpy_ref'] = numpy_reference_s(frames)
        res['frames_per_call'] = args.frames
        B, F = 8, args.frames
        bc = synthetic_batch(list(range(B)), 736, 1280, 192)
        left = [bc['img'][i % B:i % B + 1, :, :720].to(torch.uint8).to(dev) for i in range(F)]
        right = [bc['right'][i % B:i % B + 1, :, :720].to(torch.uint8).to(dev) for i in range(F)]
        kinds = dict(off=None, mesh_affine=dict(method='glme_affine'), ecc=dict(method='ecc'))
        models = {k: build(dev, B, c) for k, c in kinds.items()}
        frame = dict.fromkeys(kinds, 0)

        def call(k):
            samples = [TrackDataSample(dict(frame_id=frame[k] + i, ori_shape=(720, 1280), img_shape=(720, 1280),
                                            scale_factor=(1.0, 1.0))) for i in range(F)]
            frame[k] += F
            return models[k].test_step(dict(inputs=dict(img=left, right=right), data_samples=samples))
        for k in kinds:
            for _ in range(2):
                call(k)
        torch.cuda.synchronize()
        runs = {k: [] for k in kinds}
        for _ in range(args.repeats):
            for k in kinds:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    call(k)
                torch.cuda.synchronize()
                runs[k].append(args.calls * F / (time.perf_counter() - t0))
        med = {k: statistics.median(v) for k, v in runs.items()}
        res['test_step'] = dict({k: [round(v, 2) for v in r] for k, r in runs.items()}, unit='stereo frame-pairs/s',
                                ratio_mesh_affine=round(med['mesh_affine'] / med['off'], 4),
                                ratio_ecc=round(med['ecc'] / med['off'], 4))
    res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
