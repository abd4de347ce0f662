#!/usr/bin/env python
"""lrcheck_bench.py - cost of the stereo module's left-right check (csrc/lr_check.hip) on MI355X.  Record-only.

Prints ONE JSON line with
  * kernels: per volume size (8 x 184 x 320 x 48, the default module at the bench size, and 8 x 736 x 1280 x 192, the
    full-resolution mode), device-event time (median of --reps) of st_softargmin_right and st_lr_check_pack beside
    st_softargmin and st_disp_upsample_pack on the SAME volume / disparity, the bytes each reads or writes, and
    `right_over_left` = median(st_softargmin_right) / median(st_softargmin): the right pass reads the bytes the left one
    reads, so the left soft-argmin is its yardstick;
  * test_step: frame-pairs/s of model.test_step at --frames frames per call, the StereoCostVolume config with the check
    (stereo_yolox_s_mot_airdrone_costvolume_lrcheck.py) against the one without, alternated in one process, --repeats
    times each; ratio = median(check on) / median(check off).  Same detector, seeded random weights.

  python tools/lrcheck_bench.py [--reps 20] [--frames 64] [--repeats 7] [--out profiles/lrcheck_bench.json]
  python tools/lrcheck_bench.py --kernels-only --sizes 8x184x320x48
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
CFG_DIR = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort')


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


def kernel_ms(dev, N, H, W, D, scale, reps, temperature=32.0, lr_max_diff=None):
    """The four kernels on one peaked random volume (N,H,W,D): what the module's last two steps cost with the check off
    (st_softargmin + st_disp_upsample_pack) and what the check adds / replaces."""
    from stereotracking_amd import _lib
    from stereotracking_amd._lib import check, current_stream, ptr
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(D + W)
    vol = torch.empty(N, H, W, D, device=dev)
    for n in range(N):     # image by image: the generator's temporaries stay small beside the 5.8 GB volume
        vol[n] = torch.rand(H, W, D, device=dev, generator=g) * 0.25
        peak = torch.randint(0, D, (H, W, 1), device=dev, generator=g)
        vol[n].scatter_(2, peak, 1.0)
    dl, dr = torch.empty(N, H, W, device=dev), torch.empty(N, H, W, device=dev)
    Ho, Wo = H * scale, W * scale
    out = torch.empty(N, 3, Ho, Wo, device=dev)
    mask = torch.empty(N, 1, Ho, Wo, device=dev)
    md = float(scale) if lr_max_diff is None else float(lr_max_diff)     # one level
    st = current_stream()

    def left():
        check(lib.st_softargmin(ptr(vol), N, H, W, D, temperature, ptr(dl), st), 'st_softargmin')

    def right():
        check(lib.st_softargmin_right(ptr(vol), N, H, W, D, temperature, ptr(dr), st), 'st_softargmin_right')

    def pack():
        check(lib.st_disp_upsample_pack(ptr(dl), N, H, W, scale, Ho, Wo, Ho, Wo, ptr(out), st), 'st_disp_upsample_pack')

    def lr_pack():
        check(lib.st_lr_check_pack(ptr(dl), ptr(dr), N, H, W, scale, Ho, Wo, Ho, Wo, md, ptr(out), ptr(mask), st),
              'st_lr_check_pack')
    left()
    right()
    res = dict(volume=[N, H, W, D], scale=scale, lr_max_diff=md, volume_bytes=vol.numel() * 4,
               st_softargmin=_timed(left, reps), st_softargmin_right=_timed(right, reps),
               st_disp_upsample_pack=_timed(pack, reps), st_lr_check_pack=_timed(lr_pack, reps))
    torch.cuda.synchronize()
    res['right_over_left'] = round(res['st_softargmin_right']['median'] / res['st_softargmin']['median'], 3)
    res['pack_over_pack'] = round(res['st_lr_check_pack']['median'] / res['st_disp_upsample_pack']['median'], 3)
    res['left_read_GBps'] = round(res['volume_bytes'] / res['st_softargmin']['median'] / 1e6, 1)
    # the right pass sweeps the volume twice (maximum, then sums) and re-fetches 15 of every 143 columns
    res['right_read_GBps_two_sweeps'] = round(2 * res['volume_bytes'] / res['st_softargmin_right']['median'] / 1e6, 1)
    res['pack_write_bytes'] = out.numel() * 4
    res['lr_pack_write_bytes'] = (out.numel() + mask.numel()) * 4
    res['valid_fraction'] = round(float(mask.mean()), 4)
    del vol
    torch.cuda.empty_cache()
    return res


def build(check_on, B, max_det):
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.synthetic import synthetic_state_dict
    name = 'stereo_yolox_s_mot_airdrone_costvolume_lrcheck.py' if check_on else 'stereo_yolox_s_mot_airdrone_costvolume.py'
    cfg = Config.fromfile(os.path.join(CFG_DIR, name))
    model = MODELS.build(dict(cfg.model, dense_batch=B, inflight=3, max_det=max_det,
                              tuning_cache=os.environ.get('ST_TUNE_CACHE')))
    assert model.stereo.lr_check == check_on
    table = list(model.detector._table) + [('stereo.' + n, shp) for n, shp in model.stereo.param_table()]
    sd = synthetic_state_dict(table, seed=0)
    model.detector.load_state_dict(sd, strict=False)
    model.stereo.load_state_dict({k[len('stereo.'):]: v for k, v in sd.items() if k.startswith('stereo.')})
    return model


def test_step_rate(dev, args):
    from stereotracking_amd.structures import TrackDataSample
    from stereotracking_amd.synthetic import synthetic_stereo_pair
    h, w, B, F = 720, 1280, 8, args.frames
    fr = [synthetic_stereo_pair(i, h, w, max_disp=192) for i in range(B)]
    left = [torch.from_numpy(fr[i % B]['left']).to(dev)[None] for i in range(F)]
    right = [torch.from_numpy(fr[i % B]['right']).to(dev)[None] for i in range(F)]
    models = {False: build(False, B, args.max_det), True: build(True, B, args.max_det)}
    frame = {False: 0, True: 0}

    def call(on):
        samples = [TrackDataSample(dict(frame_id=frame[on] + i, ori_shape=(h, w), img_shape=(h, w),
                                        scale_factor=(1.0, 1.0))) for i in range(F)]
        frame[on] += F
        return models[on].test_step(dict(inputs=dict(img=left, right=right), data_samples=samples))
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
    # what the host side of test_step (the tracker) had to chew: the random head reacts to the holes in the disparity
    dets = {k: round(statistics.mean(len(o.pred_det_instances) for o in call(k)), 1) for k in (False, True)}
    trks = {k: round(statistics.mean(len(o.pred_track_instances) for o in call(k)), 1) for k in (False, True)}
    return dict(frames_per_call=F, max_det=args.max_det, size=[h, w], check_off=[round(v, 2) for v in runs[False]],
                check_on=[round(v, 2) for v in runs[True]], unit='frame-pairs/s', ratio=round(on / off, 4),
                detections_per_frame=dict(check_off=dets[False], check_on=dets[True]),
                tracks_per_frame=dict(check_off=trks[False], check_on=trks[True]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='8x184x320x48:4;8x736x1280x192:1',
                    help="'NxHxWxD:scale;...': the volumes (scale = level spacing in pixels: 4 default module, 1 full_res)")
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--calls', type=int, default=4, help='test_step calls per timed repeat')
    ap.add_argument('--max-det', type=int, default=4000,
                    help='rows of the detection buffer of both test_step models (a capacity; overflow raises - the seeded '
                         'random head keeps about 1100 boxes per frame on the module\'s disparity)')
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(metric='lrcheck_cost', kernels=[])
    for part in args.sizes.split(';'):
        shape, scale = part.split(':')
        N, H, W, D = (int(v) for v in shape.lower().split('x'))
        res['kernels'].append(kernel_ms(dev, N, H, W, D, int(scale), args.reps))
        k = res['kernels'][-1]
        print(f"{shape}: left {k['st_softargmin']['median']} ms, right {k['st_softargmin_right']['median']} ms "
              f"(x{k['right_over_left']}), pack {k['st_disp_upsample_pack']['median']} ms, lr pack "
              f"{k['st_lr_check_pack']['median']} ms", file=sys.stderr, flush=True)
    if not args.kernels_only:
        res['test_step'] = test_step_rate(dev, args)
    res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
