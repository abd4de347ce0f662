#!/usr/bin/env python
"""The annotated-frame writer (stereotracking_amd/jpeg_write.py, visualization.py) at the product size on
one MI355X.  Record only - nothing is asserted; writes profiles/jpeg_write_bench.json (or --out).

Input: 32 frames of 1280 x 720 (the synthetic frames of synthetic.py, --distinct different ones, repeated), quality 90,
4:2:0, 16 boxes per frame for the overlay.

  forward      st_jpeg_forward, device ms (hipEvents around the call), median / min / max; the bytes it must move
               (pixels in, coefficients out) and the fraction of 8 TB/s
  draw         st_draw_tracks on the same frames, likewise (bytes: the painted pixels read and written are few - set
               against the frames' bytes once, the kernel's upper bound, and against the pixels the boxes cover)
  d2h          the one non-blocking copy of the quantised coefficients into page-locked memory, device ms and GB/s
  entropy      host entropy encode (st_jpeg_entropy_encode out of page-locked memory), ms per frame on 1 / 4 / 16 threads
  encode       the whole JpegEncoder.encode call on --threads pool threads, host clock, ms per batch and frames/s
  host         encode_jpeg_host on one thread, ms per frame; Pillow's save of the same pixels if Pillow is installed
"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM = 8.0e12
H, W, N = 720, 1280, 32


def stats(ms):
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4), reps=len(ms))


def device_ms(fn, reps):
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
    return stats(ms)


def host_ms(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def boxes_for(n, k, seed=0):
    rng = np.random.default_rng(seed)
    from stereotracking_amd import visualization as vis
    per_frame = []
    for _ in range(n):
        frame = []
        for j in range(k):
            x1, y1 = rng.uniform(0, W - 80), rng.uniform(0, H - 80)
            w, h = rng.uniform(20, 260), rng.uniform(20, 200)
            frame.append(((x1, y1, x1 + w, y1 + h), vis.random_color(j)[::-1], f'{j} | {rng.uniform(0.3, 1):.2f}'))
        per_frame.append(frame)
    return per_frame


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_write_bench.json'))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--distinct', type=int, default=4)
    ap.add_argument('--threads', type=int, default=4)
    ap.add_argument('--boxes', type=int, default=16)
    a = ap.parse_args()
    from concurrent.futures import ThreadPoolExecutor
    from stereotracking_amd import jpeg_write as jw, visualization as vis
    from stereotracking_amd.synthetic import synthetic_batch
    dev = torch.device('cuda:0')
    fr = synthetic_batch(list(range(a.distinct)), H, W, 192)
    distinct = fr['img'][:, :, :H].to(torch.uint8)                                    # (distinct, 3, H, W) BGR
    frames = torch.cat([distinct[i % a.distinct:i % a.distinct + 1] for i in range(N)]).contiguous().to(dev)
    info = jw.encode_geometry(H, W, 3, '420')
    count = int(info.coef_count)
    quant = jw.quant_tables(90)
    qd = torch.from_numpy(quant.view(np.int16)).to(dev)
    coef = torch.empty((N, count), dtype=torch.int16, device=dev)
    res = dict(device=torch.cuda.get_device_name(0), frames=N, height=H, width=W, quality=90, subsampling='420',
               boxes_per_frame=a.boxes, coef_bytes_per_frame=count * 2)

    t = device_ms(lambda: jw.forward_device(frames, qd, info, coef, 'bgr'), a.reps)
    moved = N * (3 * H * W + count * 2)
    res['forward'] = dict(ms=t, bytes=moved, fraction_of_8TBs=round(moved / (t['median'] * 1e-3) / PEAK_HBM, 4))
    print('forward', res['forward'], flush=True)

    per_frame = boxes_for(N, a.boxes)
    packed, counts = vis.pack_boxes(per_frame)
    blob = torch.from_numpy(np.concatenate([counts.view(np.uint8), packed.reshape(-1).view(np.uint8)])).to(dev)
    canvas = frames.clone()
    lib = vis._api()

    def draw():
        rc = lib.st_draw_tracks(canvas.data_ptr(), N, H, W, canvas.stride(0), canvas.stride(1), canvas.stride(2),
                                blob.data_ptr() + counts.nbytes, blob.data_ptr(), a.boxes, 3, 205,
                                torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.st_last_error()
    t = device_ms(draw, a.reps)
    covered = int((canvas != frames).any(1).sum())
    res['draw'] = dict(ms=t, frame_bytes=N * 3 * H * W, painted_pixels=covered, painted_bytes_read_and_written=covered * 6,
                       fraction_of_8TBs_frames_once=round(N * 3 * H * W / (t['median'] * 1e-3) / PEAK_HBM, 4),
                       fraction_of_8TBs_painted=round(covered * 6 / (t['median'] * 1e-3) / PEAK_HBM, 6))
    print('draw', res['draw'], flush=True)

    pin = torch.empty(N * count, dtype=torch.int16).pin_memory()
    flat = coef.view(-1)
    t = device_ms(lambda: pin.copy_(flat, non_blocking=True), a.reps)
    res['d2h'] = dict(ms=t, bytes=N * count * 2, gb_per_s=round(N * count * 2 / (t['median'] * 1e-3) / 1e9, 2))
    print('d2h', res['d2h'], flush=True)

    torch.cuda.synchronize()
    host_coef = pin.numpy().reshape(N, count)
    bound = int(jw._api().st_jpeg_encode_bound(C.byref(info)))
    res['entropy_ms_per_frame'] = {}
    for threads in (1, 4, 16):
        bufs = [np.empty(bound, np.uint8) for _ in range(N)]
        with ThreadPoolExecutor(max_workers=threads) as pool:
            t = host_ms(lambda: list(pool.map(lambda i: jw.entropy_encode(host_coef[i], quant, info, bufs[i]), range(N))), a.reps)
        res['entropy_ms_per_frame'][str(threads)] = {k: (round(v / N, 4) if k != 'reps' else v) for k, v in t.items()}
    print('entropy', res['entropy_ms_per_frame'], flush=True)

    enc = jw.JpegEncoder(dev, threads=a.threads, quality=90, subsampling='420')
    blobs = enc.encode(frames)
    res['file_bytes'] = [len(b) for b in blobs[:a.distinct]]

    def whole():
        enc.encode(frames)
        torch.cuda.synchronize()
    t = host_ms(whole, a.reps)
    res['encode'] = dict(threads=a.threads, ms=t, frames_per_s=round(N / (t['median'] * 1e-3), 1))
    enc.close()
    print('encode', res['encode'], flush=True)

    rgb = np.ascontiguousarray(distinct[0].numpy()[::-1].transpose(1, 2, 0))
    res['encode_jpeg_host_ms_per_frame_1_thread'] = host_ms(lambda: jw.encode_jpeg_host(rgb, 90, '420'), max(3, a.reps // 4))
    try:
        from PIL import Image
        im = Image.fromarray(rgb, 'RGB')
        res['pillow_ms_per_frame_1_thread'] = host_ms(lambda: im.save(io.BytesIO(), 'JPEG', quality=90, subsampling=2, optimize=False),
                                                      max(3, a.reps // 4))
        buf = io.BytesIO()
        im.save(buf, 'JPEG', quality=90, subsampling=2, optimize=False)
        res['bytes_equal_pillow'] = buf.getvalue() == jw.encode_jpeg_host(rgb, 90, '420')
    except ImportError:
        res['pillow_ms_per_frame_1_thread'] = 'Pillow is not installed on this machine'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
