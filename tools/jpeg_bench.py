#!/usr/bin/env python
"""The JPEG reader (stereotracking_amd/jpeg.py) at the product size on one MI355X.  Record only; writes
profiles/jpeg_bench.json (or --out).

Input: 8 and 32 frames of 1280 x 720, 4:2:0 and 4:4:4, quality 90, written by jpeg.write_jpeg's encoder from the
synthetic frames of synthetic.py (--distinct different frames, repeated).

  entropy      host entropy decode (st_jpeg_entropy_decode into page-locked memory), ms per frame on 1 / 4 / 16 threads
  h2d          the one non-blocking copy of the quantised coefficients, device ms and GB/s
  reconstruct  st_jpeg_reconstruct (both launches), device ms (hipEvents around the call), median / min / max; the bytes
               the two launches must move (A: coefficients in, component planes out; B: planes in, pixels out) and the
               fraction of 8 TB/s.  Each launch's own time, set against its own bytes, comes from profiler runs of their
               own, one per sampling and batch: `rocprofv3 --kernel-trace --stats -- python tools/jpeg_bench.py
               --launch-loop 200 --launch-sampling 420 --launch-batch 8`, merged with --kernel-stats 420:8=<csv>
  decode       the whole JpegDecoder.decode call on --threads and on 16 pool threads, host clock to a device synchronise,
               ms per batch and frames/s
  read_jpeg    the host path on one thread, ms per frame; Pillow's decode of the same bytes if Pillow is installed
  test_step    the RGB-only config fed by decode() of each call's bytes - entropy='host' and entropy='device', legs
               alternated - against the same frames already on the device
  entropy_device  JpegDecoder(entropy='device') against entropy='host' on 4:2:0, on the noisy synthetic frames and on the
               same frames without their pixel noise, legs alternated in this process: the entropy launches alone, the
               blob's H2D copy against the coefficient copy it replaces, decode() of 8 and 32 frames on --threads and 16
               pool threads, host CPU time per frame inside decode(), passes per tile, bytes the write pass moves.  Each
               entropy kernel's own time comes from a profiler run of its own: `rocprofv3 --kernel-trace --stats -- python
               tools/jpeg_bench.py --launch-loop 20 --launch-entropy device --launch-batch 32`, merged with
               --entropy-kernel-stats 32=<csv>.  --only-entropy-device measures this section and test_step only and keeps
               the rest of the existing file.
"""
import argparse
import csv
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
CFG = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone.py')
H, W = 720, 1280


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


def host_ms(fn, reps, sync=False):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def make_files(distinct, sampling):
    from stereotracking_amd import jpeg
    from stereotracking_amd.synthetic import synthetic_batch
    fr = synthetic_batch(list(range(distinct)), H, W, 192)
    frames = fr['img'][:, :, :H].to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    return [jpeg.encode_jpeg(f, 90, sampling) for f in frames], fr


def bench_sampling(a, dev, sampling, res):
    import ctypes as C
    from concurrent.futures import ThreadPoolExecutor
    from stereotracking_amd import jpeg
    files, _ = make_files(a.distinct, sampling)
    info = jpeg._info(files[0])
    count = int(info.coef_count)
    out = dict(file_bytes=[len(f) for f in files], coef_bytes_per_frame=count * 2)
    # host entropy decode, per frame, on 1 / 4 / 16 threads (32 frames in flight)
    datas = [files[i % len(files)] for i in range(32)]
    pin = torch.empty(32 * count, dtype=torch.int16).pin_memory().numpy().reshape(32, count)
    quant = np.empty((32, 3, 64), np.uint16)
    out['entropy_ms_per_frame'] = {}
    for threads in (1, 4, 16):
        with ThreadPoolExecutor(max_workers=threads) as pool:
            t = host_ms(lambda: list(pool.map(lambda i: jpeg.entropy_decode(datas[i], pin[i], quant[i]), range(32))), a.reps)
        out['entropy_ms_per_frame'][str(threads)] = {k: (round(v / 32, 4) if k != 'reps' else v) for k, v in t.items()}
    one = host_ms(lambda: jpeg.read_jpeg(files[0]), max(3, a.reps // 4))
    out['read_jpeg_ms_per_frame_1_thread'] = one
    try:
        import io
        from PIL import Image
        out['pillow_ms_per_frame_1_thread'] = host_ms(lambda: np.asarray(Image.open(io.BytesIO(files[0])).convert('RGB')),
                                                      max(3, a.reps // 4))
    except ImportError:
        out['pillow_ms_per_frame_1_thread'] = 'Pillow is not installed on this machine'
    lib = jpeg._api()
    planes = int(info.work_bytes)
    for n in (8, 32):
        host = torch.empty(n * count * 2 + n * 384, dtype=torch.uint8).pin_memory()
        hv = host.numpy()
        coef = hv[:n * count * 2].view(np.int16).reshape(n, count)
        q = hv[n * count * 2:].view(np.uint16).reshape(n, 3, 64)
        for i in range(n):
            jpeg.entropy_decode(datas[i], coef[i], q[i])
        devbuf = torch.empty_like(host, device=dev)
        work = torch.empty(int(lib.st_jpeg_work_bytes(C.byref(info), n)), dtype=torch.uint8, device=dev)
        frames = torch.empty((n, 3, H, W), dtype=torch.uint8, device=dev)
        t_copy = device_ms(lambda: devbuf.copy_(host, non_blocking=True), a.reps)

        def launch():
            rc = lib.st_jpeg_reconstruct(devbuf.data_ptr(), devbuf.data_ptr() + n * count * 2, n, C.byref(info),
                                         work.data_ptr(), work.numel(), frames.data_ptr(), frames.stride(0), frames.stride(1),
                                         frames.stride(2), 0, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.st_last_error()
        t_rec = device_ms(launch, a.reps)
        bytes_a, bytes_b = n * (count * 2 + planes), n * (planes + 3 * H * W)
        t_dec = {}
        for threads in sorted({a.threads, 16}):
            dec = jpeg.JpegDecoder(device=dev, threads=threads)
            t = host_ms(lambda: dec.decode(datas[:n]), a.reps, sync=True)
            t_dec[str(threads)] = dict(ms=t, frames_per_s=round(n / (t['median'] * 1e-3), 1))
        out[f'batch_{n}'] = dict(
            h2d=dict(ms=t_copy, bytes=host.numel(), gb_per_s=round(host.numel() / (t_copy['median'] * 1e-3) / 1e9, 2)),
            reconstruct=dict(ms=t_rec, bytes_launch_a=bytes_a, bytes_launch_b=bytes_b,
                             bytes_per_frame=(bytes_a + bytes_b) // n,
                             fraction_of_8TBs=round((bytes_a + bytes_b) / (t_rec['median'] * 1e-3) / PEAK_HBM, 4)),
            decode_by_threads=t_dec)
        print(sampling, n, out[f'batch_{n}'], flush=True)
    res[sampling] = out


def make_low_noise_files(distinct):
    """The same synthetic frames without their pixel noise: 8 x 8 block means, bilinearly interpolated back."""
    from stereotracking_amd import jpeg
    from stereotracking_amd.synthetic import synthetic_batch
    fr = synthetic_batch(list(range(distinct)), H, W, 192)
    img = fr['img'][:, :, :H].float()
    smooth = torch.nn.functional.interpolate(torch.nn.functional.avg_pool2d(img, 8), size=(H, W), mode='bilinear', align_corners=False)
    frames = smooth.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    return [jpeg.encode_jpeg(f, 90, '420') for f in frames]


def bench_entropy_device(a, dev):
    """entropy='device' against entropy='host' on 4:2:0 frames, legs alternated in this process: the entropy launches
    alone (hipEvents around st_jpeg_entropy_decode_dev), the blob's H2D copy against the coefficient copy it replaces,
    the whole decode() of 8 and 32 frames, the host CPU time decode() costs per frame, passes per tile, and the bytes the
    write pass moves (scan bytes in, coefficients out) as a share of 8 TB/s over the entropy launches' time."""
    import ctypes as C
    from stereotracking_amd import jpeg
    lib = jpeg._api()
    out = {}
    for label, files in (('noisy', make_files(a.distinct, '420')[0]), ('low_noise', make_low_noise_files(a.distinct))):
        info = jpeg._info(files[0])
        count = int(info.coef_count)
        rec = dict(file_bytes=[len(f) for f in files])
        for n in (8, 32):
            datas = [files[i % len(files)] for i in range(n)]
            pinned = torch.empty(jpeg.blob_capacity(datas), dtype=torch.uint8).pin_memory()
            host, used = jpeg.build_blob(datas, pinned.numpy())
            blob_dev = torch.empty(used, dtype=torch.uint8, device=dev)
            coef = torch.empty((n, count), dtype=torch.int16, device=dev)
            quant = torch.empty((n, 3, 64), dtype=torch.int16, device=dev)
            status = torch.empty(n, dtype=torch.int32, device=dev)
            work = torch.empty(int(lib.st_jpeg_entropy_work_bytes(C.byref(info), n)), dtype=torch.uint8, device=dev)
            coef_host = torch.empty(n * count * 2 + n * 384, dtype=torch.uint8).pin_memory()
            coef_dev = torch.empty_like(coef_host, device=dev)
            reps = max(3, a.reps // 4)
            t_blob = device_ms(lambda: blob_dev.copy_(pinned[:used], non_blocking=True), reps)
            t_coef = device_ms(lambda: coef_dev.copy_(coef_host, non_blocking=True), reps)
            t_launch = device_ms(lambda: jpeg.entropy_launch(host, used, blob_dev, n, info, coef, quant, status, work), reps)
            torch.cuda.synchronize()
            assert status.cpu().tolist() == [0] * n
            st = work[:16 * n].view(torch.int32).reshape(n, 4).cpu().numpy()
            scan_bytes = int(sum(jpeg.entropy_prepare(d).scan_bytes for d in datas))
            moved = scan_bytes + n * count * 2
            legs = {}
            decoders = {f'{mode}_{threads}': jpeg.JpegDecoder(device=dev, threads=threads, entropy=mode)
                        for mode in ('host', 'device') for threads in sorted({a.threads, 16})}
            for dec in decoders.values():
                dec.decode(datas)
            torch.cuda.synchronize()
            samples = {k: dict(wall=[], cpu=[]) for k in decoders}
            for _ in range(reps):
                for k, dec in decoders.items():                    # alternated legs
                    c0, t0 = time.process_time(), time.perf_counter()
                    dec.decode(datas)
                    c1 = time.process_time()
                    torch.cuda.synchronize()
                    samples[k]['wall'].append((time.perf_counter() - t0) * 1e3)
                    samples[k]['cpu'].append((c1 - c0) * 1e3 / n)
            for k, s in samples.items():
                legs[k] = dict(ms=stats(s['wall']), frames_per_s=round(n / (statistics.median(s['wall']) * 1e-3), 1),
                               host_cpu_ms_per_frame_in_decode=stats(s['cpu']))
            for dec in decoders.values():
                dec.close()
            rec[f'batch_{n}'] = dict(
                h2d_blob=dict(ms=t_blob, bytes=used), h2d_coefficients=dict(ms=t_coef, bytes=coef_host.numel()),
                entropy_launches=dict(ms=t_launch, bytes_moved_by_write_pass=moved,
                                      fraction_of_8TBs=round(moved / (t_launch['median'] * 1e-3) / PEAK_HBM, 5)),
                passes_per_tile=dict(max=int(st[:, 2].max()), mean=round(float(st[:, 3].sum()) / float(st[:, 0].sum()), 2),
                                     tiles_per_frame=int(st[0, 0]), subsequences_per_frame=int(st[0, 1])),
                decode=legs)
            print(label, n, rec[f'batch_{n}'], flush=True)
        out[label] = rec
    return out


def bench_test_step(a, dev):
    from stereotracking_amd import jpeg, mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.structures import TrackDataSample
    from stereotracking_amd.synthetic import synthetic_state_dict
    files, fr = make_files(a.distinct, '420')
    Fc, ori = a.frames_per_call, (H, W)
    datas = [files[i % len(files)] for i in range(Fc)]
    disps = [fr['disp_postp'][i % a.distinct:i % a.distinct + 1, :, :H].contiguous().to(dev) for i in range(Fc)]
    masks = [fr['disp_mask'][i % a.distinct:i % a.distinct + 1, :, :H].to(torch.uint8).to(dev) for i in range(Fc)]
    cfg = Config.fromfile(CFG)
    model = MODELS.build(dict(cfg.model, dense_batch=a.batch, autotune=False))
    model.detector.load_state_dict(synthetic_state_dict(list(model.detector._table), seed=0), strict=False)
    dec = jpeg.JpegDecoder(device=dev, threads=a.threads)
    decs = dict(decoded_per_call=dec,
                decoded_per_call_device_entropy=jpeg.JpegDecoder(device=dev, threads=a.threads, entropy='device'))
    resident = dec.decode(datas).clone()
    torch.cuda.synchronize()

    def call(t0, decode):
        frames = decs[decode].decode(datas) if decode else resident
        samples = [TrackDataSample(dict(frame_id=t0 + t, ori_shape=ori, img_shape=ori, scale_factor=(1.0, 1.0))) for t in range(Fc)]
        return model.test_step(dict(inputs=dict(img=[frames[i:i + 1] for i in range(Fc)], disp_postp=disps, disp_mask=masks),
                                    data_samples=samples))

    legs = (('pre_uploaded', None), ('decoded_per_call', 'decoded_per_call'),
            ('decoded_per_call_device_entropy', 'decoded_per_call_device_entropy'))
    rates = {key: [] for key, _ in legs}
    for _, decode in legs:
        call(0, decode)
    torch.cuda.synchronize()
    for r in range(a.repeats):
        for key, decode in legs:                                                      # alternated legs
            t0 = time.perf_counter()
            n = 0
            for c in range(a.calls):
                n += len(call(1000 * (r + 1) + c * Fc, decode))
            torch.cuda.synchronize()
            rates[key].append(n / (time.perf_counter() - t0))
            print(key, round(rates[key][-1], 1), flush=True)
    return dict(config=os.path.basename(CFG), frames_per_call=Fc, calls=a.calls, dense_batch=a.batch, autotune=False,
                decoder_threads=a.threads, note='random weights; decode() runs on the calling thread, before test_step',
                frames_per_s={k: dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))
                              for k, v in rates.items()})


def kernel_stats(path, bytes_a, bytes_b):
    """rocprofv3 --stats kernel table of a --launch-loop run -> each launch's average time, its bytes, its fraction of 8 TB/s."""
    out = {}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            name = row.get('Name') or row.get('KernelName') or ''
            for k, label, nbytes in (('jpeg_idct_kernel', 'launch_a_idct', bytes_a), ('jpeg_color_kernel', 'launch_b_color', bytes_b),
                                     ('jpeg_entropy_kernel', 'entropy_a_decode', None), ('jpeg_dc_kernel', 'entropy_b_dc', None)):
                if k in name:
                    us = float(row.get('AverageNs') or row.get('Average') or row.get('AVERAGE_NS')) / 1e3
                    out[label] = dict(kernel=k, calls=int(float(row.get('Calls') or row.get('CALLS') or 0)), average_us=round(us, 3))
                    if nbytes is not None:
                        out[label].update(bytes=nbytes, fraction_of_8TBs=round(nbytes / (us * 1e-6) / PEAK_HBM, 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--distinct', type=int, default=4, help='different synthetic frames encoded (the rest repeat them)')
    ap.add_argument('--threads', type=int, default=4)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=4)
    ap.add_argument('--frames-per-call', type=int, default=32)
    ap.add_argument('--no-test-step', dest='test_step', action='store_false')
    ap.add_argument('--launch-loop', type=int, default=0, help='only decode --launch-batch frames of --launch-sampling this '
                    'many times (for a profiler run: one sampling and batch per run, the kernel table is keyed by name)')
    ap.add_argument('--launch-sampling', default='420', choices=('420', '444'))
    ap.add_argument('--launch-batch', type=int, default=8)
    ap.add_argument('--launch-entropy', default='host', choices=('host', 'device'), help='the decoder of the --launch-loop run')
    ap.add_argument('--only-entropy-device', action='store_true',
                    help='measure only the entropy_device and test_step sections and merge them into the existing --out file')
    ap.add_argument('--kernel-stats', action='append', default=[], metavar='SAMPLING:BATCH=CSV',
                    help='kernel_stats.csv of such a profiler run (repeatable): adds each launch\'s time against its bytes')
    ap.add_argument('--entropy-kernel-stats', action='append', default=[], metavar='BATCH=CSV',
                    help='kernel_stats.csv of a --launch-loop --launch-entropy device run on 4:2:0: each entropy kernel\'s time')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_bench.json'))
    a = ap.parse_args()
    import stereotracking_amd  # noqa: F401  (before the first torch.cuda call: the package sets up the HIP runtime's queues)
    if not torch.cuda.is_available():
        raise SystemExit('jpeg_bench needs a GPU: nothing here is measured on a CPU')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    if a.launch_loop:
        from stereotracking_amd import jpeg
        dec = jpeg.JpegDecoder(device=dev, threads=a.threads, entropy=a.launch_entropy)
        files, _ = make_files(a.distinct, a.launch_sampling)
        datas = [files[i % len(files)] for i in range(a.launch_batch)]
        for _ in range(a.launch_loop):
            dec.decode(datas)
        torch.cuda.synchronize()
        return
    p = torch.cuda.get_device_properties(0)
    res = dict(device=f'{p.name} ({getattr(p, "gcnArchName", "?")}, {p.multi_processor_count} CUs)', size=[H, W], quality=90,
               distinct_frames=a.distinct, peaks=dict(hbm_tbs=PEAK_HBM / 1e12))
    if a.only_entropy_device:
        with open(a.out) as f:
            res = json.load(f)                   # the other sections stay as their own runs recorded them
    for sampling in () if a.only_entropy_device else ('420', '444'):
        bench_sampling(a, dev, sampling, res)
    for spec in a.kernel_stats:
        key, path = spec.split('=', 1)
        sampling, n = key.split(':')
        rec = res[sampling][f'batch_{int(n)}']['reconstruct']
        rec['launches'] = kernel_stats(path, rec['bytes_launch_a'], rec['bytes_launch_b'])
        print(sampling, n, rec['launches'], flush=True)
    res['entropy_device'] = bench_entropy_device(a, dev)
    for spec in a.entropy_kernel_stats:          # a --launch-loop --launch-entropy device profiler run on the noisy frames
        n, path = spec.split('=', 1)
        res['entropy_device']['noisy'][f'batch_{int(n)}']['entropy_launches']['kernels'] = kernel_stats(path, None, None)
        print('entropy kernels', n, res['entropy_device']['noisy'][f'batch_{int(n)}']['entropy_launches']['kernels'], flush=True)
    if a.test_step:
        res['test_step'] = bench_test_step(a, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
