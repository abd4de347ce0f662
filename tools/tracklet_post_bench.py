#!/usr/bin/env python
"""Time InterpolateTracklets (csrc/tracklet_post.hip, stereotracking_amd/tracklets.py) with the Gaussian-smoothed
interpolation on, device against host backend, per stage.  Record-only: writes profiles/tracklet_post_bench.json, asserts
no speed.

    python tools/tracklet_post_bench.py [--runs 5 --out profiles/tracklet_post_bench.json]

Shapes: the threshold sweep of tools/mot_eval_bench.py (256 prediction sets x 512 frames x 8 objects, the same generator)
and KITTI Tracking's (21 sequences x 380 frames x 12 objects).  Device times are HIP events around the stage calls, warm,
median of --runs with the spread; 'call' is the host clock around forward_many (host preparation, upload, stages, the
copy back, the final sort).  gsi_phase_share: the workgroups' own 100 MHz clocks, summed, per phase of st_tracklet_gsi.
The host backend (numpy + scipy, one Cholesky factorisation per track) is timed once per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from mot_eval_bench import jittered_sequence, spread  # noqa: E402


def prediction_sets(seed, sets, frames, nobj):
    out = []
    for s in range(sets):
        p = jittered_sequence(seed + s, frames, nobj)[1]
        out.append(np.column_stack([p, np.full(len(p), 0.9)]))
    return out


def measure(name, sets, runs):
    import torch
    from stereotracking_amd.tracklets import InterpolateTracklets
    dev = InterpolateTracklets(use_gsi=True, backend='device')
    host = InterpolateTracklets(use_gsi=True, backend='host')
    dev.forward_many(sets, timing=True)              # warm: library load, allocator, kernels' first launch
    stages, parts, shares = {}, {}, {}
    for _ in range(runs):
        torch.cuda.synchronize()
        res, tm = dev.forward_many(sets, timing=True)
        for k, v in tm['stages_ms'].items():
            stages.setdefault(k, []).append(v)
        for k in ('host_prepare_s', 'device_and_copies_s', 'host_finish_s', 'total_s'):
            parts.setdefault(k, []).append(tm[k])
        for k, v in tm['gsi_phase_share'].items():
            shares.setdefault(k, []).append(v)
    rec = dict(shape=name, sets=len(sets), rows_in=int(sum(len(s) for s in sets)), tracks=tm['tracks'],
               rows_kept_in=tm['rows_in'], rows_out=tm['rows_out'], gsi_launches=tm['gsi_launches'])
    n = np.concatenate([np.unique(r[:, 1], return_counts=True)[1] for r in res])
    rec['track_rows'] = dict(max=int(n.max()), median=float(np.median(n)), min=int(n.min()),
                             fp64_gflop_factorisation=float((n.astype(np.float64) ** 3 / 3).sum() / 1e9))
    call = np.asarray(parts['total_s'])
    rec['device_stage_ms'] = {k: spread(v) for k, v in stages.items()}
    rec['device_stages_total_ms'] = spread(np.sum([stages[k] for k in stages], axis=0))
    rec['gsi_phase_share'] = {k: spread(v) for k, v in shares.items()}
    rec['call_s'] = spread(call)
    rec['host_prepare_s'] = spread(parts['host_prepare_s'])
    rec['upload_stages_copy_back_s'] = spread(parts['device_and_copies_s'])
    rec['host_finish_s'] = spread(parts['host_finish_s'])
    rec['host_share_of_call'] = spread((np.asarray(parts['host_prepare_s']) + np.asarray(parts['host_finish_s'])) / call)
    t0 = time.perf_counter()
    ref = host.forward_many(sets)
    rec['host_backend_s'] = dict(total=time.perf_counter() - t0, runs=1)
    rec['host_over_device_call'] = rec['host_backend_s']['total'] / rec['call_s']['median']
    rec['host_over_device_stages'] = rec['host_backend_s']['total'] / (rec['device_stages_total_ms']['median'] / 1e3)
    rec['max_abs_device_minus_host_px'] = float(max(np.abs(a[:, 2:6] - b[:, 2:6]).max() for a, b in zip(res, ref) if len(a)))
    rec['frames_ids_scores_equal_host'] = bool(all(np.array_equal(a[:, [0, 1, 6]], b[:, [0, 1, 6]]) for a, b in zip(res, ref)))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tracklet_post_bench.json'))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'tracklet_post_bench needs a GPU'
    shapes = [('256 x 512 frames x 8 objects', prediction_sets(1000, 256, 512, 8)),
              ('21 x 380 frames x 12 objects', prediction_sets(5000, 21, 380, 12))]
    out = dict(tool='tools/tracklet_post_bench.py', device=torch.cuda.get_device_name(0), runs=a.runs,
               config='InterpolateTracklets(min_num_frames=5, max_num_frames=20, use_gsi=True, smooth_tau=10)',
               host_backend='numpy + scipy.linalg.cho_factor / cho_solve, one Python iteration per track',
               host_threads=os.environ.get('OMP_NUM_THREADS'),
               shapes=[measure(n, s, a.runs) for n, s in shapes])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
