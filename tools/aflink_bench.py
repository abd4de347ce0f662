#!/usr/bin/env python
"""Time AppearanceFreeLink (csrc/aflink.hip, stereotracking_amd/aflink.py), device against host backend, per stage.
Record-only: writes profiles/aflink_bench.json, asserts no speed.

    python tools/aflink_bench.py [--runs 7 --out profiles/aflink_bench.json]

Shapes: one long video of a few hundred fragments, and a sweep of many prediction sets.  The weights are the module's
initialisation (the time does not depend on them).  Device stage times are HIP events around each stage entry
(aflink.device_stages, warm, median of --runs with [min .. max]); 'call' is the host clock around forward_many (host
preparation, the upload, st_aflink_run, the copy back, assignment and relabelling per set), 'host_share' the part of it
spent outside the device and the copies.  The host backend (numpy, one batch-1 torch CPU forward per candidate) is timed
once per shape on the same rows.  The score kernel's yardstick is the fp32 MFMA pipe itself: the MFMAs it issues (padded
row tiles included) and the useful ones among them, as a share of 157.3 TFLOP/s."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_FLOPS = 157.3e12
# MFMA layers of one temporal module + fusion block: (rows per candidate, K, N)
GEMMS = ((54, 224, 64), (36, 448, 128), (18, 896, 256), (6, 768, 256))


def spread(v):
    v = np.asarray(v, np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def fragments(seed, n_tracks, frames, extent):
    """n_tracks fragments of 5 .. 60 rows on slow random walks inside an extent x extent window."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n_tracks):
        n = int(rng.integers(5, 61))
        f = int(rng.integers(0, frames)) + np.arange(n)
        xy = rng.uniform(0, extent, 2) + np.cumsum(rng.normal(0, 2.0, (n, 2)), 0)
        rows.append(np.column_stack([f, np.full(n, k), xy, xy + 30.0, np.full(n, 0.9)]))
    return np.concatenate(rows)


def flops(candidates, group):
    useful = 2 * sum(2.0 * m * k * n for m, k, n in GEMMS) * candidates
    groups = -(-candidates // group)
    issued = 2 * sum(2.0 * (-(-group * m // 32) * 32) * k * n for m, k, n in GEMMS) * groups
    return useful, issued


def measure(name, sets, runs):
    import torch
    from stereotracking_amd import _lib
    from stereotracking_amd.aflink import AppearanceFreeLink
    torch.manual_seed(0)
    host = AppearanceFreeLink(None, backend='host')
    dev = AppearanceFreeLink(host.model.state_dict(), backend='device')
    group = int(_lib.load().st_aflink_group_pairs())
    dev.forward_many(sets)                               # warm: library load, weights upload, allocator, first launches
    dev.device_stages(sets)
    stages, parts = {}, {}
    for _ in range(runs):
        torch.cuda.synchronize()
        st = dev.device_stages(sets)
        for k, v in st['stage_ms'].items():
            stages.setdefault(k, []).append(v)
        torch.cuda.synchronize()
        res, tm = dev.forward_many(sets, timing=True)
        parts.setdefault('st_aflink_run_ms', []).append(tm['stages_ms']['st_aflink_run'])
        for k in ('host_prepare_s', 'device_and_copies_s', 'host_finish_s', 'total_s'):
            parts.setdefault(k, []).append(tm[k])
    cands = int(tm['candidates'])
    useful, issued = flops(cands, group)
    score_s = np.asarray(stages['st_aflink_score']) / 1e3
    rec = dict(shape=name, sets=len(sets), rows_in=int(sum(len(s) for s in sets)), tracks=tm['tracks'], candidates=cands,
               capacity=tm['capacity'], rounds=tm['rounds'], group_pairs=group,
               tracks_after=int(sum(len(np.unique(r[:, 1])) for r in res)),
               device_stage_ms={k: spread(v) for k, v in stages.items()},
               st_aflink_run_ms=spread(parts['st_aflink_run_ms']),
               score_us_per_candidate=spread(score_s * 1e6 / max(cands, 1)),
               score_mfma_pipe_share=dict(issued=spread(issued / score_s / PEAK_FP32_MFMA_FLOPS),
                                          useful=spread(useful / score_s / PEAK_FP32_MFMA_FLOPS)),
               call_s=spread(parts['total_s']),
               host_share=spread((np.asarray(parts['host_prepare_s']) + np.asarray(parts['host_finish_s'])) /
                                 np.asarray(parts['total_s'])),
               **{k: spread(parts[k]) for k in ('host_prepare_s', 'device_and_copies_s', 'host_finish_s')})
    print(json.dumps(rec), flush=True)
    t0 = time.perf_counter()
    want = host.forward_many(sets)
    rec['host_backend_s'] = time.perf_counter() - t0
    rec['host_backend_over_device_call'] = rec['host_backend_s'] / rec['call_s']['median']
    rec['rows_equal_host'] = bool(all(np.array_equal(a, b) for a, b in zip(res, want)))
    print(json.dumps({k: rec[k] for k in ('host_backend_s', 'host_backend_over_device_call', 'rows_equal_host')}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'aflink_bench.json'))
    a = ap.parse_args()
    import torch
    shapes = [('1 video x 300 fragments x 600 frames', [fragments(1, 300, 600, 250.0)]),
              ('sweep of 32 sets x 70 fragments x 150 frames', [fragments(100 + s, 70, 150, 200.0) for s in range(32)])]
    out = dict(tool='tools/aflink_bench.py', device=torch.cuda.get_device_name(0), runs=a.runs,
               config='AppearanceFreeLink(temporal_threshold=(0, 30), spatial_threshold=75, confidence_threshold=0.95), '
                      'initialised weights',
               host_backend='numpy gate and transform, one batch-1 torch CPU forward per candidate',
               host_threads=os.environ.get('OMP_NUM_THREADS', ''), peak_fp32_mfma_flops=PEAK_FP32_MFMA_FLOPS,
               shapes=[measure(n, s, a.runs) for n, s in shapes])
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
