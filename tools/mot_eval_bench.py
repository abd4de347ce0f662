#!/usr/bin/env python
"""Time the device MOT evaluation (csrc/mot_eval.hip, stereotracking_amd/mot_eval.py) per stage, and the host backend
of stereotracking_amd/metrics.py on the same rows.  Record-only: writes profiles/mot_eval_bench.json, asserts no speed.

    python tools/mot_eval_bench.py [--runs 7 --frames 512 --sweep 256 --host-metrics FILE --host-label TEXT
                                    --out profiles/mot_eval_bench.json]

Inputs (jittered fp32 boxes on a grid, a tenth of the predictions missing, spurious tracks, an id switch at mid
sequence): one sequence of --frames frames x 8 and x 64 objects, and --sweep sequences of --frames x 8 (the shape of a
tracker-option sweep).  Device times are HIP events around the stage calls, warm, median of --runs with the spread;
'call' is the host clock around pack_sequences + evaluate_packed (upload, stages, the copy back, Identity's assignment
and the final divisions on the host), with the host's shares listed separately.  The host backend is timed once per
shape (clear_identity and hota of every sequence).  It is this tree's metrics.py with backend='host' unless
--host-metrics names another metrics.py to load and time instead (a copy of an earlier revision's file, for example:
`git show REV:stereotracking_amd/metrics.py > FILE`); --host-label says in the record which file that is."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def jittered_sequence(seed, frames, nobj, miss=0.1, spurious=0.15):
    """(gt rows, prediction rows) of `nobj` objects on a grid drifting with constant velocity: predictions = ground
    truth + N(0, 2.5 px), `miss` of them dropped, spurious tracks, every third prediction id switched at mid sequence."""
    rng = np.random.RandomState(seed)
    k = np.arange(nobj)
    pos = np.stack([40.0 + 34.0 * (k % 10), 40.0 + 46.0 * (k // 10)], 1) + rng.uniform(-3, 3, (nobj, 2))
    vel, size = rng.uniform(-1.5, 1.5, (nobj, 2)), rng.uniform(30, 44, (nobj, 2))
    gt, pred = [], []
    for t in range(frames):
        g = np.concatenate([pos + vel * t, size], 1).astype(np.float32).astype(np.float64)
        p = (g + np.concatenate([rng.normal(0, 2.5, (nobj, 2)), rng.normal(0, 1.5, (nobj, 2))], 1)
             ).astype(np.float32).astype(np.float64)
        keep = rng.uniform(size=nobj) >= miss
        pid = 11 + k + np.where((t >= frames // 2) & (k % 3 == 0), 5 * nobj + 1, 0)
        gt.append(np.column_stack([np.full(nobj, 1.0 + t), 3.0 + k, g]))
        pred.append(np.column_stack([np.full(nobj, 1.0 + t), pid, p])[keep])
        ns = rng.binomial(max(1, nobj // 4), spurious)
        if ns:
            b = np.concatenate([rng.uniform(20, 400, (ns, 2)), rng.uniform(25, 45, (ns, 2))], 1).astype(np.float32)
            pred.append(np.column_stack([np.full(ns, 1.0 + t), 900000.0 + 17 * (t % 4) + np.arange(ns), b]))
    return np.concatenate(gt), np.concatenate(pred)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def measure(name, gts, preds, runs, M):
    import torch
    from stereotracking_amd import mot_eval
    rec = dict(shape=name, sequences=len(gts), gt_rows=int(sum(len(g) for g in gts)), pred_rows=int(sum(len(p) for p in preds)))
    packed = mot_eval.pack_sequences(gts, preds)
    mot_eval.evaluate_packed(packed, 0.5, timing=True)          # warm: library load, allocator, kernels' first launch
    stages, parts, pack_s = {}, {}, []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        packed = mot_eval.pack_sequences(gts, preds)
        t1 = time.perf_counter()
        res, tm = mot_eval.evaluate_packed(packed, 0.5, timing=True)
        pack_s.append(t1 - t0)
        for k, v in tm['stages_ms'].items():
            stages.setdefault(k, []).append(v)
        for k in ('host_prepare_s', 'device_and_copies_s', 'host_finish_s', 'total_s'):
            parts.setdefault(k, []).append(tm[k])
    call = np.asarray(pack_s) + np.asarray(parts['total_s'])
    host_share = (np.asarray(pack_s) + np.asarray(parts['host_prepare_s']) + np.asarray(parts['host_finish_s'])) / call
    rec['device_stage_ms'] = {k: spread(v) for k, v in stages.items()}
    rec['device_stages_total_ms'] = spread(np.sum([stages[k] for k in stages], axis=0))
    rec['call_s'] = spread(call)
    rec['pack_sequences_s'] = spread(pack_s)
    rec['evaluate_packed_host_prepare_s'] = spread(parts['host_prepare_s'])
    rec['evaluate_packed_upload_stages_copy_back_s'] = spread(parts['device_and_copies_s'])
    rec['evaluate_packed_host_finish_s'] = spread(parts['host_finish_s'])
    rec['host_share_of_call'] = spread(host_share)
    t0 = time.perf_counter()
    ref_c = [M.clear_identity(g, p, 0.5) for g, p in zip(gts, preds)]
    t1 = time.perf_counter()
    ref_h = [M.hota(g, p) for g, p in zip(gts, preds)]
    t2 = time.perf_counter()
    rec['host_backend_s'] = dict(clear_identity=t1 - t0, hota=t2 - t1, total=t2 - t0, runs=1)
    rec['host_over_device_call'] = (t2 - t0) / rec['call_s']['median']
    same = all(r['clear_identity']['TP'] == c['TP'] and r['clear_identity']['IDSW'] == c['IDSW'] and
               np.array_equal(r['hota']['HOTA_TP'], h['HOTA_TP']) for r, c, h in zip(res, ref_c, ref_h))
    rec['counts_equal_host'] = bool(same)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--frames', type=int, default=512)
    ap.add_argument('--sweep', type=int, default=256)
    ap.add_argument('--host-metrics', default=None, help='another metrics.py to time as the host backend')
    ap.add_argument('--host-label', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mot_eval_bench.json'))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'mot_eval_bench needs a GPU'
    if a.host_metrics:
        spec = importlib.util.spec_from_file_location('host_metrics_under_test', a.host_metrics)
        M = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(M)
        label = a.host_label or f'the file given as --host-metrics ({os.path.basename(a.host_metrics)})'
    else:
        from stereotracking_amd import metrics as M
        label = a.host_label or "this tree's stereotracking_amd/metrics.py, backend='host'"
    shapes = []
    for n in (8, 64):
        g, p = jittered_sequence(100 + n, a.frames, n)
        shapes.append((f'1 x {a.frames} frames x {n} objects', [g], [p]))
    gs, ps = zip(*(jittered_sequence(1000 + s, a.frames, 8) for s in range(a.sweep)))
    shapes.append((f'{a.sweep} x {a.frames} frames x 8 objects', list(gs), list(ps)))
    out = dict(tool='tools/mot_eval_bench.py', device=torch.cuda.get_device_name(0), runs=a.runs,
               host_backend='clear_identity + hota (numpy, scipy), one Python iteration per frame', host_backend_file=label,
               shapes=[measure(n, g, p, a.runs, M) for n, g, p in shapes])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
