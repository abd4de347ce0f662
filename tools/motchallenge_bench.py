#!/usr/bin/env python
"""Time MOTDroneMetrics' two protocols on both backends: protocol='rows' (pack_sequences + evaluate_packed) against
protocol='trackeval' (mot_eval.evaluate_motchallenge: st_mot_file_round, st_mot_challenge_preprocess, then the same four
scoring stages on the rows that are kept), and the host specification of both (stereotracking_amd/metrics.py).
Record-only: writes profiles/motchallenge_bench.json, asserts no speed.

    python tools/motchallenge_bench.py [--runs 7 --frames 512 --sweep 256 --parent-mot-eval FILE --parent-label TEXT
                                        --out profiles/motchallenge_bench.json]

Inputs: the sequences of tools/mot_eval_bench.py (jittered fp32 boxes, misses, spurious tracks, an id switch) - --sweep
sequences of --frames frames x 8 objects and one of --frames x 64 - with the ground truth's conf / class / visibility
columns added: every 4th object of class 8 (a distractor), every 7th zero-marked.  Device calls are timed with the host
clock around the whole call (it ends in the copy back and the host's finish), warm, the legs alternated run by run,
median of --runs with the spread; the stages with HIP events.  'host share' = the part of the call outside upload,
stages and copy back.  --parent-mot-eval names a copy of an earlier revision's stereotracking_amd/mot_eval.py
(`git show REV:stereotracking_amd/mot_eval.py > FILE`) whose 'rows' call is timed as a third alternated leg, on this
tree's library: the comparison for what the protocol adds.  The host backend is timed once per shape and protocol."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from mot_eval_bench import jittered_sequence, spread  # noqa: E402


def with_marks(gt):
    obj = gt[:, 1].astype(np.int64)
    return np.column_stack([gt, np.where(obj % 7 == 0, 0.0, 1.0), np.where(obj % 4 == 0, 8.0, 1.0), np.ones(len(gt))])


def host_scores(M, gts, preds, protocol, benchmark):
    t0 = time.perf_counter()
    if protocol == 'trackeval':
        ks = list(range(len(gts)))
        g, p = M.motchallenge_scored_rows(dict(zip(ks, gts)), dict(zip(ks, preds)), ks, benchmark)
        gts, preds = [g[k] for k in ks], [p[k] for k in ks]
    t1 = time.perf_counter()
    res = [(M.clear_identity(g, p, 0.5), M.hota(g, p)) for g, p in zip(gts, preds)]
    return res, dict(file_rows_and_preprocess=t1 - t0, scorers=time.perf_counter() - t1, total=time.perf_counter() - t0, runs=1)


def measure(name, gts, preds, runs, parent, benchmark='MOT17'):
    import torch
    from stereotracking_amd import metrics as M
    from stereotracking_amd import mot_eval
    rec = dict(shape=name, sequences=len(gts), gt_rows=int(sum(len(g) for g in gts)), pred_rows=int(sum(len(p) for p in preds)))

    def rows_leg(mod):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = mod.evaluate_packed(mod.pack_sequences(gts, preds), 0.5)
        return res, time.perf_counter() - t0

    def trackeval_leg():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res, tm = mot_eval.evaluate_motchallenge(gts, preds, benchmark, 0.5, timing=True)
        return res, time.perf_counter() - t0, tm

    legs = dict(rows=[], trackeval=[], parent_rows=[])
    stages, device_s = {}, []
    rows_leg(mot_eval), trackeval_leg()                        # warm: library load, allocator, the kernels' first launch
    if parent is not None:
        rows_leg(parent)
    for _ in range(runs):
        if parent is not None:
            legs['parent_rows'].append(rows_leg(parent)[1])
        res_rows, t = rows_leg(mot_eval)
        legs['rows'].append(t)
        res_te, t, tm = trackeval_leg()
        legs['trackeval'].append(t)
        for k, v in list(tm['challenge']['stages_ms'].items()) + list(tm['stages_ms'].items()):
            stages.setdefault(k, []).append(v)
        device_s.append(tm['challenge']['device_and_copies_s'] + tm['device_and_copies_s'])
    print(f'{name}: device legs done', file=sys.stderr, flush=True)
    rec['device_call_s'] = {k: spread(v) for k, v in legs.items() if v}
    rec['trackeval_stage_ms'] = {k: spread(v) for k, v in stages.items()}
    rec['trackeval_stages_total_ms'] = spread(np.sum([stages[k] for k in stages], axis=0))
    rec['trackeval_host_share_of_call'] = spread(1.0 - np.asarray(device_s) / np.asarray(legs['trackeval']))
    base = legs['parent_rows'] or legs['rows']
    rec['trackeval_minus_rows_s'] = dict(median=float(np.median(legs['trackeval']) - np.median(base)),
                                         against='parent_rows' if legs['parent_rows'] else 'rows')
    ref_rows, rec['host_rows_s'] = host_scores(M, gts, preds, 'rows', benchmark)
    print(f'{name}: host rows done', file=sys.stderr, flush=True)
    ref_te, rec['host_trackeval_s'] = host_scores(M, gts, preds, 'trackeval', benchmark)
    same = all(r['clear_identity'][k] == c[k] for res, ref in ((res_rows, ref_rows), (res_te, ref_te))
               for r, (c, _) in zip(res, ref) for k in ('TP', 'FP', 'FN', 'IDSW'))
    rec['counts_equal_host'] = bool(same)
    rec['TP_rows_vs_trackeval'] = [int(sum(c['TP'] for c, _ in ref_rows)), int(sum(c['TP'] for c, _ in ref_te))]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--frames', type=int, default=512)
    ap.add_argument('--sweep', type=int, default=256)
    ap.add_argument('--parent-mot-eval', default=None, help="an earlier revision's mot_eval.py: its 'rows' call, alternated")
    ap.add_argument('--parent-label', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'motchallenge_bench.json'))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'motchallenge_bench needs a GPU'
    parent = None
    if a.parent_mot_eval:
        import stereotracking_amd  # noqa: F401  (the package of the relative imports)
        spec = importlib.util.spec_from_file_location('stereotracking_amd._parent_mot_eval', a.parent_mot_eval)
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
    shapes = []
    gs, ps = zip(*(jittered_sequence(1000 + s, a.frames, 8) for s in range(a.sweep)))
    shapes.append((f'{a.sweep} x {a.frames} frames x 8 objects', [with_marks(g) for g in gs], list(ps)))
    g, p = jittered_sequence(164, a.frames, 64)
    shapes.append((f'1 x {a.frames} frames x 64 objects', [with_marks(g)], [p]))
    out = dict(tool='tools/motchallenge_bench.py', device=torch.cuda.get_device_name(0), runs=a.runs, benchmark='MOT17',
               parent_rows=(a.parent_label or os.path.basename(a.parent_mot_eval)) if parent is not None else None,
               shapes=[measure(n, g, p, a.runs, parent) for n, g, p in shapes])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
