"""Loop restatement of InterpolateTracklets' linear rules, the yardstick of the row-for-row tests,
the shared scenarios of tests/test_cpu_tracklets.py and tests/test_tracklets_gpu.py, and the GSI fixture's reader and
tolerance.  Plain Python floats and loops; nothing here imports the package."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gsi_truth.npz')
GOLDEN_LONG = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gsi_truth_long.npz')


def interpolate_ref(rows, min_num_frames=5, max_num_frames=20):
    """rows: iterable of (frame, id, c0, c1, c2, c3, score, ...).  Returns the (M, 7) array of the decided rules: per id in
    input order; <= 2 rows dropped; > min_num_frames rows: every gap 1 < g < max_num_frames filled with
    j / g * (right - left) + left and score 1.0; ascending frame, then ascending id."""
    tracks = {}
    for r in rows:
        tracks.setdefault(int(r[1]), []).append([float(v) for v in r[:7]])
    out = []
    for tid, tr in tracks.items():
        if len(tr) <= 2:
            continue
        fill = len(tr) > min_num_frames
        for a, b in zip(tr, tr[1:] + [None]):
            out.append(list(a))
            if b is None or not fill:
                continue
            g = int(b[0] - a[0])
            if 1 < g < max_num_frames:
                for j in range(1, g):
                    out.append([j + a[0], float(tid)] + [j / g * (b[c] - a[c]) + a[c] for c in range(2, 6)] + [1.0])
    out.sort(key=lambda r: (r[0], r[1]))
    return np.array(out, dtype=np.float64).reshape(-1, 7)


def track(tid, frames, seed=0, score=0.5):
    """A track on a slowly moving box with awkward fp64 fractions (thirds, sevenths) so that operation order shows."""
    rng = np.random.default_rng(seed + 1000 * (tid % 97))
    f = np.asarray(frames, dtype=np.float64)
    x = 600.0 + f * (10.0 / 3.0) + rng.standard_normal(len(f))
    y = 400.0 + f * (5.0 / 7.0) + rng.standard_normal(len(f))
    return np.column_stack([f, np.full(len(f), float(tid)), x, y, x + 50.0 + f / 9.0, y + 80.0 - f / 11.0,
                            np.full(len(f), score) + rng.random(len(f)) * 0.25])


def linear_scenarios(min_num_frames=5, max_num_frames=20):
    """name -> rows.  Track lengths 2, 3, min and min + 1; gaps 1, 2, max - 1 and max; several gaps in one track; sparse
    and negative ids; tracks interleaved in input order."""
    m, M = min_num_frames, max_num_frames
    out = {}
    out['lengths'] = np.concatenate([track(1, [1, 4]), track(2, [1, 3, 7]), track(3, np.arange(m) * 3 + 2),
                                     track(4, np.arange(m + 1) * 3 + 1)])
    out['gaps'] = np.concatenate([track(7, [1, 2, 4, 5, 5 + M - 1, 6 + M - 1, 6 + 2 * M - 1, 7 + 2 * M - 1]),
                                  track(9, [3, 4, 5, 6, 7, 8, 8 + M, 9 + M])])
    out['several_gaps'] = track(5, [2, 5, 6, 11, 12, 13, 20, 38, 39, 45])
    rows = np.concatenate([track(-3, [1, 3, 4, 8, 9, 10, 12]), track(1000003, [2, 3, 9, 10, 11, 12, 30]),
                           track(0, [1, 2, 3, 4, 5, 9]), track(41, [4, 6])])
    out['sparse_negative_ids'] = rows[np.argsort(rows[:, 0], kind='stable')]          # frame-major, as a tracker emits
    wide = np.column_stack([out['several_gaps'], np.arange(10.0), np.arange(10.0)])   # extra columns are ignored
    out['wide_rows'] = wide
    return out


def gsi_cases():
    """name -> dict(frames, y (4, n), tau, len_scale, truth (4, n), sklearn (4, n), ref_err) of the committed fixture."""
    z = np.load(GOLDEN)
    return {str(n): {k: z[f'{n}/{k}'] for k in ('frames', 'y', 'tau', 'len_scale', 'truth', 'sklearn', 'ref_err')}
            for n in z['names']}


def gsi_long_case():
    """The 512-row case of tests/golden/gsi_truth_long.npz (make_gsi_golden.py --long), same keys."""
    z = np.load(GOLDEN_LONG)
    return {k: z[f'n512/{k}'] for k in ('frames', 'y', 'tau', 'len_scale', 'truth', 'sklearn', 'ref_err')}


def gsi_rows(case, tid=1, score=0.75):
    n = len(case['frames'])
    return np.column_stack([case['frames'].astype(np.float64), np.full(n, float(tid)), case['y'].T, np.full(n, score)])


def gsi_tolerance(case):
    """max(4 * ref_err, n * ulp(max |y|)): 4 = the project's margin for another correct summation order, the floor for
    the cases where K is nearly the identity and both errors are a few ulp."""
    n = len(case['frames'])
    return max(4.0 * float(case['ref_err']), n * float(np.spacing(np.abs(case['y']).max())))


def feed_metric(metric, video, pred_rows, gt_rows):
    """Rows (frame, id, x1, y1, x2, y2, score) / (frame, id, x1, y1, x2, y2) through MOTDroneMetrics.process(), frame by
    frame (frames from 0; process() stores frame + 1 and x, y, w, h)."""
    import torch
    from stereotracking_amd.structures import InstanceData, TrackDataSample
    pred_rows = np.asarray(pred_rows, dtype=np.float64).reshape(-1, 7)
    gt_rows = np.asarray(gt_rows, dtype=np.float64).reshape(-1, 6)
    for f in sorted(set(pred_rows[:, 0].astype(int)) | set(gt_rows[:, 0].astype(int))):
        p = pred_rows[pred_rows[:, 0].astype(int) == f]
        s = TrackDataSample(dict(frame_id=int(f)))
        s.pred_track_instances = InstanceData(bboxes=torch.from_numpy(p[:, 2:6].copy()), scores=torch.from_numpy(p[:, 6].copy()),
                                              labels=torch.zeros(len(p), dtype=torch.long),
                                              instances_id=torch.from_numpy(p[:, 1].astype(np.int64)))
        gt = [dict(instance_id=int(r[1]), bbox=r[2:6].tolist(), location=[0.0, 0.0, 20.0])
              for r in gt_rows[gt_rows[:, 0].astype(int) == f]]
        metric.process(video, s, gt)
    return metric


def metric_videos():
    """video -> (pred rows, gt rows) of the known-answer scenario.  'gap': one ground-truth object over 12 frames on a
    linear path; the predicted track follows it exactly but misses frames 4, 5, 6, and a spurious track has 2 rows.
    'plain': two complete tracks on their objects (nothing to fill, nothing to drop)."""
    def path(tid, frames, x0, y0):
        f = np.asarray(frames, dtype=np.float64)
        x, y = x0 + 4.0 * f, y0 + 2.0 * f
        return np.column_stack([f, np.full(len(f), float(tid)), x, y, x + 40.0, y + 60.0])
    def with_score(r):
        return np.column_stack([r, np.full(len(r), 0.9)])
    gap_gt = path(1, range(12), 100.0, 80.0)
    gap_pred = np.concatenate([with_score(path(5, [0, 1, 2, 3, 7, 8, 9, 10, 11], 100.0, 80.0)),
                               with_score(path(9, [2, 3], 700.0, 500.0))])
    plain_gt = np.concatenate([path(1, range(8), 50.0, 50.0), path(2, range(8), 400.0, 300.0)])
    plain_pred = np.concatenate([with_score(path(3, range(8), 51.0, 50.5)), with_score(path(4, range(8), 400.5, 301.0))])
    return dict(gap=(gap_pred, gap_gt), plain=(plain_pred, plain_gt))
