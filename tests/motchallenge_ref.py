"""Test-side restatement of MOTDroneMetrics(protocol='trackeval') and the inputs of its tests (a helper module).

Written independently of stereotracking_amd/metrics.py: the file values come from Python's own '%d' / '%.3f' formatting
of whole text lines, parsed back with float() - the reference's format strings (mot_drone_metrics.py:223-253) and what a
reader of those files does; the preprocessing is the loop form of what TrackEval's MotChallenge2DBox does for the class
'pedestrian' [upstream-memory], with a scalar IoU."""
import functools

import numpy as np
from scipy.optimize import linear_sum_assignment

EPS = np.finfo(float).eps
DISTRACTORS = {'MOT15': (), 'MOT16': (2, 7, 8, 12), 'MOT17': (2, 7, 8, 12), 'MOT20': (2, 6, 7, 8, 12),
               'DanceTrack': (2, 7, 8, 12)}


# ---- the files -------------------------------------------------------------------------------------------------------
def gt_line(row):
    return '%d,%d,%d,%d,%d,%d,%d,%d,%.5f' % tuple(row[:9])


def pred_line(row):
    return '%d,%d,%.3f,%.3f,%.3f,%.3f,%.3f,-1,-1,-1' % tuple(row[:7])


def file_rows_ref(gt_rows, pred_rows):
    """(gt (n, 8), pred (m, 7)): the fields of the written lines, through float()."""
    g = [[float(t) for t in gt_line(r).split(',')[:8]] for r in np.asarray(gt_rows, dtype=np.float64).reshape(-1, 9)]
    p = [[float(t) for t in pred_line(r).split(',')[:7]] for r in np.asarray(pred_rows, dtype=np.float64).reshape(-1, 7)]
    return np.array(g, dtype=np.float64).reshape(-1, 8), np.array(p, dtype=np.float64).reshape(-1, 7)


def round3_ref(values):
    return np.array([float('%.3f' % v) for v in np.asarray(values, dtype=np.float64).tolist()])


# ---- the preprocessing -----------------------------------------------------------------------------------------------
def iou_xywh(a, b):
    iw = min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0])
    ih = min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1])
    inter = max(iw, 0.0) * max(ih, 0.0)
    union = a[2] * a[3] + b[2] * b[3] - inter
    return inter / union if union > 0 else 0.0


def frame_matrix(g, p):
    """The thresholded matching matrix of one frame (g: gt rows, p: prediction rows)."""
    m = np.array([[iou_xywh(a[2:6], b[2:6]) for b in p] for a in g], dtype=np.float64).reshape(len(g), len(p))
    m[m < 0.5 - EPS] = 0
    return m


def matched_pairs(m):
    r, c = linear_sum_assignment(-m)
    ok = m[r, c] > EPS
    return r[ok], c[ok]


def preprocess_ref(gt, pred, benchmark):
    """(gt_keep, pred_keep, stats) of file rows; stats counts the removals and the frames whose optimum is tied (a
    row-permuted matrix gives another removed set)."""
    gt, pred = np.asarray(gt, dtype=np.float64).reshape(-1, 8), np.asarray(pred, dtype=np.float64).reshape(-1, 7)
    stats = dict(removed=0, matched=0, ties=0, frames=0)
    pred_keep = np.ones(len(pred), bool)
    if benchmark == 'MOT15':
        return gt[:, 6] != 0, pred_keep, stats
    rng = np.random.RandomState(11)
    for f in sorted(set(gt[:, 0].astype(int).tolist()) & set(pred[:, 0].astype(int).tolist())):
        gi, pi = np.nonzero(gt[:, 0].astype(int) == f)[0], np.nonzero(pred[:, 0].astype(int) == f)[0]
        m = frame_matrix(gt[gi], pred[pi])
        r, c = matched_pairs(m)
        removed = {int(pi[j]) for i, j in zip(r, c) if int(gt[gi[i], 7]) in DISTRACTORS[benchmark]}
        perm = rng.permutation(len(gi))
        r2, c2 = matched_pairs(m[perm])
        removed2 = {int(pi[j]) for i, j in zip(r2, c2) if int(gt[gi[perm[i]], 7]) in DISTRACTORS[benchmark]}
        stats['ties'] += removed != removed2
        stats['removed'] += len(removed)
        stats['matched'] += len(r)
        stats['frames'] += 1
        pred_keep[list(removed)] = False
    return (gt[:, 6] != 0) & (gt[:, 7] == 1), pred_keep, stats


# ---- inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adversarial_values(n_half=12000, n_other=4000, seed=0):
    """Values on which rounding x * 1000 first goes wrong: the half-way points (2k + 1) / 2000 with their 0 .. 3 ulp
    neighbours on either side (negatives included), uniform values, and differences of two fp32 coordinates (what a box
    width is)."""
    rng = np.random.RandomState(seed)
    k = rng.randint(-2_000_000, 2_000_001, n_half)
    x = (2 * k + 1) / 2000.0
    steps = rng.randint(0, 4, n_half)
    up = rng.rand(n_half) < 0.5
    for s in range(1, 4):
        move = steps >= s
        x[move] = np.nextafter(x[move], np.where(up[move], np.inf, -np.inf))
    uni = rng.uniform(-3000, 3000, n_other)
    diff = (rng.uniform(0, 1300, n_other).astype(np.float32) - rng.uniform(0, 1300, n_other).astype(np.float32)).astype(np.float64)
    out = np.concatenate([x, uni, diff])
    out.setflags(write=False)
    return out


def video(seed, frames=12, objects=6, classes=(1, 1, 1, 8, 2, 3), zero_marked=(2,)):
    """(gt (n, 9), pred (m, 7)) float rows of one synthetic video: `objects` tracks drifting over `frames` frames, object
    o of class classes[o % len], the objects of `zero_marked` with conf 0; predictions = the boxes plus sub-pixel noise
    (every 5th detection dropped, a false positive in every 3rd frame), ids offset by 100.  Coordinates carry many
    decimals, so truncation and rounding both change them."""
    rng = np.random.RandomState(seed)
    x0 = rng.uniform(20, 400, objects) + 150.0 * np.arange(objects)
    y0 = rng.uniform(20, 300, objects)
    w, h = rng.uniform(30, 80, objects), rng.uniform(40, 110, objects)
    vx, vy = rng.uniform(-3, 3, objects), rng.uniform(-2, 2, objects)
    gt, pred = [], []
    for f in range(1, frames + 1):
        for o in range(objects):
            box = [x0[o] + vx[o] * f, y0[o] + vy[o] * f, w[o] + 0.37 * f, h[o] + 0.21 * f]
            gt.append([f, o + 1] + box + [0 if o in zero_marked else 1, classes[o % len(classes)], rng.uniform(0.2, 1.0)])
            if (f * objects + o) % 5 != 4:
                noise = rng.uniform(-2.5, 2.5, 4)
                pred.append([f, 100 + o] + [b + n for b, n in zip(box, noise)] + [rng.uniform(0.3, 1.0)])
        if f % 3 == 0:
            pred.append([f, 200 + f, 1200.5 + f, 40.25, 50.125, 60.0625, 0.5])
    return np.array(gt, dtype=np.float64), np.array(pred, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def videos(n=3, frames=12, objects=6):
    return {f'v{k}': video(40 + k, frames, objects, classes=((1, 1, 1, 8, 2, 3), (1, 7, 1, 12, 1, 6), (1, 1, 2, 1, 8, 1))[k % 3],
                           zero_marked=((2,), (0, 3), ())[k % 3]) for k in range(n)}


def frame(g, p, f=1, classes=None, conf=None, seed=0):
    """One frame of g x p rows: gt i and prediction i (i < min(g, p)) overlap well, everything else lies apart."""
    rng = np.random.RandomState(seed + 131 * g + p)
    classes = [1] * g if classes is None else classes
    conf = [1] * g if conf is None else conf
    gt = [[f, i + 1, 40.0 * (i % 32) + rng.uniform(0, 3), 150.0 * (i // 32) + rng.uniform(0, 3), 30 + rng.uniform(0, 5),
           100 + rng.uniform(0, 9), conf[i], classes[i], 1.0] for i in range(g)]
    pred = [[f, 500 + j, 40.0 * (j % 32) + rng.uniform(0, 3), 150.0 * (j // 32) + rng.uniform(0, 3), 30 + rng.uniform(0, 5),
             100 + rng.uniform(0, 9), 0.9] for j in range(p)]
    return np.array(gt, dtype=np.float64).reshape(-1, 9), np.array(pred, dtype=np.float64).reshape(-1, 7)


def crowd(g, p, f=1, seed=0):
    """One frame whose boxes stand 8 px apart at 32 px width: every row has several candidates above 0.5, so the
    maxima are no assignment and the augmenting-path search runs.  Every third ground-truth row is a distractor."""
    rng = np.random.RandomState(seed + 17 * g + p)
    gt = [[f, i + 1, 8.0 * i + rng.uniform(0, 2), rng.uniform(0, 4), 32 + rng.uniform(0, 2), 100 + rng.uniform(0, 4), 1,
           (1, 1, 8)[i % 3], 1.0] for i in range(g)]
    pred = [[f, 500 + j, 8.0 * j + rng.uniform(0, 2), rng.uniform(0, 4), 32 + rng.uniform(0, 2), 100 + rng.uniform(0, 4), 0.9]
            for j in range(p)]
    return np.array(gt, dtype=np.float64).reshape(-1, 9), np.array(pred, dtype=np.float64).reshape(-1, 7)


def stack(*parts):
    """Frames / videos (gt, pred) one after the other as one sequence, frame numbers 1, 2, ... in the order given."""
    gts, preds = [], []
    for k, (g, p) in enumerate(parts):
        g, p = g.copy(), p.copy()
        g[:, 0], p[:, 0] = k + 1, k + 1
        gts.append(g)
        preds.append(p)
    return np.concatenate(gts), np.concatenate(preds)
