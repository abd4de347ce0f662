"""Scenario builders shared by tests/test_cpu_mot_eval.py and tests/test_mot_eval_gpu.py: small, seeded, and built so that
the host scorer alone is insensitive to how assignment ties break (boxes are fp32 values with a random jitter widened
to fp64; the CPU test proves the precondition for every scenario).  A scenario is (gt_by_video, pred_by_video): dicts
video -> list of rows (frame, id, x, y, w, h)."""
import functools

import numpy as np

INT_KEYS = ('TP', 'FN', 'FP', 'IDSW', 'Frag', 'MT', 'PT', 'ML', 'IDTP', 'IDFN', 'IDFP')
FLOAT_KEYS = ('MOTA', 'MOTP', 'IDF1', 'IDP', 'IDR')
HOTA_INT_KEYS = ('HOTA_TP', 'HOTA_FN', 'HOTA_FP')
HOTA_FLOAT_KEYS = ('LocA', 'AssA', 'AssRe', 'AssPr', 'DetA', 'DetRe', 'DetPr', 'HOTA')


def jittered_sequence(seed, frames, nobj, frame_step=1, id_scale=1, switch_at=None, miss=0.1, spurious=0.15,
                      sizes=None, pred_sizes=None):
    """`nobj` objects on a grid (neighbours overlap a little, so the assignment has competing candidates) drifting with
    constant velocity; predictions = ground truth + N(0, 2.5 px) jitter, `miss` of them dropped, spurious tracks with
    ids of their own, the prediction ids of every third object switched at frame index `switch_at`.  Frame numbers
    1 + frame_step * t (gaps), ids multiplied by id_scale and offset (large, non-contiguous).  sizes / pred_sizes:
    objects per frame on either side (lists over the frames) instead of all `nobj`."""
    rng = np.random.RandomState(seed)
    k = np.arange(nobj)
    pos = np.stack([40.0 + 34.0 * (k % 10), 40.0 + 46.0 * (k // 10)], 1) + rng.uniform(-3, 3, (nobj, 2))
    vel = rng.uniform(-1.5, 1.5, (nobj, 2))
    size = rng.uniform(30, 44, (nobj, 2))
    gt, pred = [], []
    for t in range(frames):
        frame = 1 + frame_step * t
        g = np.concatenate([pos + vel * t, size], 1).astype(np.float32).astype(np.float64)
        p = (g + np.concatenate([rng.normal(0, 2.5, (nobj, 2)), rng.normal(0, 1.5, (nobj, 2))], 1)
             ).astype(np.float32).astype(np.float64)
        keep = rng.uniform(size=nobj) >= miss
        n_g = nobj if sizes is None else sizes[t]
        n_p = nobj if pred_sizes is None else pred_sizes[t]
        for i in range(n_g):
            gt.append([frame, 3 + id_scale * i, *g[i]])
        for i in range(n_p):
            if not keep[i] and pred_sizes is None:
                continue
            pid = 11 + id_scale * i
            if switch_at is not None and t >= switch_at and i % 3 == 0:
                pid += 5 * id_scale * nobj + 1
            pred.append([frame, pid, *p[i]])
        if pred_sizes is None:
            for j in range(rng.binomial(max(1, nobj // 4), spurious)):
                b = np.concatenate([rng.uniform(20, 400, 2), rng.uniform(25, 45, 2)]).astype(np.float32).astype(np.float64)
                pred.append([frame, 900000 + 17 * (t % 4) + j, *b])
    return gt, pred


def random_b1():
    g, p = jittered_sequence(1, 12, 3, frame_step=3, id_scale=1000003, switch_at=6)
    return {'solo': g}, {'solo': p}


def random_b3():
    out = {}
    for name, (seed, T, n) in dict(a=(2, 12, 3), b=(3, 40, 20), c=(4, 5, 7)).items():
        out[name] = jittered_sequence(seed, T, n, frame_step=2 if name != 'c' else 1, id_scale=1000003 if name == 'a' else 7,
                                      switch_at=T // 2)
    return {k: v[0] for k, v in out.items()}, {k: v[1] for k, v in out.items()}


def wave_sizes():
    """Frames of 1, 63, 64 and 65 objects per side, and a rectangular frame in each direction, in one sequence."""
    sizes = [1, 63, 64, 65, 65, 3]
    psizes = [1, 63, 64, 65, 3, 65]
    g, p = jittered_sequence(5, len(sizes), 65, sizes=sizes, pred_sizes=psizes)
    return {'waves': g}, {'waves': p}


def limit_frame(n):
    """A two-object frame, then one frame of n objects per side."""
    g, p = jittered_sequence(6, 2, n, sizes=[2, n], pred_sizes=[2, n])
    return {'limit': g}, {'limit': p}


def at_limit():
    return limit_frame(256)


def clear_continuity():
    """gt 1: the previous frame's partner (IoU 0.6) beats a newcomer with the higher IoU (0.9).  gt 2: matched to
    tracker 5, unmatched for two frames, then matched to tracker 6: one IDSW against the last match ever, one Frag, PT.
    gt 3: tracked throughout (MT).  gt 4: never tracked (ML)."""
    gt, pred = [], []
    for f in range(1, 6):
        gt += [[f, 1, 0, 0, 20, 20], [f, 2, 100, 0, 20, 20], [f, 3, 200, 0, 20, 20], [f, 4, 300, 0, 20, 20]]
        pred.append([f, 1, 4 if f == 1 else 5, 0, 20, 20])
        if f >= 2:
            pred.append([f, 2, 1, 0, 20, 20])              # the newcomer, closer to gt 1 than its partner
        if f <= 2:
            pred.append([f, 5, 101.5, 0, 20, 20])
        if f == 5:
            pred.append([f, 6, 102.25, 0, 20, 20])
        pred.append([f, 7, 200.75 + 0.125 * f, 0, 20, 20])
    return {'bonus': gt}, {'bonus': pred}


def empty_kinds():
    """Frames with gt only (3), predictions only (5) and a missing frame number (6) between matched frames; in frames 4
    and 7 a newcomer with the higher IoU competes with the partner of the last matched frame, so a wrong reset of the
    previous-frame state changes IDSW and Frag.  Plus a video without predictions, one without gt, one without rows."""
    gt, pred = [], []
    for f in (1, 2, 3, 4, 7):
        gt.append([f, 10, 0, 0, 20, 20])
        gt.append([f, 11, 100, 0, 20, 20])
    for f in (1, 2, 4, 5, 7):
        pred.append([f, 1, 5.25, 0, 20, 20])               # partner of gt 10, IoU about 0.58
        pred.append([f, 3, 100.5 + 0.25 * f, 0, 20, 20])
        if f in (4, 7):
            pred.append([f, 2, 1.125, 0, 20, 20])          # newcomer, IoU about 0.89
    only_gt = [[f, 1, 10.5 * f, 0, 20, 20] for f in (2, 3, 5)]
    only_pred = [[f, 4, 10.25 * f, 3, 20, 20] for f in (1, 4)]
    return ({'mixed': gt, 'nopred': only_gt, 'nogt': [], 'zero': []},
            {'mixed': pred, 'nopred': [], 'nogt': only_pred, 'zero': []})


def thresholds():
    """One frame: IoU exactly 0.5 (a CLEAR match at iou_thr 0.5, a HOTA TP at the alpha stored as 0.5), a pair just
    below 0.5, and two pairs straddling the alpha whose fp64 value is 0.15000000000000002.  The pairs are far apart."""
    gt = [[1, 1, 0, 0, 2, 1], [1, 2, 100, 0, 2, 1], [1, 3, 200, 0, 1, 1], [1, 4, 300, 0, 1, 1]]
    pred = [[1, 1, 0, 0, 1, 1], [1, 2, 100, 0, 0.999, 1], [1, 3, 200, 0, 0.1500001, 1], [1, 4, 300, 0, 0.1499999, 1]]
    return {'thr': gt}, {'thr': pred}


def _chains(specs):
    """Chains of heavily overlapping objects (width 20, 8 px apart) with the predictions shifted by 5 px: a gt's best
    prediction is also its neighbour's best, and a prediction's best gt is also its neighbour's, so neither the row
    maxima nor the column maxima form an assignment and only the augmenting-path search finds the optimum.
    specs: video -> (chains, gt positions of a chain, prediction positions of a chain, frames, seed)."""
    out_g, out_p = {}, {}
    for name, (chains, gpos, ppos, frames, seed) in specs.items():
        rng = np.random.RandomState(seed)
        length = max(max(gpos), max(ppos)) + 1
        gt, pred = [], []
        for f in range(1, frames + 1):
            for c in range(chains):
                for k in range(length):
                    i = c * length + k
                    g = np.array([8.0 * k + 0.5 * f, 60.0 * c, 20.0, 20.0])
                    p = g + np.array([5.0, 0.0, 0.0, 0.0]) + rng.normal(0, 0.3, 4)
                    if k in gpos:
                        gt.append([f, 1 + i, *g.astype(np.float32).astype(np.float64)])
                    if k in ppos:
                        pred.append([f, 501 + i, *p.astype(np.float32).astype(np.float64)])
        out_g[name], out_p[name] = gt, pred
    return out_g, out_p


def contested():
    """'clusters': four chains of four; 'long_chain': one chain of 70 (more columns than a wave has lanes)."""
    return _chains(dict(clusters=(4, range(4), range(4), 6, 11), long_chain=(1, range(70), range(70), 3, 12)))


def contested_shapes():
    """The search (not the maxima bound) at 63 / 64 / 65 columns, rectangular in each direction with more than 64
    columns on the long side, and near the per-frame limit (four columns per lane)."""
    return _chains(dict(c63=(1, range(63), range(63), 2, 13), c64=(1, range(64), range(64), 2, 14),
                        c65=(1, range(65), range(65), 2, 15), r65x40=(1, range(65), range(25, 65), 2, 16),
                        r40x65=(1, range(40), range(65), 2, 17), c250=(1, range(250), range(250), 1, 18)))


SCENARIOS = dict(contested=contested, contested_shapes=contested_shapes, random_b1=random_b1, random_b3=random_b3, wave_sizes=wave_sizes, at_limit=at_limit,
                 clear_continuity=clear_continuity, empty_kinds=empty_kinds, thresholds=thresholds)


@functools.lru_cache(maxsize=None)
def scenario(name):
    return SCENARIOS[name]()


def host_scores(gt_by_video, pred_by_video, iou_thr=0.5):
    from stereotracking_amd import metrics as M
    return {v: dict(clear_identity=M.clear_identity(gt_by_video.get(v, []), pred_by_video.get(v, []), iou_thr),
                    hota=M.hota(gt_by_video.get(v, []), pred_by_video.get(v, [])))
            for v in sorted(set(gt_by_video) | set(pred_by_video))}


@functools.lru_cache(maxsize=None)
def host_reference(name):
    """The host backend's scores of a scenario, computed once and shared (treat as read-only)."""
    return host_scores(*scenario(name))


def assert_same_scores(got, ref, float_tol, where=''):
    """Integers equal, floats within float_tol * max(1, |ref|); got / ref: dict(clear_identity=..., hota=...)."""
    c, rc = got['clear_identity'], ref['clear_identity']
    assert set(c) == set(rc), (where, set(c) ^ set(rc))
    for k in INT_KEYS:
        assert c[k] == rc[k], (where, k, c[k], rc[k])
    for k in FLOAT_KEYS:
        assert abs(c[k] - rc[k]) <= float_tol * max(1.0, abs(rc[k])), (where, k, c[k], rc[k])
    h, rh = got['hota'], ref['hota']
    if rh is None or h is None:
        assert h is None and rh is None, where
        return
    assert set(h) == set(rh), (where, set(h) ^ set(rh))
    for k in HOTA_INT_KEYS:
        assert np.array_equal(h[k], rh[k]), (where, k, h[k], rh[k])
    for k in HOTA_FLOAT_KEYS:
        assert h[k].shape == rh[k].shape
        assert np.all(np.abs(h[k] - rh[k]) <= float_tol * np.maximum(1.0, np.abs(rh[k]))), (where, k, h[k], rh[k])


def shuffled_and_relabelled(rows, seed):
    """The rows in a random order with every id relabelled in reverse order (permutes every matrix scipy sees)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6).copy()
    if len(rows) == 0:
        return rows
    ids = rows[:, 1].astype(np.int64)
    rows[:, 1] = ids.max() + ids.min() - ids
    return rows[np.random.RandomState(seed).permutation(len(rows))]


def detection_stream_with_gt(seed=51, T=24, K=6):
    """stereotracking_amd.synthetic.synthetic_detection_stream and the ground truth behind it: the generator's
    random draws replayed, so that every object's true box of every frame (dropped and occluded ones included) is
    known.  The stream's boxes are DEPTH-SCALED (what the tracker consumes, scale = clip(depth^2 / 400, 1, 3), up to
    3 here); the ground truth is in IMAGE space, as MOTDroneMetrics collects it: the true box scaled back about its
    centre by the object's true scale.  -> (stream rows, gt rows (frame, object, x, y, w, h) with fp32-valued boxes)."""
    from stereotracking_amd.synthetic import synthetic_detection_stream
    occlusion = (3, 20, 28)
    stream = synthetic_detection_stream(seed=seed, T=T, K=K, occlusion=occlusion)
    rng = np.random.RandomState(seed)
    pos = rng.uniform([100, 80], [1100, 600], (K, 2))
    vel = rng.uniform(-4, 4, (K, 2))
    size = rng.uniform(12, 50, (K, 2))
    depth = rng.uniform(5, 60, K)
    rng.uniform(0.35, 0.95, K)
    scale = np.clip(depth * depth / 400.0, 1.0, 3.0)
    assert scale.max() > 2.0 and scale.min() < 1.5
    gt, kept = [], 0
    for t in range(T):
        rng.normal(0, 0.4, (K, 2))
        keep = (rng.uniform(size=K) > 0.1) | (t == 0)
        keep[occlusion[0]] &= not (occlusion[1] <= t < occlusion[2])
        n = int(keep.sum())
        rng.normal(0, 0.02, n)
        rng.normal(0, 0.2, n)
        kept += n
        c = pos + vel * t
        wh = size / scale[:, None]
        b = np.concatenate([c - wh / 2, wh], 1).astype(np.float32).astype(np.float64)
        gt += [[t, 100 + k, *b[k]] for k in range(K)]
    assert kept == len(stream), 'the replay of synthetic_detection_stream went out of step'
    return stream, np.asarray(gt)


def thinned_streams(stream, T):
    """Four different drops of one detection stream, as per-frame detection arrays (None: the sequence has no frame in
    that step): 0 the stream itself, 1 a fifth of the detections dropped, 2 lacks frame 10, 3 drops a third and ends
    after frame 17."""
    out = []
    for b, (drop, missing, end) in enumerate(((0.0, (), T), (0.2, (), T), (0.05, (10,), T), (0.33, (), 18))):
        rng = np.random.RandomState(70 + b)
        frames = []
        for t in range(T):
            d = stream[stream[:, 0] == t]
            d = d[rng.uniform(size=len(d)) >= drop]
            frames.append(None if (t in missing or t >= end) else d)
        out.append(frames)
    return out
