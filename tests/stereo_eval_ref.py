"""The dense stereo evaluator's definitions in numpy, operation by operation (a helper module, not a test file).

csrc/stereo_eval.hip is held to this file: `counts` and `hist` equal, `sums` up to the order of summation.  Every
per-pixel value is a numpy float32 formed by ONE float32 operation at a time (numpy rounds each to float32, as the
kernel's unfused IEEE operations do), every term of the sums a float64 formed from those float32 values.

  ground truth   depth: gz = g, gd = bf / gz        disp: gd = g, gz = bf / gd
                 valid iff g finite, g > 0, E_0 < gz <= E_K;   depth bin b: E_b < gz <= E_{b+1}
  prediction     valid iff p finite, p > 0;   pz = bf / p
  region         1 iff some box row r < count has x1 <= float(x) < x2 and y1 <= float(y) < y2, else 0
  both valid     e = |p - gd|;  bad_t: e > tau_t;  d1: e > 3 and e > 0.05f * gd;  r = max(pz / gz, gz / pz);
                 delta_k: r < 1.25^k;  histogram bin: 511 if e * 16 >= 511 else int(e * 16);  dz = f64(pz) - f64(gz)
  cell (n, region, bin)   counts = n_gt, n_both, n_bad[T], n_d1, n_delta[3]     sums = e, e^2, |dz| / gz, dz^2 / gz, dz^2
"""
import numpy as np

HIST_BINS = 512
NUM_SUMS = 5
F = np.float32


def accumulate(pred, gt, gt_kind, bf, extent=None, boxes=None, box_counts=None, depth_edges=(0, 20, 40, 80),
               bad_thresholds=(0.5, 1, 2, 3)):
    """pred (N, C, H, W) / gt (N, Cg, H, W) float32 (plane 0 is read) -> counts (N, 2, K, T + 6) int64,
    sums (N, 2, K, 5) float64, hist (N, 2, K, 512) int64."""
    pred, gt = np.asarray(pred, F), np.asarray(gt, F)
    N, _, H, W = pred.shape
    edges = np.asarray(depth_edges, F)
    taus = np.asarray(bad_thresholds, F)
    K, T = len(edges) - 1, len(taus)
    bf = F(bf)
    counts = np.zeros((N, 2, K, T + 6), np.int64)
    sums = np.zeros((N, 2, K, NUM_SUMS), np.float64)
    hist = np.zeros((N, 2, K, HIST_BINS), np.int64)
    for n in range(N):
        hn, wn = (H, W) if extent is None else (int(extent[n][0]), int(extent[n][1]))
        p, g = pred[n, 0, :hn, :wn], gt[n, 0, :hn, :wn]
        with np.errstate(all='ignore'):
            if gt_kind == 'depth':
                gz = g
                gd = bf / gz
            elif gt_kind == 'disp':
                gd = g
                gz = bf / gd
            else:
                raise ValueError(gt_kind)
            gt_valid = np.isfinite(g) & (g > 0) & (edges[0] < gz) & (gz <= edges[K])
            b = np.zeros(g.shape, np.int64)
            for k in range(1, K):
                b += gz > edges[k]
            region = np.zeros(g.shape, np.int64)
            if boxes is not None:
                ys, xs = np.meshgrid(np.arange(hn).astype(F), np.arange(wn).astype(F), indexing='ij')
                for r in range(int(box_counts[n])):
                    x1, y1, x2, y2 = (F(v) for v in boxes[n][r])
                    region |= ((x1 <= xs) & (xs < x2) & (y1 <= ys) & (ys < y2)).astype(np.int64)
            pred_valid = np.isfinite(p) & (p > 0)
            both = gt_valid & pred_valid
            pz = bf / p
            e = np.abs(p - gd)
            flags = [gt_valid, both] + [both & (e > t) for t in taus]
            flags.append(both & (e > F(3.0)) & (e > F(0.05) * gd))
            r = np.maximum(pz / gz, gz / pz)
            flags += [both & (r < F(c)) for c in (1.25, 1.5625, 1.953125)]
            e16 = e * F(16.0)
            hbin = np.where(e16 >= F(HIST_BINS - 1), HIST_BINS - 1, np.where(both, e16, 0).astype(np.int64))
            ed, gzd = e.astype(np.float64), gz.astype(np.float64)
            dz = pz.astype(np.float64) - gzd
            terms = [ed, ed * ed, np.abs(dz) / gzd, dz * dz / gzd, dz * dz]
        cell = (region * K + b).ravel()
        for j, f in enumerate(flags):
            counts[n].reshape(2 * K, -1)[:, j] = np.bincount(cell[f.ravel()], minlength=2 * K)
        bm = both.ravel()
        for j, t in enumerate(terms):
            sums[n].reshape(2 * K, -1)[:, j] = np.bincount(cell[bm], weights=t.ravel()[bm], minlength=2 * K)
        hist[n] = np.bincount(cell[bm] * HIST_BINS + hbin.ravel()[bm], minlength=2 * K * HIST_BINS).reshape(2, K, HIST_BINS)
    return counts, sums, hist


def _div(a, b):
    return float(a) / float(b) if b else float('nan')


def summarize(counts, sums, hist, bad_thresholds=(0.5, 1, 2, 3), invalid='skip'):
    """One cell's (already added) accumulators -> the summary dict: counts (T + 6,), sums (5,), hist (512,)."""
    counts, sums, hist = np.asarray(counts), np.asarray(sums), np.asarray(hist)
    T = len(bad_thresholds)
    n_gt, n_both = int(counts[0]), int(counts[1])
    out = dict(n_gt=n_gt, n_both=n_both, EPE=_div(sums[0], n_both),
               RMSE=float(np.sqrt(_div(sums[1], n_both))), density=_div(n_both, n_gt))

    def rate(k):
        if invalid == 'skip':
            return _div(int(k), n_both)
        if invalid == 'bad':
            return _div(int(k) + n_gt - n_both, n_gt)
        raise ValueError(invalid)
    for t, tau in enumerate(bad_thresholds):
        out['bad_%g' % tau] = rate(counts[2 + t])
    out['D1'] = rate(counts[2 + T])
    cum = np.cumsum(hist)
    for name, q in (('A50', 0.5), ('A90', 0.9), ('A99', 0.99)):
        if n_both == 0:
            out[name] = float('nan')
        else:
            need = int(np.ceil(q * n_both))
            out[name] = (int(np.argmax(cum >= need)) + 1) / 16.0
    out['abs_rel'] = _div(sums[2], n_both)
    out['sq_rel'] = _div(sums[3], n_both)
    out['depth_rmse'] = float(np.sqrt(_div(sums[4], n_both)))
    for k in range(3):
        out['delta%d' % (k + 1)] = _div(int(counts[3 + T + k]), n_both)
    return out


# ---- the inputs the CPU and the GPU tests share -------------------------------------------------------------------------
BF = 160.0        # 0.25 m x 640 px, exact in float32


def _up(v):
    return float(np.nextafter(F(v), F(np.inf)))


def boundary_pixels():
    """[(name, p, g)] for gt_kind='depth', bf = BF, the default edges and thresholds: every boundary of the definitions,
    placed so that gd = BF / g is exact (g = 20 -> 8 px, 16 -> 10 px, 2 -> 80 px, 80 -> 2 px, 40 -> 4 px)."""
    nan, inf = float('nan'), float('inf')
    return [
        ('e==0.5', 8.5, 20.0), ('e==1', 9.0, 20.0), ('e==2', 10.0, 20.0), ('e==3', 11.0, 20.0),
        ('e>3,rel<e', _up(11.0), 20.0),                      # 0.05f * 8 = 0.4 < e: D1
        ('e==3.5,rel>e', 83.5, 2.0),                         # 0.05f * 80 = 4 > e: bad_3, not D1
        ('e==4==rel', 84.0, 2.0),                            # e == 0.05f * gd: not D1
        ('e==5,rel<e', 85.0, 2.0),
        ('gz==20', 8.0, 20.0), ('gz>20', 8.0, _up(20.0)),    # bin 0 / bin 1
        ('gz==40', 4.0, 40.0), ('gz>40', 4.0, _up(40.0)),
        ('gz==80', 2.0, 80.0), ('gz>80', 2.0, _up(80.0)),    # valid / gt-invalid
        ('r==1.25', 8.0, 16.0),                              # pz = 20, gz = 16: not delta1
        ('r==1.5625', 6.4, 16.0), ('r<1.25', 10.0, 16.0),
        ('p==0', 0.0, 20.0), ('p==-1', -1.0, 20.0), ('p==nan', nan, 20.0), ('p==inf', inf, 20.0),
        ('g==0', 8.0, 0.0), ('g==nan', 8.0, nan), ('g==inf', 8.0, inf), ('g<0', 8.0, -5.0),
        ('e==31.875', 39.875, 20.0), ('e==31.9375', 39.9375, 20.0), ('e==32', 40.0, 20.0), ('e==500', 508.0, 20.0),
    ]


def seeded_maps(seed, N, C, Cg, H, W, gt_kind='depth', bf=BF, z_hi=100.0):
    """Seeded (pred (N, C, H, W), gt (N, Cg, H, W)) float32: depths in (0.3, z_hi), a third of the errors exact multiples of
    1/16 px (so that e == tau happens), 4 % invalid pixels of every kind on either side, NaN in every plane but 0, and
    the boundary pixels above at the start of frame 0 (as far as they fit; gt_kind='disp' stores BF / g)."""
    rng = np.random.RandomState(seed)
    z = rng.uniform(0.3, z_hi, (N, H, W)).astype(F)
    gd = (F(bf) / z).astype(F)
    gd_q = (np.rint(gd * 16) / 16).astype(F)
    pick = rng.rand(N, H, W) < 0.33
    gd = np.where(pick & (gd_q > 0), gd_q, gd)
    z = np.where(pick & (gd_q > 0), F(bf) / gd, z).astype(F)
    err = np.where(rng.rand(N, H, W) < 0.5, rng.randint(-64, 65, (N, H, W)) / 16.0, rng.normal(0, 4.0, (N, H, W)))
    p = (gd + err.astype(F)).astype(F)
    g = (z if gt_kind == 'depth' else gd).astype(F)
    bad = (float('nan'), float('inf'), 0.0, -1.0)
    for arr in (p, g):
        k = rng.rand(N, H, W)
        for i, v in enumerate(bad):
            arr[(k >= 0.01 * i) & (k < 0.01 * (i + 1))] = v
    flat_p, flat_g = p.reshape(-1), g.reshape(-1)
    for i, (_, bp, bg) in enumerate(boundary_pixels()[:H * W]):
        flat_p[i] = bp
        flat_g[i] = bg if gt_kind == 'depth' or not (np.isfinite(bg) and bg > 0) else float(F(bf) / F(bg))
    pred = np.full((N, C, H, W), np.nan, F)
    gt = np.full((N, Cg, H, W), np.nan, F)
    pred[:, 0], gt[:, 0] = p, g
    return pred, gt


def sum_bound(counts, sums):
    """The tolerance of the fp64 sums, per cell: 2 n_both 2^-53 S, the distance between two summation orders of n_both
    non-negative doubles whose sum is S."""
    return 2.0 * counts[..., 1:2].astype(np.float64) * 2.0 ** -53 * sums
