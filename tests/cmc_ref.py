"""TEST INFRASTRUCTURE: numpy restatement of the Mesh-Affine camera-motion estimate (csrc/cmc_flow.hip).

Reference: mmtrack/models/trackers/utils.py:6-55 (GLME_affine) on top of cv2.resize / cvtColor / equalizeHist /
calcOpticalFlowFarneback / estimateAffinePartial2D.  OpenCV is absent: the rules are restated from the published
algorithms [upstream-memory]; the module header of csrc/cmc_flow.hip lists them, and DESIGN.md ("Camera-motion
compensation") says what is restated, what deviates (the deterministic consensus fit in place of RANSAC) and what stays
unpinned.  The float stages run in `dtype` (np.float32 or np.float64) so that a GPU result can be held to the float64
restatement relative to the float32 restatement's own distance.  Nothing under stereotracking_amd/ imports this.
"""
import numpy as np

SIDE = 255


# ---- front (integer: bit-exact) ------------------------------------------------------------------------------------
def _taps_u8(n_dst, n_src, zero_at_border):
    scale = np.float64(n_src) / np.float64(n_dst)
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if zero_at_border:
        lo, hi = s < 0, s >= n_src - 1
        f = np.where(lo | hi, np.float32(0), f)
        s = np.where(lo, 0, np.where(hi, n_src - 1, s))
    a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    a1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s, a0, a1


def resize_u8(img, h2, w2):
    """uint8 (h, w, c) -> (h2, w2, c), cv2 8-bit INTER_LINEAR (11-bit taps; the exact 2x2 decimation never occurs at 255)."""
    h, w = img.shape[:2]
    x = img.astype(np.int64)
    sx, ax0, ax1 = _taps_u8(w2, w, True)
    sy, b0, b1 = _taps_u8(h2, h, False)
    x1 = np.minimum(sx + 1, w - 1)
    H = x[:, sx] * ax0[None, :, None] + x[:, x1] * ax1[None, :, None]
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    v = (((b0[:, None, None] * (H[y0] >> 4)) >> 16) + ((b1[:, None, None] * (H[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def rgb2gray(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    return ((r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15).astype(np.uint8)


def equalize_hist(g):
    hist = np.bincount(g.ravel(), minlength=256)
    i0 = int(np.nonzero(hist)[0][0])
    total = g.size
    if hist[i0] == total:
        return np.full_like(g, i0)
    scale = np.float32(255.0) / np.float32(total - hist[i0])
    lut = np.zeros(256, np.uint8)
    csum = np.cumsum(hist[i0 + 1:]).astype(np.float32)
    lut[i0 + 1:] = np.clip(np.rint(csum * scale), 0, 255).astype(np.uint8)
    return lut[g]


def front(img_bgr_chw, h, w):
    """One frame as the tracker receives it ((3, H, W) BGR, uint8 or integral float) -> equalised 255 x 255 grey."""
    x = np.asarray(img_bgr_chw)
    x = np.clip(x, 0, 255).astype(np.uint8) if x.dtype != np.uint8 else x
    hwc = np.transpose(x[:3, :h, :w], (1, 2, 0))[:, :, ::-1]      # crop, HWC, BGR -> RGB
    return equalize_hist(rgb2gray(resize_u8(np.ascontiguousarray(hwc), SIDE, SIDE)))


# ---- Farneback --------------------------------------------------------------------------------------------------------
def levels():
    """[(side, ksize, kernel)] finest first: 255 * 0.5^k >= 32, each blurred from full resolution."""
    out, k, scale = [], 0, 1.0
    while k <= 5:
        if k > 0:
            scale *= 0.5
            if SIDE * scale < 32:
                break
        sigma = (1.0 / scale - 1.0) * 0.5
        ks = max(int(np.rint(sigma * 5)) | 1, 3)
        if sigma <= 0 and ks == 3:
            kern = np.array([0.25, 0.5, 0.25], np.float32)
        else:
            x = np.arange(ks) - (ks - 1) * 0.5
            t = np.exp(-x * x / (2 * sigma * sigma))
            kern = (t / t.sum()).astype(np.float32)
        out.append((int(np.rint(SIDE * scale)), ks, kern))
        k += 1
    return out


def poly_gauss(n=5, sigma=1.2):
    x = np.arange(-n, n + 1)
    g = np.exp(-x * x / (2 * sigma * sigma)).astype(np.float32)
    g = (g.astype(np.float64) / g.astype(np.float64).sum()).astype(np.float32)
    xg, xxg = (x * g).astype(np.float32), (x * x * g).astype(np.float32)
    gd = g.astype(np.float64)
    G = np.zeros((6, 6))
    yy, xx = np.meshgrid(x, x, indexing='ij')
    w2 = gd[:, None] * gd[None, :]
    G[0, 0] = w2.sum()
    G[1, 1] = (w2 * xx * xx).sum()
    G[3, 3] = (w2 * xx ** 4).sum()
    G[5, 5] = (w2 * xx * xx * yy * yy).sum()
    G[2, 2] = G[0, 3] = G[0, 4] = G[3, 0] = G[4, 0] = G[1, 1]
    G[4, 4] = G[3, 3]
    G[3, 4] = G[4, 3] = G[5, 5]
    iG = np.linalg.inv(G)
    return g[n:], xg[n:], xxg[n:], iG[1, 1], iG[0, 3], iG[3, 3], iG[5, 5]


def _sep_blur(img, kern, dt):
    r = len(kern) // 2
    k = kern.astype(dt)
    p = np.pad(img, ((0, 0), (r, r)), mode='reflect')
    h = sum(k[i] * p[:, i:i + img.shape[1]] for i in range(len(k)))
    p = np.pad(h, ((r, r), (0, 0)), mode='reflect')
    return sum(k[j] * p[j:j + img.shape[0]] for j in range(len(k))).astype(dt)


def _ftaps(n_dst, n_src, dt):
    scale = np.float64(n_src) / np.float64(n_dst)
    d = np.arange(n_dst, dtype=np.float64)
    fx = ((d + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int64)
    fx = (fx - sx).astype(dt)
    fy = fx.copy()
    lo, hi = sx < 0, sx >= n_src - 1
    fxz = np.where(lo | hi, dt(0), fx)
    sxz = np.where(lo, 0, np.where(hi, n_src - 1, sx))
    return sxz, fxz, sx, fy


def resize_f(a, h2, w2, dt):
    """float INTER_LINEAR (h, w[, c]) -> (h2, w2[, c]): columns zero the fraction at the border, rows clamp the index."""
    h, w = a.shape[:2]
    sx, fx, _, _ = _ftaps(w2, w, dt)
    _, _, sy, fy = _ftaps(h2, h, dt)
    x1 = np.minimum(sx + 1, w - 1)
    fxb = fx[:, None] if a.ndim > 2 else fx
    H = a[:, sx] * (1 - fxb) + a[:, x1] * fxb
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    fyb = fy[:, None, None] if a.ndim > 2 else fy[:, None]
    return (H[y0] * (1 - fyb) + H[y1] * fyb).astype(dt)


def poly_exp(I, dt):
    g, xg, xxg, ig11, ig03, ig33, ig55 = poly_gauss()
    g, xg, xxg = g.astype(dt), xg.astype(dt), xxg.astype(dt)
    n = 5
    h, w = I.shape
    P = np.pad(I, ((n, n), (0, 0)), mode='edge')
    v0 = I * g[0]
    v1 = np.zeros_like(I)
    v2 = np.zeros_like(I)
    for k in range(1, n + 1):
        a, b = P[n - k:n - k + h], P[n + k:n + k + h]
        v0 = v0 + g[k] * (a + b)
        v1 = v1 + xg[k] * (b - a)
        v2 = v2 + xxg[k] * (a + b)
    pv = [np.pad(v, ((0, 0), (n, n)), mode='edge') for v in (v0, v1, v2)]
    b1 = v0 * g[0]
    b3 = v1 * g[0]
    b5 = v2 * g[0]
    b2 = np.zeros_like(I)
    b4 = np.zeros_like(I)
    b6 = np.zeros_like(I)
    for k in range(1, n + 1):
        L = [p[:, n - k:n - k + w] for p in pv]
        R = [p[:, n + k:n + k + w] for p in pv]
        b1 = b1 + (R[0] + L[0]) * g[k]
        b4 = b4 + (R[0] + L[0]) * xxg[k]
        b2 = b2 + (R[0] - L[0]) * xg[k]
        b3 = b3 + (R[1] + L[1]) * g[k]
        b6 = b6 + (R[1] - L[1]) * xg[k]
        b5 = b5 + (R[2] + L[2]) * g[k]
    c = lambda v: dt(v)  # noqa: E731
    return np.stack([b3 * c(ig11), b2 * c(ig11), b1 * c(ig03) + b5 * c(ig33), b1 * c(ig03) + b4 * c(ig33),
                     b6 * c(ig55)], -1).astype(dt)


def update_matrices(R0, R1, flow, dt):
    h, w = flow.shape[:2]
    dx, dy = flow[..., 0], flow[..., 1]
    yy, xx = np.mgrid[0:h, 0:w]
    fx, fy = (xx + dx).astype(dt), (yy + dy).astype(dt)
    x1, y1 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    fx, fy = (fx - x1).astype(dt), (fy - y1).astype(dt)
    inside = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
    xc, yc = np.clip(x1, 0, w - 2), np.clip(y1, 0, h - 2)
    a00, a01, a10, a11 = (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy
    smp = (a00[..., None] * R1[yc, xc] + a01[..., None] * R1[yc, xc + 1] + a10[..., None] * R1[yc + 1, xc] +
           a11[..., None] * R1[yc + 1, xc + 1])
    r2 = np.where(inside, smp[..., 0], 0)
    r3 = np.where(inside, smp[..., 1], 0)
    r4 = np.where(inside, (R0[..., 2] + smp[..., 2]) * dt(0.5), R0[..., 2])
    r5 = np.where(inside, (R0[..., 3] + smp[..., 3]) * dt(0.5), R0[..., 3])
    r6 = np.where(inside, (R0[..., 4] + smp[..., 4]) * dt(0.25), R0[..., 4] * dt(0.5))
    r2 = (R0[..., 0] - r2) * dt(0.5)
    r3 = (R0[..., 1] - r3) * dt(0.5)
    r2 = r2 + (r4 * dy + r6 * dx)
    r3 = r3 + (r6 * dy + r5 * dx)
    bw = np.array([0.14, 0.14, 0.4472, 0.4472, 0.4472], np.float32).astype(dt)

    def side(n):
        s = np.ones(n, dt)
        s[:5] = bw
        s[n - 5:] *= bw[::-1]
        return s
    sc = side(h)[:, None] * side(w)[None, :]
    r2, r3, r4, r5, r6 = (v * sc for v in (r2, r3, r4, r5, r6))
    return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3],
                    -1).astype(dt)


def box_solve(M, m, dt, reverse=False):
    """reverse: the box sums accumulated from the far end (the same sums in another rounding order)."""
    h, w = M.shape[:2]
    order = range(2 * m, -1, -1) if reverse else range(2 * m + 1)
    P = np.pad(M, ((m, m), (0, 0), (0, 0)), mode='edge')
    V = sum(P[d:d + h] for d in order)
    P = np.pad(V, ((0, 0), (m, m), (0, 0)), mode='edge')
    S = sum(P[:, d:d + w] for d in order).astype(dt)
    S = S * dt(1.0 / ((2 * m + 1) ** 2))
    g11, g12, g22, h1, h2 = (S[..., i] for i in range(5))
    idet = dt(1) / (g11 * g22 - g12 * g12 + dt(1e-3))
    return np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], -1).astype(dt)


def farneback(prev, curr, winsize=31, dtype=np.float64, per_level=False, reverse_box=False):
    """Dense flow prev -> curr (uint8 255 x 255 planes) -> (255, 255, 2) in dtype (per_level: every level, finest first)."""
    dt = np.dtype(dtype).type
    lv = levels()
    R = []
    for side, ks, kern in lv:
        R.append([poly_exp(resize_f(_sep_blur(im.astype(dt), kern, dt), side, side, dt), dt) for im in (prev, curr)])
    flow, out = None, []
    m = winsize // 2
    for k in range(len(lv) - 1, -1, -1):
        side = lv[k][0]
        if flow is None:
            flow = np.zeros((side, side, 2), dt)
        else:
            flow = (resize_f(flow, side, side, dt) * dt(2.0)).astype(dt)
        M = update_matrices(R[k][0], R[k][1], flow, dt)
        for it in range(3):
            flow = box_solve(M, m, dt, reverse_box)
            if it < 2:
                M = update_matrices(R[k][0], R[k][1], flow, dt)
        out.insert(0, flow)
    return out if per_level else flow


# ---- mesh + deterministic consensus fit -----------------------------------------------------------------------------------
def mesh(flow, img_h, img_w, step=16):
    """-> src, dst (P, 2) float32 (cell centres in (img_h, img_w) crop coordinates; dst = centre + median flow)."""
    sfx, sfy = img_w / SIDE, img_h / SIDE
    f = np.asarray(flow, np.float32) * np.array([sfx, sfy])          # float64, as the reference
    gh = gw = SIDE // step
    cells = f[:gh * step, :gw * step].reshape(gh, step, gw, step, 2)
    med = np.median(cells, axis=(1, 3)).reshape(-1, 2)
    ys, xs = np.mgrid[0:gh, 0:gw]
    src = np.stack([(xs + 0.5) * step * sfx, (ys + 0.5) * step * sfy], -1).reshape(-1, 2).astype(np.float32)
    return src, (src + med).astype(np.float32)


def consensus_fit(src, dst, thr=5.0, min_ratio=0.3, dtype=np.float32, with_winner=False):
    """Every two-point similarity (i < j), largest inlier set (squared residual <= thr^2; ties: lowest (i, j)), linear
    least-squares refit of [a -b tx; b a ty] over it.  -> (warp (2, 3) float32 or None, ratio, inliers bool (P,));
    with_winner: also the winning hypothesis (i, j, its residuals in dtype), None when no hypothesis is usable."""
    dt = np.dtype(dtype).type
    p, q = src.astype(dt), dst.astype(dt)
    P = len(p)
    i, j = np.triu_indices(P, 1)
    dp, dq = p[j] - p[i], q[j] - q[i]
    den = dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1]
    ok = den > 0
    den = np.where(ok, den, dt(1))
    a = (dq[:, 0] * dp[:, 0] + dq[:, 1] * dp[:, 1]) / den
    b = (dq[:, 1] * dp[:, 0] - dq[:, 0] * dp[:, 1]) / den
    tx = q[i, 0] - (a * p[i, 0] - b * p[i, 1])
    ty = q[i, 1] - (b * p[i, 0] + a * p[i, 1])
    thr2 = dt(thr) * dt(thr)
    counts = np.zeros(len(i), np.int64)
    for s in range(0, len(i), 4096):
        sl = slice(s, s + 4096)
        ex = a[sl, None] * p[None, :, 0] - b[sl, None] * p[None, :, 1] + tx[sl, None] - q[None, :, 0]
        ey = b[sl, None] * p[None, :, 0] + a[sl, None] * p[None, :, 1] + ty[sl, None] - q[None, :, 1]
        counts[sl] = ((ex * ex + ey * ey) <= thr2).sum(1)
    counts[~ok] = 0
    h = int(np.argmax(counts))
    if counts[h] == 0:
        res = (None, 0.0, np.zeros(P, bool))
        return res + (None,) if with_winner else res
    ex = a[h] * p[:, 0] - b[h] * p[:, 1] + tx[h] - q[:, 0]
    ey = b[h] * p[:, 0] + a[h] * p[:, 1] + ty[h] - q[:, 1]
    inl = (ex * ex + ey * ey) <= thr2
    warp = lsq_similarity(src[inl], dst[inl])
    ratio = float(inl.sum()) / P
    res = ((warp if ratio >= min_ratio else None), ratio, inl)
    return res + ((int(i[h]), int(j[h]), np.sqrt(ex * ex + ey * ey)),) if with_winner else res


def lsq_similarity(src, dst):
    p, q = src.astype(np.float64), dst.astype(np.float64)
    pc, qc = p.mean(0), q.mean(0)
    u, v = p - pc, q - qc
    sxx = (u * u).sum()
    a = (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]).sum() / sxx
    b = (u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]).sum() / sxx
    tx, ty = qc[0] - (a * pc[0] - b * pc[1]), qc[1] - (b * pc[0] + a * pc[1])
    return np.array([[a, -b, tx], [b, a, ty]], np.float32)


def residuals(src, dst, warp):
    """|warp(src) - dst| per point (float64)."""
    w = np.asarray(warp, np.float64)
    pr = src.astype(np.float64) @ w[:, :2].T + w[:, 2]
    return np.sqrt(((pr - dst.astype(np.float64)) ** 2).sum(1))


def estimate(prev_plane, curr_plane, img_h, img_w, step=16, winsize=31, ransac_thr=5.0, min_inlier_ratio=0.3,
             dtype=np.float32):
    """The whole estimate from two grey planes -> (warp or None, ratio, src, dst, inliers)."""
    flow = farneback(prev_plane, curr_plane, winsize, dtype)
    src, dst = mesh(flow, img_h, img_w, step)
    warp, ratio, inl = consensus_fit(src, dst, ransac_thr, min_inlier_ratio, np.float32)
    return warp, ratio, src, dst, inl


# ---- test scenes ------------------------------------------------------------------------------------------------------------
def texture(h, w, seed=0, cutoff=0.08):
    """Band-limited random texture in [0, 1] (float64), periodic: a low-pass of white noise in the Fourier domain."""
    rng = np.random.default_rng(seed)
    F = np.fft.fft2(rng.standard_normal((h, w)))
    fy = np.fft.fftfreq(h)[:, None]
    fx = np.fft.fftfreq(w)[None, :]
    F *= np.exp(-(fx * fx + fy * fy) / (2 * cutoff * cutoff))
    t = np.real(np.fft.ifft2(F))
    return (t - t.min()) / (t.max() - t.min())


def warp_texture(h, w, A, seed=0, cutoff=0.08):
    """Frame whose pixel (x, y) shows the texture at A^-1 (x, y): the texture moved BY the similarity A (2 x 3), sampled
    exactly from its Fourier series (no interpolation error) -> uint8 (h, w)."""
    rng = np.random.default_rng(seed)
    nb = 200
    k = rng.normal(0, cutoff, (nb, 2))
    ph = rng.uniform(0, 2 * np.pi, nb)
    amp = np.exp(-0.5 * ((k ** 2).sum(1) / (cutoff ** 2)))
    A = np.asarray(A, np.float64)
    Ai = np.linalg.inv(np.vstack([A, [0, 0, 1]]))[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    sx = Ai[0, 0] * xx + Ai[0, 1] * yy + Ai[0, 2]
    sy = Ai[1, 0] * xx + Ai[1, 1] * yy + Ai[1, 2]
    v = np.zeros((h, w))
    for b in range(nb):
        v += amp[b] * np.cos(2 * np.pi * (k[b, 0] * sx + k[b, 1] * sy) + ph[b])
    v = v / (3 * np.sqrt((amp ** 2).sum() / 2)) * 100 + 128
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def similarity(tx=0.0, ty=0.0, deg=0.0, scale=1.0, cx=0.0, cy=0.0):
    """2 x 3 similarity: rotate by `deg` and scale about (cx, cy), then translate by (tx, ty)."""
    c, s = scale * np.cos(np.deg2rad(deg)), scale * np.sin(np.deg2rad(deg))
    R = np.array([[c, -s], [s, c]])
    t = np.array([cx, cy]) - R @ np.array([cx, cy]) + np.array([tx, ty])
    return np.hstack([R, t[:, None]])
