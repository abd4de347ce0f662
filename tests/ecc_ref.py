"""numpy restatement of the ECC camera-motion estimate (csrc/cmc_ecc.hip) - the executable spec the kernels are held to.

cv2 is absent; the rules are restated from OpenCV 4.x ecc.cpp (findTransformECC) [upstream-memory], PARITY UNPINNED
against cv2 itself.  Every function takes `dt`: np.float64 (everything in float64) or np.float32 (planes and per-pixel
arithmetic in float32 - the device's arithmetic - under float64 sums, solve and warp state).

The rules (T = template plane, I = input plane, fp32 ph x pw; M = 2 x 3 warp, T(x, y) ~ I(M (x, y, 1)), from identity):
  E0  front: crop to img_shape; grey = (R 9798 + G 19235 + B 3735 + 2^14) >> 15 of the BGR frame; s x s box mean
      (s = downscale in {1, 2, 4}) over the top-left floor(h / s) x floor(w / s) blocks -> fp32, a multiple of 1 / s^2:
      exact.  New, not cv2.
  E1  blur of T and I: {1}, {1/4, 1/2, 1/4}, {1/16, 1/4, 3/8, 1/4, 1/16} (cv2's fixed kernels for sigma <= 0),
      separable, BORDER_REFLECT_101.  Dyadic weights on <= 12-bit values: exact in fp32 in any order.
  E2  gx = 0.5 (I[y][x+1] - I[y][x-1]), gy vertically, of the blurred I, REFLECT_101 (border gradient 0).  Exact.
  E3  per template pixel p = (x, y): q = M p, q_x = (m00 x + m01 y) + m02 (likewise q_y), M rounded to `dt`;
      Iw, gxw, gyw = bilinear samples of I, gx, gy at q: x0 = floor(q_x), fx = q_x - x0, ...,
      v = (v00 (1 - fx) + v01 fx) (1 - fy) + (v10 (1 - fx) + v11 fx) fy, taps outside the plane read 0;
      mask m = 1 when (floor(q_x + 0.5), floor(q_y + 0.5)) lies inside the plane.
      DEVIATION (stated): cv2's warpAffine quantises q to 1/32 px and its weights to a table; here plain bilinear.
      SIMPLIFICATION (stated): a pixel with m = 0 contributes to NO sum (cv2 leaves un-centred border values in).
  E4  over the mask: n, means and population standard deviations of Iw and T; Iz = Iw - mean, Tz = T - mean;
      imgNorm = sqrt(n stdI^2), tmpNorm = sqrt(n stdT^2).
  E5  Jacobian row (in `dt`): TRANSLATION (gxw, gyw); EUCLIDEAN, c = m00, s = m10:
      (gxw ((-(x s)) - y c) + gyw (x c - y s), gxw, gyw); AFFINE (gxw x, gyw x, gxw y, gyw y, gxw, gyw).
  E6  H = sum J^T J, iP = sum J^T Iz, tP = sum J^T Tz, corr = sum Tz Iz (products and sums float64);
      rho = corr / (imgNorm tmpNorm).
  E7  a = H^-1 iP, b = H^-1 tP (Cholesky; a pivot that is not > 0 = singular);
      lambda = (imgNorm^2 - iP . a) / (corr - tP . a); dp = lambda b - a  (= H^-1 (lambda tP - iP)).
  E8  TRANSLATION: M02 += dp0, M12 += dp1.  EUCLIDEAN: theta = asin(clamp(M10, -1, 1)) + dp0; M02 += dp1, M12 += dp2;
      M00 = M11 = cos theta, M10 = sin theta, M01 = -M10.  AFFINE: M00, M10, M01, M11, M02, M12 += dp0..dp5.
  E9  rho = -1, last = -stop_eps; for i in 1..num_iters while |rho - last| >= stop_eps: E3-E6, last = rho, rho = new,
      E7, E8.  cv2's test: iteration 1 always runs, the returned rho belongs to the warp BEFORE the last update.
  E10 n = 0, a NaN / infinite rho, a singular H, or a denominator of lambda <= 0 end the estimate with valid = 0
      (cv2 raises there); the row is then [0, 0, identity].
  Precision: sums, solve and warp state float64 (cv2's warp is fp32: stated deviation); output warp fp32.
  Plane -> image: plane pixel i sits at image coordinate s i + c, c = (s - 1) / 2; [A | t] -> [A | s t + c - A c].
"""
import numpy as np

TRANSLATION, EUCLIDEAN, AFFINE = 0, 1, 2
N_PARAMS = {TRANSLATION: 2, EUCLIDEAN: 3, AFFINE: 6}
IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
BLUR = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625]}


# ---- E0 -------------------------------------------------------------------------------------------------------------
def grey(img_bgr_chw, h, w):
    """uint8 (3, fh, fw) frame or padded fp32 canvas (values cast to uint8 as the device does) -> int32 (h, w)."""
    a = np.asarray(img_bgr_chw)[:3, :h, :w]
    if a.dtype != np.uint8:
        a = np.clip(a.astype(np.int32), 0, 255)
    a = a.astype(np.int32)
    return (a[2] * 9798 + a[1] * 19235 + a[0] * 3735 + (1 << 14)) >> 15


def plane_size(h, w, s):
    return h // s, w // s


def front(img_bgr_chw, h, w, s=2):
    g = grey(img_bgr_chw, h, w)
    ph, pw = plane_size(h, w, s)
    box = g[:ph * s, :pw * s].reshape(ph, s, pw, s).sum((1, 3))
    return (box.astype(np.float32) / np.float32(s * s)).astype(np.float32)


# ---- E1, E2 ---------------------------------------------------------------------------------------------------------
def blur(p, size, dt=np.float64):
    k = np.asarray(BLUR[size], dt)
    r = size // 2
    p = np.asarray(p, dt)
    if r == 0:
        return p.copy()
    a = np.pad(p, ((0, 0), (r, r)), mode='reflect')
    h = sum(k[i] * a[:, i:i + p.shape[1]] for i in range(size))
    a = np.pad(h, ((r, r), (0, 0)), mode='reflect')
    return sum(k[i] * a[i:i + p.shape[0], :] for i in range(size)).astype(dt)


def gradients(p, dt=np.float64):
    a = np.pad(np.asarray(p, dt), 1, mode='reflect')
    half = dt(0.5)
    return half * (a[1:-1, 2:] - a[1:-1, :-2]), half * (a[2:, 1:-1] - a[:-2, 1:-1])


def prepare(T, I, size=1, dt=np.float64):
    """-> blurred T, blurred I, gx, gy."""
    Tb, Ib = blur(T, size, dt), blur(I, size, dt)
    gx, gy = gradients(Ib, dt)
    return Tb, Ib, gx, gy


# ---- E3 .. E8: one iteration ----------------------------------------------------------------------------------------
def _sample(planes, qx, qy, dt):
    ph, pw = planes[0].shape
    x0f, y0f = np.floor(qx), np.floor(qy)
    fx, fy = (qx - x0f).astype(dt), (qy - y0f).astype(dt)
    near = (qx >= -1) & (qx < pw) & (qy >= -1) & (qy < ph)          # any tap inside (false for NaN)
    x0 = np.where(near, x0f, -2).astype(np.int64)
    y0 = np.where(near, y0f, -2).astype(np.int64)
    one = dt(1)
    gx1, gy1 = one - fx, one - fy
    out = []
    for P in planes:
        def tap(yy, xx):
            ok = (xx >= 0) & (xx < pw) & (yy >= 0) & (yy < ph)
            return np.where(ok, P[np.clip(yy, 0, ph - 1), np.clip(xx, 0, pw - 1)], dt(0)).astype(dt)
        top = tap(y0, x0) * gx1 + tap(y0, x0 + 1) * fx
        bot = tap(y0 + 1, x0) * gx1 + tap(y0 + 1, x0 + 1) * fx
        out.append((top * gy1 + bot * fy).astype(dt))
    return out


def cholesky_solve(H, rhs):
    """H (K, K) SPD, rhs list of (K,) -> solutions, or None when a pivot is not > 0 (singular)."""
    K = H.shape[0]
    L = np.zeros((K, K))
    for j in range(K):
        d = H[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0 or not np.isfinite(d):
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, K):
            L[i, j] = (H[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    sols = []
    for b in rhs:
        y = np.zeros(K)
        for i in range(K):
            y[i] = (b[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
        x = np.zeros(K)
        for i in range(K - 1, -1, -1):
            x[i] = (y[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
        sols.append(x)
    return sols


def update_warp(M, dp, mode):
    M = np.array(M, np.float64)
    if mode == TRANSLATION:
        M[0, 2] += dp[0]
        M[1, 2] += dp[1]
    elif mode == EUCLIDEAN:
        th = np.arcsin(min(max(M[1, 0], -1.0), 1.0)) + dp[0]
        M[0, 2] += dp[1]
        M[1, 2] += dp[2]
        M[0, 0] = M[1, 1] = np.cos(th)
        M[1, 0] = np.sin(th)
        M[0, 1] = -M[1, 0]
    else:
        M[0, 0] += dp[0]
        M[1, 0] += dp[1]
        M[0, 1] += dp[2]
        M[1, 1] += dp[3]
        M[0, 2] += dp[4]
        M[1, 2] += dp[5]
    return M


def step(Tb, Ib, gx, gy, M, mode=EUCLIDEAN, dt=np.float64):
    """One iteration from the float64 warp M on prepared planes -> dict(valid, n, mean_i, mean_t, std_i, std_t,
    img_norm, tmp_norm, corr, rho, lam, H, iP, tP, dp, warp).  valid False = E10 (later fields may be missing)."""
    K = N_PARAMS[mode]
    ph, pw = Tb.shape
    Tb, Ib, gx, gy = (np.asarray(a, dt) for a in (Tb, Ib, gx, gy))
    M = np.asarray(M, np.float64)
    m = M.astype(dt)
    x = np.arange(pw, dtype=dt)[None, :]
    y = np.arange(ph, dtype=dt)[:, None]
    qx = ((m[0, 0] * x + m[0, 1] * y) + m[0, 2]).astype(dt)
    qy = ((m[1, 0] * x + m[1, 1] * y) + m[1, 2]).astype(dt)
    Iw, gxw, gyw = _sample((Ib, gx, gy), qx, qy, dt)
    half = dt(0.5)
    rx, ry = np.floor(qx + half), np.floor(qy + half)
    mask = (rx >= 0) & (rx <= pw - 1) & (ry >= 0) & (ry <= ph - 1)
    xb, yb = np.broadcast_to(x, (ph, pw)), np.broadcast_to(y, (ph, pw))
    if mode == TRANSLATION:
        J = [gxw, gyw]
    elif mode == EUCLIDEAN:
        c, s = m[0, 0], m[1, 0]
        hx = ((-(xb * s)) - yb * c).astype(dt)
        hy = (xb * c - yb * s).astype(dt)
        J = [(gxw * hx + gyw * hy).astype(dt), gxw, gyw]
    else:
        J = [(gxw * xb).astype(dt), (gyw * xb).astype(dt), (gxw * yb).astype(dt), (gyw * yb).astype(dt), gxw, gyw]
    J = np.stack([j[mask].astype(np.float64) for j in J], 1)           # (n, K)
    iw, t = Iw[mask].astype(np.float64), Tb[mask].astype(np.float64)
    n = int(mask.sum())
    out = dict(valid=False, n=n, warp=M.copy())
    if n == 0:
        return out
    mean_i, mean_t = iw.sum() / n, t.sum() / n
    iz, tz = iw - mean_i, t - mean_t
    std_i, std_t = np.sqrt((iz * iz).sum() / n), np.sqrt((tz * tz).sum() / n)
    img_norm, tmp_norm = np.sqrt(n * std_i * std_i), np.sqrt(n * std_t * std_t)
    H, iP, tP, corr = J.T @ J, J.T @ iz, J.T @ tz, float((tz * iz).sum())
    with np.errstate(all='ignore'):
        rho = corr / (img_norm * tmp_norm)
    out.update(mean_i=mean_i, mean_t=mean_t, std_i=std_i, std_t=std_t, img_norm=img_norm, tmp_norm=tmp_norm, corr=corr,
               rho=rho, H=H, iP=iP, tP=tP)
    if not np.isfinite(rho):
        return out
    sol = cholesky_solve(H, [iP, tP])
    if sol is None:
        return out
    a, b = sol
    den = corr - np.dot(tP, a)
    if not den > 0:
        return out
    lam = (img_norm * img_norm - np.dot(iP, a)) / den
    dp = lam * b - a
    out.update(valid=True, lam=lam, dp=dp, warp=update_warp(M, dp, mode))
    return out


# ---- E9, E10 --------------------------------------------------------------------------------------------------------
def to_image(M, s):
    """Plane warp -> image warp: plane pixel i sits at image coordinate s i + c, c = (s - 1) / 2."""
    M = np.asarray(M, np.float64)
    c = (s - 1) / 2.0
    A = M[:, :2]
    return np.hstack([A, (s * M[:, 2] + c - A @ np.array([c, c]))[:, None]])


def estimate(T, I, mode=EUCLIDEAN, num_iters=50, stop_eps=1e-3, gauss_filt_size=1, dt=np.float64, downscale=1,
             M0=None, trace=False):
    """-> (valid, rho, plane warp float64, iterations run[, per-iteration |rho - last|]).  `iterations` counts the
    failing iteration too.  The device row is [valid, rho, to_image(warp, downscale) as fp32]."""
    Tb, Ib, gx, gy = prepare(T, I, gauss_filt_size, dt)
    M = IDENTITY.copy() if M0 is None else np.array(M0, np.float64)
    rho, last, it, gaps = -1.0, -float(stop_eps), 0, []
    while it < num_iters and abs(rho - last) >= stop_eps:
        it += 1
        r = step(Tb, Ib, gx, gy, M, mode, dt)
        if not r['valid']:
            res = (False, 0.0, IDENTITY.copy(), it)
            return res + (gaps,) if trace else res
        last, rho, M = rho, r['rho'], r['warp']
        gaps.append(abs(rho - last))
    res = (True, rho, M, it)
    return res + (gaps,) if trace else res


def row(valid, rho, M, s):
    """The (8,) fp32 row the device writes."""
    if not valid:
        return np.array([0, 0, 1, 0, 0, 0, 1, 0], np.float32)
    return np.concatenate([[1.0, rho], to_image(M, s).ravel()]).astype(np.float32)


def corner_error(M, A, ph, pw):
    """Largest distance (plane px) between M and A applied to the four plane corners."""
    c = np.array([[0, 0, 1], [pw - 1, 0, 1], [0, ph - 1, 1], [pw - 1, ph - 1, 1]], float)
    return float(np.sqrt((((c @ np.asarray(M, float).T) - (c @ np.asarray(A, float).T)) ** 2).sum(1)).max())
