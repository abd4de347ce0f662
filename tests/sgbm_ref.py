"""TEST INFRASTRUCTURE: numpy restatement of OpenCV's StereoSGBM in mode SGBM_3WAY (csrc/sgbm.hip).

The reference's disparity PNGs are OpenCV StereoSGBM results (reproducibility.md section 3).  OpenCV is absent, so the
rules are restated from OpenCV 4.x stereosgbm.cpp [upstream-memory] and parity with cv2 stays UNPINNED (DESIGN.md
"Stereo SGBM").  This module is the executable spec: every stage is integer arithmetic and the GPU kernels are held to it
bit for bit (tests/test_sgbm_gpu.py).  Nothing under stereotracking_amd/ imports it.

Rules (D = num_disparities, ftzero = max(pre_filter_cap, 15) | 1, cn = 3 BGR channels or 1 grey channel):
  1 prefilter  per channel, columns 1..w-2: sob = 2 (p[y][x+1] - p[y][x-1]) + the same difference of rows y-1 and y+1
               (rows replicated at the top and bottom); value = clip(sob, -ftzero, ftzero) + ftzero.  Columns 0 and w-1
               hold ftzero in BOTH the prefiltered and the raw-intensity rows (OpenCV fills all 2 cn rows with tab[0]).
  2 BT cost    x in [D, w), d in [0, D): left x against right x - d.  Envelopes u0 / u1 = min / max(u, (u + u_left) / 2,
               (u + u_right) / 2) (integer /2, the pixel itself at the row ends), the same for the right image; cost =
               min(max(0, u - v1, v0 - u), max(0, v - u1, u0 - v)); summed over the cn prefiltered channels at full
               weight plus each of the cn raw-intensity channels >> 2.
  3 block sum  block_size x block_size box, indices clamped to the computed columns [D, w) and to the rows [0, h).
  4 paths      left->right, right->left, top->bottom: L(p, d) = C(p, d) + min(L(p-r, d), L(p-r, d +- 1) + P1,
               minL(p-r) + P2') - minL(p-r), P2' = max(P2, P1 + 1), L = C at the start of a path; S = sum of the three.
               One stripe over the whole image (OpenCV with setNumThreads(1)).
  5 decision   best = lowest d of min S.  Uniqueness (uniqueness_ratio > 0): thresh = (100 minS) // (100 - ratio), the
               pixel is invalid when some d with |d - best| > 1 has S[d] <= thresh  [uncertain: the classic mode's
               strict S (100 - ratio) < 100 minS differs at equality; the 3-way form is taken].  Subpixel for
               0 < best < D-1: denom2 = max(S[b-1] + S[b+1] - 2 S[b], 1), d16 = 16 b + ((S[b-1] - S[b+1]) 16 + denom2)
               / (2 denom2), C division (truncation toward zero); else d16 = 16 b.  Invalid = -16; x < D invalid.
  6 LR check   disp2: every unique pixel, in descending x, writes disp2[x - best] = best when its minS is strictly below
               the stored cost (ties: the highest x wins).  A pixel is invalidated when both floor(d16 / 16) and
               ceil(d16 / 16) hit an in-range, set disp2 entry differing by more than max(disp12_max_diff, 1)
               [uncertain: the code maps <= 0 to 1, the documentation says <= 0 disables the check; the code is taken].
  7 median     medianBlur(disp, 3): 3 x 3 median of the int16 map, replicated borders.
  8 speckles   filterSpeckles(newVal -16, maxSpeckleSize, maxDiff 16 speckle_range): 4-connected components over the
               pixels != -16, neighbours joined when their values differ by <= maxDiff; components of <= maxSpeckleSize
               pixels become -16 (speckle_window_size 0 skips the filter).
  9 output     disp_postp = max(d16, 0) / 16, fp32, the same in all three channels (0 in the padding).
  grey         color=False: the fixed-point BGR2GRAY (R 9798 + G 19235 + B 3735 + 2^14) >> 15, channel 2 = R.
"""
import numpy as np

INVALID = -16


def ftzero_of(pre_filter_cap):
    return max(int(pre_filter_cap), 15) | 1


def to_grey(bgr):
    b, g, r = (bgr[i].astype(np.int64) for i in range(3))
    return ((r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15)[None]


def prefilter(img, ftzero):
    """uint8 (cn, h, w) -> int64 (2 cn, h, w): the prefiltered rows, then the raw-intensity rows (rule 1)."""
    p = img.astype(np.int64)
    up = np.concatenate([p[:, :1], p[:, :-1]], 1)
    dn = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    sob = 2 * (p[..., 2:] - p[..., :-2]) + (up[..., 2:] - up[..., :-2]) + (dn[..., 2:] - dn[..., :-2])
    pf = np.full_like(p, ftzero)
    pf[..., 1:-1] = np.clip(sob, -ftzero, ftzero) + ftzero
    raw = p.copy()
    raw[..., 0] = ftzero
    raw[..., -1] = ftzero
    return np.concatenate([pf, raw], 0)


def envelopes(a):
    """(..., w) -> (min, max) envelopes of the half-sample interpolants (rule 2)."""
    left = np.concatenate([a[..., :1], a[..., :-1]], -1)
    right = np.concatenate([a[..., 1:], a[..., -1:]], -1)
    hl, hr = (a + left) // 2, (a + right) // 2
    return np.minimum(np.minimum(a, hl), hr), np.maximum(np.maximum(a, hl), hr)


def pixel_cost(PL, PR, D, cn):
    """Prefiltered (2 cn, h, w) pair -> BT cost (h, w - D, D) of the columns [D, w) (rule 2)."""
    w = PL.shape[-1]
    L0, L1 = envelopes(PL)
    R0, R1 = envelopes(PR)
    u, u0, u1 = PL[..., D:], L0[..., D:], L1[..., D:]
    shift = np.array([0] * cn + [2] * cn)[:, None, None]
    out = np.empty(PL.shape[1:2] + (w - D, D), np.int64)
    for d in range(D):
        v, v0, v1 = PR[..., D - d:w - d], R0[..., D - d:w - d], R1[..., D - d:w - d]
        c0 = np.maximum(np.maximum(0, u - v1), v0 - u)
        c1 = np.maximum(np.maximum(0, v - u1), u0 - v)
        out[..., d] = (np.minimum(c0, c1) >> shift).sum(0)
    return out


def block_sum(pc, block_size):
    """(h, w', D) -> (h, w', D) box sums with clamped indices (rule 3)."""
    r = block_size // 2
    p = np.pad(pc, ((r, r), (r, r), (0, 0)), mode='edge')
    h, w = pc.shape[:2]
    acc = np.zeros_like(pc)
    for dy in range(block_size):
        for dx in range(block_size):
            acc += p[dy:dy + h, dx:dx + w]
    return acc


def _path(C, P1, P2, reverse=False):
    """Aggregate along axis 0 (vectorised over the rest; d last) (rule 4)."""
    n = C.shape[0]
    order = range(n - 1, -1, -1) if reverse else range(n)
    L = np.empty_like(C)
    prev = None
    big = np.int64(1) << 40
    for i in order:
        if prev is None:
            cur = C[i].copy()
        else:
            m = prev.min(-1, keepdims=True)
            nb = np.full_like(prev, big)
            nb[..., 1:] = prev[..., :-1]
            nb2 = np.full_like(prev, big)
            nb2[..., :-1] = prev[..., 1:]
            cur = C[i] + np.minimum(np.minimum(prev, np.minimum(nb, nb2) + P1), m + P2) - m
        L[i] = cur
        prev = cur
    return L


def paths(C, P1, P2):
    """-> S = L_lr + L_rl + L_tb (h, w', D)."""
    P2 = max(P2, P1 + 1)
    tb = _path(C, P1, P2)
    Ct = C.transpose(1, 0, 2)
    lr = _path(Ct, P1, P2).transpose(1, 0, 2)
    rl = _path(Ct, P1, P2, reverse=True).transpose(1, 0, 2)
    return lr + rl + tb


def trunc_div(a, b):
    """C integer division (truncation toward zero); b > 0."""
    q = np.abs(a) // b
    return np.where(a < 0, -q, q)


def decide(S, D, w, uniqueness_ratio, disp12_max_diff):
    """S (h, w', D) -> int16 map (h, w) after uniqueness, subpixel and the LR check (rules 5, 6)."""
    h, wp, _ = S.shape
    minS = S.min(-1)
    best = S.argmin(-1)
    dd = np.arange(D)
    if uniqueness_ratio > 0:
        thresh = (100 * minS) // (100 - uniqueness_ratio)
        bad = ((np.abs(dd[None, None] - best[..., None]) > 1) & (S <= thresh[..., None])).any(-1)
    else:
        bad = np.zeros(best.shape, bool)
    inner = (best > 0) & (best < D - 1)
    bm, bp = np.clip(best - 1, 0, D - 1), np.clip(best + 1, 0, D - 1)
    Sb = np.take_along_axis(S, best[..., None], -1)[..., 0]
    Sm = np.take_along_axis(S, bm[..., None], -1)[..., 0]
    Sp = np.take_along_axis(S, bp[..., None], -1)[..., 0]
    denom2 = np.maximum(Sm + Sp - 2 * Sb, 1)
    d16 = np.where(inner, 16 * best + trunc_div((Sm - Sp) * 16 + denom2, 2 * denom2), 16 * best)
    disp = np.full((h, w), INVALID, np.int64)
    disp[:, D:] = np.where(bad, INVALID, d16)
    # disp2: per row, the lowest cost wins, ties to the highest x (the descending scan with a strict test)
    ys, xs = np.nonzero(~bad)
    x = xs + D
    x2 = x - best[ys, xs]
    cost = minS[ys, xs]
    order = np.lexsort((-x, cost, x2, ys))
    key = ys[order] * w + x2[order]
    first = np.ones(len(order), bool)
    first[1:] = key[1:] != key[:-1]
    disp2 = np.full((h, w), -1, np.int64)
    sel = order[first]
    disp2[ys[sel], x2[sel]] = best[ys[sel], xs[sel]]
    # LR check
    tol = disp12_max_diff if disp12_max_diff > 0 else 1
    d1 = disp[:, D:]
    fl, ce = d1 >> 4, (d1 + 15) >> 4
    xx = np.arange(D, w)[None]
    rows = np.arange(h)[:, None]

    def hit(dq):
        xq = xx - dq
        inr = (xq >= 0) & (xq < w)
        v = disp2[rows, np.clip(xq, 0, w - 1)]
        return inr & (v >= 0) & (np.abs(v - dq) > tol)

    kill = (d1 != INVALID) & hit(fl) & hit(ce)
    d1[kill] = INVALID
    return disp


def median3(disp):
    h, w = disp.shape
    p = np.pad(disp, 1, mode='edge')
    st = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])
    return np.sort(st, 0)[4]


def speckles(disp, max_size, max_diff, new_val=INVALID):
    """filterSpeckles (rule 8) via connected components of the 4-neighbour graph."""
    if max_size <= 0:
        return disp.copy()
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    h, w = disp.shape
    idx = np.arange(h * w).reshape(h, w)
    ok = disp != new_val
    ea = [idx[:, :-1][ok[:, :-1] & ok[:, 1:] & (np.abs(disp[:, :-1] - disp[:, 1:]) <= max_diff)],
          idx[:-1][ok[:-1] & ok[1:] & (np.abs(disp[:-1] - disp[1:]) <= max_diff)]]
    eb = [ea[0] + 1, ea[1] + w]
    a, b = np.concatenate(ea), np.concatenate(eb)
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(h * w, h * w))
    _, lab = connected_components(g, directed=False)
    size = np.bincount(lab[ok.ravel()], minlength=h * w)
    small = (size[lab] <= max_size).reshape(h, w) & ok
    out = disp.copy()
    out[small] = new_val
    return out


DEFAULTS = dict(num_disparities=48, block_size=3, P1=96, P2=384, disp12_max_diff=0, uniqueness_ratio=10,
                speckle_window_size=400, speckle_range=10, pre_filter_cap=63, color=True)


def aggregate(left, right, **kw):
    """uint8 (3, h, w) BGR left / right -> int64 (block-summed cost C, aggregated cost S), both (h, w - D, D)
    (rules 1 - 4).  tests/test_cpu_sgbm.py counts the tied minima of S with it."""
    p = dict(DEFAULTS, **kw)
    ft = ftzero_of(p['pre_filter_cap'])
    if p['color']:
        cn, l, r = 3, left, right
    else:
        cn, l, r = 1, to_grey(left), to_grey(right)
    PL, PR = prefilter(l, ft), prefilter(r, ft)
    C = block_sum(pixel_cost(PL, PR, p['num_disparities'], cn), p['block_size'])
    return C, paths(C, p['P1'], p['P2'])


def sgbm(left, right, stages=False, **kw):
    """uint8 (3, h, w) BGR left / right -> int16 (h, w) disparity x 16 (-16 invalid).  stages=True: a dict with the
    block-summed cost 'cost' (h, w - D, D), 'raw' (before the median), 'median' and 'final'."""
    p = dict(DEFAULTS, **kw)
    D = p['num_disparities']
    w = left.shape[-1]
    C, S = aggregate(left, right, **kw)
    raw = decide(S, D, w, p['uniqueness_ratio'], p['disp12_max_diff'])
    med = median3(raw)
    fin = speckles(med, p['speckle_window_size'], 16 * p['speckle_range'])
    if stages:
        return dict(cost=C.astype(np.int16), raw=raw.astype(np.int16), median=med.astype(np.int16),
                    final=fin.astype(np.int16))
    return fin.astype(np.int16)


def disp_postp(final, H, W):
    """int16 (h, w) -> fp32 (3, H, W) as the PNG loader gives it: max(d16, 0) / 16, 0 in the padding (rule 9)."""
    h, w = final.shape
    out = np.zeros((3, H, W), np.float32)
    out[:, :h, :w] = np.maximum(final, 0).astype(np.float32) / 16.0
    return out
