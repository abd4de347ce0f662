"""A numpy restatement of the JPEG reconstruction from coefficient arrays: the third statement
next to the host C++ (csrc/jpeg_io.cpp) and the kernels (csrc/jpeg_decode.hip).  Test infrastructure, not a test.

libjpeg-turbo's default decode [upstream-memory; pinned by tests/golden/jpeg]: jidctint.c's JDCT_ISLOW inverse DCT
(CONST_BITS 13, PASS1_BITS 2, columns then rows), jdsample.c's fancy upsampling (components wider than two samples;
narrower ones are replicated), jdcolor.c's 16-bit fixed-point YCbCr -> RGB.  Sums and products are int32 and wrap, as
the product's do; the final sample is a plain clamp to [0, 255].
"""
import numpy as np

CONST_BITS, PASS1_BITS = 13, 2
F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137,
         f1_961=16069, f2_053=16819, f2_562=20995, f3_072=25172)


def _descale(x, n):
    return (x + np.int32(1 << (n - 1))) >> np.int32(n)


def idct_1d(v, shift):
    """v: int32 (..., 8) -> int32 (..., 8), one pass of jpeg_idct_islow along the last axis."""
    c = {k: np.int32(x) for k, x in F.items()}
    i = [v[..., k].astype(np.int32) for k in range(8)]
    with np.errstate(over='ignore'):
        z1 = (i[2] + i[6]) * c['f0_541']
        tmp2 = z1 - i[6] * c['f1_847']
        tmp3 = z1 + i[2] * c['f0_765']
        tmp0 = (i[0] + i[4]) * np.int32(1 << CONST_BITS)          # a left shift that wraps
        tmp1 = (i[0] - i[4]) * np.int32(1 << CONST_BITS)
        t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
        tmp0, tmp1, tmp2, tmp3 = i[7], i[5], i[3], i[1]
        z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
        z5 = (z3 + z4) * c['f1_175']
        tmp0, tmp1, tmp2, tmp3 = tmp0 * c['f0_298'], tmp1 * c['f2_053'], tmp2 * c['f3_072'], tmp3 * c['f1_501']
        z1, z2, z3, z4 = -(z1 * c['f0_899']), -(z2 * c['f2_562']), -(z3 * c['f1_961']) + z5, -(z4 * c['f0_390']) + z5
        tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
        out = [t10 + tmp3, t11 + tmp2, t12 + tmp1, t13 + tmp0, t13 - tmp0, t12 - tmp1, t11 - tmp2, t10 - tmp3]
        return np.stack([_descale(o, shift) for o in out], -1)


def component_plane(coef, quant, bh, bw):
    """coef int16 (bh * bw * 64,) natural order, quant uint16 (64,) -> uint8 (8 bh, 8 bw)."""
    d = coef.reshape(bh, bw, 8, 8).astype(np.int32) * quant.reshape(8, 8).astype(np.int32)
    ws = idct_1d(d.swapaxes(-1, -2), CONST_BITS - PASS1_BITS).swapaxes(-1, -2)        # columns
    with np.errstate(over='ignore'):
        px = idct_1d(ws, CONST_BITS + PASS1_BITS + 3) + np.int32(128)                     # rows
    return np.clip(px, 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw)


def upsample_h(p):
    """h2v1_fancy_upsample over true-size rows: (h, cw) -> (h, 2 cw)."""
    p = p.astype(np.int32)
    cw = p.shape[1]
    if cw <= 2:
        return np.repeat(p, 2, 1)
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * cw), np.int32)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    return out


def upsample_hv(p):
    """h2v2_fancy_upsample over the true-size plane: (ch, cw) -> (2 ch, 2 cw)."""
    p = p.astype(np.int32)
    ch, cw = p.shape
    if cw <= 2:
        return np.repeat(np.repeat(p, 2, 0), 2, 1)
    up = np.concatenate([p[:1], p[:-1]], 0)
    down = np.concatenate([p[1:], p[-1:]], 0)
    out = np.empty((2 * ch, 2 * cw), np.int32)
    for phase, far in ((0, up), (1, down)):
        s = 3 * p + far
        left = np.concatenate([s[:, :1], s[:, :-1]], 1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        out[phase::2, 0::2] = (3 * s + left + 8) >> 4
        out[phase::2, 1::2] = (3 * s + right + 7) >> 4
    return out


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def reconstruct(coef, quant, info):
    """coef int16 (coef_count,), quant uint16 (3, 64), info = jpeg.jpeg_info(...) dict -> uint8 (h, w, 3) RGB (gray:
    three equal channels)."""
    h, w = info['height'], info['width']
    planes, off = [], 0
    for c, (bh, bw) in enumerate(info['blocks']):
        planes.append(component_plane(coef[off:off + 64 * bh * bw], np.asarray(quant).reshape(3, 64)[c], bh, bw))
        off += 64 * bh * bw
    y = planes[0][:h, :w]
    if info['components'] == 1:
        return np.repeat(y[..., None], 3, -1)
    chroma = []
    for c in (1, 2):
        ch, cw = info['comp_shape'][c]
        p = planes[c][:ch, :cw]
        if info['sampling'] == '422':
            p = upsample_h(p)
        elif info['sampling'] == '420':
            p = upsample_hv(p)
        chroma.append(p[:h, :w])
    return ycc_to_rgb(y, chroma[0], chroma[1])
