"""Records tests/golden/jpeg_write: source arrays and the JPEG files Pillow (libjpeg-turbo) writes for them.

Run by hand on a machine that has Pillow (`python tests/make_jpeg_write_golden.py`); pytest does not collect it.  It writes
  sources.npz     name -> the uint8 source array, (h, w, 3) RGB or (h, w) gray
  <name>.jpg      Pillow's file for it (standard Huffman tables, optimize=False)
  manifest.json   the Pillow and libjpeg-turbo versions and each file's save arguments
libjpeg-turbo's default compress path is integer arithmetic end to end, so these files pin the writer byte for byte
(tests/test_cpu_jpeg_write.py on the host, tests/test_jpeg_write_gpu.py on the device).
"""
import io
import json
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_write')
SIZES = [(1, 1), (2, 3), (7, 9), (8, 8), (16, 16), (17, 13), (31, 33), (48, 80)]          # (h, w)
SAMPLINGS = {'444': 0, '422': 1, '420': 2}                                               # Pillow's `subsampling`
QUALITIES = (1, 30, 85, 100)
MAX_FILE, MAX_TOTAL = 12 * 1024, 150 * 1024


def content(h, w, seed, full=False):
    """A gradient plus seeded noise; full: noise of +-127 around mid-grey, so that large coefficients and the long
    Huffman codes occur at quality 100 (not on 48x80, whose file would pass the size limit)."""
    rng = np.random.default_rng(seed)
    if full:
        return np.clip(128 + rng.integers(-127, 128, (h, w, 3)), 0, 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(h + w - 2, 1)], -1)
    return np.clip(img + rng.integers(-24, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def cases():
    """(name, array, mode, save arguments)"""
    out = []
    for si, (h, w) in enumerate(SIZES):
        for ki, (sname, sub) in enumerate(SAMPLINGS.items()):
            q = QUALITIES[(si + ki) % 4]
            out.append((f'rgb_{h}x{w}_{sname}_q{q}', content(h, w, 100 * si + ki, full=q == 100 and h * w <= 31 * 33), 'RGB',
                        dict(quality=q, subsampling=sub)))
    for q in QUALITIES:                                       # every quality on one geometry with dummy blocks
        out.append((f'quality_17x13_420_q{q}', content(17, 13, 50, full=q == 100), 'RGB', dict(quality=q, subsampling=2)))
    out.append(('gray_31x33_q85', content(31, 33, 7)[..., 0], 'L', dict(quality=85)))
    out.append(('gray_7x9_q100_rstrows1', content(7, 9, 8, full=True)[..., 0], 'L', dict(quality=100, restart_marker_rows=1)))
    for ki, (sname, sub) in enumerate(SAMPLINGS.items()):
        out.append((f'rstrows1_31x33_{sname}_q30', content(31, 33, 40 + ki), 'RGB',
                    dict(quality=30, subsampling=sub, restart_marker_rows=1)))
    out.append(('rstrows1_48x80_420_q85', content(48, 80, 60), 'RGB', dict(quality=85, subsampling=2, restart_marker_rows=1)))
    return out


def main():
    import PIL
    from PIL import Image, features
    os.makedirs(OUT, exist_ok=True)
    sources, files, total = {}, {}, 0
    for name, arr, mode, args in cases():
        buf = io.BytesIO()
        Image.fromarray(arr, mode).save(buf, 'JPEG', optimize=False, **args)
        blob = buf.getvalue()
        assert len(blob) < MAX_FILE, (name, len(blob))
        total += len(blob)
        with open(os.path.join(OUT, name + '.jpg'), 'wb') as f:
            f.write(blob)
        sources[name] = arr
        files[name] = dict(mode=mode, height=int(arr.shape[0]), width=int(arr.shape[1]), save=dict(optimize=False, **args),
                           bytes=len(blob))
    assert total < MAX_TOTAL, total
    np.savez_compressed(os.path.join(OUT, 'sources.npz'), **sources)
    with open(os.path.join(OUT, 'manifest.json'), 'w') as f:
        json.dump(dict(pillow=PIL.__version__, libjpeg=features.version('jpg'), libjpeg_turbo=features.version('libjpeg_turbo'),
                       files=files), f, indent=1, sort_keys=True)
    print(f'{len(files)} files, {total} bytes of JPEG')


if __name__ == '__main__':
    main()
