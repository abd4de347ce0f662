"""Records tests/golden/jpeg: JPEG files written by Pillow (libjpeg-turbo) and Pillow's own decode of each.

Run by hand on a machine that has Pillow (`python tests/make_jpeg_golden.py`); pytest does not collect it.  It writes
  <name>.jpg      the files (deterministic gradients plus seeded noise, so that every AC coefficient is populated)
  expected.npz    name -> Image.open(file).convert('RGB') as uint8 (h, w, 3), for every decodable file
  manifest.json   the Pillow and libjpeg-turbo versions and each file's save arguments
libjpeg-turbo's default decode is integer arithmetic end to end, so these arrays pin the decoder bit for bit
(tests/test_cpu_jpeg.py on the host, tests/test_jpeg_gpu.py on the device).
"""
import io
import json
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg')
SIZES = [(1, 1), (2, 3), (8, 8), (17, 13), (33, 31), (48, 80)]           # (h, w)
SAMPLINGS = {'444': 0, '422': 1, '420': 2}                               # Pillow's `subsampling`
QUALITIES = (30, 85, 100)
MAX_FILE, MAX_TOTAL = 12 * 1024, 150 * 1024


def content(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(h + w - 2, 1)], -1)
    return np.clip(img + rng.integers(-24, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def cases():
    """(name, array, mode, save arguments, decodable)"""
    out = []
    for si, (h, w) in enumerate(SIZES):
        for ki, (sname, sub) in enumerate(SAMPLINGS.items()):
            q = QUALITIES[(si + ki) % 3]
            out.append((f'rgb_{h}x{w}_{sname}_q{q}', content(h, w, 100 * si + ki), 'RGB', dict(quality=q, subsampling=sub), True))
    out.append(('gray_33x31_q85', content(33, 31, 7)[..., 0], 'L', dict(quality=85), True))
    for ki, (sname, sub) in enumerate(SAMPLINGS.items()):
        out.append((f'opt_33x31_{sname}_q85', content(33, 31, 20 + ki), 'RGB', dict(quality=85, subsampling=sub, optimize=True), True))
        out.append((f'rstblocks3_48x80_{sname}_q85', content(48, 80, 30 + ki), 'RGB',
                    dict(quality=85, subsampling=sub, restart_marker_blocks=3), True))
        out.append((f'rstrows1_33x31_{sname}_q30', content(33, 31, 40 + ki), 'RGB',
                    dict(quality=30, subsampling=sub, restart_marker_rows=1), True))
    for q in QUALITIES:
        out.append((f'quality_17x13_420_q{q}', content(17, 13, 50), 'RGB', dict(quality=q, subsampling=2), True))
    yy, xx = np.mgrid[0:16, 0:16]
    checker = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    out.append(('checker_16x16_444_q100', checker, 'RGB', dict(quality=100, subsampling=0), True))
    out.append(('multigroup_96x160_420_q85_rstrows1', content(96, 160, 60), 'RGB',
                dict(quality=85, subsampling=2, restart_marker_rows=1), True))
    out.append(('refuse_progressive_33x31', content(33, 31, 70), 'RGB', dict(quality=85, progressive=True), False))
    out.append(('refuse_cmyk_17x13', np.concatenate([content(17, 13, 71), content(17, 13, 72)[..., :1]], -1), 'CMYK',
                dict(quality=85), False))
    return out


def main():
    import PIL
    from PIL import Image, features
    os.makedirs(OUT, exist_ok=True)
    expected, files, total = {}, {}, 0
    for name, arr, mode, args, decodable in cases():
        buf = io.BytesIO()
        Image.fromarray(arr, mode).save(buf, 'JPEG', **args)
        blob = buf.getvalue()
        assert len(blob) < MAX_FILE, (name, len(blob))
        total += len(blob)
        with open(os.path.join(OUT, name + '.jpg'), 'wb') as f:
            f.write(blob)
        if decodable:
            expected[name] = np.asarray(Image.open(io.BytesIO(blob)).convert('RGB'))
        files[name] = dict(mode=mode, height=int(arr.shape[0]), width=int(arr.shape[1]), save=args, decodable=decodable,
                           bytes=len(blob))
    assert total < MAX_TOTAL, total
    np.savez_compressed(os.path.join(OUT, 'expected.npz'), **expected)
    with open(os.path.join(OUT, 'manifest.json'), 'w') as f:
        json.dump(dict(pillow=PIL.__version__, libjpeg=features.version('jpg'), libjpeg_turbo=features.version('libjpeg_turbo'), decode="Image.open(f).convert('RGB')",
                       files=files), f, indent=1, sort_keys=True)
    print(f'{len(files)} files, {total} bytes of JPEG')


if __name__ == '__main__':
    main()
