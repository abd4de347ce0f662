"""CPU: the JPEG reader's host half (stereotracking_amd/jpeg.py on csrc/jpeg_io.cpp) - DESIGN.md section 25.

The hard pin is tests/golden/jpeg (recorded by tests/make_jpeg_golden.py): files written by Pillow's libjpeg-turbo and
Pillow's own decode of each.  Everything against it is an equality: read_jpeg, and tests/jpeg_ref.py (the numpy
restatement) fed with the native entropy decoder's coefficients.  Then the header fields, the refusals and their
exception types, LoadImageFromFile, the numpy encoder's round trip, and reentrancy.
"""
import io
import json
import os
import threading

import numpy as np
import pytest

import jpeg_ref
from stereotracking_amd import datasets, jpeg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg')
with open(os.path.join(GOLDEN, 'manifest.json')) as _f:
    MANIFEST = json.load(_f)
DECODABLE = sorted(n for n, m in MANIFEST['files'].items() if m['decodable'])


@pytest.fixture(scope='module')
def expected():
    with np.load(os.path.join(GOLDEN, 'expected.npz')) as z:
        return {k: z[k] for k in z.files}


def blob(name):
    with open(os.path.join(GOLDEN, name + '.jpg'), 'rb') as f:
        return f.read()


def as_rgb(a):
    return np.repeat(a[..., None], 3, -1) if a.ndim == 2 else a


def test_fixture_set_is_what_the_generator_describes(expected):
    assert sorted(expected) == DECODABLE and len(MANIFEST['files']) == len(DECODABLE) + 2
    sizes = [os.path.getsize(os.path.join(GOLDEN, n + '.jpg')) for n in MANIFEST['files']]
    assert max(sizes) < 12 * 1024 and sum(sizes) < 150 * 1024
    checker = expected['checker_16x16_444_q100']
    assert checker.min() == 0 and checker.max() == 255          # clamping at both ends occurs


@pytest.mark.parametrize('name', DECODABLE)
def test_read_jpeg_equals_libjpeg_turbo(name, expected):
    got = jpeg.read_jpeg(blob(name))
    assert got.dtype == np.uint8 and got.ndim == (2 if MANIFEST['files'][name]['mode'] == 'L' else 3)
    assert np.array_equal(as_rgb(got), expected[name])


@pytest.mark.parametrize('name', DECODABLE)
def test_numpy_restatement_on_native_coefficients_equals_libjpeg_turbo(name, expected):
    data = blob(name)
    _, coef, quant = jpeg.entropy_decode(data)
    assert np.array_equal(jpeg_ref.reconstruct(coef, quant, jpeg.jpeg_info(data)), expected[name])


def test_read_jpeg_takes_a_path(expected):
    name = DECODABLE[0]
    assert np.array_equal(as_rgb(jpeg.read_jpeg(os.path.join(GOLDEN, name + '.jpg'))), expected[name])


def test_jpeg_info_fields():
    i = jpeg.jpeg_info(blob('multigroup_96x160_420_q85_rstrows1'))
    assert (i['height'], i['width'], i['components'], i['sampling']) == (96, 160, 3, '420')
    assert i['mcus'] == (6, 10) and i['restart_interval'] == 10          # restart_marker_rows=1: one MCU row
    assert i['blocks'] == [(12, 20), (6, 10), (6, 10)] and i['comp_shape'] == [(96, 160), (48, 80), (48, 80)]
    assert i['coef_count'] == 64 * (240 + 60 + 60) and i['work_bytes'] == i['coef_count']
    i = jpeg.jpeg_info(blob('rgb_17x13_422_q85'))
    assert (i['height'], i['width'], i['sampling'], i['mcus']) == (17, 13, '422', (3, 1))
    assert i['blocks'] == [(3, 2), (3, 1), (3, 1)] and i['comp_shape'] == [(17, 13), (17, 7), (17, 7)]
    i = jpeg.jpeg_info(blob('rstblocks3_48x80_444_q85'))
    assert (i['sampling'], i['restart_interval'], i['mcus'], i['blocks']) == ('444', 3, (6, 10), [(6, 10)] * 3)
    i = jpeg.jpeg_info(blob('gray_33x31_q85'))
    assert (i['components'], i['sampling'], i['blocks'], i['comp_shape']) == (1, 'gray', [(5, 4)], [(33, 31)])
    i = jpeg.jpeg_info(blob('rgb_1x1_420_q100'))
    assert (i['mcus'], i['blocks'], i['comp_shape']) == ((1, 1), [(2, 2), (1, 1), (1, 1)], [(1, 1)] * 3)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _patched(data, marker, fn):
    """The file with fn(payload bytearray) applied to its first segment `marker`."""
    d = bytearray(data)
    p = 2
    while p < len(d):
        assert d[p] == 0xFF
        m, n = d[p + 1], (d[p + 2] << 8) | d[p + 3]
        if m == marker:
            seg = bytearray(d[p + 4:p + 2 + n])
            fn(seg)
            d[p + 4:p + 2 + n] = seg
            return bytes(d)
        p += 2 + n
    raise AssertionError('marker not found')


def _set(idx, value):
    def fn(seg):
        seg[idx] = value
    return fn


def _with_marker(data, old, new):
    d = bytearray(data)
    p = d.index(bytes([0xFF, old]))
    d[p + 1] = new
    return bytes(d)


BASE = 'rgb_17x13_420_q100'
REFUSALS = {
    'progressive': (lambda: blob('refuse_progressive_33x31'), 'progressive'),
    'cmyk': (lambda: blob('refuse_cmyk_17x13'), '4-component'),
    'arithmetic': (lambda: _with_marker(blob(BASE), 0xC0, 0xC9), 'arithmetic'),
    'lossless': (lambda: _with_marker(blob(BASE), 0xC0, 0xC3), 'lossless'),
    '12-bit': (lambda: _patched(blob(BASE), 0xC0, _set(0, 12)), '12-bit'),
    'sampling 1x2': (lambda: _patched(blob(BASE), 0xC0, _set(7, 0x12)), 'sampling'),
    'sampling 4x1': (lambda: _patched(blob(BASE), 0xC0, _set(7, 0x41)), 'sampling'),
    'chroma 2x1': (lambda: _patched(blob(BASE), 0xC0, _set(10, 0x21)), 'sampling'),
    'multi-scan': (lambda: _patched(blob(BASE), 0xDA, _set(0, 1)), 'multi-scan'),
    'adobe transform 0': (lambda: blob(BASE)[:2] + b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00' + blob(BASE)[2:], 'Adobe'),
}


@pytest.mark.parametrize('case', sorted(REFUSALS))
def test_unsupported_features_are_refused_by_name(case):
    make, word = REFUSALS[case]
    data = make()
    for fn in (jpeg.read_jpeg, jpeg.jpeg_info):
        with pytest.raises(NotImplementedError, match=word):
            fn(data)


def test_corrupt_and_truncated_data_is_a_value_error(expected):
    for name in ('rgb_48x80_420_q85', 'rstblocks3_48x80_422_q85', 'gray_33x31_q85'):
        data = blob(name)
        with pytest.raises(ValueError, match='truncated|restart'):
            jpeg.read_jpeg(data[:len(data) * 6 // 10])                    # cut at 60 % of its length
    with pytest.raises(ValueError, match='not a JPEG'):
        jpeg.read_jpeg(b'\x89PNG\r\n\x1a\n' + bytes(32))
    with pytest.raises(ValueError):
        jpeg.read_jpeg(blob(BASE)[:30])                                   # ends inside the headers
    # a restart marker with the wrong number
    data = bytearray(blob('rstblocks3_48x80_444_q85'))
    data[data.index(b'\xff\xd0') + 1] = 0xD3
    with pytest.raises(ValueError, match='restart'):
        jpeg.read_jpeg(bytes(data))


@pytest.mark.parametrize('length,count', [(1, 3), (1, 200), (3, 9), (7, 129)])
@pytest.mark.parametrize('table_class', [0, 1])
def test_a_huffman_table_with_more_codes_of_a_length_than_fit_is_a_value_error(length, count, table_class):
    """A DHT whose counts break the Kraft bound while its segment length is consistent (the symbol total matches): the
    table builder must refuse it before it writes an entry of that length - stand-alone, and spliced into a real file."""
    counts = bytes(count if n == length else 0 for n in range(1, 17))
    body = bytes([table_class << 4 | 3]) + counts + bytes(k % 12 for k in range(count))
    seg = b'\xff\xc4' + (len(body) + 2).to_bytes(2, 'big') + body
    base = blob(BASE)
    for data in (b'\xff\xd8' + seg + b'\xff\xd9', base[:2] + seg + base[2:]):
        for fn in (jpeg.jpeg_info, jpeg.read_jpeg):
            with pytest.raises(ValueError, match='more codes of length'):
                fn(data)
    # the largest table that does fit is taken: 2 codes of length 1 (unused by the scan, so the file still decodes)
    ok = bytes([table_class << 4 | 3]) + bytes([2] + [0] * 15) + bytes([0, 1])
    jpeg.read_jpeg(base[:2] + b'\xff\xc4' + (len(ok) + 2).to_bytes(2, 'big') + ok + base[2:])


def test_reconstruct_host_refuses_a_struct_that_is_not_st_jpeg_infos():
    """The host routine indexes memory with the struct's grids, like the device entry: an inconsistent one is an error."""
    info, coef, quant = jpeg.entropy_decode(blob(BASE))
    want = jpeg.reconstruct_host(coef, quant, info)
    for field, index, value in (('blocks_w', 0, -5), ('blocks_w', 0, 1), ('blocks_h', 1, 4096), ('comp_w', 2, 64),
                                ('coef_offset', 1, 0), ('width', None, 300), ('sampling', None, 1), ('components', None, 1)):
        bad = jpeg.StJpegInfo.from_buffer_copy(info)
        if index is None:
            setattr(bad, field, value)
        else:
            getattr(bad, field)[index] = value
        out = np.empty((bad.height, bad.width, 3), np.uint8)
        rc = jpeg._api().st_jpeg_reconstruct_host(coef.ctypes.data, quant.ctypes.data, bad, out.ctypes.data, 1, 3 * bad.width, 3, 1)
        assert rc == -1, (field, index, value)
    assert np.array_equal(jpeg.reconstruct_host(coef, quant, info), want)


def test_sixteen_bit_quantisation_tables_and_tables_sharing_a_segment(expected):
    """Rewrites a fixture's DQT segments as ONE segment of 16-bit entries and its DHT segments as one: same pixels."""
    name = 'rgb_33x31_422_q100'
    d = blob(name)
    p, head, dqt, dht = 2, b'', b'', b''
    while d[p + 1] != 0xDA:
        m, n = d[p + 1], (d[p + 2] << 8) | d[p + 3]
        body = d[p + 4:p + 2 + n]
        if m == 0xDB:
            o = 0
            while o < len(body):
                assert body[o] >> 4 == 0
                dqt += bytes([0x10 | body[o]]) + b''.join(bytes([0, v]) for v in body[o + 1:o + 65])
                o += 65
        elif m == 0xC4:
            dht += body
        else:
            head += d[p:p + 2 + n]
        p += 2 + n

    def seg(m, body):
        return bytes([0xFF, m, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + body
    rebuilt = d[:2] + b'\xff\xfe\x00\x05hi!' + head + seg(0xDB, dqt) + seg(0xC4, dht) + b'\xff' + d[p:]   # + COM, + a fill byte
    assert np.array_equal(jpeg.read_jpeg(rebuilt), expected[name])


# ---- the dataset transform ---------------------------------------------------------------------------------------------
def test_load_image_from_file_sniffs_the_format(tmp_path, expected):
    name = 'rgb_48x80_420_q85'
    path = os.path.join(GOLDEN, name + '.jpg')
    r = datasets.LoadImageFromFile()(dict(img_path=path))
    assert r['img'].dtype == np.uint8 and np.array_equal(r['img'], expected[name][..., ::-1])      # BGR
    assert r['img_shape'] == r['ori_shape'] == (48, 80)
    r = datasets.LoadImageFromFile(to_float32=True, key='right_path', out='right')(dict(right_path=path))
    assert r['right'].dtype == np.float32 and np.array_equal(r['right'], expected[name][..., ::-1]) and 'img_shape' not in r
    g = datasets.LoadImageFromFile()(dict(img_path=os.path.join(GOLDEN, 'gray_33x31_q85.jpg')))
    assert np.array_equal(g['img'], expected['gray_33x31_q85'])
    # a PNG is still read
    png = str(tmp_path / 'a.png')
    datasets.write_png(png, expected[name])
    assert np.array_equal(datasets.LoadImageFromFile()(dict(img_path=png))['img'], expected[name][..., ::-1])
    # anything else is the error of before
    other = tmp_path / 'a.bin'
    other.write_bytes(b'GIF89a' + bytes(20))
    with pytest.raises(ValueError, match='not a PNG file'):
        datasets.LoadImageFromFile()(dict(img_path=str(other)))
    # defer: the bytes are kept, the shapes come from the header, nothing is decoded
    r = datasets.LoadImageFromFile(decode='defer')(dict(img_path=path))
    assert r['img_bytes'] == blob(name) and 'img' not in r and r['img_shape'] == r['ori_shape'] == (48, 80)
    r = datasets.LoadImageFromFile(decode='defer', key='right_path', out='right')(dict(right_path=path))
    assert r['right_bytes'] == blob(name) and 'right' not in r and 'img_shape' not in r
    assert 'img' in datasets.LoadImageFromFile(decode='defer')(dict(img_path=png))                 # a PNG is decoded as ever
    with pytest.raises(ValueError):
        datasets.LoadImageFromFile(decode='device')


# ---- the numpy encoder ---------------------------------------------------------------------------------------------------
def source(h, w, seed=0):
    """A smooth colour gradient with +-6 of seeded noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([40 + xx * 170 // max(w - 1, 1), 60 + yy * 150 // max(h - 1, 1), 200 - (xx + yy) * 120 // max(h + w - 2, 1)], -1)
    return np.clip(img + rng.integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)


# Mean absolute error of read_jpeg(write_jpeg(source, quality=90)) to the source, as measured with the host decoder over
# the 15 size x restart cases of each sampling: at most 3.21 (4:4:4), 4.40 (4:2:2), 5.40 (4:2:0), each at 7x9 - the noise
# is independent per channel, so subsampled chroma loses it, most of all where one chroma block covers the whole image.
# The bounds are twice those: a sanity check that the encoder encodes the picture it was given, not a parity claim.
ROUND_TRIP_MAE = {'444': 6.5, '422': 8.8, '420': 10.8}


@pytest.mark.parametrize('restart', [0, 1, 5])
@pytest.mark.parametrize('sampling', ['444', '422', '420'])
@pytest.mark.parametrize('size', [(1, 1), (7, 9), (16, 16), (31, 33), (40, 72)])
def test_write_jpeg_round_trip(tmp_path, size, sampling, restart):
    img = source(*size)
    path = str(tmp_path / 'a.jpg')
    jpeg.write_jpeg(path, img, quality=90, subsampling=sampling, restart_interval=restart)
    info = jpeg.jpeg_info(path)
    assert (info['height'], info['width'], info['sampling'], info['restart_interval']) == (*size, sampling, restart)
    got = jpeg.read_jpeg(path)
    with open(path, 'rb') as f:
        _, coef, quant = jpeg.entropy_decode(f.read())
    assert np.array_equal(got, jpeg_ref.reconstruct(coef, quant, info))
    mae = np.abs(got.astype(np.int32) - img).mean()
    print(f'{size} {sampling} restart {restart}: mean abs error {mae:.3f}')
    assert mae < ROUND_TRIP_MAE[sampling]


def test_write_jpeg_gray_and_quality(tmp_path):
    img = source(24, 40)[..., 1]
    sizes = []
    for q in (30, 90, 100):
        path = str(tmp_path / f'g{q}.jpg')
        jpeg.write_jpeg(path, img, quality=q)
        got = jpeg.read_jpeg(path)
        assert got.shape == img.shape and jpeg.jpeg_info(path)['sampling'] == 'gray'
        sizes.append((os.path.getsize(path), np.abs(got.astype(int) - img).mean()))
    assert sizes[0][0] < sizes[1][0] < sizes[2][0] and sizes[0][1] > sizes[1][1] > sizes[2][1]
    with pytest.raises(TypeError):
        jpeg.write_jpeg(str(tmp_path / 'x.jpg'), img.astype(np.float32))
    with pytest.raises(ValueError):
        jpeg.write_jpeg(str(tmp_path / 'x.jpg'), img, subsampling='411')


def test_random_pillow_files_decode_equal():
    """Widens the committed pin on machines that have Pillow: 60 seeded random images and save options."""
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(2024)
    for k in range(60):
        h, w = (int(v) for v in rng.integers(1, 65, 2))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if k % 3 else source(h, w, k)
        args = dict(quality=int(rng.integers(1, 101)), subsampling=int(rng.integers(0, 3)))
        which = int(rng.integers(0, 4))
        if which == 1:
            args['restart_marker_blocks'] = int(rng.integers(1, 9))
        elif which == 2:
            args['restart_marker_rows'] = int(rng.integers(1, 4))
        elif which == 3:
            args['optimize'] = True
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, 'JPEG', **args)
        want = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert('RGB'))
        assert np.array_equal(jpeg.read_jpeg(buf.getvalue()), want), (k, h, w, args)


def test_two_threads_decode_different_files_concurrently(expected):
    names = ['multigroup_96x160_420_q85_rstrows1', 'rstblocks3_48x80_444_q85']
    blobs = [blob(n) for n in names]
    results, errors = [[], []], []
    start = threading.Barrier(2)

    def work(i):
        try:
            start.wait()
            for _ in range(25):
                results[i].append(jpeg.read_jpeg(blobs[i]))
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for i, n in enumerate(names):
        assert len(results[i]) == 25 and all(np.array_equal(r, expected[n]) for r in results[i])


def test_the_abi_lives_in_a_header_of_its_own(stlib):
    from stereotracking_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'stereotrack_jpeg.h')) as f:
        text = f.read()
    for name in jpeg._PROTOS:
        assert hasattr(stlib, name) and name + '(' in text and name not in _lib._PROTOS
    assert jpeg._api().st_jpeg_reconstruct.argtypes[-1] is __import__('ctypes').c_void_p


def test_a_directory_of_jpeg_frames_reads_through_load_video(tmp_path):
    """tools/make_tiny_airdrone.py --jpeg: left / right as .jpg beside .png disparity and depth (the '.jpg' -> '.png' rule
    of the reference's selma_dataset.py:42-46); load_video reads it through the host decoder with no other change."""
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    from make_tiny_airdrone import make
    base, _ = make(str(tmp_path), videos=1, frames=3, height=48, width=96, max_disp=16, objects=2, jpeg=True)
    d = datasets.MOTDispDataset(ann_file='annotations/val_cocoformat_80.json', data_root=base + os.sep,
                                data_prefix=dict(img_path='val/'), depth_dir_name='depth')
    info = d.get_data_info(1)
    assert info['img_path'].endswith(os.path.join('left', '000001.jpg')) and info['right_path'].endswith(os.path.join('right', '000001.jpg'))
    assert info['disp_path'].endswith(os.path.join('disparity', '000001.png')) and info['depth_path'].endswith(os.path.join('depth', '000001.png'))
    for use_right in (True, False):
        seq, gts, metas, depth = datasets.load_video(d, d.video_indices()[0][1], use_right, with_depth=True, pin=False)
        assert tuple(seq.left.shape) == (3, 3, 48, 96) and depth.shape == (3, 48, 96) and len(gts) == len(metas) == 3
        want = jpeg.read_jpeg(info['img_path'])[..., ::-1].transpose(2, 0, 1)                      # BGR planes
        assert np.array_equal(seq.left[1].numpy(), want)
        if use_right:
            assert np.array_equal(seq.right[1].numpy(), jpeg.read_jpeg(info['right_path'])[..., ::-1].transpose(2, 0, 1))
