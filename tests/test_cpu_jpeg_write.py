"""The JPEG writer's host path (stereotracking_amd/jpeg_write.py, csrc/jpeg_encode.cpp on jpeg_fwd_core.h) against the
files Pillow (libjpeg-turbo) wrote for the same pixels: tests/golden/jpeg_write, recorded by
tests/make_jpeg_write_golden.py.  No GPU."""
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest

from stereotracking_amd import jpeg, jpeg_write as jw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_write')
with open(os.path.join(GOLDEN, 'manifest.json')) as _f:
    MANIFEST = json.load(_f)
NAMES = sorted(MANIFEST['files'])
SUBSAMPLING = {0: '444', 1: '422', 2: '420'}


def fixture(name):
    """-> (source array, Pillow's bytes, encode_jpeg_host keyword arguments)"""
    with np.load(os.path.join(GOLDEN, 'sources.npz')) as z:
        src = z[name]
    with open(os.path.join(GOLDEN, name + '.jpg'), 'rb') as f:
        blob = f.read()
    save = MANIFEST['files'][name]['save']
    kw = dict(quality=save['quality'], restart_marker_rows=save.get('restart_marker_rows', 0))
    if src.ndim == 3:
        kw['subsampling'] = SUBSAMPLING[save['subsampling']]
    return src, blob, kw


def info_fields(info):
    return {name: (list(v) if hasattr(v, '__len__') else v) for name, v in
            ((name, getattr(info, name)) for name, _ in jpeg.StJpegInfo._fields_)}


def test_fixture_set_is_what_the_issue_lists():
    sizes = {(m['height'], m['width']) for m in MANIFEST['files'].values()}
    assert sizes >= {(1, 1), (2, 3), (7, 9), (8, 8), (16, 16), (17, 13), (31, 33), (48, 80)}
    saves = [m['save'] for m in MANIFEST['files'].values()]
    assert {s['quality'] for s in saves} == {1, 30, 85, 100}
    assert {s.get('subsampling') for s in saves} == {0, 1, 2, None}
    assert any(m['mode'] == 'L' for m in MANIFEST['files'].values())
    assert any(s.get('restart_marker_rows') == 1 for s in saves)
    assert all(s['optimize'] is False for s in saves)
    total = 0
    for n in NAMES:
        size = os.path.getsize(os.path.join(GOLDEN, n + '.jpg'))
        assert size < 12 * 1024
        total += size
    assert total < 150 * 1024


@pytest.mark.parametrize('name', NAMES)
def test_host_encode_equals_fixture_bytes(name):
    src, blob, kw = fixture(name)
    assert jw.encode_jpeg_host(src, **kw) == blob


@pytest.mark.parametrize('name', NAMES)
def test_forward_host_equals_fixture_coefficients(name):
    """the WHOLE padded array, dummy blocks included, and the tables"""
    src, blob, kw = fixture(name)
    info, coef, quant = jpeg.entropy_decode(blob)
    nc = 1 if src.ndim == 2 else 3
    mine = jw.encode_geometry(src.shape[0], src.shape[1], nc, kw.get('subsampling', '420'), info.restart_interval)
    assert info_fields(info) == info_fields(mine)
    q = jw.quant_tables(kw['quality'])
    assert np.array_equal(q[:nc], quant[:nc])
    got = jw.forward_host(src, q, mine)
    assert got.shape == coef.shape and np.array_equal(got, coef)


def test_bgr_order_reads_the_same_pixels():
    src, blob, kw = fixture('quality_17x13_420_q85')
    assert jw.encode_jpeg_host(np.ascontiguousarray(src[..., ::-1]), order='bgr', **kw) == blob


@pytest.mark.parametrize('name', NAMES)
def test_round_trip_through_the_projects_reader(name):
    src, blob, kw = fixture(name)
    mine = jw.encode_jpeg_host(src, **kw)
    back = jpeg.read_jpeg(mine)
    assert back.shape == src.shape and back.dtype == np.uint8
    info, coef, quant = jpeg.entropy_decode(mine)
    nc = 1 if src.ndim == 2 else 3
    info2 = jw.encode_geometry(src.shape[0], src.shape[1], nc, kw.get('subsampling', '420'), info.restart_interval)
    assert np.array_equal(coef, jw.forward_host(src, quant, info2))      # lossless from the coefficients on
    want = jpeg.reconstruct_host(coef, quant, info, order='rgb')
    assert np.array_equal(back, want[..., 0] if nc == 1 else want)


def test_pillow_sweep_byte_for_byte():
    """every (h, w) in 1..18 x 1..18, each sampling and gray: our bytes equal Pillow's, so Pillow's decode of our file
    equals Pillow's decode of its own (checked on the bytes and, for one file per size, on the pixels)"""
    pytest.importorskip('PIL')
    from PIL import Image
    rng = np.random.default_rng(5)
    qualities = (1, 30, 85, 100)
    k = 0
    for h in range(1, 19):
        for w in range(1, 19):
            a = np.clip(rng.integers(0, 256, (1, 1, 3)) + rng.integers(-90, 91, (h, w, 3)), 0, 255).astype(np.uint8)
            for s, sub in (('444', 0), ('422', 1), ('420', 2), ('gray', None)):
                k += 1
                q, rr = qualities[k % 4], (k // 4) % 2
                buf = io.BytesIO()
                if sub is None:
                    Image.fromarray(a[..., 1].copy(), 'L').save(buf, 'JPEG', quality=q, optimize=False, restart_marker_rows=rr)
                    mine = jw.encode_jpeg_host(a[..., 1].copy(), q, restart_marker_rows=rr)
                else:
                    Image.fromarray(a, 'RGB').save(buf, 'JPEG', quality=q, subsampling=sub, optimize=False, restart_marker_rows=rr)
                    mine = jw.encode_jpeg_host(a, q, s, restart_marker_rows=rr)
                assert mine == buf.getvalue(), (h, w, s, q, rr)
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(mine))), np.asarray(Image.open(buf)))


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refuses_wrong_dtype_and_shape():
    with pytest.raises(TypeError, match='uint8'):
        jw.encode_jpeg_host(np.zeros((8, 8, 3), np.float32))
    with pytest.raises(TypeError, match='uint8'):
        jw.encode_jpeg_host(np.zeros((8, 8, 4), np.uint8))
    with pytest.raises(TypeError, match='uint8'):
        jw.encode_jpeg_host(np.zeros((8,), np.uint8))


def test_refuses_bad_sizes_and_sampling():
    with pytest.raises(ValueError, match='1..65535'):
        jw.encode_jpeg_host(np.zeros((0, 8, 3), np.uint8))
    with pytest.raises(ValueError, match='1..65535'):
        jw.encode_geometry(65536, 8)
    with pytest.raises(ValueError, match='1..65535'):
        jw.encode_geometry(8, 0)
    with pytest.raises(ValueError, match='subsampling'):
        jw.encode_jpeg_host(np.zeros((8, 8, 3), np.uint8), subsampling='411')
    info = jpeg.StJpegInfo(struct_size=C.sizeof(jpeg.StJpegInfo))
    with pytest.raises(ValueError, match='unknown sampling'):
        jpeg._check(jw._api().st_jpeg_encode_geometry(8, 8, 3, 7, 0, C.byref(info)), 'x')
    with pytest.raises(ValueError, match='unknown sampling'):
        jpeg._check(jw._api().st_jpeg_encode_geometry(8, 8, 3, 0, 0, C.byref(info)), 'x')
    with pytest.raises(ValueError, match='restart_interval'):
        jw.encode_geometry(8, 8, 3, '420', 65536)


def test_refuses_a_struct_that_is_not_the_geometry():
    info = jw.encode_geometry(17, 13)
    info.blocks_w[0] += 1
    with pytest.raises(ValueError, match='st_jpeg_encode_geometry'):
        jw.forward_host(np.zeros((17, 13, 3), np.uint8), jw.quant_tables(90), info)
    info = jw.encode_geometry(17, 13)
    info.struct_size -= 4
    with pytest.raises(ValueError, match='struct_size'):
        jw.entropy_encode(np.zeros(int(info.coef_count), np.int16), jw.quant_tables(90), info)


def test_refuses_small_capacity_and_bad_coefficients():
    info = jw.encode_geometry(17, 13)
    bound = int(jw._api().st_jpeg_encode_bound(C.byref(info)))
    assert bound == 1024 + 416 * (int(info.coef_count) // 64) + 4 * info.mcus_x * info.mcus_y
    coef, q = np.zeros(int(info.coef_count), np.int16), jw.quant_tables(90)
    with pytest.raises(Exception, match=f'capacity of {bound - 1} bytes, {bound} needed'):
        jw.entropy_encode(coef, q, info, np.empty(bound - 1, np.uint8))
    assert jw.entropy_encode(coef, q, info, np.empty(bound, np.uint8))[:2] == b'\xff\xd8'
    coef[5] = 1024
    with pytest.raises(ValueError, match='baseline range'):
        jw.entropy_encode(coef, q, info)
    coef[5] = 0
    q[0, 3] = 256
    with pytest.raises(ValueError, match='1..255'):
        jw.entropy_encode(coef, q, info)


def test_worst_case_block_fits_the_bound():
    """every coefficient at the largest magnitude, alternating sign: the longest codes, and FF bytes to stuff"""
    info = jw.encode_geometry(16, 16, 3, '444')
    coef = np.full(int(info.coef_count), 1023, np.int16)
    coef[1::2] = -1023
    blob = jw.entropy_encode(coef, jw.quant_tables(100), info)
    assert len(blob) <= int(jw._api().st_jpeg_encode_bound(C.byref(info)))
    assert np.array_equal(jpeg.entropy_decode(blob)[1], coef)


def test_misaligned_dev_pointers_are_refused_by_name():
    """st_jpeg_forward's 16-byte pointers, passed as host memory at +4 bytes: refused on the host before any launch"""
    info = jw.encode_geometry(8, 8)
    buf = np.zeros(4096, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data % 16)
    for quant, coef in ((base + 4, base + 1024), (base, base + 1024 + 4)):
        rc = jw._api().st_jpeg_forward(base + 2048, 192, 64, 8, 0, quant, 1, C.byref(info), coef, None)
        assert rc == -1
        with pytest.raises(ValueError, match='quant_dev and coef_dev must be 16-byte aligned'):
            jpeg._check(rc, 'st_jpeg_forward')


# ---- the new header's pointer contract -------------------------------------------------------------------------------
# every pointer parameter of include/stereotrack_vis.h: 'host', or for `_dev` pointers 'aligned16' / 'aligned4' (refused
# by name when misaligned) or 'bytes' (accessed element-sized, no alignment asked)
VIS_POINTERS = {
    ('st_jpeg_encode_geometry', 'info'): 'host',
    ('st_jpeg_quant_tables', 'quant_out'): 'host',
    ('st_jpeg_forward_host', 'pixels'): 'host', ('st_jpeg_forward_host', 'quant'): 'host',
    ('st_jpeg_forward_host', 'info'): 'host', ('st_jpeg_forward_host', 'coef_out'): 'host',
    ('st_jpeg_forward', 'in_dev'): 'bytes', ('st_jpeg_forward', 'quant_dev'): 'aligned16',
    ('st_jpeg_forward', 'info'): 'host', ('st_jpeg_forward', 'coef_dev'): 'aligned16',
    ('st_jpeg_encode_bound', 'info'): 'host',
    ('st_jpeg_entropy_encode', 'coef'): 'host', ('st_jpeg_entropy_encode', 'quant'): 'host',
    ('st_jpeg_entropy_encode', 'info'): 'host', ('st_jpeg_entropy_encode', 'out'): 'host',
    ('st_jpeg_entropy_encode', 'out_bytes'): 'host',
    ('st_draw_tracks', 'frames_dev'): 'bytes', ('st_draw_tracks', 'boxes_dev'): 'aligned4',
    ('st_draw_tracks', 'counts_dev'): 'aligned4',
}


def test_every_pointer_of_the_new_header_has_a_contract_row():
    with open(os.path.join(ROOT, 'include', 'stereotrack_vis.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    found = set()
    for m in re.finditer(r'\b(?:int|size_t)\s+(st_\w+)\s*\(([^)]*)\)\s*;', text):
        for arg in m.group(2).split(','):
            if '*' in arg:
                found.add((m.group(1), re.findall(r'\w+', arg)[-1]))
    assert found == set(VIS_POINTERS)
    for (fn, arg), kind in VIS_POINTERS.items():
        assert (kind == 'host') == (not arg.endswith('_dev')), (fn, arg)
    # the aligned ones are named in the refusal message of their entry point
    for src in ('jpeg_forward.hip', 'draw_tracks.hip'):
        with open(os.path.join(ROOT, 'stereotracking_amd', 'csrc', src)) as f:
            code = f.read()
        for (fn, arg), kind in VIS_POINTERS.items():
            if kind.startswith('aligned') and f'"{fn}:' in code:
                assert re.search(rf'"{fn}: [^"]*\b{arg}\b[^"]*must be {kind[7:]}-byte aligned"', code), (fn, arg)


def test_exports_are_bound_outside_the_main_table():
    from stereotracking_amd import _lib
    assert not set(jw._PROTOS) & set(_lib._PROTOS)
    lib = jw._api()
    for name in jw._PROTOS:
        assert getattr(lib, name).argtypes is not None
