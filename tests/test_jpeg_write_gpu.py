"""GPU: the JPEG writer's device half - jpeg_write.JpegEncoder on st_jpeg_forward (csrc/jpeg_forward.hip), DESIGN.md 26.

Everything is an equality: the device coefficients against the host routine (st_jpeg_forward_host, the executable
specification) on every fixture source and over a geometry sweep in both channel orders; the encoder's bytes against
Pillow's recorded files (tests/golden/jpeg_write); the round trip through JpegDecoder against the host reconstruction;
then batch independence, repeatability, the memory contract of DESIGN.md 2 (guard bands, strided input inside a wider
buffer at non-zero offsets, stale output) and stream ordering with slot reuse."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import guard_memory as gm
from stream_pool import keep_pool_position  # noqa: F401  (autouse: the streams this module takes shift no later test's)
from stereotracking_amd import jpeg, jpeg_write as jw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_write')
with open(os.path.join(GOLDEN, 'manifest.json')) as _f:
    MANIFEST = json.load(_f)['files']
NAMES = sorted(MANIFEST)
SUBSAMPLING = {0: '444', 1: '422', 2: '420'}
# (h, w): one pixel, partial blocks, whole blocks, widths % 4 != 0, dummy luma blocks (17x13 at 4:2:0: 3 x 2 real blocks
# in a 4 x 2 grid), several MCU rows and columns (48x80: 90 blocks at 4:2:0, more than one workgroup of 32)
SIZES = [(1, 1), (2, 3), (7, 9), (8, 8), (16, 16), (17, 13), (31, 33), (48, 80)]


@pytest.fixture(scope='module')
def sources():
    with np.load(os.path.join(GOLDEN, 'sources.npz')) as z:
        return {k: z[k] for k in z.files}


def fixture_args(name):
    save = MANIFEST[name]['save']
    return save['quality'], SUBSAMPLING.get(save.get('subsampling'), '420'), save.get('restart_marker_rows', 0)


def fixture_bytes(name):
    with open(os.path.join(GOLDEN, name + '.jpg'), 'rb') as f:
        return f.read()


def picture(h, w, seed=0):
    rng = np.random.default_rng(1000 * h + w + seed)
    return np.clip(rng.integers(0, 256, (1, 1, 3)) + rng.integers(-80, 81, (h, w, 3)), 0, 255).astype(np.uint8)


def planar(src, order):
    """host (H, W, 3) RGB or (H, W) gray -> (1, C, H, W) uint8 tensor with planes in `order`"""
    if src.ndim == 2:
        return torch.from_numpy(np.ascontiguousarray(src))[None, None]
    a = src if order == 'rgb' else src[..., ::-1]
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))[None]


def device_forward(frames, quality, subsampling, order, coef=None):
    """st_jpeg_forward on a (N, C, H, W) device view -> (info, quant, coef (N, coef_count) device tensor)"""
    n, nc, h, w = frames.shape
    info = jw.encode_geometry(h, w, nc, subsampling)
    quant = jw.quant_tables(quality)
    qd = torch.from_numpy(quant.view(np.int16)).to(frames.device)
    if coef is None:
        coef = torch.full((n, int(info.coef_count)), 0x5A5A, dtype=torch.int16, device=frames.device)      # stale
    jw.forward_device(frames, qd, info, coef, order)
    return info, quant, coef


def host_forward(src, quality, subsampling):
    nc = 1 if src.ndim == 2 else 3
    info = jw.encode_geometry(src.shape[0], src.shape[1], nc, subsampling)
    return jw.forward_host(src, jw.quant_tables(quality), info)


@pytest.mark.parametrize('name', NAMES)
def test_forward_equals_host_on_fixture_sources(name, sources, cuda):
    src = sources[name]
    q, s, _ = fixture_args(name)
    _, _, coef = device_forward(planar(src, 'bgr').to(cuda), q, s, 'bgr')
    assert np.array_equal(coef.cpu().numpy()[0], host_forward(src, q, s))


@pytest.mark.parametrize('order', ['bgr', 'rgb'])
@pytest.mark.parametrize('sampling', ['444', '422', '420', 'gray'])
def test_forward_equals_host_over_geometries(sampling, order, cuda):
    for k, (h, w) in enumerate(SIZES):
        src = picture(h, w, k)
        if sampling == 'gray':
            src = np.ascontiguousarray(src[..., 0])
        q = (1, 30, 85, 100)[k % 4]
        _, _, coef = device_forward(planar(src, order).to(cuda), q, sampling, order)
        assert np.array_equal(coef.cpu().numpy()[0], host_forward(src, q, sampling)), (h, w, sampling, order, q)


@pytest.mark.parametrize('name', NAMES)
def test_encoder_bytes_equal_fixture_bytes(name, sources, cuda):
    src = sources[name]
    q, s, rr = fixture_args(name)
    enc = jw.JpegEncoder(cuda, quality=q, subsampling=s)
    try:
        got = enc.encode(planar(src, 'bgr').to(cuda), order='bgr', restart_marker_rows=rr)
    finally:
        enc.close()
    assert got == [fixture_bytes(name)]


def test_round_trip_on_the_device(cuda):
    """JpegDecoder.decode(JpegEncoder.encode(x)) equals the host reconstruction of the same coefficients"""
    enc, dec = jw.JpegEncoder(cuda, quality=85, subsampling='420'), jpeg.JpegDecoder(device=cuda)
    try:
        src = np.stack([picture(31, 33, i) for i in range(2)])
        x = torch.from_numpy(np.ascontiguousarray(src[..., ::-1].transpose(0, 3, 1, 2))).to(cuda)
        blobs = enc.encode(x)
        back = dec.decode(blobs).cpu().numpy()
    finally:
        enc.close()
        dec.close()
    for i, b in enumerate(blobs):
        info, coef, quant = jpeg.entropy_decode(b)
        assert np.array_equal(coef, host_forward(src[i], 85, '420'))
        assert np.array_equal(back[i], jpeg.reconstruct_host(coef, quant, info, order='bgr', planar=True))


def test_batch_independence_and_repeatability(cuda):
    src = [picture(17, 13, i) for i in range(3)]
    x = torch.cat([planar(s, 'bgr') for s in src]).to(cuda)
    _, _, c3 = device_forward(x, 85, '420', 'bgr')
    _, _, c1 = device_forward(x[:1], 85, '420', 'bgr')
    _, _, again = device_forward(x, 85, '420', 'bgr')
    assert torch.equal(c3[0], c1[0])
    assert torch.equal(c3, again)
    for i in range(3):
        assert np.array_equal(c3[i].cpu().numpy(), host_forward(src[i], 85, '420'))


@pytest.mark.parametrize('sampling', ['444', '420'])
def test_memory_contract_guard_bands_strided_input_stale_output(sampling, cuda):
    """Input planes inside a wider buffer (non-zero offsets, row_stride > width, a width % 4 != 0) whose every other byte
    is 0xFF; coefficients stale inside guard bands.  Result unchanged, every element written, bands and the input intact.
    The forward launch has no work memory."""
    n, h, w = 2, 17, 13
    src = [picture(h, w, 7 + i) for i in range(n)]
    wide = gm.arena(torch.full((n, 4, h + 3, w + 9), 0xFF, dtype=torch.uint8), device=cuda)
    view = wide[:, 1:4, 2:2 + h, 5:5 + w]
    view.copy_(torch.cat([planar(s, 'bgr') for s in src]).to(cuda))
    before = wide.clone()
    info = jw.encode_geometry(h, w, 3, sampling)
    coef = gm.arena(torch.full((n, int(info.coef_count)), -1, dtype=torch.int16), device=cuda)
    device_forward(view, 30, sampling, 'bgr', coef)
    torch.cuda.synchronize()
    assert gm.bands_intact(wide, coef)
    assert torch.equal(wide, before)
    for i in range(n):
        assert np.array_equal(coef[i].cpu().numpy(), host_forward(src[i], 30, sampling))


def test_misaligned_device_pointers_are_refused(cuda):
    x = planar(picture(8, 8), 'bgr').to(cuda)
    info = jw.encode_geometry(8, 8, 3, '420')
    qd = torch.zeros(192 + 8, dtype=torch.int16, device=cuda)
    coef = torch.zeros(int(info.coef_count) + 8, dtype=torch.int16, device=cuda)
    for q, c in ((qd[2:], coef), (qd, coef[2:])):
        with pytest.raises(ValueError, match='quant_dev and coef_dev must be 16-byte aligned'):
            jw.forward_device(x, q, info, c[:int(info.coef_count)].view(1, -1), 'bgr')


def test_stream_ordering_with_slot_reuse(cuda):
    """three consecutive encode calls on a side stream, two slots: the third reuses the first's staging memory"""
    enc = jw.JpegEncoder(cuda, slots=2, quality=85, subsampling='422')
    src = [picture(31, 33, 20 + i) for i in range(3)]
    side = torch.cuda.Stream(cuda)
    try:
        with torch.cuda.stream(side):
            frames = [planar(s, 'bgr').to(cuda, non_blocking=True) for s in src]
            got = [enc.encode(f)[0] for f in frames]
        side.synchronize()
    finally:
        enc.close()
    assert got == [jw.encode_jpeg_host(s, 85, '422') for s in src]
