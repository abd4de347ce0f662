"""GPU: the JPEG reader's device half - jpeg.JpegDecoder on st_jpeg_reconstruct (csrc/jpeg_decode.hip), DESIGN.md 25.

Everything is an equality: against Pillow's recorded decode of tests/golden/jpeg, against the host routine
(st_jpeg_reconstruct_host, the executable specification) over a geometry sweep and over coefficients no encoder emits,
against tests/jpeg_ref.py; then batch independence, the memory contract of DESIGN.md 2 (guard bands, strided output
inside a wider buffer, stale work memory), stream ordering with slot reuse, and the wiring into test_step."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import guard_memory as gm
import jpeg_ref
from stereotracking_amd import jpeg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg')
CFG_RGB = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone.py')
with open(os.path.join(GOLDEN, 'manifest.json')) as _f:
    DECODABLE = sorted(n for n, m in json.load(_f)['files'].items() if m['decodable'])
# (h, w): one pixel, narrower than a quad, partial blocks, whole blocks, a width % 4 != 0 (the unaligned store path: every
# other row of a plane starts off a 4-byte boundary), several MCU rows and columns
SIZES = [(1, 1), (2, 3), (7, 9), (8, 8), (16, 16), (17, 13), (31, 33), (48, 80)]


@pytest.fixture(scope='module')
def expected():
    with np.load(os.path.join(GOLDEN, 'expected.npz')) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def decoder(cuda):
    return jpeg.JpegDecoder(device=cuda)


def blob(name):
    with open(os.path.join(GOLDEN, name + '.jpg'), 'rb') as f:
        return f.read()


def picture(h, w, seed=0):
    rng = np.random.default_rng(1000 * h + w + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), 255 - (xx + yy) * 255 // max(h + w - 2, 1)], -1)
    return np.clip(img + rng.integers(-30, 31, (h, w, 3)), 0, 255).astype(np.uint8)


def host_planes(data, order='bgr'):
    info, coef, quant = jpeg.entropy_decode(data)
    return jpeg.reconstruct_host(coef, quant, info, order=order, planar=True)


def device_reconstruct(info, coef, quant, cuda, out=None, work=None, order='bgr'):
    """st_jpeg_reconstruct on numpy coefficients (N, coef_count) int16 and tables (N, 3, 64) uint16."""
    lib = jpeg._api()
    n = coef.shape[0]
    c = torch.from_numpy(np.ascontiguousarray(coef)).to(cuda)
    q = torch.from_numpy(np.ascontiguousarray(quant).view(np.int16)).to(cuda)
    if work is None:
        work = torch.empty(int(lib.st_jpeg_work_bytes(C.byref(info), n)), dtype=torch.uint8, device=cuda)
    if out is None:
        out = torch.empty((n, 3, info.height, info.width), dtype=torch.uint8, device=cuda)
    rc = lib.st_jpeg_reconstruct(c.data_ptr(), q.data_ptr(), n, C.byref(info), work.data_ptr(), work.numel(), out.data_ptr(),
                                 out.stride(0), out.stride(1), out.stride(2), int(order == 'rgb'),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.st_last_error()
    return out


@pytest.mark.parametrize('name', DECODABLE)
def test_fixture_decodes_to_pillows_pixels(name, expected, decoder):
    want = torch.from_numpy(expected[name].transpose(2, 0, 1).copy())             # RGB planes
    bgr = decoder.decode([blob(name)])
    rgb = decoder.decode([blob(name)], order='rgb')
    assert bgr.dtype == torch.uint8 and bgr.is_cuda and tuple(bgr.shape) == (1,) + tuple(want.shape)
    assert torch.equal(rgb[0].cpu(), want)
    assert torch.equal(bgr[0].cpu(), want.flip(0))


@pytest.mark.parametrize('sampling', ['444', '422', '420', 'gray'])
@pytest.mark.parametrize('size', SIZES)
def test_geometry_sweep_device_equals_host_routine(size, sampling, decoder):
    img = picture(*size)
    for restart in (0, 1):
        data = jpeg.encode_jpeg(img[..., 1] if sampling == 'gray' else img, 90, '420' if sampling == 'gray' else sampling, restart)
        assert jpeg.jpeg_info(data)['sampling'] == sampling
        got = decoder.decode([data])
        assert torch.equal(got[0].cpu(), torch.from_numpy(host_planes(data))), (size, sampling, restart)


@pytest.fixture(scope='module')
def random_coefficients():
    """3 images of 24x40 4:2:0: int16 coefficients in [-2048, 2047] and a different table in [1, 255] per image - beyond
    what an encoder emits, so both clamps fire (and the 32-bit sums wrap)."""
    info = jpeg._info(jpeg.encode_jpeg(np.zeros((24, 40, 3), np.uint8), 90, '420'))
    rng = np.random.default_rng(77)
    coef = rng.integers(-2048, 2048, (3, int(info.coef_count))).astype(np.int16)
    quant = rng.integers(1, 256, (3, 3, 64)).astype(np.uint16)
    host = np.stack([jpeg.reconstruct_host(coef[i], quant[i], info, order='bgr', planar=True) for i in range(3)])
    return info, coef, quant, host


def test_random_coefficients_device_host_and_numpy_agree(random_coefficients, cuda):
    info, coef, quant, host = random_coefficients
    assert (host == 0).mean() > 0.05 and (host == 255).mean() > 0.05
    desc = dict(height=24, width=40, components=3, sampling='420', blocks=[(4, 6), (2, 3), (2, 3)],
                comp_shape=[(24, 40), (12, 20), (12, 20)])
    for i in range(3):
        ref = jpeg_ref.reconstruct(coef[i], quant[i], desc)                       # RGB, interleaved
        assert np.array_equal(ref[..., ::-1].transpose(2, 0, 1), host[i])
    got = device_reconstruct(info, coef, quant, cuda)
    assert torch.equal(got.cpu(), torch.from_numpy(host))
    # batch independence, and two runs byte-identical
    one = device_reconstruct(info, coef[:1], quant[:1], cuda)
    assert torch.equal(one[0], got[0])
    assert torch.equal(device_reconstruct(info, coef, quant, cuda), got)
    assert torch.equal(device_reconstruct(info, coef, quant, cuda, order='rgb'), got.flip(1))


@pytest.mark.parametrize('offset', [3, 4])
def test_memory_contract_guard_bands_strided_output_stale_work(random_coefficients, offset, cuda):
    """The output as a view inside a wider 0xFF buffer (rows off / on a 4-byte boundary, non-unit image, plane and row
    strides), itself inside guard bands; work memory stale 0xFF inside guard bands.  Result unchanged, every byte
    outside h x w of each plane untouched."""
    info, coef, quant, host = random_coefficients
    n, h, w = 3, info.height, info.width
    wide = gm.arena(torch.full((n, 4, h + 3, w + 9), 0xFF, dtype=torch.uint8), device=cuda)
    view = wide[:, 1:4, 2:2 + h, offset:offset + w]
    work_bytes = int(jpeg._api().st_jpeg_work_bytes(C.byref(info), n))
    assert work_bytes == n * int(info.work_bytes)
    work = gm.arena(torch.full((work_bytes,), 0xFF, dtype=torch.uint8), device=cuda)
    device_reconstruct(info, coef, quant, cuda, out=view, work=work)
    torch.cuda.synchronize()
    assert torch.equal(view.cpu(), torch.from_numpy(host))
    outside = wide.clone()
    outside[:, 1:4, 2:2 + h, offset:offset + w] = 0xFF
    assert bool((outside == 0xFF).all()), 'bytes outside h x w of the planes were written'
    assert gm.bands_intact(wide, work)
    # the decoder's `out` takes the same view; a too small work buffer is refused before any launch
    lib = jpeg._api()
    small = torch.empty(work_bytes - 16, dtype=torch.uint8, device=cuda)
    c = torch.from_numpy(coef).to(cuda)
    q = torch.from_numpy(quant.view(np.int16)).to(cuda)
    rc = lib.st_jpeg_reconstruct(c.data_ptr(), q.data_ptr(), n, C.byref(info), small.data_ptr(), small.numel(),
                                 view.data_ptr(), view.stride(0), view.stride(1), view.stride(2), 0,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == -4 and b'work memory' in lib.st_last_error()


def test_decode_into_a_given_view(decoder, cuda):
    data = [jpeg.encode_jpeg(picture(31, 33, s), 90, '420', 1) for s in range(2)]
    want = torch.from_numpy(np.stack([host_planes(d) for d in data]))
    wide = torch.full((2, 3, 40, 64), 0xFF, dtype=torch.uint8, device=cuda)
    view = wide[:, :, 5:36, 7:40]
    assert decoder.decode(data, out=view) is view
    assert torch.equal(view.cpu(), want)
    wide[:, :, 5:36, 7:40] = 0xFF
    assert bool((wide == 0xFF).all())
    with pytest.raises(ValueError, match='out must be'):
        decoder.decode(data, out=torch.empty((2, 3, 31, 32), dtype=torch.uint8, device=cuda))


def test_device_without_an_index_takes_out_tensors(cuda):
    """JpegDecoder(device='cuda') is the current device: an `out` tensor, whose device always carries its index, is taken."""
    data = [jpeg.encode_jpeg(picture(17, 13), 90, '422')]
    for device in ('cuda', None, 'cuda:0'):
        dec = jpeg.JpegDecoder(device=device, threads=1, slots=1)
        assert dec.dev == torch.device('cuda', torch.cuda.current_device())
        out = torch.empty((1, 3, 17, 13), dtype=torch.uint8, device=cuda)
        assert dec.decode(data, out=out) is out and torch.equal(out[0].cpu(), torch.from_numpy(host_planes(data[0])))
        dec.close()
    with pytest.raises(ValueError, match='GPU'):
        jpeg.JpegDecoder(device='cpu')


def test_a_failed_image_leaves_no_worker_writing_the_slot(cuda):
    """One image of a batch is corrupt: decode() raises only after every worker has finished, so the one staging slot is
    quiet when the next call fills it - whose result is right, ten times over."""
    good = [jpeg.encode_jpeg(picture(96, 160, s), 90, '420', 0) for s in range(6)]
    bad = good[0][:len(good[0]) * 6 // 10]
    want = torch.from_numpy(np.stack([host_planes(d) for d in good]))
    dec = jpeg.JpegDecoder(device=cuda, threads=4, slots=1)
    seen = []
    real = jpeg.entropy_decode

    def spy(data, coef, quant):
        try:
            return real(data, coef, quant)
        finally:
            seen.append(len(data))
    jpeg.entropy_decode = spy
    try:
        for _ in range(10):
            del seen[:]
            with pytest.raises(ValueError, match='truncated'):
                dec.decode([bad] + good[1:])
            assert len(seen) == 6                     # all six workers ran to their end before the error left decode()
            assert torch.equal(dec.decode(good).cpu(), want)
    finally:
        jpeg.entropy_decode = real
        dec.close()


def test_side_stream_and_slot_reuse(cuda):
    """Decode on a side stream while the default stream is busy, consume behind wait_stream; five calls in a row on two
    staging slots (each reused, the second time with a different batch size) against a one-slot decoder."""
    batches = [[jpeg.encode_jpeg(picture(48, 80, 10 * k + i), 90, '420', 0) for i in range(1 + k % 3)] for k in range(5)]
    want = [torch.from_numpy(np.stack([host_planes(d) for d in b])) for b in batches]
    two, one = jpeg.JpegDecoder(device=cuda, slots=2), jpeg.JpegDecoder(device=cuda, slots=1, threads=1)
    side = torch.cuda.Stream(device=cuda)
    busy = torch.randn(2048, 2048, device=cuda)
    torch.cuda.synchronize()
    outs = []
    for _ in range(4):
        busy = busy @ busy * 1e-3
    with torch.cuda.stream(side):
        for b in batches:
            outs.append(two.decode(b))
    torch.cuda.current_stream().wait_stream(side)
    copies = [o.clone() for o in outs]                  # consumed on the default stream
    single = [one.decode(b) for b in batches]
    torch.cuda.synchronize()
    for c, s, w in zip(copies, single, want):
        assert torch.equal(c.cpu(), w) and torch.equal(s.cpu(), w)
    assert two._k == 5 and all(sl['used'] for sl in two._slots)


def test_mixed_geometry_in_one_call_is_refused(decoder):
    a = jpeg.encode_jpeg(picture(16, 16), 90, '420')
    with pytest.raises(ValueError, match='image 2'):
        decoder.decode([a, a, jpeg.encode_jpeg(picture(16, 24), 90, '420')])
    with pytest.raises(ValueError, match='image 1'):
        decoder.decode([a, jpeg.encode_jpeg(picture(16, 16), 90, '444')])
    with pytest.raises(NotImplementedError, match='progressive'):
        decoder.decode([blob('refuse_progressive_33x31')])
    big = jpeg.encode_jpeg(picture(48, 80), 90, '420')         # large enough for 60 % of it to end inside the scan
    with pytest.raises(ValueError, match='truncated'):
        decoder.decode([big, big[:len(big) * 6 // 10]])
    assert torch.equal(decoder.decode([a, a])[1].cpu(), torch.from_numpy(host_planes(a)))      # and the decoder still works


def test_decoded_frames_through_test_step_equal_host_decoded_frames(tmp_path, decoder, cuda):
    """A 64x96 stereo pair written with write_jpeg, through the RGB-only config's test_step: frames decoded on the device
    against read_jpeg's frames uploaded as uint8 - every result array equal (seeded random weights)."""
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.structures import TrackDataSample
    from stereotracking_amd.synthetic import synthetic_batch, synthetic_state_dict
    ori = (64, 96)
    fr = synthetic_batch([60], ori[0], ori[1], 32)
    paths = []
    for key in ('img', 'right'):
        paths.append(str(tmp_path / f'{key}.jpg'))
        jpeg.write_jpeg(paths[-1], fr[key][0, :, :ori[0]].to(torch.uint8).permute(1, 2, 0).contiguous().numpy(), quality=90)
    datas = [open(p, 'rb').read() for p in paths]
    cfg = Config.fromfile(CFG_RGB)
    for part in ('backbone', 'neck'):
        cfg.model.detector[part]['widen_factor'] = 0.375
    cfg.model.detector.bbox_head.head_module['widen_factor'] = 0.375
    cfg.model.tracker['init_track_thr'] = 0.03
    cfg.model.tracker['obj_score_thr'] = 0.02
    model = MODELS.build(dict(cfg.model, autotune=False))
    assert model.detector.rgb_only
    model.detector.load_state_dict(synthetic_state_dict(list(model.detector._table), seed=5, prior_prob=0.2, logit_std=2.5),
                                   strict=False)
    on_device = decoder.decode(datas)                                              # (2, 3, 64, 96) BGR planes
    on_host = [torch.from_numpy(np.ascontiguousarray(jpeg.read_jpeg(d)[..., ::-1].transpose(2, 0, 1)))[None].to(cuda)
               for d in datas]
    assert torch.equal(on_device.cpu(), torch.cat(on_host).cpu())

    def run(frames):
        model.tracker.reset()
        samples = [TrackDataSample(dict(frame_id=t, ori_shape=ori, img_shape=ori, scale_factor=(1.0, 1.0))) for t in range(2)]
        inputs = dict(img=frames, disp_postp=[fr['disp_postp'][0:1, :, :ori[0]]] * 2,
                      disp_mask=[fr['disp_mask'][0:1, :, :ori[0]].to(torch.uint8)] * 2)
        outs = model.test_step(dict(inputs=inputs, data_samples=samples))
        torch.cuda.synchronize()
        return outs

    a = run([on_device[i:i + 1] for i in range(2)])
    b = run(on_host)
    assert len(a) == len(b) == 2 and sum(len(o.pred_det_instances) for o in a) > 0
    for x, y in zip(a, b):
        for part in ('pred_det_instances', 'pred_track_instances'):
            p, q = getattr(x, part), getattr(y, part)
            assert p.keys() == q.keys()
            for k in p.keys():
                u, v = p[k], q[k]
                if isinstance(u, torch.Tensor):
                    assert gm.same_bits(u, v), (part, k)
                else:
                    assert np.array_equal(np.asarray(u), np.asarray(v)), (part, k)
