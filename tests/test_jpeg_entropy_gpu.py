"""GPU: the device entropy decoder - jpeg.JpegDecoder(entropy='device') on st_jpeg_entropy_decode_dev
(csrc/jpeg_entropy.hip over csrc/jpeg_entropy_core.h), DESIGN.md 25 "Entropy decode on the device".

Every comparison is an equality against jpeg.entropy_decode, the host routine, on the same bytes: status non-zero
exactly when the host raises, and coefficients and tables equal element for element where it accepts.  No tolerances.
The inputs were chosen with the CPU emulation (tests/native/jpeg_entropy_check.cpp) so that the stated preconditions
hold; each test asserts its precondition before it compares."""
import contextlib
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import guard_memory as gm
from stereotracking_amd import jpeg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg')
with open(os.path.join(GOLDEN, 'manifest.json')) as _f:
    DECODABLE = sorted(n for n, m in json.load(_f)['files'].items() if m['decodable'])
SMALL = (16, 4)           # 64-byte tiles: the golden files span several
MANY = (16, 64)


@pytest.fixture(scope='module')
def expected():
    with np.load(os.path.join(GOLDEN, 'expected.npz')) as z:
        return {k: z[k] for k in z.files}


def blob(name):
    with open(os.path.join(GOLDEN, name + '.jpg'), 'rb') as f:
        return f.read()


def picture(h, w, seed=0):
    rng = np.random.default_rng(1000 * h + w + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), 255 - (xx + yy) * 255 // max(h + w - 2, 1)], -1)
    return np.clip(img + rng.integers(-30, 31, (h, w, 3)), 0, 255).astype(np.uint8)


_noise = {}


def noise(h, w, sampling):
    """Seeded noise at quality 100: a long scan of long codes, dense in FF bytes."""
    if (h, w, sampling) not in _noise:
        rng = np.random.default_rng(1000 * h + w)
        _noise[h, w, sampling] = jpeg.encode_jpeg(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), 100, sampling)
    return _noise[h, w, sampling]


def scan_of(data):
    d = jpeg.entropy_prepare(data)
    return d.scan_offset, np.frombuffer(data, np.uint8, d.scan_bytes, d.scan_offset)


def host(data):
    """(coef, quant) of the host routine, or the exception it raises."""
    try:
        _, coef, quant = jpeg.entropy_decode(data)
        return coef, quant
    except ValueError as e:
        return e


def device(datas, cuda, setting=(None, None)):
    info, coef, quant, status, stats = jpeg.entropy_decode_device(datas, cuda, *setting)
    torch.cuda.synchronize()
    return coef.cpu().numpy(), quant.cpu().numpy().view(np.uint16), status.cpu().numpy(), stats.cpu().numpy()


def assert_equals_host(datas, cuda, setting=(None, None), labels=None):
    """One device call over `datas` against the host routine per image -> (accepted count, stats)."""
    coef, quant, status, stats = device(datas, cuda, setting)
    accepted = 0
    for i, data in enumerate(datas):
        what = (labels[i] if labels else i, setting)
        want = host(data)
        if isinstance(want, Exception):
            assert status[i] != 0, (what, 'the host refuses', str(want))
        else:
            assert status[i] == 0, (what, 'the host accepts, device status', int(status[i]))
            assert np.array_equal(coef[i], want[0]), what
            assert np.array_equal(quant[i], want[1]), what
            accepted += 1
    return accepted, stats


# ---- golden files ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', DECODABLE)
def test_golden_file_coefficients_tables_status_and_pixels(name, expected, cuda):
    data = blob(name)
    for setting in ((None, None), SMALL):
        accepted, stats = assert_equals_host([data], cuda, setting)
        assert accepted == 1 and stats[0, 1] == -(-len(scan_of(data)[1]) // (setting[0] or 32))
    on_device, on_host = jpeg.JpegDecoder(device=cuda, entropy='device'), jpeg.JpegDecoder(device=cuda)
    got = on_device.decode([data], order='rgb')
    assert torch.equal(got[0].cpu(), torch.from_numpy(expected[name].transpose(2, 0, 1).copy()))
    assert torch.equal(on_device.decode([data]), on_host.decode([data]))
    assert on_device.last_status.dtype == torch.int32 and on_device.last_status.is_cuda and on_device.last_status.tolist() == [0]
    on_device.close()
    on_host.close()


# ---- several tiles, slow synchronisation, stuffing on a subsequence boundary -----------------------------------------------
@pytest.mark.parametrize('sampling', ['444', '420'])
@pytest.mark.parametrize('size', [(48, 80), (96, 160)])
def test_noise_spans_tiles_and_needs_passes(size, sampling, cuda):
    data = noise(*size, sampling)
    accepted, stats = assert_equals_host([data], cuda, MANY)
    tiles, subsequences, max_passes, sum_passes = (int(v) for v in stats[0])
    print(f'{size} {sampling}: scan {len(scan_of(data)[1])} bytes, {tiles} tiles, {subsequences} subsequences, '
          f'max passes {max_passes}, mean {sum_passes / tiles:.2f}')
    assert accepted == 1
    assert tiles >= 3 and max_passes >= 2, 'the sync loop and the tile carry were not exercised'
    assert max_passes <= 64 and tiles <= sum_passes <= 64 * tiles
    if size == (48, 80) and sampling == '444':
        assert tiles == 16


@pytest.mark.parametrize('size', [(48, 80), (96, 160)])
def test_stuffing_pairs_split_by_a_subsequence_boundary(size, cuda):
    data = noise(*size, '444')
    _, scan = scan_of(data)
    pairs = np.nonzero((scan[:-1] == 0xFF) & (scan[1:] == 0x00))[0]
    split = int((pairs % 16 == 15).sum())
    print(f'{size}: {len(pairs)} FF 00 pairs, {split} with the FF as the last byte of a 16-byte subsequence')
    assert split >= 1
    for setting in (MANY, SMALL, (16, 256)):
        assert assert_equals_host([data], cuda, setting)[0] == 1


# ---- restart intervals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sampling', ['444', '422', '420'])
def test_restart_intervals(sampling, cuda):
    img = picture(40, 72)
    mcus_x = jpeg.jpeg_info(jpeg.encode_jpeg(img, 90, sampling))['mcus'][1]
    datas = [jpeg.encode_jpeg(img, 90, sampling, ri) for ri in (1, 3, mcus_x)]
    assert [jpeg.jpeg_info(d)['restart_interval'] for d in datas] == [1, 3, mcus_x]
    for setting in ((None, None), SMALL):
        assert assert_equals_host(datas, cuda, setting)[0] == 3
    # FF fill bytes in front of a marker: the host skips them, so does the device (also where they fill a whole subsequence)
    for fills in (1, 2, 40):
        filled = []
        for d in datas:
            off, scan = scan_of(d)
            p = off + bytes(scan).index(b'\xff\xd0')
            filled.append(d[:p] + b'\xff' * fills + d[p:])
        assert not isinstance(host(filled[0]), Exception)
        assert assert_equals_host(filled, cuda, SMALL)[0] == 3


@pytest.mark.parametrize('name', ['rstblocks3_48x80_420_q85', 'rstblocks3_48x80_422_q85', 'rstblocks3_48x80_444_q85',
                                  'rstrows1_33x31_420_q30', 'multigroup_96x160_420_q85_rstrows1'])
def test_golden_restart_files_at_every_setting(name, cuda):
    for setting in ((None, None), SMALL, MANY, (8, 1), (24, 7)):
        assert assert_equals_host([blob(name)], cuda, setting)[0] == 1


# ---- tiny and odd inputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sampling', ['444', '422', '420', 'gray'])
def test_tiny_and_odd_sizes(sampling, cuda):
    for size in ((1, 1), (2, 3), (17, 13)):
        img = picture(*size)
        data = jpeg.encode_jpeg(img[..., 1] if sampling == 'gray' else img, 90, '420' if sampling == 'gray' else sampling)
        for setting in ((None, None), SMALL):
            assert assert_equals_host([data], cuda, setting)[0] == 1


def test_a_scan_shorter_than_one_subsequence_and_long_codes(cuda):
    flat = jpeg.encode_jpeg(np.full((8, 8, 3), 128, np.uint8), 90, '444')
    assert len(scan_of(flat)[1]) < 16                        # scan + EOI
    for setting in ((None, None), SMALL):
        accepted, stats = assert_equals_host([flat], cuda, setting)
        assert accepted == 1 and tuple(stats[0]) == (1, 1, 1, 1)
    for name in [n for n in DECODABLE if n.startswith('opt_')]:
        d = jpeg.entropy_prepare(blob(name))
        assert any((np.ctypeslib.as_array(d.ac[s].fast) == 0).any() for s in set(d.ac_slot)), 'no code longer than 9 bits'
        assert assert_equals_host([blob(name)], cuda, SMALL)[0] == 1


# ---- batch -----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def permuted_tables(seed):
    """The numpy encoder with other Huffman tables: the Annex K code lengths with the symbols dealt to the codes in a
    seeded order (a complete prefix code over the same symbols; frequent symbols get 16-bit codes)."""
    names = ('_DC_LUMA', '_DC_CHROMA', '_AC_LUMA', '_AC_CHROMA')
    saved = {n: getattr(jpeg, n) for n in names}
    rng = np.random.default_rng(seed)
    try:
        for n in names:
            bits, vals = saved[n]
            setattr(jpeg, n, (bits, [int(v) for v in rng.permutation(vals)]))
        yield
    finally:
        for n in names:
            setattr(jpeg, n, saved[n])


def test_batch_of_different_content_tables_and_lengths(cuda):
    datas = [blob('opt_33x31_420_q85'), blob('rgb_33x31_420_q30'), blob('rstrows1_33x31_420_q30')]
    for seed in (1, 2):
        with permuted_tables(seed):
            datas.append(jpeg.encode_jpeg(picture(33, 31, seed), 95, '420', seed - 1))
    tables = {bytes(jpeg.entropy_prepare(d).ac[0].vals) for d in datas}
    assert len(tables) >= 4 and len({len(scan_of(d)[1]) for d in datas}) >= 4
    for setting in ((None, None), SMALL):
        coef, quant, status, stats = device(datas, cuda, setting)
        assert assert_equals_host(datas, cuda, setting)[0] == 5
        for i, d in enumerate(datas):                          # each equal to its own single-image call (N = 1)
            c1, q1, s1, t1 = device([d], cuda, setting)
            assert np.array_equal(c1[0], coef[i]) and np.array_equal(q1[0], quant[i]) and s1[0] == status[i] == 0
            assert np.array_equal(t1[0], stats[i])


# ---- refusals --------------------------------------------------------------------------------------------------------------
def corruptions(name):
    """[(label, bytes)] of one base file; all keep its headers, so one call decodes them together."""
    data = blob(name)
    off, scan = scan_of(data)
    scan = bytes(scan)
    out = []
    for pct in (30, 60, 90):
        out.append((f'cut at {pct} %', data[:len(data) * pct // 100]))
    rng = np.random.default_rng(len(data))
    for k in range(40):
        p, bit = off + int(rng.integers(0, len(scan) - 2)), int(rng.integers(0, 8))
        d = bytearray(data)
        d[p] ^= 1 << bit
        out.append((f'flip {k}: byte {p} bit {bit}', bytes(d)))
    rst = [off + i for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    if rst:
        p = rst[len(rst) // 2]
        out.append(('RSTn removed', data[:p] + data[p + 2:]))
        first = bytearray(data)
        first[rst[0] + 1] = 0xD3
        out.append(('RST0 renumbered RST3', bytes(first)))
        out.append(('a byte in front of an RSTn', data[:p] + b'\x55' + data[p:]))
        out.append(('an RSTn twice', data[:p] + data[p:p + 2] + data[p:]))
    else:
        p = off + len(scan) // 2
        while data[p - 1] == 0xFF or data[p] == 0xFF:          # not inside a stuffing pair
            p += 1
        out.append(('an RSTn in a file without DRI', data[:p] + b'\xff\xd0' + data[p:]))
        out.append(('an RSTn behind the last MCU of a file without DRI', data[:-2] + b'\xff\xd0' + data[-2:]))
    return out


@pytest.mark.parametrize('name', ['rgb_48x80_420_q85', 'rstblocks3_48x80_444_q85', 'gray_33x31_q85'])
def test_corruptions_are_refused_exactly_when_the_host_refuses(name, cuda):
    cases = corruptions(name)
    in_headers = [(label, d) for label, d in cases if isinstance(_header(d), Exception)]
    in_scan = [(label, d) for label, d in cases if not isinstance(_header(d), Exception)]
    for label, d in in_headers:                                  # a cut inside the headers: refused before any launch
        with pytest.raises(ValueError):
            jpeg.entropy_decode_device([d], cuda)
    assert len(in_scan) >= 44
    labels, datas = [c[0] for c in in_scan], [c[1] for c in in_scan]
    verdicts = [isinstance(host(d), Exception) for d in datas]
    print(f'{name}: {len(datas)} corruptions, the host refuses {sum(verdicts)}')
    assert 0 < sum(verdicts) and (name == 'gray_33x31_q85' or sum(verdicts) < len(verdicts))
    for setting in ((None, None), SMALL):
        assert_equals_host(datas, cuda, setting, labels)


def _header(data):
    try:
        return jpeg._info(data)
    except (ValueError, NotImplementedError) as e:
        return e


def test_corruption_families_fall_as_the_host_says(cuda):
    """The structural families one by one, with the host's verdict spelled out (not only mirrored)."""
    by_label = dict(corruptions('rstblocks3_48x80_444_q85') + corruptions('rgb_48x80_420_q85'))
    for label, refused in (('RSTn removed', True), ('RST0 renumbered RST3', True), ('a byte in front of an RSTn', True),
                           ('an RSTn twice', True), ('an RSTn in a file without DRI', True),
                           ('an RSTn behind the last MCU of a file without DRI', False), ('cut at 60 %', True)):
        assert isinstance(host(by_label[label]), Exception) == refused, label
        _, _, status, _ = device([by_label[label]], cuda, SMALL)
        assert (status[0] != 0) == refused, label


def test_check_raises_the_hosts_error_and_leaves_the_other_images(cuda):
    good = [jpeg.encode_jpeg(picture(48, 80, s), 90, '420', 0) for s in range(4)]
    bad = good[2][:len(good[2]) * 6 // 10]
    dec = jpeg.JpegDecoder(device=cuda, entropy='device', slots=1)
    clean = dec.decode(good).clone()
    out = torch.zeros_like(clean)
    with pytest.raises(ValueError, match='truncated|restart|corrupt') as raised:
        dec.decode(good[:2] + [bad] + good[3:], out=out)
    with pytest.raises(ValueError) as want:
        jpeg.entropy_decode(bad)
    assert str(raised.value) == str(want.value)
    torch.cuda.synchronize()
    for i in (0, 1, 3):
        assert torch.equal(out[i], clean[i])
    # check=False: nothing raises, the status words are the caller's
    dec.decode(good[:2] + [bad] + good[3:], out=out, check=False)
    status = dec.last_status.tolist()
    assert status[2] != 0 and [status[i] for i in (0, 1, 3)] == [0, 0, 0]
    assert torch.equal(dec.decode(good), clean)
    dec.close()


# ---- the memory contract ---------------------------------------------------------------------------------------------------
def guarded_call(datas, cuda, fill, setting):
    """One st_jpeg_entropy_decode_dev with blob, coef, quant, status and work each inside guard bands, work and outputs
    pre-filled with `fill`."""
    info = jpeg._info(datas[0])
    n, count = len(datas), int(info.coef_count)
    pinned = torch.empty(jpeg.blob_capacity(datas), dtype=torch.uint8).pin_memory()
    host_blob, used = jpeg.build_blob(datas, pinned.numpy())
    blob_dev = gm.arena(pinned[:used].clone(), device=cuda)
    coef = gm.arena(torch.full((n, count), fill * 0x0101, dtype=torch.int16), device=cuda)
    quant = gm.arena(torch.full((n, 3, 64), fill * 0x0101, dtype=torch.int16), device=cuda)
    status = gm.arena(torch.full((n,), fill * 0x01010101, dtype=torch.int32), device=cuda)
    work_bytes = int(jpeg._api().st_jpeg_entropy_work_bytes(C.byref(info), n))
    work = gm.arena(torch.full((work_bytes,), fill, dtype=torch.uint8), device=cuda)
    jpeg.entropy_launch(host_blob, used, blob_dev, n, info, coef, quant, status, work, *setting)
    torch.cuda.synchronize()
    assert gm.bands_intact(blob_dev, coef, quant, status, work), 'a guard band was written'
    assert torch.equal(blob_dev.cpu(), pinned[:used]), 'the blob was written'
    return coef.cpu().numpy(), quant.cpu().numpy().view(np.uint16), status.cpu().numpy(), work[:16 * n].cpu().numpy().view(np.int32)


@pytest.mark.parametrize('setting', [(None, None), SMALL])
def test_guard_bands_and_stale_memory(setting, cuda):
    base = jpeg.encode_jpeg(picture(48, 80, 3), 90, '420', 5)
    flipped = bytearray(base)
    off, scan = scan_of(base)
    flipped[off + len(scan) // 3] ^= 0x10
    datas = [base, base[:len(base) // 2], bytes(flipped), base[:off + 1], base[:off], noise(48, 80, '420')]
    wants = [host(d) for d in datas]
    assert [isinstance(w, Exception) for w in wants] == [False, True, isinstance(wants[2], Exception), True, True, False]
    runs = [guarded_call(datas, cuda, fill, setting) for fill in (0x00, 0x7F)]
    for coef, quant, status, stats in runs:
        for i, w in enumerate(wants):
            assert (status[i] != 0) == isinstance(w, Exception), i
            if not isinstance(w, Exception):
                assert np.array_equal(coef[i], w[0]) and np.array_equal(quant[i], w[1])
    a, b = runs
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[1], b[1])
    ok = a[2] == 0
    assert np.array_equal(a[0][ok], b[0][ok])
    # a refused image's coefficients stay inside its own extent: its neighbours' are the host's (above), and elements the
    # device did not write keep the fill
    assert (a[0][4] == 0).all() and (b[0][4] == 0x7F7F).all()                  # an empty scan writes nothing


def test_slot_reuse_and_a_side_stream(cuda):
    batches = [[jpeg.encode_jpeg(picture(48, 80, 10 * k + i), 90, '420', k) for i in range(1 + k % 3)] for k in range(4)]
    ref = jpeg.JpegDecoder(device=cuda)
    want = [ref.decode(b).clone() for b in batches]
    one, two = jpeg.JpegDecoder(device=cuda, entropy='device', slots=1), jpeg.JpegDecoder(device=cuda, entropy='device', slots=2)
    first = [one.decode(b, check=False).clone() for b in batches]            # consecutive calls on ONE slot
    again = [one.decode(b).clone() for b in batches]
    side = torch.cuda.Stream(device=cuda)
    busy = torch.randn(1024, 1024, device=cuda)
    for _ in range(4):
        busy = busy @ busy * 1e-3
    with torch.cuda.stream(side):
        outs = [two.decode(b, check=False) for b in batches]
    torch.cuda.current_stream().wait_stream(side)
    copies = [o.clone() for o in outs]
    torch.cuda.synchronize()
    for w, f, a, c in zip(want, first, again, copies):
        assert torch.equal(f, w) and torch.equal(a, w) and torch.equal(c, w)
    for d in (ref, one, two):
        d.close()


# ---- entry refusals ----------------------------------------------------------------------------------------------------------
def test_entry_refusals(cuda):
    with pytest.raises(ValueError, match='entropy'):
        jpeg.JpegDecoder(device=cuda, entropy='bogus')
    dec = jpeg.JpegDecoder(device=cuda, entropy='device')
    a = jpeg.encode_jpeg(picture(16, 16), 90, '420')
    with pytest.raises(ValueError, match='image 2'):
        dec.decode([a, a, jpeg.encode_jpeg(picture(16, 24), 90, '420')])
    with pytest.raises(ValueError, match='image 1'):
        dec.decode([a, jpeg.encode_jpeg(picture(16, 16), 90, '444')])
    with pytest.raises(NotImplementedError, match='progressive'):
        dec.decode([blob('refuse_progressive_33x31')])
    with pytest.raises(ValueError, match='geometry'):
        jpeg.entropy_decode_device([a, jpeg.encode_jpeg(picture(16, 24), 90, '420')], cuda)
    # the native entry: a descriptor that does not match the StJpegInfo, a scan outside the blob, a bad tuning - each
    # refused on the host, before any launch (the outputs keep their fill)
    other = jpeg._info(jpeg.encode_jpeg(picture(16, 24), 90, '420'))
    info = jpeg._info(a)
    pinned = torch.empty(jpeg.blob_capacity([a]), dtype=torch.uint8).pin_memory()
    host_blob, used = jpeg.build_blob([a], pinned.numpy())
    blob_dev = pinned[:used].to(cuda)
    coef = torch.full((1, int(other.coef_count)), 7, dtype=torch.int16, device=cuda)
    quant = torch.full((1, 3, 64), 7, dtype=torch.int16, device=cuda)
    status = torch.full((1,), 7, dtype=torch.int32, device=cuda)
    work = torch.full((256,), 7, dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError, match='does not match the StJpegInfo geometry'):
        jpeg.entropy_launch(host_blob, used, blob_dev, 1, other, coef, quant, status, work)
    with pytest.raises(ValueError, match='does not lie inside the blob'):
        jpeg.entropy_launch(host_blob, used - 16, blob_dev, 1, info, coef, quant, status, work)
    for subseq_bytes, tile in ((4, 4), (16, 300), (512, 256)):
        with pytest.raises(ValueError, match='subseq_bytes'):
            jpeg.entropy_launch(host_blob, used, blob_dev, 1, info, coef, quant, status, work, subseq_bytes, tile)
    bad = jpeg.StJpegInfo.from_buffer_copy(info)
    bad.blocks_w[0] = 1
    with pytest.raises(ValueError, match='not what st_jpeg_info returns'):
        jpeg.entropy_launch(host_blob, used, blob_dev, 1, bad, coef, quant, status, work)
    torch.cuda.synchronize()
    assert bool((coef == 7).all()) and bool((quant == 7).all()) and status.tolist() == [7] and bool((work == 7).all())
    assert torch.equal(dec.decode([a, a])[1], jpeg.JpegDecoder(device=cuda).decode([a])[0])     # and the decoder still works
    dec.close()
