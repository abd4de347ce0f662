"""CPU: the device entropy decoder's algorithm and host half - DESIGN.md section 25, "Entropy decode on the device".

tests/native/jpeg_entropy_check.cpp runs the text the kernels compile (csrc/jpeg_entropy_core.h) with the threads of a
workgroup as serial loops - tiles, speculative pass, re-decode passes, count scan, write pass, DC chain - and compares
verdict, coefficients and tables with st_jpeg_entropy_decode, the specification, over the golden files and 200 seeded
corruptions at six (subseq_bytes, tile) settings.  Built here as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process.  Then st_jpeg_entropy_prepare: its scan offset and length against
a marker walk in Python, its tables against the quantisation tables the host routine returns, its refusals against
st_jpeg_info's, and the blob layout JpegDecoder uploads."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

from stereotracking_amd import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg')
ROCM = os.environ.get('ROCM_PATH', '/opt/rocm')
FLAGS = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__',
         '-I' + os.path.join(ROCM, 'include')]


def files():
    return sorted(glob.glob(os.path.join(GOLDEN, '*.jpg')))


def blob(path):
    with open(path, 'rb') as f:
        return f.read()


@pytest.fixture(scope='module')
def check_program(tmp_path_factory):
    cxx = os.path.join(ROCM, 'llvm', 'bin', 'clang++')
    assert os.path.exists(cxx), f'the ROCm clang is not at {cxx}'
    exe = str(tmp_path_factory.mktemp('jpeg_entropy') / 'jpeg_entropy_check')
    csrc = os.path.join(ROOT, 'stereotracking_amd', 'csrc')
    build = subprocess.run([cxx] + FLAGS + [os.path.join(ROOT, 'tests', 'native', 'jpeg_entropy_check.cpp'),
                                            os.path.join(csrc, 'jpeg_io.cpp'), os.path.join(csrc, 'st_common.cpp'), '-o', exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, f'{cxx} failed:\n{build.stderr}'
    return exe


def test_emulated_kernels_equal_the_host_routine_under_sanitizers(check_program):
    run = subprocess.run([check_program] + files(), capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, f'exit status {run.returncode}:\n{run.stderr}'
    assert run.stderr == ''
    assert '200 corruptions' in run.stdout and 'verdicts and coefficients equal' in run.stdout


def test_small_files_span_several_tiles_and_need_several_passes(check_program, tmp_path):
    """The precondition of the GPU file's multi-tile cases, established here with the emulation: noise at quality 100
    makes scans of many 16-byte subsequences whose decoders do not settle in one pass."""
    rng = np.random.default_rng(4880)
    path = str(tmp_path / 'noise.jpg')
    jpeg.write_jpeg(path, rng.integers(0, 256, (48, 80, 3), dtype=np.uint8), quality=100, subsampling='444')
    run = subprocess.run([check_program, '--probe', path, '16', '64'], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == '', run.stderr
    print(run.stdout)
    words = run.stdout.split()
    stats = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    assert stats['status'] == 0 and stats['tiles'] >= 3 and stats['max_passes'] >= 2
    assert stats['subsequences'] == -(-stats['scan_bytes'] // 16) and stats['sum_passes'] >= stats['tiles']


def marker_walk(data):
    """(offset of the first entropy-coded byte, restart interval) by walking the segments in Python."""
    p, ri = 2, 0
    while True:
        assert data[p] == 0xFF
        m, n = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        if m == 0xDD:
            ri = (data[p + 4] << 8) | data[p + 5]
        p += 2 + n
        if m == 0xDA:
            return p, ri


@pytest.mark.parametrize('path', [p for p in files() if 'refuse_' not in p], ids=os.path.basename)
def test_prepare_describes_the_file(path):
    data = blob(path)
    d = jpeg.entropy_prepare(data)
    off, ri = marker_walk(data)
    assert (d.scan_offset, d.scan_bytes, d.blob_offset) == (off, len(data) - off, 0)
    info, _, quant = jpeg.entropy_decode(data)
    assert (d.components, d.sampling, d.restart_interval, d.mcus_x, d.mcus_y) == \
        (info.components, info.sampling, ri, info.mcus_x, info.mcus_y)
    assert np.array_equal(np.ctypeslib.as_array(d.quant).reshape(3, 64), quant)
    for c in range(info.components):
        assert 0 <= d.dc_slot[c] <= c and 0 <= d.ac_slot[c] <= c
        for lut, is_dc in ((d.dc[d.dc_slot[c]], True), (d.ac[d.ac_slot[c]], False)):
            fast = np.ctypeslib.as_array(lut.fast)
            assert fast.any() and (fast >> 8).max() <= 9
            if is_dc:
                assert (fast & 255).max() <= 11
    if info.components == 3:                       # Pillow and the numpy encoder give both chroma components one table pair
        assert d.dc_slot[2] == d.dc_slot[1] and d.ac_slot[2] == d.ac_slot[1]


def test_prepare_refuses_what_st_jpeg_info_refuses():
    base = blob(os.path.join(GOLDEN, 'rgb_17x13_420_q100.jpg'))
    cases = [blob(os.path.join(GOLDEN, 'refuse_progressive_33x31.jpg')), blob(os.path.join(GOLDEN, 'refuse_cmyk_17x13.jpg')),
             b'\x89PNG\r\n\x1a\n' + bytes(32), base[:30], base[:2] + b'\xff\xd9']
    for data in cases:
        with pytest.raises((ValueError, NotImplementedError)) as want:
            jpeg.jpeg_info(data)
        with pytest.raises(type(want.value)) as got:
            jpeg.entropy_prepare(data)
        assert str(got.value) == str(want.value)
    # a scan that names a Huffman table the file does not define: st_jpeg_info accepts, the host entropy decode refuses
    p = base.index(b'\xff\xda')
    bad = bytearray(base)
    bad[p + 6] = 0x33
    with pytest.raises(ValueError, match='Huffman table the file does not define') as want:
        jpeg.entropy_decode(bytes(bad))
    with pytest.raises(ValueError) as got:
        jpeg.entropy_prepare(bytes(bad))
    assert str(got.value) == str(want.value)
    d = jpeg.StJpegEntropyDesc()
    d.struct_size = 12
    assert jpeg._api().st_jpeg_entropy_prepare(base, len(base), C.addressof(d)) == -1


def test_blob_is_descriptors_then_scan_bytes():
    datas = [blob(os.path.join(GOLDEN, n + '.jpg')) for n in ('rgb_48x80_420_q85', 'rstblocks3_48x80_420_q85', 'rgb_48x80_420_q85')]
    host, used = jpeg.build_blob(datas)
    assert used <= jpeg.blob_capacity(datas) == host.size and used % 16 == 0
    end = len(datas) * jpeg.DESC_BYTES
    for i, data in enumerate(datas):
        d = jpeg.StJpegEntropyDesc.from_buffer(host, i * jpeg.DESC_BYTES)
        assert d.struct_size == jpeg.DESC_BYTES and d.blob_offset == end and d.blob_offset % 16 == 0
        assert bytes(host[d.blob_offset:d.blob_offset + d.scan_bytes]) == data[d.scan_offset:]
        end = d.blob_offset + (d.scan_bytes + 15) // 16 * 16
    assert end == used
    with pytest.raises(ValueError, match='not a JPEG'):
        jpeg.build_blob([datas[0], b'nothing'])


def test_the_new_exports_are_declared_and_bound(stlib):
    with open(os.path.join(ROOT, 'include', 'stereotrack_jpeg.h')) as f:
        text = f.read()
    for name in ('st_jpeg_entropy_prepare', 'st_jpeg_entropy_work_bytes', 'st_jpeg_entropy_decode_dev'):
        assert name in jpeg._PROTOS and hasattr(stlib, name) and name + '(' in text
    assert C.sizeof(jpeg.StJpegEntropyDesc) == 9376 and stlib.st_version() == 430
