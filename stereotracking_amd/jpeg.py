"""JPEG frames (ABI: include/stereotrack_jpeg.h).

The reference reads every image through mmcv.imfrombytes and its dataset zoo is mostly JPEG (configs/_base_/datasets/
mot_challenge.py, dancetrack, selma_dataset.py:42-46, every '%06d.jpg' template under mmtrack/datasets); cameras deliver
MJPEG.  A decoder splits along this package's host / device line:

  jpeg_info / read_jpeg   host: marker parse, Huffman entropy decode and the reconstruction in C++ (csrc/jpeg_io.cpp) -
                          the counterpart of datasets.read_png, what LoadImageFromFile calls
  JpegDecoder             entropy decode on a few host threads into page-locked memory, ONE H2D copy of the quantised
                          coefficients, then dequantisation + inverse DCT + chroma upsampling + YCbCr -> BGR in HIP
                          (csrc/jpeg_decode.hip): uint8 planar (N,3,h,w) frames on the device, what RawFrames and the raw
                          stem kernels take.  entropy='device' (opt-in): the host only parses headers and copies the raw scan
                          bytes; the Huffman decode runs in HIP too (csrc/jpeg_entropy.hip), equal to the host routine in
                          coefficients, tables and accept / refuse verdict
  write_jpeg              a small numpy baseline ENCODER (Annex K tables, IJG quality scaling), the counterpart of
                          write_png: tests and tools make JPEGs of any geometry without an imaging library

Decoded: baseline / extended-sequential Huffman, 8-bit, one scan, gray or YCbCr 4:4:4 / 4:2:2 / 4:2:0, restart markers,
8- and 16-bit quantisation tables.  The arithmetic is libjpeg-turbo's default (JDCT_ISLOW, fancy upsampling), pinned
bit for bit by tests/golden/jpeg.  Refused with NotImplementedError: progressive, arithmetic, lossless, 12-bit, CMYK,
Adobe transform 0, other sampling factors, several scans.  Corrupt or truncated data: ValueError.
"""
import ctypes as C
import struct
import threading

import numpy as np

from . import _lib

ST_ERR_UNSUPPORTED = -6
SAMPLING_NAMES = ('gray', '444', '422', '420')


class StJpegInfo(C.Structure):
    _fields_ = [('struct_size', C.c_int), ('height', C.c_int), ('width', C.c_int), ('components', C.c_int),
                ('sampling', C.c_int), ('restart_interval', C.c_int), ('mcus_x', C.c_int), ('mcus_y', C.c_int),
                ('blocks_w', C.c_int * 3), ('blocks_h', C.c_int * 3), ('comp_w', C.c_int * 3), ('comp_h', C.c_int * 3),
                ('reserved', C.c_int), ('coef_offset', C.c_size_t * 3), ('coef_count', C.c_size_t),
                ('coef_bytes', C.c_size_t), ('work_bytes', C.c_size_t)]


class StJpegHuffLut(C.Structure):
    _fields_ = [('fast', C.c_uint16 * 512), ('maxcode', C.c_int32 * 18), ('valptr', C.c_int32 * 17),
                ('mincode', C.c_int32 * 17), ('vals', C.c_uint8 * 256)]


class StJpegEntropyDesc(C.Structure):
    _fields_ = [('struct_size', C.c_int), ('components', C.c_int), ('sampling', C.c_int), ('restart_interval', C.c_int),
                ('mcus_x', C.c_int), ('mcus_y', C.c_int), ('dc_slot', C.c_int * 3), ('ac_slot', C.c_int * 3),
                ('scan_offset', C.c_uint), ('scan_bytes', C.c_uint), ('blob_offset', C.c_uint), ('reserved', C.c_int),
                ('quant', C.c_uint16 * 64 * 3), ('dc', StJpegHuffLut * 3), ('ac', StJpegHuffLut * 3)]


class StJpegEntropyTuning(C.Structure):
    _fields_ = [('struct_size', C.c_int), ('subseq_bytes', C.c_int), ('tile', C.c_int)]


DESC_BYTES = C.sizeof(StJpegEntropyDesc)
assert DESC_BYTES % 16 == 0

_PROTOS = {
    'st_jpeg_info': (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(StJpegInfo)]),
    'st_jpeg_entropy_decode': (C.c_int, [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    'st_jpeg_reconstruct_host': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(StJpegInfo), C.c_void_p, C.c_ssize_t,
                                           C.c_ssize_t, C.c_ssize_t, C.c_int]),
    'st_jpeg_work_bytes': (C.c_size_t, [C.POINTER(StJpegInfo), C.c_int]),
    'st_jpeg_reconstruct': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(StJpegInfo), C.c_void_p, C.c_size_t,
                                      C.c_void_p, C.c_ssize_t, C.c_ssize_t, C.c_ssize_t, C.c_int, C.c_void_p]),
    'st_jpeg_entropy_prepare': (C.c_int, [C.c_char_p, C.c_size_t, C.c_void_p]),
    'st_jpeg_entropy_work_bytes': (C.c_size_t, [C.POINTER(StJpegInfo), C.c_int]),
    'st_jpeg_entropy_decode_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(StJpegInfo),
                                             C.POINTER(StJpegEntropyTuning), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_size_t, C.c_void_p]),
}
_bound = None
_bind_lock = threading.Lock()


def _api():
    """The library handle with the prototypes of stereotrack_jpeg.h set on it (they are not part of _lib._PROTOS, which
    mirrors stereotrack.h name for name)."""
    global _bound
    if _bound is None:
        with _bind_lock:
            if _bound is None:
                lib = _lib.load()
                for name, (res, args) in _PROTOS.items():
                    fn = getattr(lib, name)
                    fn.restype, fn.argtypes = res, args
                _bound = lib
    return _bound


def _check(rc, what):
    if rc == 0:
        return
    msg = _lib.load().st_last_error()
    msg = msg.decode() if msg else what
    if rc == ST_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == -1:                          # ST_ERR_INVALID
        raise ValueError(msg)
    _lib.check(rc, what)


def _bytes_of(path_or_bytes):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return bytes(path_or_bytes)
    with open(path_or_bytes, 'rb') as f:
        return f.read()


def _info(data):
    info = StJpegInfo(struct_size=C.sizeof(StJpegInfo))
    _check(_api().st_jpeg_info(data, len(data), C.byref(info)), 'st_jpeg_info')
    return info


def jpeg_info(data):
    """Header of a JPEG (path or bytes) -> dict: height, width, components, sampling ('gray' | '444' | '422' | '420'),
    restart_interval, mcus (y, x), blocks [(rows, cols) per component, padded to whole MCUs], comp_shape [(h, w) true
    sample size per component], coef_count (int16 elements) and work_bytes (device work memory per image)."""
    i = _info(_bytes_of(data))
    nc = i.components
    return dict(height=i.height, width=i.width, components=nc, sampling=SAMPLING_NAMES[i.sampling],
                restart_interval=i.restart_interval, mcus=(i.mcus_y, i.mcus_x),
                blocks=[(i.blocks_h[c], i.blocks_w[c]) for c in range(nc)],
                comp_shape=[(i.comp_h[c], i.comp_w[c]) for c in range(nc)],
                coef_count=int(i.coef_count), work_bytes=int(i.work_bytes))


def entropy_decode(data, coef=None, quant=None):
    """bytes -> (StJpegInfo, coef int16 (coef_count,), quant uint16 (3, 64)); the arrays may be given (views of a
    page-locked slot).  Coefficients are quantised, in natural order, [component][block_row][block_col][64]."""
    info = _info(data)
    if coef is None:
        coef = np.empty(int(info.coef_count), np.int16)
    if quant is None:
        quant = np.empty((3, 64), np.uint16)
    assert coef.dtype == np.int16 and coef.size == info.coef_count and coef.flags.c_contiguous
    assert quant.dtype == np.uint16 and quant.size == 192 and quant.flags.c_contiguous
    _check(_api().st_jpeg_entropy_decode(data, len(data), coef.ctypes.data, quant.ctypes.data), 'st_jpeg_entropy_decode')
    return info, coef, quant


def entropy_prepare(data, into=None, index=0):
    """The header parse of the device entropy decode (st_jpeg_entropy_prepare, O(header)) -> StJpegEntropyDesc with
    blob_offset 0; `into`: a writable uint8 numpy array that holds descriptors, the struct is then a view of slot `index`."""
    d = StJpegEntropyDesc() if into is None else StJpegEntropyDesc.from_buffer(into, index * DESC_BYTES)
    d.struct_size = DESC_BYTES
    _check(_api().st_jpeg_entropy_prepare(data, len(data), C.addressof(d)), 'st_jpeg_entropy_prepare')
    return d


def blob_capacity(datas):
    """Bytes that build_blob needs at most for these files."""
    return len(datas) * DESC_BYTES + sum((len(d) + 15) // 16 * 16 for d in datas)


def build_blob(datas, host=None, pool=None):
    """The ONE blob of a device entropy decode: N descriptors, then every file's bytes from its scan on, each at a
    16-byte aligned offset.  host: a uint8 numpy array of at least blob_capacity(datas) (page-locked in JpegDecoder).
    pool: an executor for the per-image work.  -> (host, bytes used).  Raises the first offending image's error once
    every worker has finished."""
    n = len(datas)
    if host is None:
        host = np.zeros(blob_capacity(datas), np.uint8)
    assert host.dtype == np.uint8 and host.flags.c_contiguous and host.size >= blob_capacity(datas)
    run = (lambda fn, *cols: list(map(fn, *cols))) if pool is None else (lambda fn, *cols: _gather(pool, fn, *cols))
    descs = run(lambda i: entropy_prepare(datas[i], host, i), range(n))
    offsets, off = [], n * DESC_BYTES
    for d in descs:
        offsets.append(off)
        d.blob_offset = off
        off += (d.scan_bytes + 15) // 16 * 16

    def copy_scan(i):
        d = descs[i]
        host[offsets[i]:offsets[i] + d.scan_bytes] = np.frombuffer(datas[i], np.uint8, d.scan_bytes, d.scan_offset)
    run(copy_scan, range(n))
    return host, off


def _gather(pool, fn, *cols):
    """pool.map that lets every worker finish before the first error leaves."""
    futures = [pool.submit(fn, *args) for args in zip(*cols)]
    errors = [f.exception() for f in futures]
    for e in errors:
        if e is not None:
            raise e
    return [f.result() for f in futures]


def _tuning(subseq_bytes, tile):
    if subseq_bytes is None and tile is None:
        return None
    return StJpegEntropyTuning(C.sizeof(StJpegEntropyTuning), int(subseq_bytes or 0), int(tile or 0))


def entropy_launch(host, used, blob_dev, n, info, coef, quant, status, work, subseq_bytes=None, tile=None):
    """st_jpeg_entropy_decode_dev on the current stream of blob_dev's device: `host` the blob of build_blob, blob_dev its
    device copy (enqueued by the caller in front of this), coef / quant / status / work device tensors."""
    import torch
    tuning = _tuning(subseq_bytes, tile)
    with torch.cuda.device(blob_dev.device):
        rc = _api().st_jpeg_entropy_decode_dev(host.ctypes.data, blob_dev.data_ptr(), used, n, C.byref(info),
                                               C.byref(tuning) if tuning is not None else None, coef.data_ptr(),
                                               quant.data_ptr(), status.data_ptr(), work.data_ptr(),
                                               work.numel() * work.element_size(),
                                               torch.cuda.current_stream(blob_dev.device).cuda_stream)
    _check(rc, 'st_jpeg_entropy_decode_dev')


def entropy_decode_device(datas, device, subseq_bytes=None, tile=None):
    """Test and bench facing: the device entropy decode of N files of one geometry on `device` ->
    (StJpegInfo, coef int16 (N, coef_count), quant int16 (N, 3, 64) holding the uint16 bit patterns, status int32 (N,),
    stats int32 (N, 4): tiles, subsequences, max passes, sum of passes), all device tensors, enqueued on the current
    stream.  subseq_bytes / tile: the tuning (None: the library's defaults)."""
    import torch
    datas = [bytes(d) for d in datas]
    if not datas:
        raise ValueError('entropy_decode_device: no images')
    infos = [_info(d) for d in datas]
    info = infos[0]
    for i, other in enumerate(infos):
        if not JpegDecoder._same_geometry(info, other):
            raise ValueError(f'entropy_decode_device: image {i} differs from image 0 in geometry or sampling class')
    dev = torch.device(device)
    n, count = len(datas), int(info.coef_count)
    host, used = build_blob(datas, torch.empty(blob_capacity(datas), dtype=torch.uint8).pin_memory().numpy())
    blob_dev = torch.empty(used, dtype=torch.uint8, device=dev)
    coef = torch.empty((n, count), dtype=torch.int16, device=dev)
    quant = torch.empty((n, 3, 64), dtype=torch.int16, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    work = torch.empty(int(_api().st_jpeg_entropy_work_bytes(C.byref(info), n)), dtype=torch.uint8, device=dev)
    pinned = torch.from_numpy(host)
    blob_dev.copy_(pinned[:used], non_blocking=True)
    entropy_launch(host, used, blob_dev, n, info, coef, quant, status, work, subseq_bytes, tile)
    stats = work[:16 * n].view(torch.int32).reshape(n, 4).clone()
    torch.cuda.current_stream(dev).synchronize()         # the page-locked blob is this call's own: keep it until the copy is done
    return info, coef, quant, status, stats


def reconstruct_host(coef, quant, info, order='rgb', planar=False):
    """The host reconstruction (the executable specification of the kernels): (h, w, 3) interleaved, or (3, h, w) planar."""
    h, w = info.height, info.width
    coef, quant = np.ascontiguousarray(coef, np.int16), np.ascontiguousarray(quant, np.uint16)
    assert coef.size == info.coef_count and quant.size == 192
    out = np.empty((3, h, w) if planar else (h, w, 3), np.uint8)
    strides = (h * w, w, 1) if planar else (1, 3 * w, 3)
    _check(_api().st_jpeg_reconstruct_host(coef.ctypes.data, quant.ctypes.data, C.byref(info), out.ctypes.data, *strides,
                                           int(order == 'rgb')), 'st_jpeg_reconstruct_host')
    return out


def read_jpeg(path_or_bytes):
    """Decode a JPEG on the host -> numpy uint8 (H, W, 3) in RGB order, or (H, W) for a one-component file: the
    counterpart of datasets.read_png (channel order as stored)."""
    info, coef, quant = entropy_decode(_bytes_of(path_or_bytes))
    out = reconstruct_host(coef, quant, info, order='rgb')
    return np.ascontiguousarray(out[..., 0]) if info.components == 1 else out


# ---- encoder ---------------------------------------------------------------------------------------------------------
_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                    7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                    39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# ITU-T T.81 Annex K.1: quantisation tables (natural order)
_Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
_Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                      47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
# Annex K.3: Huffman tables (code counts per length 1..16, symbols in code order)
_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], list(bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738'
    '393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5'
    'a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa')))
_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637'
    '38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3'
    'a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa')))
for _bits, _vals in (_DC_LUMA, _DC_CHROMA, _AC_LUMA, _AC_CHROMA):
    assert sum(_bits) == len(_vals) == len(set(_vals))


def _huff_codes(bits, vals):
    """Annex C: canonical codes -> (code[256], length[256])."""
    code_of, len_of = np.zeros(256, np.int64), np.zeros(256, np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            code_of[vals[k]], len_of[vals[k]] = code, length
            code += 1
            k += 1
        code <<= 1
    return code_of, len_of


def _dct_matrix():
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    d = np.cos((2 * n + 1) * k * np.pi / 16) * 0.5
    d[0] *= np.sqrt(0.5)
    return d


def _bit_size(v):
    """Number of bits of |v| (the coefficient's category), elementwise."""
    a, s = np.abs(v), np.zeros(v.shape, np.int64)
    for b in range(16):
        s += (a >> b) > 0
    return s


def _plane_blocks(plane, bh, bw, quant):
    """(H, W) float samples -> quantised coefficients (bh, bw, 64) in zigzag order; the plane is padded to the block
    grid by repeating its last row / column."""
    h, w = plane.shape
    p = np.pad(plane, ((0, bh * 8 - h), (0, bw * 8 - w)), mode='edge') - 128.0
    x = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
    d = _dct_matrix()
    c = np.einsum('ij,abjk,lk->abil', d, x, d).reshape(bh, bw, 64)
    q = np.rint(c / quant.astype(np.float64)).astype(np.int64)
    q[..., 0] = np.clip(q[..., 0], -1024, 1023)
    q[..., 1:] = np.clip(q[..., 1:], -1023, 1023)
    return q[..., _ZIGZAG]


def _pack_tokens(keys, vals, lens):
    """Tokens (value, bit length) sorted by key -> bytes, padded with 1-bits, FF bytes stuffed."""
    o = np.argsort(keys, kind='stable')
    vals, lens = vals[o], lens[o]
    ends = np.cumsum(lens)
    total = int(ends[-1]) if len(ends) else 0
    bits = np.ones((total + 7) // 8 * 8, np.uint8)
    starts = ends - lens
    for j in range(int(lens.max()) if len(lens) else 0):
        m = lens > j
        bits[starts[m] + j] = (vals[m] >> (lens[m] - 1 - j)) & 1
    return np.packbits(bits).tobytes().replace(b'\xff', b'\xff\x00')


def _entropy_segment(blocks, comp, tables):
    """blocks (n, 64) zigzag coefficients in stream order, comp (n,) table set per block (0 luma / 1 chroma); DC
    differences are already in column 0.  -> the segment's bytes."""
    n = blocks.shape[0]
    keys, vals, lens = [], [], []
    blk = np.arange(n, dtype=np.int64) * 1024
    dc = blocks[:, 0]
    size = _bit_size(dc)
    for t in (0, 1):
        m = comp == t
        code, length = tables[t][0]
        keys += [blk[m] + 1]
        vals += [code[size[m]]]
        lens += [length[size[m]]]
    keys += [blk + 2]
    vals += [np.where(dc < 0, dc + (1 << size) - 1, dc)]
    lens += [size]
    bi, ki = np.nonzero(blocks[:, 1:])
    ki = ki + 1
    v = blocks[bi, ki]
    prev = np.concatenate([[0], ki[:-1]])[:len(ki)]
    prev[np.concatenate([[True], bi[1:] != bi[:-1]])[:len(bi)]] = 0               # first coefficient of a block
    run = ki - prev - 1
    size = _bit_size(v)
    for t in (0, 1):
        m = comp[bi] == t
        code, length = tables[t][1]
        for z in range(1, 4):                                 # ZRL symbols in front of a coefficient with a run >= 16 z
            mz = m & (run >= 16 * z)
            keys += [blk[bi[mz]] + ki[mz] * 4]
            vals += [np.full(int(mz.sum()), code[0xF0])]
            lens += [np.full(int(mz.sum()), length[0xF0])]
        sym = ((run[m] & 15) << 4) | size[m]
        keys += [blk[bi[m]] + ki[m] * 4 + 1]
        vals += [code[sym]]
        lens += [length[sym]]
    keys += [blk[bi] + ki * 4 + 2]
    vals += [np.where(v < 0, v + (1 << size) - 1, v)]
    lens += [size]
    last = np.zeros(n, np.int64)
    np.maximum.at(last, bi, ki)
    for t in (0, 1):                                          # EOB unless coefficient 63 is present
        m = (comp == t) & (last < 63)
        code, length = tables[t][1]
        keys += [blk[m] + 64 * 4]
        vals += [np.full(int(m.sum()), code[0])]
        lens += [np.full(int(m.sum()), length[0])]
    return _pack_tokens(np.concatenate(keys), np.concatenate(vals).astype(np.int64), np.concatenate(lens).astype(np.int64))


def encode_jpeg(arr, quality=90, subsampling='420', restart_interval=0):
    """uint8 (H, W, 3) RGB or (H, W) gray -> the bytes of a baseline JFIF file (see write_jpeg)."""
    arr = np.asarray(arr)
    if arr.dtype != np.uint8 or arr.ndim not in (2, 3) or (arr.ndim == 3 and arr.shape[2] != 3):
        raise TypeError('write_jpeg takes uint8 (H, W) or (H, W, 3) arrays')
    if subsampling not in ('420', '422', '444'):
        raise ValueError("subsampling is '420', '422' or '444'")
    h, w = arr.shape[:2]
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError('JPEG sizes are 1..65535')
    quality = min(max(int(quality), 1), 100)
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality                  # IJG jpeg_quality_scaling
    qt = [np.clip((t * scale + 50) // 100, 1, 255) for t in (_Q_LUMA, _Q_CHROMA)]
    gray = arr.ndim == 2
    fh, fv = (1, 1) if gray or subsampling == '444' else ((2, 1) if subsampling == '422' else (2, 2))
    mx, my = -(-w // (8 * fh)), -(-h // (8 * fv))
    if gray:
        planes = [arr.astype(np.float64)]
    else:
        r, g, b = (arr[..., i].astype(np.float64) for i in range(3))
        ycc = [0.299 * r + 0.587 * g + 0.114 * b, -0.168736 * r - 0.331264 * g + 0.5 * b + 128.0,
               0.5 * r - 0.418688 * g - 0.081312 * b + 128.0]
        planes = [np.clip(np.rint(p), 0, 255) for p in ycc]
        for c in (1, 2):                                       # box downsampling over the edge-padded plane
            p = np.pad(planes[c], ((0, my * 8 * fv - h), (0, mx * 8 * fh - w)), mode='edge')
            p = p.reshape(my * 8, fv, mx * 8, fh).mean(axis=(1, 3))
            planes[c] = np.clip(np.rint(p), 0, 255)
    seq, comp = [], []
    for c, p in enumerate(planes):
        f_h, f_v = (fh, fv) if c == 0 else (1, 1)
        q = _plane_blocks(p, my * f_v, mx * f_h, qt[min(c, 1)])
        seq.append(q.reshape(my, f_v, mx, f_h, 64).transpose(0, 2, 1, 3, 4).reshape(my * mx, f_v * f_h, 64))
        comp.append(np.full((my * mx, f_v * f_h), min(c, 1)))
    nm = my * mx
    ri = int(restart_interval)
    if not 0 <= ri <= 65535:
        raise ValueError('restart_interval is 0..65535')
    seg = ri if ri else nm
    for s in seq:                                              # DC prediction per component, reset at every restart
        dc = s[..., 0].copy()
        flat = dc.reshape(-1)
        prev = np.concatenate([[0], flat[:-1]]).reshape(dc.shape)
        prev[::seg, 0] = 0
        s[..., 0] = dc - prev
    blocks = np.concatenate(seq, axis=1)
    comp = np.concatenate(comp, axis=1)
    tables = [(_huff_codes(*_DC_LUMA), _huff_codes(*_AC_LUMA)), (_huff_codes(*_DC_CHROMA), _huff_codes(*_AC_CHROMA))]
    body = bytearray()
    for k, a in enumerate(range(0, nm, seg)):
        if k:
            body += bytes([0xFF, 0xD0 + (k - 1) % 8])
        body += _entropy_segment(blocks[a:a + seg].reshape(-1, 64), comp[a:a + seg].reshape(-1), tables)

    def segment(marker, payload):
        return bytes([0xFF, marker]) + struct.pack('>H', len(payload) + 2) + payload
    nc = len(planes)
    out = bytearray(b'\xff\xd8')
    out += segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for i in range(1 if gray else 2):
        out += segment(0xDB, bytes([i]) + bytes(qt[i][_ZIGZAG].astype(np.uint8)))
    sof = struct.pack('>BHHB', 8, h, w, nc)
    for c in range(nc):
        sof += bytes([c + 1, (fh << 4 | fv) if c == 0 else 0x11, min(c, 1)])
    out += segment(0xC0, sof)
    for i, (dc, ac) in enumerate(((_DC_LUMA, _AC_LUMA), (_DC_CHROMA, _AC_CHROMA))[:1 if gray else 2]):
        out += segment(0xC4, bytes([i]) + bytes(dc[0]) + bytes(dc[1]))
        out += segment(0xC4, bytes([0x10 | i]) + bytes(ac[0]) + bytes(ac[1]))
    if ri:
        out += segment(0xDD, struct.pack('>H', ri))
    sos = bytes([nc])
    for c in range(nc):
        sos += bytes([c + 1, 0x11 * min(c, 1)])
    out += segment(0xDA, sos + b'\x00\x3f\x00')
    out += body
    out += b'\xff\xd9'
    return bytes(out)


def write_jpeg(path, arr, quality=90, subsampling='420', restart_interval=0):
    """Encode uint8 (H, W, 3) RGB or (H, W) gray as a baseline JFIF JPEG: Annex K Huffman and quantisation tables with
    IJG quality scaling, floating-point DCT, box-filtered chroma, `restart_interval` MCUs between RSTn markers (0: none).
    The counterpart of write_png - it exists so that tests and tools can make JPEGs of any geometry; nothing is pinned
    to its bytes, only to what decoders make of them."""
    blob = encode_jpeg(arr, quality, subsampling, restart_interval)
    with open(path, 'wb') as f:
        f.write(blob)


# ---- device decoder --------------------------------------------------------------------------------------------------
class JpegDecoder:
    """JPEG bytes -> uint8 planar frames on the device.

    decode(datas) reads the headers, entropy-decodes on `threads` host threads (the native routine runs without the GIL)
    straight into a page-locked staging slot, enqueues ONE non-blocking H2D copy of the quantised coefficients and the
    two reconstruction launches on the CURRENT stream, and returns without waiting for the device.  `slots` staging
    slots (page-locked host memory, its device twin and the component-plane work memory) alternate, each guarded by an
    event recorded behind the launches: the host waits only when it is `slots` calls ahead, and a slot's device memory
    is reused on another stream only behind that event.

    entropy='device' (opt-in): the host threads only parse the headers and copy the raw scan bytes into
    ONE page-locked blob; the Huffman decode runs in HIP (csrc/jpeg_entropy.hip) in front of the reconstruction, with
    coefficients, tables and accept / refuse verdict equal to the host routine's."""

    def __init__(self, device=None, threads=4, slots=2, entropy='host'):
        import torch
        from concurrent.futures import ThreadPoolExecutor
        if not torch.cuda.is_available():
            raise RuntimeError('JpegDecoder reconstructs on the GPU (st_jpeg_reconstruct); no GPU here - read_jpeg is the host path')
        if entropy not in ('host', 'device'):
            raise ValueError(f"JpegDecoder: entropy is 'host' or 'device', not {entropy!r}")
        self.entropy = entropy
        self.last_status = None                                # entropy='device': the last call's per-image status words
        dev = torch.device('cuda') if device is None else torch.device(device)
        if dev.type != 'cuda':
            raise ValueError(f'JpegDecoder decodes on a GPU, not on {dev}')
        # always an indexed device: a tensor's .device is 'cuda:0', never the bare 'cuda'
        self.dev = torch.device('cuda', torch.cuda.current_device() if dev.index is None else dev.index)
        self.threads = min(max(int(threads), 1), 16)           # never sized from the machine's CPU count
        self._pool = ThreadPoolExecutor(max_workers=self.threads)
        self._slots = [dict(pin=None, dev=None, work=None, blob=None, ework=None, done=torch.cuda.Event(), used=False)
                       for _ in range(max(int(slots), 1))]
        self._k = 0
        _api()

    def close(self):
        """Stop the pool's threads (idle ones also end with the interpreter)."""
        self._pool.shutdown(wait=True)

    @staticmethod
    def _same_geometry(a, b):
        return (a.height, a.width, a.components, a.sampling) == (b.height, b.width, b.components, b.sampling)

    def _decode_device_entropy(self, sl, datas, info, out, order, check, cur):
        """entropy='device': header parse on the pool, ONE page-locked blob (descriptors + raw scan bytes), ONE
        non-blocking H2D copy, the entropy launches and st_jpeg_reconstruct on the current stream."""
        import torch
        n, count = len(datas), int(info.coef_count)
        coef_bytes, nbytes = n * count * 2, n * count * 2 + n * 384
        cap = blob_capacity(datas)
        if sl['blob'] is None or sl['blob'][0].numel() < cap:
            sl['blob'] = (torch.empty(cap, dtype=torch.uint8).pin_memory(), torch.empty(cap, dtype=torch.uint8, device=self.dev))
        if sl['dev'] is None or sl['dev'].numel() < nbytes:    # coefficients and tables: device memory only
            sl['dev'] = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        work_bytes = int(_api().st_jpeg_work_bytes(C.byref(info), n))
        if sl['work'] is None or sl['work'].numel() < work_bytes:
            sl['work'] = torch.empty(work_bytes, dtype=torch.uint8, device=self.dev)
        ework_bytes = int(_api().st_jpeg_entropy_work_bytes(C.byref(info), n))
        if sl['ework'] is None or sl['ework'].numel() < ework_bytes:
            sl['ework'] = torch.empty(ework_bytes, dtype=torch.uint8, device=self.dev)
        pinned, blob_dev = sl['blob']
        host, used = build_blob(datas, pinned.numpy(), self._pool)
        status = torch.empty(n, dtype=torch.int32, device=self.dev)
        with torch.cuda.device(self.dev):
            blob_dev[:used].copy_(pinned[:used], non_blocking=True)
            coef, quant = sl['dev'][:coef_bytes], sl['dev'][coef_bytes:nbytes]
            entropy_launch(host, used, blob_dev, n, info, coef, quant, status, sl['ework'])
            _check(_api().st_jpeg_reconstruct(coef.data_ptr(), quant.data_ptr(), n, C.byref(info), sl['work'].data_ptr(),
                                              sl['work'].numel(), out.data_ptr(), out.stride(0), out.stride(1),
                                              out.stride(2), int(order == 'rgb'), cur.cuda_stream), 'st_jpeg_reconstruct')
            sl['done'].record(cur)
        sl['used'] = True
        self.last_status = status
        if check:
            refused = torch.nonzero(status.cpu()).flatten().tolist()       # waits for the N status words
            if refused:
                i = refused[0]
                entropy_decode(datas[i])                       # the host's own ValueError and message
                raise RuntimeError(f'JpegDecoder.decode: the device refused the entropy data of image {i} (status '
                                   f'{int(status[i])}) which the host routine accepts')

    def decode(self, datas, out=None, order='bgr', check=True):
        """datas: a sequence of N JPEG byte strings of ONE geometry and sampling class -> torch.uint8 (N, 3, h, w) on the
        device, planes in `order` ('bgr' | 'rgb'), produced on the current stream.  out: write there instead of a fresh
        allocation (a (N,3,h,w) uint8 device view with unit stride along w; it may sit inside a wider buffer).
        entropy='device' only: with check=True the call waits for the N status words and raises the host routine's
        ValueError for the first refused image; with check=False nothing waits and `last_status` (device int32 (N,),
        0 = accepted) is the caller's to read."""
        import torch
        if order not in ('bgr', 'rgb'):
            raise ValueError("order is 'bgr' or 'rgb'")
        datas = [bytes(d) if not isinstance(d, bytes) else d for d in datas]
        if not datas:
            raise ValueError('JpegDecoder.decode: no images')
        infos = [_info(d) for d in datas]
        info = infos[0]
        for i, other in enumerate(infos):
            if not self._same_geometry(info, other):
                raise ValueError(f'JpegDecoder.decode: image {i} is {other.height}x{other.width} '
                                 f'{SAMPLING_NAMES[other.sampling]}, image 0 is {info.height}x{info.width} '
                                 f'{SAMPLING_NAMES[info.sampling]}: one call decodes one geometry and sampling class')
        n, h, w = len(datas), info.height, info.width
        count = int(info.coef_count)
        coef_bytes, nbytes = n * count * 2, n * count * 2 + n * 384
        work_bytes = int(_api().st_jpeg_work_bytes(C.byref(info), n))
        if out is None:
            out = torch.empty((n, 3, h, w), dtype=torch.uint8, device=self.dev)
        elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and tuple(out.shape) == (n, 3, h, w) and
                  out.device == self.dev and out.stride(3) == 1 and min(out.stride()[:3]) > 0):
            raise ValueError(f'out must be a uint8 ({n}, 3, {h}, {w}) tensor on {self.dev} with unit stride along w')
        sl = self._slots[self._k % len(self._slots)]
        self._k += 1
        cur = torch.cuda.current_stream(self.dev)
        if sl['used']:
            sl['done'].synchronize()         # the copy that last read this staging slot has finished
            cur.wait_event(sl['done'])       # ... and, on whatever stream that was, the launches that used its device memory
        if self.entropy == 'device':
            self._decode_device_entropy(sl, datas, info, out, order, check, cur)
            return out
        if sl['pin'] is None or sl['pin'].numel() < nbytes:
            sl['pin'] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            sl['dev'] = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        if sl['work'] is None or sl['work'].numel() < work_bytes:
            sl['work'] = torch.empty(work_bytes, dtype=torch.uint8, device=self.dev)
        host = sl['pin'].numpy()
        coef = host[:coef_bytes].view(np.int16).reshape(n, count)
        quant = host[coef_bytes:nbytes].view(np.uint16).reshape(n, 3, 64)
        # every worker has finished before this returns or raises: a failed image must not leave others still writing
        # into the slot that the next call (or, with one slot, this caller's retry) hands out again
        futures = [self._pool.submit(entropy_decode, datas[i], coef[i], quant[i]) for i in range(n)]
        errors = [f.exception() for f in futures]        # .exception() waits for the future
        for e in errors:
            if e is not None:
                raise e                                  # the first offending image's error
        with torch.cuda.device(self.dev):
            sl['dev'][:nbytes].copy_(sl['pin'][:nbytes], non_blocking=True)
            base = sl['dev'].data_ptr()
            _check(_api().st_jpeg_reconstruct(base, base + coef_bytes, n, C.byref(info), sl['work'].data_ptr(),
                                              sl['work'].numel(), out.data_ptr(), out.stride(0), out.stride(1),
                                              out.stride(2), int(order == 'rgb'), cur.cuda_stream), 'st_jpeg_reconstruct')
            sl['done'].record(cur)
        sl['used'] = True
        return out
