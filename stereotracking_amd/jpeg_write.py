"""Write JPEG frames (ABI: include/stereotrack_vis.h): the mirror image of jpeg.py's reader.

  encode_jpeg_host        host: colour conversion, downsampling, forward DCT and quantisation in C++
                          (csrc/jpeg_encode.cpp, st_jpeg_forward_host), then the Huffman entropy encode and the file
                          layout (st_jpeg_entropy_encode) - the CPU product path
  JpegEncoder             the forward path in HIP (csrc/jpeg_forward.hip) on uint8 planar device frames, ONE D2H copy
                          of the quantised coefficients into page-locked memory, then the entropy encode on a few host
                          threads (the native routine runs without the GIL)

Written: baseline JFIF, gray or YCbCr 4:4:4 / 4:2:2 / 4:2:0, Annex K tables at an IJG quality, optional restart
markers.  The bytes are what libjpeg-turbo (Pillow's save with optimize=False) writes for the same pixels, quality and
subsampling, pinned by tests/golden/jpeg_write.  jpeg.encode_jpeg / write_jpeg stay what they are: a float-DCT numpy
utility for making test files.
"""
import ctypes as C
import threading

import numpy as np

from . import _lib
from .jpeg import SAMPLING_NAMES, StJpegInfo, _check

_PROTOS = {
    'st_jpeg_encode_geometry': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(StJpegInfo)]),
    'st_jpeg_quant_tables': (C.c_int, [C.c_int, C.c_void_p]),
    'st_jpeg_forward_host': (C.c_int, [C.c_void_p, C.c_ssize_t, C.c_ssize_t, C.c_ssize_t, C.c_int, C.c_void_p,
                                       C.POINTER(StJpegInfo), C.c_void_p]),
    'st_jpeg_forward': (C.c_int, [C.c_void_p, C.c_ssize_t, C.c_ssize_t, C.c_ssize_t, C.c_int, C.c_void_p, C.c_int,
                                  C.POINTER(StJpegInfo), C.c_void_p, C.c_void_p]),
    'st_jpeg_encode_bound': (C.c_size_t, [C.POINTER(StJpegInfo)]),
    'st_jpeg_entropy_encode': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(StJpegInfo), C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_size_t)]),
}
_bound = None
_bind_lock = threading.Lock()


def _api():
    """The library handle with the JPEG-writer prototypes of stereotrack_vis.h set on it (a binding table of its own,
    as jpeg._api() has: _lib._PROTOS mirrors stereotrack.h name for name)."""
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


def encode_geometry(height, width, components=3, subsampling='420', restart_interval=0):
    """-> the StJpegInfo of a file to be written (st_jpeg_encode_geometry).  subsampling: '444' | '422' | '420' for
    three components; one component is always 'gray'."""
    if components == 1:
        sampling = 0
    elif subsampling in ('444', '422', '420'):
        sampling = SAMPLING_NAMES.index(subsampling)
    else:
        raise ValueError(f"subsampling is '444', '422' or '420', not {subsampling!r}")
    info = StJpegInfo(struct_size=C.sizeof(StJpegInfo))
    _check(_api().st_jpeg_encode_geometry(int(height), int(width), int(components), sampling, int(restart_interval),
                                          C.byref(info)), 'st_jpeg_encode_geometry')
    return info


def quant_tables(quality):
    """The Annex K tables at IJG `quality` -> uint16 (3, 64), natural order, per component."""
    q = np.empty((3, 64), np.uint16)
    _check(_api().st_jpeg_quant_tables(int(quality), q.ctypes.data), 'st_jpeg_quant_tables')
    return q


def _restart_interval(info_or_mcus_x, restart_marker_rows):
    rows = int(restart_marker_rows)
    if rows < 0:
        raise ValueError('restart_marker_rows is >= 0')
    return rows * int(info_or_mcus_x)


def forward_host(arr, quant, info, order='rgb'):
    """st_jpeg_forward_host on a host array: uint8 (H, W, 3) interleaved in `order`, or (H, W) gray -> int16 (coef_count,)."""
    arr = np.ascontiguousarray(arr)
    quant = np.ascontiguousarray(quant, np.uint16)
    assert quant.size == 192
    coef = np.empty(int(info.coef_count), np.int16)
    h, w = arr.shape[:2]
    strides = (0, w, 1) if arr.ndim == 2 else (1, 3 * w, 3)
    _check(_api().st_jpeg_forward_host(arr.ctypes.data, *strides, int(order == 'rgb'), quant.ctypes.data, C.byref(info),
                                       coef.ctypes.data), 'st_jpeg_forward_host')
    return coef


def entropy_encode(coef, quant, info, out=None):
    """st_jpeg_entropy_encode: coefficients, tables, geometry -> the file's bytes.  out: a uint8 numpy array of at least
    st_jpeg_encode_bound(info) bytes to write into (a fresh one otherwise)."""
    coef = np.ascontiguousarray(coef, np.int16)
    quant = np.ascontiguousarray(quant, np.uint16)
    if coef.size != info.coef_count or quant.size != 192:
        raise ValueError(f'entropy_encode: {coef.size} coefficients and {quant.size} table entries, the geometry has '
                         f'{int(info.coef_count)} and 192')
    if out is None:
        out = np.empty(int(_api().st_jpeg_encode_bound(C.byref(info))), np.uint8)
    assert out.dtype == np.uint8 and out.flags.c_contiguous
    n = C.c_size_t(0)
    _check(_api().st_jpeg_entropy_encode(coef.ctypes.data, quant.ctypes.data, C.byref(info), out.ctypes.data, out.size,
                                         C.byref(n)), 'st_jpeg_entropy_encode')
    return out[:n.value].tobytes()


def _host_image(arr):
    arr = np.asarray(arr)
    if arr.dtype != np.uint8 or arr.ndim not in (2, 3) or (arr.ndim == 3 and arr.shape[2] != 3):
        raise TypeError(f'encode_jpeg_host takes uint8 (H, W) or (H, W, 3) arrays, not {arr.dtype} {arr.shape}')
    h, w = arr.shape[:2]
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f'JPEG sizes are 1..65535, got {h} x {w}')
    return arr


def encode_jpeg_host(arr, quality=90, subsampling='420', restart_marker_rows=0, order='rgb'):
    """uint8 (H, W, 3) in `order` ('rgb' | 'bgr'), or (H, W) gray -> the bytes of a baseline JFIF file, equal to
    libjpeg-turbo's for the same pixels, quality and subsampling.  restart_marker_rows: MCU rows per restart interval
    (0: none), as Pillow's save argument."""
    arr = _host_image(arr)
    if order not in ('rgb', 'bgr'):
        raise ValueError("order is 'rgb' or 'bgr'")
    h, w = arr.shape[:2]
    nc = 1 if arr.ndim == 2 else 3
    info = encode_geometry(h, w, nc, subsampling)
    if restart_marker_rows:
        info = encode_geometry(h, w, nc, subsampling, _restart_interval(info.mcus_x, restart_marker_rows))
    quant = quant_tables(quality)
    return entropy_encode(forward_host(arr, quant, info, order), quant, info)


def write_jpeg_host(path, arr, **kw):
    """encode_jpeg_host into a file."""
    blob = encode_jpeg_host(arr, **kw)
    with open(path, 'wb') as f:
        f.write(blob)


def forward_device(frames, quant_dev, info, coef, order='bgr'):
    """st_jpeg_forward on the current stream of frames' device: frames a uint8 (N, C, H, W) device view with unit
    stride along W, quant_dev the (3, 64) tables as a device tensor, coef an (N, coef_count) int16 device tensor."""
    import torch
    n = frames.shape[0]
    with torch.cuda.device(frames.device):
        rc = _api().st_jpeg_forward(frames.data_ptr(), frames.stride(0), frames.stride(1), frames.stride(2),
                                    int(order == 'rgb'), quant_dev.data_ptr(), n, C.byref(info), coef.data_ptr(),
                                    torch.cuda.current_stream(frames.device).cuda_stream)
    _check(rc, 'st_jpeg_forward')


class JpegEncoder:
    """uint8 planar frames on the device -> JPEG bytes.

    encode(frames) enqueues the forward launch and ONE non-blocking D2H copy of the quantised coefficients on the
    CURRENT stream, waits for that copy, and entropy-encodes on `threads` host threads out of the page-locked slot.
    `slots` staging slots (device coefficients and their page-locked twin) alternate, each guarded by an event recorded
    behind the copy: a slot's device memory is reused on another stream only behind that event, as in JpegDecoder."""

    def __init__(self, device=None, threads=4, slots=2, quality=90, subsampling='420'):
        import torch
        from concurrent.futures import ThreadPoolExecutor
        if not torch.cuda.is_available():
            raise RuntimeError('JpegEncoder runs the forward path on the GPU (st_jpeg_forward); no GPU here - '
                               'encode_jpeg_host is the host path')
        if subsampling not in ('444', '422', '420'):
            raise ValueError(f"subsampling is '444', '422' or '420', not {subsampling!r}")
        dev = torch.device('cuda') if device is None else torch.device(device)
        if dev.type != 'cuda':
            raise ValueError(f'JpegEncoder encodes on a GPU, not on {dev}')
        self.dev = torch.device('cuda', torch.cuda.current_device() if dev.index is None else dev.index)
        self.quality, self.subsampling = int(quality), subsampling
        self.threads = min(max(int(threads), 1), 16)           # never sized from the machine's CPU count
        self._pool = ThreadPoolExecutor(max_workers=self.threads)
        self._quant = quant_tables(self.quality)
        self._quant_dev = torch.from_numpy(self._quant.view(np.int16)).to(self.dev)
        self._slots = [dict(pin=None, dev=None, done=torch.cuda.Event(), used=False) for _ in range(max(int(slots), 1))]
        self._scratch = threading.local()                      # one output buffer per pool thread
        self._k = 0
        _api()

    def close(self):
        """Stop the pool's threads (idle ones also end with the interpreter)."""
        self._pool.shutdown(wait=True)

    def _encode_one(self, coef, info, bound):
        buf = getattr(self._scratch, 'buf', None)
        if buf is None or buf.size < bound:
            buf = self._scratch.buf = np.empty(bound, np.uint8)
        return entropy_encode(coef, self._quant, info, buf)

    def encode(self, frames, order='bgr', restart_marker_rows=0):
        """frames: torch.uint8 (N, 3, H, W) with planes in `order` ('bgr' | 'rgb'), or (N, 1, H, W) gray, on the device,
        unit stride along W (it may be a view into a wider buffer) -> a list of N `bytes`."""
        import torch
        if order not in ('bgr', 'rgb'):
            raise ValueError("order is 'bgr' or 'rgb'")
        if not (isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8 and frames.dim() == 4 and
                frames.shape[1] in (1, 3) and frames.shape[0] >= 1):
            raise TypeError('JpegEncoder.encode takes a uint8 (N, 3, H, W) or (N, 1, H, W) tensor')
        if frames.device != self.dev or frames.stride(3) != 1 or frames.stride(2) < frames.shape[3]:
            raise ValueError(f'frames must be on {self.dev} with unit stride along W')
        n, nc, h, w = frames.shape
        info = encode_geometry(h, w, nc, self.subsampling)
        if restart_marker_rows:
            info = encode_geometry(h, w, nc, self.subsampling, _restart_interval(info.mcus_x, restart_marker_rows))
        count = int(info.coef_count)
        sl = self._slots[self._k % len(self._slots)]
        self._k += 1
        cur = torch.cuda.current_stream(self.dev)
        if sl['used']:
            sl['done'].synchronize()         # the copy that last wrote this staging slot has finished
            cur.wait_event(sl['done'])       # ... and, on whatever stream that was, the launch that used its device memory
        if sl['pin'] is None or sl['pin'].numel() < n * count:
            sl['pin'] = torch.empty(n * count, dtype=torch.int16).pin_memory()
            sl['dev'] = torch.empty(n * count, dtype=torch.int16, device=self.dev)
        coef_dev = sl['dev'][:n * count].view(n, count)
        forward_device(frames, self._quant_dev, info, coef_dev, order)
        with torch.cuda.device(self.dev):
            sl['pin'][:n * count].copy_(sl['dev'][:n * count], non_blocking=True)
            sl['done'].record(cur)
        sl['used'] = True
        sl['done'].synchronize()             # the coefficients are in host memory
        coef = sl['pin'].numpy()[:n * count].reshape(n, count)
        bound = int(_api().st_jpeg_encode_bound(C.byref(info)))
        futures = [self._pool.submit(self._encode_one, coef[i], info, bound) for i in range(n)]
        errors = [f.exception() for f in futures]              # every worker has finished before this returns or raises
        for e in errors:
            if e is not None:
                raise e
        return [f.result() for f in futures]

    def write(self, frames, paths, order='bgr', restart_marker_rows=0):
        """encode(frames), one file per frame."""
        paths = list(paths)
        if len(paths) != frames.shape[0]:
            raise ValueError(f'{frames.shape[0]} frames, {len(paths)} paths')
        blobs = self.encode(frames, order, restart_marker_rows)
        for path, blob in zip(paths, blobs):
            with open(path, 'wb') as f:
                f.write(blob)
        return blobs
