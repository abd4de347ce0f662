"""Forced adverse stream schedules (test infrastructure; DESIGN.md 2, "Stream contract").

The package runs a stream graph: context streams, a side stream, a CMC stream, copy streams, rings of buffers reused
behind events.  On an idle GPU with test-sized shapes every stage finishes long before the host enqueues the next, so a
missing ordering edge never shows.  The tools here make one stream at a time LATE on purpose - a device-side delay in
front of a chosen entry point, or at the head of a chosen stream - so that a consumer which is not ordered behind the
delayed producer reads the previous round's (valid, stale) data and its result changes.

  delay(stream, ms)              a spinning kernel of `ms` milliseconds on `stream` (torch.cuda._sleep, calibrated once)
  exports_with_stream()          {export: position of its st_stream_t parameter}, parsed from include/stereotrack.h
  package_used()                 those the package calls (their name occurs in stereotracking_amd/*.py outside _lib.py)
  Recorder / Delayed             wrap the attributes of the loaded ctypes handle: log (entry, stream), refuse a stream
                                 that is not the current one (or is the legacy stream 0), delay chosen entries, note
                                 whether the entry returned before the device got to it
  recording_streams()            torch.cuda.Stream replaced by a registering subclass: every stream the package creates
  StreamDelayed                  a delay at the head of one stream before every product call
  same_results(a, b)             bit equality of everything a scenario returns

Every product module reaches the library through `_lib.load().st_*` at call time (`self.lib = _lib.load()` keeps the
HANDLE, never a function object), so patching the handle's attributes reaches every call; there is no second reference
to patch.
"""
import contextlib
import ctypes as C
import os
import re
import statistics

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'stereotrack.h')
PACKAGE = os.path.join(ROOT, 'stereotracking_amd')


# ---- the header: which exports take a stream, and where ------------------------------------------------------------
def _declarations(text):
    """(name, [parameter text]) of every function declaration of a C header."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    text = '\n'.join(line for line in text.split('\n') if not line.lstrip().startswith('#'))
    out = []
    for piece in text.split(';'):
        m = re.search(r'\b(st_\w+)\s*\(([^()]*)\)\s*$', piece, flags=re.S)
        if m and not re.search(r'\btypedef\b', piece):
            out.append((m.group(1), [p.strip() for p in m.group(2).split(',')]))
    return out


def exports_with_stream(header=HEADER):
    """{export name: index of its st_stream_t parameter} for every declaration of the header that has one."""
    with open(header) as f:
        decls = _declarations(f.read())
    out = {}
    for name, params in decls:
        pos = [i for i, p in enumerate(params) if re.match(r'^st_stream_t\b', p)]
        if pos:
            assert len(pos) == 1, f'{name}: more than one st_stream_t parameter'
            out[name] = pos[0]
    return out


def package_used(header=HEADER, package=PACKAGE):
    """The stream-taking exports whose name occurs in a module of the package other than _lib.py (the binding names them
    all)."""
    src = ''
    for fn in sorted(os.listdir(package)):
        if fn.endswith('.py') and fn != '_lib.py':
            with open(os.path.join(package, fn)) as f:
                src += f.read()
    words = set(re.findall(r'\bst_\w+', src))
    return {n: p for n, p in exports_with_stream(header).items() if n in words}


# ---- the delay -----------------------------------------------------------------------------------------------------
_CAL = {}


def _sleep_calibration():
    """Spin cycles of torch.cuda._sleep per millisecond: median of three short sleeps between events, once."""
    import torch
    if 'sleep' not in _CAL:
        probe = 2_000_000
        torch.cuda._sleep(probe)      # first launch: module load
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(probe)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        _CAL['sleep'] = probe / max(statistics.median(ms), 1e-3)
    return _CAL['sleep']


def _aggressor_calibration():
    """The fall-back for a torch build without _sleep: the co-run test's busy kernel (tests/helpers), iterations per ms.
    A weaker delay: its 512 workgroups occupy every CU, so the streams that should race ahead are slowed as well.  The
    torch builds this suite has run under all have _sleep; this path has not been executed on a GPU."""
    import torch
    if 'busy' not in _CAL:
        lib = C.CDLL(os.path.join(ROOT, 'tests', 'helpers', 'libmfma_aggressor.so'))
        fn = lib.st_test_bf16_mfma_busy
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        scratch = torch.zeros(64 * 1024, dtype=torch.float32, device='cuda')     # 256 KB
        probe = 20000

        def launch(iters):
            rc = fn(scratch.data_ptr(), int(iters), 2, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, f'st_test_bf16_mfma_busy: hipError {rc}'
        launch(probe)
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch(probe)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        _CAL['busy'] = (launch, probe / max(statistics.median(ms), 1e-3))
    return _CAL['busy']


def calibrate():
    """Calibrate the delay now (on the current stream), outside anything that is timed or compared."""
    import torch
    if hasattr(torch.cuda, '_sleep'):
        _sleep_calibration()
    else:
        _aggressor_calibration()


def delay(stream, ms):
    """Enqueue about `ms` milliseconds of device-side spinning on `stream`; returns at once."""
    import torch
    with torch.cuda.stream(stream):
        if hasattr(torch.cuda, '_sleep'):
            torch.cuda._sleep(int(_sleep_calibration() * ms))
        else:
            launch, per_ms = _aggressor_calibration()
            launch(max(1, int(per_ms * ms)))


# ---- wrapping the ctypes handle ------------------------------------------------------------------------------------
def _stream_value(a):
    if a is None:
        return 0
    if isinstance(a, C.c_void_p):
        return a.value or 0
    return int(a)


def _current_stream_pointer():
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


class StreamViolation(AssertionError):
    """An entry point was handed a stream that is not the caller's current stream, or the legacy stream 0."""


class Recorder(contextlib.AbstractContextManager):
    """While active, every stream-taking export of `handle` named in `positions` is called through a wrapper that logs
    (entry, stream pointer) into `calls` and raises StreamViolation unless that pointer is the current stream's and not
    0.  The handle's attributes are restored on exit.  `current`: () -> the current stream's pointer."""

    def __init__(self, handle, positions=None, current=_current_stream_pointer):
        self.handle = handle
        self.positions = dict(exports_with_stream() if positions is None else positions)
        self.current = current
        self.calls = []          # (entry, stream pointer), in call order
        self.returned_early = {}     # entry -> [marker.query() after the call returned], Delayed only
        self._saved = {}

    def entries(self):
        """The entry points seen, in order of first call."""
        return list(dict.fromkeys(n for n, _ in self.calls))

    def streams(self):
        return sorted({s for _, s in self.calls})

    def _before(self, name, stream):       # Delayed overrides
        return None

    def _after(self, name, token):
        pass

    def _wrap(self, name, pos, fn):
        def wrapper(*args):
            if pos >= len(args):
                raise StreamViolation(f'{name}: called with {len(args)} arguments, its stream is argument {pos}')
            stream = _stream_value(args[pos])
            self.calls.append((name, stream))
            if stream == 0:
                raise StreamViolation(f'{name}: called on the legacy stream (0)')
            cur = self.current()
            if stream != cur:
                raise StreamViolation(f'{name}: stream {stream:#x} is not the current stream {cur:#x}')
            token = self._before(name, stream)
            rc = fn(*args)
            self._after(name, token)
            return rc
        wrapper.__wrapped__ = fn
        wrapper.__name__ = name
        return wrapper

    def __enter__(self):
        for name, pos in self.positions.items():
            fn = getattr(self.handle, name)
            self._saved[name] = fn
            setattr(self.handle, name, self._wrap(name, pos, fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(self.handle, name, fn)
        self._saved = {}
        return False


class Delayed(Recorder):
    """Recorder that also enqueues `ms` of delay on the call's stream in front of every call of the `entries`, records a
    marker event behind the delay, and notes marker.query() once the real call has returned: False = the entry point
    returned without waiting for the device."""

    def __init__(self, handle, entries, ms, positions=None):
        super().__init__(handle, positions)
        self.delayed, self.ms = set(entries), float(ms)
        unknown = self.delayed - set(self.positions)
        if unknown:
            raise KeyError(f'not stream-taking exports: {sorted(unknown)}')

    def _before(self, name, stream):
        if name not in self.delayed:
            return None
        import torch
        cur = torch.cuda.current_stream()
        delay(cur, self.ms)
        marker = torch.cuda.Event()
        marker.record(cur)
        return marker

    def _after(self, name, marker):
        if marker is not None:
            self.returned_early.setdefault(name, []).append(not marker.query())


# ---- streams the package creates -----------------------------------------------------------------------------------
@contextlib.contextmanager
def recording_streams():
    """torch.cuda.Stream replaced by a subclass that registers every NEWLY created stream (the objects
    torch.cuda.current_stream() builds around an existing stream are not new).  Yields the list."""
    import torch
    created = []
    real = torch.cuda.Stream

    class RecordingStream(real):
        def __new__(cls, *args, **kwargs):
            s = super().__new__(cls, *args, **kwargs)
            if 'stream_id' not in kwargs and 'stream_ptr' not in kwargs:
                created.append(s)
            return s

    torch.cuda.Stream = RecordingStream
    try:
        yield created
    finally:
        torch.cuda.Stream = real


class StreamDelayed:
    """before-call hook of a scenario: `ms` of delay at the head of `stream` before every product call."""

    def __init__(self, stream, ms):
        self.stream, self.ms = stream, float(ms)

    def __call__(self):
        delay(self.stream, self.ms)


def independent(held, other, ms=20.0):
    """True when work enqueued on `other` AFTER a delay on `held` completes while that delay is still running: the two
    streams do not share a hardware queue (streams that do serialise, which hides a race and never invents one)."""
    import torch
    held.synchronize()
    other.synchronize()
    delay(held, ms)
    marker = torch.cuda.Event()
    marker.record(held)
    with torch.cuda.stream(other):
        torch.zeros(1, device=other.device).add_(1)
        done = torch.cuda.Event()
        done.record(other)
    done.synchronize()
    free = not marker.query()
    held.synchronize()
    return free


def independent_stream(later, device, tries=16):
    """A new stream that can be held by a delay while every stream of `later` keeps running (the sabotage checks need
    the delayed stream and its racing consumer on different hardware queues); raises when `tries` streams found none."""
    import torch
    kept = []
    for _ in range(tries):
        s = torch.cuda.Stream(device=device)
        kept.append(s)        # held until the search ends, so that the runtime hands out another queue next time
        if all(independent(s, o) for o in later):
            return s
    raise RuntimeError(f'none of {tries} new streams runs independently of the {len(later)} given streams')


def delay_length(t0_s):
    """D = max(50 ms, 2 x t0), capped at 500 ms; t0 = host wall time of one plain product call in seconds."""
    return min(500.0, max(50.0, 2e3 * t0_s))


# ---- comparing what a scenario returns -----------------------------------------------------------------------------
def flatten(obj, path='', out=None):
    """Every tensor / array / scalar reachable from a scenario's result -> {path: value}.  Understands dicts, sequences,
    the package's InstanceData / TrackDataSample (fields and metainfo) and plain objects holding arrays (StereoStats)."""
    import torch
    out = {} if out is None else out
    if obj is None or isinstance(obj, (bool, int, float, str, np.generic)) or torch.is_tensor(obj) or \
            isinstance(obj, np.ndarray):
        out[path] = obj
    elif isinstance(obj, dict):
        for k in sorted(obj, key=str):
            flatten(obj[k], f'{path}.{k}', out)
    elif isinstance(obj, (list, tuple)):
        out[path + '.len'] = len(obj)
        for i, v in enumerate(obj):
            flatten(v, f'{path}[{i}]', out)
    elif type(obj).__name__ == 'TrackDataSample':
        flatten(dict(obj.metainfo), path + '.meta', out)
        for k in ('pred_det_instances', 'pred_track_instances', 'dense_depth_map'):
            if k in obj:
                flatten(getattr(obj, k), f'{path}.{k}', out)
    elif type(obj).__name__ == 'InstanceData':
        flatten({k: obj[k] for k in obj.keys()}, path, out)
    elif hasattr(obj, '__dict__'):
        flatten({k: v for k, v in vars(obj).items() if not k.startswith('_')}, f'{path}<{type(obj).__name__}>', out)
    else:
        raise TypeError(f'{path}: cannot compare a {type(obj).__name__}')
    return out


def _same(x, y):
    import torch
    if torch.is_tensor(x) or torch.is_tensor(y):
        import guard_memory
        return torch.is_tensor(x) and torch.is_tensor(y) and guard_memory.same_bits(x, y)
    return _bits(x) == _bits(y)


def _bits(v):
    if isinstance(v, (np.ndarray, np.generic)):
        v = np.ascontiguousarray(v)
        return (str(v.dtype), tuple(v.shape), v.tobytes())
    if isinstance(v, float):
        return ('float', (), np.float64(v).tobytes())
    return (type(v).__name__, (), repr(v))


def differences(a, b):
    """Paths at which two scenario results differ bit for bit (a path only one of them has differs)."""
    fa, fb = flatten(a), flatten(b)
    return [k for k in sorted(set(fa) | set(fb)) if k not in fa or k not in fb or not _same(fa[k], fb[k])]


def same_results(a, b):
    return not differences(a, b)
