"""Hostile surroundings for a kernel's memory (test infrastructure; a helper module, not a conftest).

The contract: an entry point reads only the cells its arguments describe - the channel slice of a wider
NHWC buffer, the rows of its map - and treats workspace and output memory as arbitrary bits.  The parity tests surround
inputs with finite data and hand out fresh allocations, so `0 * garbage = 0` passes them.  Here the surroundings are
made of the values that do not cancel:

  arena(t)            the tensor inside one larger allocation, 0xFF bytes (a NaN as fp32 / fp64, -1 as an integer) in a
                      guard band before and after it;  bands_intact(t) compares the bands bytewise afterwards
  slack(x, off, cin)  NaN, +Inf, -Inf in turn in every channel outside [off, off + cin)
  poisoned_empty(b)   torch.empty / torch.empty_like / Tensor.new_empty return memory filled with byte b, and count
  session(...)        the ambient mode the buffer builders of the test files read (default: finite garbage, no arena,
                      nothing recorded - what the parity tests have always run), and the record of the buffers built
                      under it;  Session.framed: +Inf images around a buffer that a max reduction reads (fmaxf drops a NaN)
  run_both(fn)        fn under the friendly and under the hostile session, and what the contract promises of the two
  guarded_test(fns)   the parametrized test that puts the case tables of existing tests through run_both

Patterns: 0x00 the baseline; 0xFF a NaN / -1; 0x7F 3.39e38 as fp32 - for float-only memory.
"""
import contextlib

import pytest
import torch

GUARD = -777.0
NONFINITE = (float('nan'), float('inf'), float('-inf'))


def _extent(t):
    """Elements between the first and the last cell of `t`, inclusive (its strides may skip cells)."""
    if t.numel() == 0:
        return 0
    return sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1


def min_band(t):
    """Two rows of the tensor (2 * W * ld * itemsize for an NHWC map: a halo row and more than a K-chunk) plus 4096
    bytes, rounded up to a multiple of 256."""
    row = t.stride(-3) if t.dim() >= 3 else (t.stride(0) if t.dim() >= 1 and t.numel() else 1)
    return (2 * row * t.element_size() + 4096 + 255) // 256 * 256


def arena(t, band=None, device=None, offset_bytes=0):
    """`t`'s shape, strides and values on `device` (default: t's own), inside one uint8 allocation with `band` bytes of
    0xFF before and after it.  band: a multiple of 256 (the bands start on a 256-byte boundary, so the 16-byte
    alignment the kernels require survives), at least min_band(t).  offset_bytes (0 .. 255, a multiple of the element
    size): the tensor starts that many bytes past the 256-byte boundary - a pointer the pointer-contract tests hand to
    an entry point; the band in front of it grows by the same bytes, the band behind it stays whole."""
    band = min_band(t) if band is None else band
    assert band % 256 == 0 and band >= min_band(t), f'band {band}: need a multiple of 256, at least {min_band(t)}'
    assert 0 <= offset_bytes < 256 and offset_bytes % t.element_size() == 0, f'offset_bytes {offset_bytes}'
    device = t.device if device is None else torch.device(device)
    nbytes = _extent(t) * t.element_size()
    front = band + offset_bytes
    raw = torch.full((front + nbytes + band + 256,), 0xFF, dtype=torch.uint8, device=device)
    shift = -raw.data_ptr() % 256       # 0 on the device; host allocations are only 64-byte aligned
    base = raw[shift:shift + front + nbytes + band]
    inner = base[front:front + nbytes].view(t.dtype) if nbytes else base[front:front].view(t.dtype)
    view = inner.as_strided(t.shape, t.stride())
    view.copy_(t)
    view._arena = (base, front, nbytes)     # keeps the allocation alive with the view
    return view


def bands_intact(*tensors):
    """True if both guard bands of every arena tensor still hold 0xFF in every byte."""
    for t in tensors:
        base, band, nbytes = t._arena
        if not (bool((base[:band] == 0xFF).all()) and bool((base[band + nbytes:] == 0xFF).all())):
            return False
    return True


def slack(x, in_off, cin):
    """NaN, +Inf, -Inf in turn in every channel of `x` (last dimension) outside [in_off, in_off + cin); in place."""
    ld = x.shape[-1]
    for n, c in enumerate([c for c in range(ld) if not in_off <= c < in_off + cin]):
        x[..., c] = NONFINITE[n % 3]
    return x


def bits(t):
    """The tensor's cells as integers, so that a NaN compares equal to itself."""
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def assert_unaffected(got, base, what='output', finite=True):
    """The harness's check: the result over hostile surroundings is finite and bit-identical to the friendly one.
    finite=False: for outputs whose contract includes a NaN (a box depth over an empty slice) - bits only."""
    got, base = torch.as_tensor(got), torch.as_tensor(base)
    if finite and got.is_floating_point():
        assert bool(torch.isfinite(got).all()), f'{what}: non-finite values - the kernel read memory it does not own'
    assert same_bits(got, base), f'{what}: differs from the run over finite surroundings'


class poisoned_empty(contextlib.ContextDecorator):
    """Inside the block torch.empty, torch.empty_like and Tensor.new_empty return tensors, device or host, whose every
    byte is `pattern` - what a long-running process gets from the caching allocator instead of fresh zero pages.
    .count = tensors filled, .device_count = those on a GPU."""

    def __init__(self, pattern):
        assert 0 <= pattern <= 0xFF
        self.pattern, self.count, self.device_count = pattern, 0, 0

    def _fill(self, t):
        if isinstance(t, torch.Tensor) and t.numel() and t.layout == torch.strided and t.device.type != 'meta':
            raw = self._orig[0](0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
            raw.fill_(self.pattern)
            self.count += 1
            self.device_count += t.device.type == 'cuda'
        return t

    def __enter__(self):
        self._orig = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
        e, el, ne = self._orig

        def empty(*a, **k):
            return e(*a, **k) if k.get('out') is not None else self._fill(e(*a, **k))

        def empty_like(*a, **k):
            return self._fill(el(*a, **k))

        def new_empty(*a, **k):
            return self._fill(ne(*a, **k))

        torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like, torch.Tensor.new_empty = self._orig
        return False


# ---- the ambient mode of the buffer builders -------------------------------------------------------------------------
class Session:
    """What the buffer builders of the kernel tests do around a kernel's memory, and - inside session() only - the
    record of what they built.  garbage: 'finite' (randn * 3, as ever) or 'nonfinite' (slack());  arena: buffers
    inside guard bands.  The default session (no guard test running) records nothing: a buffer lives as long as its
    test holds it, as it always has."""

    def __init__(self, garbage='finite', arena=False, record=True):
        assert garbage in ('finite', 'nonfinite')
        self.garbage, self.arena, self.record = garbage, arena, record
        self.inputs, self.outputs, self.framed_buffers = [], [], []

    def input(self, host, dev, off=0, cin=None):
        """The host tensor `host` (values in channels [off, off + cin) of its last dimension, finite garbage in the
        others) on the device, its slack non-finite and itself in an arena if the mode says so; recorded, so that
        unchanged() can tell a kernel that wrote its input."""
        host = host.contiguous()
        if self.garbage == 'nonfinite' and cin is not None:
            host = slack(host.clone(), off, cin)
        d = arena(host, device=dev) if self.arena else host.to(dev)
        if self.record:
            self.inputs.append((d, bits(host)))
        return d

    def output(self, shape, dev, fill=GUARD, dtype=torch.float32):
        """An output buffer pre-filled with `fill`, in an arena if the mode says so; recorded."""
        if self.arena:
            d = arena(torch.full(shape, fill, dtype=dtype), device=dev)
        else:
            d = torch.full(shape, fill, dtype=dtype, device=dev)
        return self.track(d)

    def framed(self, host, dev, off=0, cin=None, written=False, value=float('inf')):
        """As input(), for a kernel that reduces with max / min: a NaN band cannot expose its reads (fmaxf drops a NaN),
        so with arenas on the (N, ...) tensor stands between two more images filled with `value` (+Inf wins every max),
        and those inside the arena.  written=True: the kernel works in place - its slice is recorded as an output; the
        test itself holds the slack to the bytes it had."""
        host = host.contiguous()
        if self.garbage == 'nonfinite' and cin is not None:
            host = slack(host.clone(), off, cin)
        if self.arena:
            big = torch.full((host.shape[0] + 2,) + tuple(host.shape[1:]), value, dtype=host.dtype)
            big[1:-1] = host
            whole = arena(big, device=dev)
            self.framed_buffers.append((whole, value))
            d = whole[1:-1]
        else:
            d = host.to(dev)
        if written:      # compared between the runs: the slice the kernel owns (the slack differs by construction)
            self.track(d if cin is None else d[..., off:off + cin])
            return d
        if self.record:
            self.inputs.append((d, bits(host)))
        return d

    def track(self, d):
        """Record a buffer the test built itself (an in-place input / output) as an output."""
        if self.record:
            self.outputs.append(d)
        return d

    def arenas(self):
        return [t for t in [d for d, _ in self.inputs] + self.outputs + [w for w, _ in self.framed_buffers]
                if hasattr(t, '_arena')]

    def bands_intact(self):
        return bands_intact(*self.arenas())

    def frames_intact(self):
        return all(bool((w[0] == v).all()) and bool((w[-1] == v).all()) for w, v in self.framed_buffers)

    def unchanged(self):
        """Every recorded input, slack included, still holds the bytes it was built with."""
        return all(torch.equal(bits(d), h) for d, h in self.inputs if not any(d is o for o in self.outputs))

    def results(self):
        return [o.detach().cpu().clone() for o in self.outputs]


_current = [Session(record=False)]


def current():
    return _current[-1]


@contextlib.contextmanager
def session(garbage='finite', arena=False):
    s = Session(garbage, arena)
    _current.append(s)
    try:
        yield s
    finally:
        _current.pop()


def device_input(host, dev, off=0, cin=None):
    """A numpy array or host tensor as a device input of the ambient session (Session.input)."""
    return current().input(torch.as_tensor(host), dev, off, cin)


def device_planes(host, dev, read=1):
    """An (N, C, H, W) map of which an entry point reads the first `read` planes only (img_pitch steps over the
    others): as device_input, with NaN in the unread planes when the ambient garbage is non-finite."""
    host = torch.as_tensor(host)
    if current().garbage == 'nonfinite' and host.is_floating_point() and host.shape[1] > read:
        host = host.clone()
        host[:, read:] = float('nan')
    return current().input(host, dev)


def device_output(shape, dev, fill=GUARD, dtype=torch.float32):
    """An output buffer of the ambient session (Session.output)."""
    return current().output(tuple(shape), dev, fill, dtype)


def run_both(fn, *args, finite=True, **kwargs):
    """fn(*args) under finite garbage without arenas, then under non-finite garbage inside arenas (fn seeds its own
    random numbers, so both runs see the same problem).  Asserts what the contract promises: every output buffer of
    the hostile run is finite and bit-identical to the friendly run's, the guard bands and the inputs - slack included
    - are unchanged bytewise.  fn's own assertions (fp64 parity, output guard columns) hold in both runs."""
    with session('finite', False) as friendly:
        fn(*args, **kwargs)
    base = friendly.results()
    del friendly
    with session('nonfinite', True) as hostile:
        fn(*args, **kwargs)
    torch.cuda.synchronize()
    got = hostile.results()
    assert len(got) == len(base) and len(got) > 0, 'the two runs built different buffers'
    assert len(hostile.arenas()) > 0, 'nothing ran inside an arena'
    for k, (g, b) in enumerate(zip(got, base)):
        assert_unaffected(g, b, f'output buffer {k}', finite)
    assert hostile.bands_intact(), 'a guard band was written'
    assert hostile.frames_intact(), 'a +Inf frame around a max-reduced buffer was written'
    assert hostile.unchanged(), 'an input buffer (slack channels included) was written'
    return len(got)


def cases_of(fn):
    """The keyword sets of a test function's own @pytest.mark.parametrize table(s): [(id, {argname: value})]."""
    sets = [('', {})]
    for m in reversed([m for m in getattr(fn, 'pytestmark', []) if m.name == 'parametrize']):
        names = [n.strip() for n in m.args[0].split(',')] if isinstance(m.args[0], str) else list(m.args[0])
        new = []
        for ident, kw in sets:
            for v in m.args[1]:
                vals = (v,) if len(names) == 1 else tuple(v)
                tag = '-'.join(str(x) for x in vals).replace(' ', '')
                new.append(((ident + '|' if ident else '') + tag, dict(kw, **dict(zip(names, vals)))))
        sets = new
    return sets


def guarded_test(functions, nan_by_contract=(), applies=lambda fn, kw: True, doc=None):
    """A parametrized test that puts every case of every function of `functions` (their own parametrize tables)
    through run_both.  Fixtures the functions take (cuda, stlib, ...) are looked up by name.  nan_by_contract: functions
    whose outputs may hold a NaN by contract - compared as bits only.  applies(fn, kw): False for a table entry that
    fn itself skips.  Assign the result to a test_* name of the module."""
    params = [pytest.param(fn, kw, id=f'{fn.__name__[5:]}[{ident}]' if ident else fn.__name__[5:])
              for fn in functions for ident, kw in cases_of(fn) if applies(fn, kw)]

    @pytest.mark.parametrize('fn,kw', params)
    def test(fn, kw, request):
        code = fn.__code__
        names = code.co_varnames[:code.co_argcount]
        fixtures = {n: request.getfixturevalue(n) for n in names if n not in kw}
        run_both(fn, finite=fn not in nan_by_contract, **kw, **fixtures)

    test.__doc__ = doc
    return test
