"""CPU: the guard-memory harness itself (tests/guard_memory.py), its sensitivity on a numpy model of the bug class it is
for, and the host weight packers into hostile destinations."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_memory as gm  # noqa: E402
from stereotracking_amd import _lib, aflink  # noqa: E402
from stereotracking_amd._lib import check, ptr  # noqa: E402


# ---- arena / slack / poisoned_empty ----------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,dtype', [((2, 3, 5, 12), torch.float32), ((1, 1, 1, 4), torch.float32),
                                         ((3, 7, 9), torch.uint8), ((5,), torch.int64), ((4, 8), torch.float64)])
def test_arena_preserves_values_strides_and_alignment(shape, dtype):
    g = torch.Generator().manual_seed(len(shape))
    t = (torch.rand(shape, generator=g) * 200).to(dtype)
    for offset in (0, 4, 8, 12):        # 0: what every buffer builder asks for; the others: tests/pointer_contract.py
        _arena_at(t, shape, dtype, offset)


def _arena_at(t, shape, dtype, offset):
    if offset % t.element_size():       # a tensor cannot start between two of its own elements
        with pytest.raises(AssertionError):
            gm.arena(t, offset_bytes=offset)
        return
    a = gm.arena(t, offset_bytes=offset) if offset else gm.arena(t)     # the default is offset 0
    base, front, nbytes = a._arena
    band = front - offset
    assert a.shape == t.shape and a.stride() == t.stride() and a.dtype == t.dtype and torch.equal(a, t)
    assert band % 256 == 0 and band >= gm.min_band(t) and nbytes == t.numel() * t.element_size()
    if t.dim() == 4:      # two rows of an NHWC map (2 * W * ld * 4 bytes) and a K-chunk
        assert band >= 2 * shape[2] * shape[3] * t.element_size() + 4096
    assert a.data_ptr() % 256 == offset and a.data_ptr() == base.data_ptr() + band + offset
    assert base.data_ptr() % 256 == 0
    if offset == 0:
        assert a.data_ptr() % 256 == 0 and a.data_ptr() % 16 == 0
    else:
        assert a.data_ptr() % 16 == offset
    assert base.numel() == 2 * band + offset + nbytes          # both bands whole, the shift on top of the front one
    assert gm.bands_intact(a)
    assert bool((base[:front] == 0xFF).all()) and bool((base[front + nbytes:] == 0xFF).all())
    assert base[front + nbytes:].numel() == band
    if dtype == torch.float32:      # the cell before and the cell after the tensor read as NaN
        assert torch.isnan(base[front - 4:front].view(torch.float32)).all()
        assert torch.isnan(base[front + nbytes:front + nbytes + 4].view(torch.float32)).all()
    a.view(-1)[0] = 1                   # a write inside the tensor leaves the bands alone ...
    assert gm.bands_intact(a)
    if offset:                          # ... one into the bytes the shift skipped does not
        base[band] = 0
        assert not gm.bands_intact(a)


def test_arena_keeps_the_strides_of_a_view_and_refuses_a_short_band():
    t = torch.arange(2 * 4 * 6 * 10, dtype=torch.float32).view(2, 4, 6, 10)[..., 2:8]     # a channel slice: ld 10
    a = gm.arena(t)
    assert a.stride() == t.stride() and torch.equal(a, t) and not a.is_contiguous()
    assert gm.bands_intact(a)
    with pytest.raises(AssertionError):
        gm.arena(torch.zeros(1, 4, 6, 10), band=256)           # under two rows + 4096
    with pytest.raises(AssertionError):
        gm.arena(torch.zeros(1, 4, 6, 10), band=8200)          # not a multiple of 256


@pytest.mark.parametrize('where', ['before', 'after', 'last byte'])
def test_bands_intact_sees_one_changed_byte(where):
    a = gm.arena(torch.zeros(1, 2, 3, 8))
    base, band, nbytes = a._arena
    base[{'before': band - 1, 'after': band + nbytes, 'last byte': base.numel() - 1}[where]] = 0xFE
    assert not gm.bands_intact(a)
    a.fill_(5.0)                                                # writing the tensor itself is not a band write
    b = gm.arena(torch.zeros(1, 2, 3, 8))
    b.fill_(5.0)
    assert gm.bands_intact(b)


def test_slack_fills_only_the_channels_outside_the_slice():
    x = torch.arange(2 * 3 * 10, dtype=torch.float32).view(2, 3, 10).clone()
    keep = x[..., 3:7].clone()
    gm.slack(x, 3, 4)
    assert torch.equal(x[..., 3:7], keep)
    out = torch.cat([x[..., :3], x[..., 7:]], -1)
    assert not torch.isfinite(out).any()
    assert torch.isnan(out[..., 0]).all() and (out[..., 1] == float('inf')).all() and (out[..., 2] == float('-inf')).all()
    assert torch.isnan(out[..., 3]).all()                       # in turn: the pattern repeats
    full = torch.ones(2, 4)
    assert torch.equal(gm.slack(full.clone(), 0, 4), full)      # no slack: untouched


@pytest.mark.parametrize('pattern', [0x00, 0xFF, 0x7F])
def test_poisoned_empty_fills_and_counts(pattern):
    originals = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with gm.poisoned_empty(pattern) as p:
        a = torch.empty(3, 5)
        b = torch.empty((7,), dtype=torch.int64)
        c = torch.empty_like(a, dtype=torch.float64)
        d = a.new_empty((2, 2), dtype=torch.uint8)
        e = torch.empty(0)                                      # nothing to fill: not counted
        assert p.count == 4 and p.device_count == 0
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == originals
    for t in (a, b, c, d):
        assert bool((gm.bits(t).view(torch.uint8) == pattern).all())
    assert e.numel() == 0
    if pattern == 0xFF:
        assert torch.isnan(a).all() and torch.isnan(c).all() and bool((b == -1).all())
    if pattern == 0x7F:
        assert bool((a > 3.0e38).all()) and torch.isfinite(a).all()
    before = p.count
    torch.empty(4)
    assert p.count == before                                    # restored on exit, also after an exception:
    with pytest.raises(ZeroDivisionError):
        with gm.poisoned_empty(0xFF):
            1 / 0
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == originals


def test_cases_of_reads_a_tests_own_parametrize_tables():
    @pytest.mark.parametrize('b', [False, True])
    @pytest.mark.parametrize('x,y', [(1, 2), (3, 4)])
    def fn(x, y, b):
        pass
    got = [kw for _, kw in gm.cases_of(fn)]
    assert len(got) == 4 and dict(x=3, y=4, b=True) in got and dict(x=1, y=2, b=False) in got
    assert len({ident for ident, _ in gm.cases_of(fn)}) == 4
    assert gm.cases_of(lambda: None) == [('', {})]


# ---- sensitivity: a numpy model of the bug class ---------------------------------------------------------------------
def _conv1x1_model(buf, in_off, cin, w, masked):
    """1x1 conv over the channel slice [in_off, in_off + cin) of `buf`, K padded to 32 with zero weights, the way an
    MFMA kernel walks whole K-chunks.  masked: padded channels are loaded as 0;  else: loaded and multiplied by 0."""
    kpad = (cin + 31) // 32 * 32
    wp = np.zeros((w.shape[0], kpad), np.float32)
    wp[:, :cin] = w
    flat = np.concatenate([buf.reshape(-1), np.full(kpad, np.nan, np.float32)])     # what follows the buffer: a guard band
    M, ld = buf.shape[0] * buf.shape[1] * buf.shape[2], buf.shape[3]
    idx = (np.arange(M) * ld + in_off)[:, None] + np.arange(kpad)[None, :]
    a = flat[idx]                                                                   # (M, kpad): runs past the slice
    if masked:
        a = np.where(np.arange(kpad)[None, :] < cin, a, np.float32(0.0))
    with np.errstate(invalid='ignore'):
        return (a @ wp.T).reshape(buf.shape[:3] + (w.shape[0],))


@pytest.mark.parametrize('cin,ld,off', [(24, 40, 8), (12, 12, 0), (32, 48, 16)])
def test_harness_tells_a_multiplied_load_from_a_masked_one(cin, ld, off):
    """The gap this harness closes: over finite garbage the multiplying kernel is bit-identical to the masked one, so a
    parity test passes both.  Over slack() / a guard band the multiplying one turns NaN and assert_unaffected fails
    it; the masked one passes."""
    rng = np.random.default_rng(cin)
    x = rng.normal(size=(1, 3, 5, cin)).astype(np.float32)
    w = rng.normal(size=(6, cin)).astype(np.float32)
    friendly = (rng.normal(size=(1, 3, 5, ld)) * 3.0).astype(np.float32)
    friendly[..., off:off + cin] = x
    hostile = gm.slack(torch.from_numpy(friendly.copy()), off, cin).numpy()
    base = {m: _conv1x1_model(friendly, off, cin, w, m) for m in (True, False)}
    got = {m: _conv1x1_model(hostile, off, cin, w, m) for m in (True, False)}
    if cin % 32:
        # finite garbage hides the difference on every pixel whose K-chunk ends inside the buffer
        kpad, M = (cin + 31) // 32 * 32, 15
        inside = [p for p in range(M) if p * ld + off + kpad <= M * ld]
        assert len(inside) >= M - 2
        assert np.array_equal(base[True].reshape(-1, 6)[inside], base[False].reshape(-1, 6)[inside])
        with pytest.raises(AssertionError):
            gm.assert_unaffected(got[False], base[True], 'multiplying model')
        assert not np.isfinite(got[False]).all()
    else:                                   # Cin = 32 = ld: nothing is padded, nothing can be read - both are clean
        gm.assert_unaffected(got[False], base[True], 'multiplying model, no padding')
    gm.assert_unaffected(got[True], base[True], 'masked model')


def test_assert_unaffected_rejects_a_hidden_nan_and_a_changed_bit():
    base = torch.tensor([1.0, 2.0, 3.0])
    gm.assert_unaffected(base.clone(), base)
    with pytest.raises(AssertionError, match='non-finite'):
        gm.assert_unaffected(torch.tensor([1.0, float('nan'), 3.0]), base)
    with pytest.raises(AssertionError, match='differs'):
        gm.assert_unaffected(torch.tensor([1.0, 2.0000002, 3.0]), base)
    with pytest.raises(AssertionError, match='differs'):
        gm.assert_unaffected(torch.tensor([1.0, 2.0, -0.0]), torch.tensor([1.0, 2.0, 0.0]))    # bitwise, not ==
    ids = torch.tensor([-1, 4], dtype=torch.int64)
    gm.assert_unaffected(ids.clone(), ids)


def test_session_records_buffers_and_sees_a_written_input():
    with gm.session('nonfinite', True) as s:
        assert gm.current() is s
        host = torch.ones(1, 2, 3, 8)
        x = s.input(host, 'cpu', 2, 4)
        o = s.output((1, 2, 3, 4), 'cpu')
        assert torch.equal(x[..., 2:6], host[..., 2:6]) and not torch.isfinite(x[..., :2]).any()
        assert bool((o == gm.GUARD).all()) and len(s.arenas()) == 2
        assert s.bands_intact() and s.unchanged()
        x[0, 0, 0, 7] = 1.0                                     # a slack cell
        assert not s.unchanged() and s.bands_intact()
    assert gm.current().garbage == 'finite' and not gm.current().arena


def test_default_session_records_nothing_and_frames_hold_inf():
    """Outside a guard test the builders keep no reference to what they hand out (a parity test's buffers die with it);
    inside one, framed() puts +Inf images around a buffer, since a max reduction drops the NaN of a guard band."""
    d = gm.current()
    assert not d.record and d.garbage == 'finite' and not d.arena
    d.input(torch.ones(1, 2, 3, 8), 'cpu', 2, 4)
    d.output((1, 2, 3, 4), 'cpu')
    d.framed(torch.ones(2, 2, 3, 8), 'cpu', written=True)
    d.track(torch.ones(3))
    assert d.inputs == [] and d.outputs == [] and d.framed_buffers == []
    with gm.session('nonfinite', True) as s:
        host = torch.arange(2 * 2 * 3 * 8, dtype=torch.float32).view(2, 2, 3, 8)
        x = s.framed(host, 'cpu', 2, 4)
        whole, value = s.framed_buffers[0]
        assert whole.shape == (4, 2, 3, 8) and value == float('inf') and x.data_ptr() == whole[1].data_ptr()
        assert torch.equal(x[..., 2:6], host[..., 2:6]) and bool((x[..., 1] == float('inf')).all())
        assert bool((whole[0] == float('inf')).all()) and bool((whole[-1] == float('inf')).all())
        assert s.frames_intact() and s.bands_intact() and s.unchanged() and len(s.arenas()) == 1
        whole[-1, 0, 0, 0] = 1.0
        assert not s.frames_intact()


# ---- host packers into a NaN-prefilled destination -------------------------------------------------------------------
def _both(n, fill):
    """fill(dst) into a zero-prefilled and a NaN-prefilled fp32 destination of n floats -> the two results."""
    out = []
    for v in (0.0, float('nan')):
        dst = torch.full((n,), v, dtype=torch.float32)
        fill(dst)
        out.append(dst)
    return out


def _conv_packed(lib, cout, cin, k, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, k, k, generator=g)
    b = torch.randn(cout, generator=g)
    wp = torch.zeros(lib.st_conv_packed_floats(cout, cin, k, k), dtype=torch.float32)
    bp = torch.zeros((cout + 31) // 32 * 32, dtype=torch.float32)
    check(lib.st_conv_pack_weights(ptr(w), ptr(b), None, None, None, None, 0.0, cout, cin, k, k, ptr(wp), ptr(bp)))
    return w, b, wp, bp


@pytest.mark.parametrize('cout,cin,k', [(5, 128, 1), (48, 24, 3), (40, 16, 3), (64, 72, 1), (32, 12, 3)])
def test_conv_pack_writes_its_own_padding(cout, cin, k, stlib):
    """st_conv_pack_weights: Cout padded to 32 rows, K = k * k * Cin padded to 32 columns, bias padded to 32 - every
    cell of both destinations is written, the padding as zeros."""
    g = torch.Generator().manual_seed(cout + cin)
    w, b = torch.randn(cout, cin, k, k, generator=g), torch.randn(cout, generator=g)
    bn = [torch.rand(cout, generator=g) + 0.5 for _ in range(4)]
    res = []
    for v in (0.0, float('nan')):
        wp = torch.full((stlib.st_conv_packed_floats(cout, cin, k, k),), v, dtype=torch.float32)
        bp = torch.full(((cout + 31) // 32 * 32,), v, dtype=torch.float32)
        check(stlib.st_conv_pack_weights(ptr(w), ptr(b), ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), 1e-3, cout, cin,
                                         k, k, ptr(wp), ptr(bp)))
        res.append((wp, bp))
    assert gm.same_bits(res[0][0], res[1][0]) and gm.same_bits(res[0][1], res[1][1])
    kpad = (cin * k * k + 31) // 32 * 32
    wp = res[1][0].view(-1, kpad)
    assert torch.isfinite(wp).all() and bool((wp[cout:] == 0).all()) and bool((wp[:, cin * k * k:] == 0).all())
    assert bool((res[1][1][cout:] == 0).all())


@pytest.mark.parametrize('cout,cin', [(32, 16), (48, 36), (48, 52), (64, 32), (96, 64)])
def test_wino_pack_writes_its_own_padding(cout, cin, stlib):
    _, _, wp, _ = _conv_packed(stlib, cout, cin, 3, cout * cin)
    n = stlib.st_wino_packed_floats(cout, cin)
    assert n > 0
    zero, nan = _both(n, lambda dst: check(stlib.st_wino_pack_weights(ptr(wp), cout, cin, ptr(dst))))
    assert torch.isfinite(nan).all() and gm.same_bits(zero, nan)


@pytest.mark.parametrize('cout,planes', [(32, 3), (24, 3), (8, 1), (64, 1)])
def test_stem_pack_writes_its_own_padding(cout, planes, stlib):
    g = torch.Generator().manual_seed(cout)
    w = torch.randn(cout, 12, 3, 3, generator=g)
    bn = [torch.rand(cout, generator=g) + 0.5 for _ in range(4)]
    res = []
    for v in (0.0, float('nan')):
        wp = torch.full((stlib.st_stem_packed_floats(cout),), v, dtype=torch.float32)
        bp = torch.full(((cout + 31) // 32 * 32,), v, dtype=torch.float32)
        check(stlib.st_stem_pack_weights(ptr(w), None, ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), 1e-3, cout, planes,
                                         ptr(wp), ptr(bp)))
        res.append((wp, bp))
    assert torch.isfinite(res[1][0]).all() and torch.isfinite(res[1][1]).all()
    assert gm.same_bits(res[0][0], res[1][0]) and gm.same_bits(res[0][1], res[1][1])


@pytest.mark.parametrize('cout,cin', [(64, 64), (32, 32)])
def test_front_pack_frags_writes_every_cell(cout, cin, stlib):
    _, _, wp, _ = _conv_packed(stlib, cout, cin, 1, cout + cin)
    zero, nan = _both(stlib.st_front_frag_floats(cout, cin),
                      lambda dst: check(stlib.st_front_pack_frags(ptr(wp), cout, cin, ptr(dst))))
    assert torch.isfinite(nan).all() and gm.same_bits(zero, nan)


def test_csp_tail_pack_frags_writes_every_cell(stlib):
    _, _, wp, _ = _conv_packed(stlib, 64, 64, 1, 9)
    zero, nan = _both(stlib.st_csp_tail_frag_floats(), lambda dst: check(stlib.st_csp_tail_pack_frags(ptr(wp), ptr(dst))))
    assert torch.isfinite(nan).all() and gm.same_bits(zero, nan)


def test_aflink_pack_weights_over_stale_allocations():
    """pack_weights owns its destination (it returns a fresh array): every allocation it makes through torch.empty* is
    poisoned instead, and the packed bytes must not move."""
    torch.manual_seed(0)
    sd = aflink.AFLinkModel().state_dict()
    with gm.poisoned_empty(0x00):
        zero = aflink.pack_weights(sd)
    with gm.poisoned_empty(0xFF):
        nan = aflink.pack_weights(sd)
    assert np.isfinite(nan).all() and zero.tobytes() == nan.tobytes()
    assert nan.size == int(_lib.load().st_aflink_packed_floats())


@pytest.mark.parametrize('kind', ['agg', 'fullres'])
def test_stereo_module_packing_over_stale_allocations(kind):
    """StereoCostVolume packs its aggregation convs (plain + Winograd form) and its reduce conv into torch.empty
    destinations: over 0xFF-filled ones the packed tensors are the bytes they are over zero-filled ones."""
    from stereotracking_amd.stereo import StereoCostVolume

    def packed(pattern):
        torch.manual_seed(4)
        if kind == 'agg':
            m = StereoCostVolume(max_disp=192, agg_layers=2)            # 48 levels: Cout padded to 64, K tail
            for conv in m.agg:
                conv.weight.normal_()
                conv.bias.normal_()
        else:
            m = StereoCostVolume(max_disp=32, full_res=True, agg3d_layers=1, full_res_channels=8)
            m.reduce.weight.normal_()
            m.reduce.bias.normal_()
        with gm.poisoned_empty(pattern) as p:
            out = [t for layer in m._pack('cpu') for t in layer if t is not None] if kind == 'agg' else \
                list(m._pack_reduce('cpu'))
        assert p.count >= 2, 'the packing did not allocate through torch.empty'
        return out

    zero, nan = packed(0x00), packed(0xFF)
    assert len(zero) == len(nan) and len(nan) >= 2
    for z, n in zip(zero, nan):
        assert torch.isfinite(n).all() and gm.same_bits(z, n)
