"""GPU: st_disp_fuse, the launch that builds the map the per-box depth stage reads from the completion head's output.

Everything here is an equality: mode 1 against st_disp_head_resize bit for bit, mode 2 against numpy's
where(disp > 0, disp, mode 1), `filled` against numpy's count over the extent; then the memory contract of DESIGN.md 2
(0xFF-filled outputs inside guard bands, NaN in the planes that are not read, two runs, batch independence) and the
refusals, which must leave the output bytes as they were."""
import numpy as np
import pytest
import torch

import guard_memory as gm
from stereotracking_amd._lib import current_stream, ptr

pytestmark = pytest.mark.gpu

# (N, H, W, (ext_h, ext_w)): one quad per row tail-free; several workgroups and a narrower extent; W/2 = 10 - source rows
# that are not 16-byte aligned - with H, W no multiple of the block and an extent cut on both axes
SHAPES = [(1, 16, 16, (13, 16)), (2, 32, 48, (32, 45)), (3, 24, 20, (22, 19))]
SPECIALS = (0.0, -0.0, -3.5, float('nan'), float('inf'), 1e-40)       # 1e-40: a positive denormal, valid like any > 0


def _dense(N, H, W):
    g = torch.Generator().manual_seed(1000 * N + H + W)
    return torch.relu(torch.randn(N, 1, H // 2, W // 2, generator=g) * 20 + 5)       # zeros and positives, as the head yields


def _disp(N, C, H, W, kind):
    """(N, C, H, W): plane 0 = ordinary values in (0.5, 60) with every special value on about a tenth of the pixels each
    ('mixed'), all ordinary ('valid'), or only the specials that are not > 0 ('invalid'); planes 1.. = NaN."""
    g = torch.Generator().manual_seed(7 * N + 3 * H + W + C)
    plane = torch.rand(N, H, W, generator=g) * 59.5 + 0.5
    pick = torch.randint(0, 10, (N, H, W), generator=g)
    if kind == 'mixed':
        for k, v in enumerate(SPECIALS):
            plane[pick == k] = v
    elif kind == 'invalid':
        for k in range(10):
            plane[pick == k] = SPECIALS[k % 4]
    d = torch.full((N, C, H, W), float('nan'))
    d[:, 0] = plane
    return d


def _ff(shape, dtype=torch.float32):
    """A host tensor whose every byte is 0xFF."""
    return torch.full(shape, -1, dtype=torch.int32).view(dtype) if dtype == torch.float32 else torch.full(shape, -1, dtype=dtype)


def _resize(stlib, dense, H, W):
    N, _, h, w = dense.shape
    out = torch.empty(N, 1, H, W, device=dense.device)
    assert stlib.st_disp_head_resize(ptr(dense), N, h, w, ptr(out), H, W, current_stream()) == 0
    return out


def _fuse(stlib, dense, disp, ext, mode, out, filled):
    N, C, H, W = disp.shape
    return stlib.st_disp_fuse(ptr(dense), ptr(disp), C * H * W, N, H, W, ext[0], ext[1], mode, ptr(out),
                              ptr(filled) if filled is not None else None, current_stream())


def _run(stlib, cuda, dense_h, disp_h, ext, mode):
    """One call with every buffer inside guard bands and the outputs pre-filled with 0xFF -> (out, filled) on the host."""
    N, C, H, W = disp_h.shape
    dense, disp = gm.arena(dense_h, device=cuda), gm.arena(disp_h, device=cuda)
    out, filled = gm.arena(_ff((N, 1, H, W)), device=cuda), gm.arena(_ff((N,), torch.int32), device=cuda)
    before = gm.bits(dense), gm.bits(disp)
    assert _fuse(stlib, dense, disp, ext, mode, out, filled) == 0, stlib.st_last_error()
    torch.cuda.synchronize()
    assert gm.bands_intact(dense, disp, out, filled), 'a guard band was written'
    assert torch.equal(gm.bits(dense), before[0]) and torch.equal(gm.bits(disp), before[1]), 'an input was written'
    return out.cpu(), filled.cpu()


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope='module')
def up2(stlib, cuda):
    """st_disp_head_resize of every shape's dense map, computed once and shared (read-only)."""
    res = {}
    for N, H, W, _ in SHAPES:
        res[(N, H, W)] = _resize(stlib, _dense(N, H, W).to(cuda), H, W).cpu().numpy()
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'N%d_%dx%d' % s[:3])
def test_modes_and_filled_against_numpy(stlib, cuda, up2, shape, C):
    N, H, W, ext = shape
    want1 = up2[(N, H, W)]
    assert np.isfinite(want1).all() and (want1 == 0).any() and (want1 > 0).any()
    dense = _dense(N, H, W)
    for kind in ('mixed', 'valid', 'invalid'):
        disp = _disp(N, C, H, W, kind)
        plane = disp[:, :1].numpy()
        out1, filled1 = _run(stlib, cuda, dense, disp, ext, 1)
        assert _same(out1.numpy(), want1), f'mode 1 differs from st_disp_head_resize ({kind})'
        assert filled1.tolist() == [ext[0] * ext[1]] * N
        out2, filled2 = _run(stlib, cuda, dense, disp, ext, 2)
        with np.errstate(invalid='ignore'):
            valid = plane > 0
        want2 = np.where(valid, plane, want1)
        assert _same(out2.numpy(), want2), f'mode 2 differs from where(disp > 0, disp, up2) ({kind})'
        count = (~valid)[:, 0, :ext[0], :ext[1]].reshape(N, -1).sum(1)
        assert filled2.tolist() == count.tolist(), kind
        if kind == 'mixed':      # every special value is present inside the map, and each went the way the rule says
            assert np.isinf(out2.numpy()).any() and (out2.numpy() == np.float32(1e-40)).any()
            assert not np.isnan(out2.numpy()).any() and not (out2.numpy() < 0).any()
            assert 0 < count.min() and count.max() < ext[0] * ext[1]
        elif kind == 'valid':
            assert filled2.tolist() == [0] * N and _same(out2.numpy(), plane)
        else:
            assert filled2.tolist() == [ext[0] * ext[1]] * N and _same(out2.numpy(), want1)


def test_filled_may_be_null_and_the_map_is_the_same(stlib, cuda):
    N, H, W, ext = SHAPES[1]
    dense, disp = _dense(N, H, W).to(cuda), _disp(N, 3, H, W, 'mixed').to(cuda)
    filled = torch.empty(N, dtype=torch.int32, device=cuda)
    a, b = torch.empty(N, 1, H, W, device=cuda), torch.empty(N, 1, H, W, device=cuda)
    assert _fuse(stlib, dense, disp, ext, 2, a, filled) == 0 and _fuse(stlib, dense, disp, ext, 2, b, None) == 0
    torch.cuda.synchronize()
    assert gm.same_bits(a, b)


@pytest.mark.parametrize('mode', [1, 2])
def test_two_runs_are_bytewise_equal_and_image_0_does_not_depend_on_its_batch(stlib, cuda, mode):
    N, H, W, ext = SHAPES[2]
    dense, disp = _dense(N, H, W), _disp(N, 3, H, W, 'mixed')
    a, fa = _run(stlib, cuda, dense, disp, ext, mode)
    b, fb = _run(stlib, cuda, dense, disp, ext, mode)
    assert gm.same_bits(a, b) and fa.tolist() == fb.tolist()
    one, f1 = _run(stlib, cuda, dense[:1].contiguous(), disp[:1].contiguous(), ext, mode)
    assert gm.same_bits(one, a[:1]) and f1.tolist() == fa[:1].tolist()
    assert not gm.same_bits(a[:1], a[1:2])


def test_an_unaligned_map_takes_the_scalar_path(stlib, cuda):
    """disp and out 4 bytes off a 16-byte boundary: no 16-byte access is possible, the result is the same."""
    N, H, W, ext = SHAPES[1]
    dense, disp_h = _dense(N, H, W).to(cuda), _disp(N, 1, H, W, 'mixed')
    base_out = torch.empty(N, 1, H, W, device=cuda)
    filled = torch.empty(N, dtype=torch.int32, device=cuda)
    assert _fuse(stlib, dense, disp_h.to(cuda), ext, 2, base_out, filled) == 0
    raw_d = torch.full((N * H * W + 1,), float('nan'), device=cuda)
    raw_o = _ff((N * H * W + 2,)).to(cuda)
    disp, out = raw_d[1:].view(N, 1, H, W), raw_o[1:-1].view(N, 1, H, W)
    disp.copy_(disp_h)
    assert disp.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    filled2 = torch.empty(N, dtype=torch.int32, device=cuda)
    assert _fuse(stlib, dense, disp, ext, 2, out, filled2) == 0
    torch.cuda.synchronize()
    assert gm.same_bits(out, base_out) and filled.tolist() == filled2.tolist()
    assert gm.bits(raw_o[:1]).tolist() == [-1] and gm.bits(raw_o[-1:]).tolist() == [-1]


def test_refusals_return_non_zero_and_write_nothing(stlib, cuda):
    N, H, W = 2, 16, 24
    dense, disp = _dense(N, H, W).to(cuda), _disp(N, 3, H, W, 'mixed').to(cuda)
    out, filled = _ff((N, 1, H, W)).to(cuda), _ff((N,), torch.int32).to(cuda)
    s = current_stream()
    good = dict(dense=ptr(dense), disp=ptr(disp), stride=3 * H * W, N=N, H=H, W=W, eh=H, ew=W, mode=2, out=ptr(out),
                filled=ptr(filled))
    bad = [dict(dense=None), dict(disp=None), dict(out=None), dict(H=15), dict(W=23), dict(H=0), dict(N=0), dict(eh=0),
           dict(eh=H + 1), dict(ew=0), dict(ew=W + 1), dict(mode=0), dict(mode=3), dict(stride=H * W - 1)]
    for b in bad:
        k = dict(good, **b)
        rc = stlib.st_disp_fuse(k['dense'], k['disp'], k['stride'], k['N'], k['H'], k['W'], k['eh'], k['ew'], k['mode'],
                                k['out'], k['filled'], s)
        assert rc != 0 and b'st_disp_fuse' in stlib.st_last_error(), b
    torch.cuda.synchronize()
    assert bool((gm.bits(out) == -1).all()) and bool((gm.bits(filled) == -1).all()), 'a refused call wrote its output'
    k = good
    assert stlib.st_disp_fuse(k['dense'], k['disp'], k['stride'], N, H, W, H, W, 2, k['out'], k['filled'], s) == 0
    torch.cuda.synchronize()
    assert not bool((gm.bits(out) == -1).any()) and int(filled.min()) >= 0
