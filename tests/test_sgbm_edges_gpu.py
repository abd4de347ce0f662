"""GPU: StereoSGBM (csrc/sgbm.hip) bit for bit against the numpy restatement (tests/sgbm_ref.py) where wave code goes wrong:
tied minima of the aggregated cost, edge geometries, every option, the int16 bound, both entry points with padding,
crops and more than 32 frames, a dirty workspace, and the median / speckle kernels on adversarial maps - the scenarios of
tests/sgbm_cases.py, whose preconditions tests/test_cpu_sgbm.py asserts without a GPU."""
import numpy as np
import pytest
import torch

import sgbm_cases as K
import sgbm_ref as R
from sgbm_check import assert_stages_bit_exact, batch, up

pytestmark = pytest.mark.gpu


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _stages(cuda, pairs, kw, **more):
    L, Rt = [p[0] for p in pairs], [p[1] for p in pairs]
    return assert_stages_bit_exact(cuda, L, Rt, kw, refs=[K.reference(a, b, kw) for a, b in pairs], **more)


# ---- every scenario, stage by stage, as slot 0 of an N = 2 batch ---------------------------------------------------------
@pytest.mark.parametrize('uniq', K.TIES_UNIQ)
@pytest.mark.parametrize('D', K.TIES_D)
@pytest.mark.parametrize('name', list(K.TIES))
def test_ties_bit_exact(cuda, name, D, uniq):
    """Tied minima of S: the lowest d wins, the uniqueness test at equality, disp2 ties to the highest x."""
    _stages(cuda, [K.TIES[name], K.TIES[K.ties_partner(name)]], K.ties_kw(D, uniq))


@pytest.mark.parametrize('g', K.GEOMETRY, ids=K.geometry_id)
def test_geometry_bit_exact(cuda, g):
    """One computed column, partial blocks of the column waves and partial chunks of the row pass, h below the block
    radius, block_size 7 and 9."""
    _stages(cuda, K.geometry_pairs(g), K.geometry_kw(g))


@pytest.mark.parametrize('kw', K.OPTIONS, ids=K.options_id)
def test_options_bit_exact(cuda, kw):
    _stages(cuda, K.options_pairs(), kw)


def test_bound_bit_exact(cuda):
    """P2 at the int16 bound: S up to 23035 through the int16 C, L_tb and S1 volumes."""
    _stages(cuda, K.bound_pairs(), K.BOUND_KW)


# ---- the entry points ------------------------------------------------------------------------------------------------------
PADDING = [('ties', [K.TIES['stripes-rolled'], K.TIES['halfplane-rolled']], K.ties_kw(48, 0)),
           ('geometry', K.geometry_pairs(K.GEOMETRY[8]), K.geometry_kw(K.GEOMETRY[8]))]


@pytest.mark.parametrize('pairs,kw', [p[1:] for p in PADDING], ids=[p[0] for p in PADDING])
def test_f32_entry_never_reads_the_padding(cuda, pairs, kw):
    """Random values 0..255 outside (h, w) instead of 114: every stage still equals the restatement, and the results
    equal the run with 114 bit for bit."""
    h, w = pairs[0][0].shape[1:]
    H, W = up(h), up(w)
    assert W > w and w % 32 != 0
    noise = np.random.RandomState(3).randint(0, 256, (2, 3, H, W)).astype(np.float32)
    assert (noise[:, :, :, w:] != 114.0).mean() > 0.9
    _, plain = _stages(cuda, pairs, kw)
    _, noisy = _stages(cuda, pairs, kw, pad=noise)
    for key in ('cost', 'raw', 'out'):
        assert torch.equal(plain[key], noisy[key]), key


def test_u8_entry_crops_larger_frames(cuda):
    """uint8 frames of (40, 96) with valid_hw (33, 67): the restatement of the top-left crop, and the fp32 entry on it."""
    from stereotracking_amd.engine import RawChunk
    from stereotracking_amd.sgbm import StereoSGBM
    g = K.GEOMETRY[8]
    (h, w), kw, pairs = g[:2], K.geometry_kw(g), K.geometry_pairs(g)
    assert (h, w) == (33, 67)
    fh, fw, H, W = 40, 96, 64, 96
    rng = np.random.RandomState(4)
    frames = []
    for side in range(2):
        fs = []
        for p in pairs:
            f = rng.randint(0, 256, (3, fh, fw)).astype(np.uint8)
            f[:, :h, :w] = p[side]
            fs.append(_dev(f, cuda))
        frames.append(fs)
    m = StereoSGBM(**kw)
    a = torch.full((2, 3, H, W), -1.0, device=cuda)
    b = torch.full((2, 3, H, W), -1.0, device=cuda)
    m.compute(RawChunk(frames[0], 114.0), RawChunk(frames[1], 114.0), (h, w), a)
    st_u8 = int(m.last_status.item())
    m.compute(batch([p[0] for p in pairs], H, W, cuda), batch([p[1] for p in pairs], H, W, cuda), (h, w), b)
    torch.cuda.synchronize()
    for i, p in enumerate(pairs):
        want = R.disp_postp(K.reference(p[0], p[1], kw)['final'], H, W)
        assert np.array_equal(a[i].cpu().numpy(), want), f'pair {i}: uint8 entry'
        assert want.any()
    assert torch.equal(a, b)
    assert st_u8 == 0 and int(m.last_status.item()) == 0


def test_u8_entry_more_than_32_frames(cuda):
    """35 pairs of 8 x 40 at D 16 cross the 32-frame pointer table of the uint8 prefilter."""
    from stereotracking_amd.engine import RawChunk
    from stereotracking_amd.sgbm import StereoSGBM
    N, h, w, D = 35, 8, 40, 16
    kw = dict(num_disparities=D, speckle_window_size=4)
    pairs = [K.texture_pair(200 + i, h, w, D) for i in range(N)]
    m = StereoSGBM(**kw)
    H, W = 32, 64
    out = torch.full((N + 1, 3, H, W), -1.0, device=cuda)
    m.compute(RawChunk([_dev(p[0], cuda) for p in pairs], 114.0), RawChunk([_dev(p[1], cuda) for p in pairs], 114.0),
              (h, w), out[:N])
    got = out.cpu().numpy()
    for i, p in enumerate(pairs):
        assert np.array_equal(got[i], R.disp_postp(K.reference(p[0], p[1], kw)['final'], H, W)), f'pair {i} of {N}'
    assert int(m.last_status.item()) == 0
    assert (got[N] == -1.0).all(), 'wrote past the last pair'
    for i, j in ((31, 32), (31, 34), (32, 34)):
        assert got[i].any() and not np.array_equal(got[i], got[j]), f'pairs {i} and {j}'


@pytest.mark.parametrize('order', [(0, 1), (1, 0)], ids=['valid-then-invalid', 'invalid-then-valid'])
def test_second_compute_on_a_dirty_workspace(cuda, order):
    from stereotracking_amd.sgbm import StereoSGBM
    h, w = K.TIES_HW
    H, W = up(h), up(w)
    m = StereoSGBM()
    for k in order:
        left, right = K.TIES[K.DIRTY[k]]
        out = torch.full((1, 3, H, W), -1.0, device=cuda)
        m.compute(batch([left], H, W, cuda), batch([right], H, W, cuda), (h, w), out)
        assert len(m._ws) == 1, 'both scenarios share one workspace'
        assert np.array_equal(out[0].cpu().numpy(), R.disp_postp(K.reference(left, right, {})['final'], H, W)), K.DIRTY[k]
        assert int(m.last_status.item()) == 0


# ---- median and speckle kernels on their own maps --------------------------------------------------------------------------
@pytest.mark.parametrize('hw', K.MEDIAN_HW, ids=lambda hw: '%dx%d' % hw)
def test_median_edge_maps(cuda, hw):
    from stereotracking_amd.sgbm import StereoSGBM
    maps = K.median_maps(hw)
    got = StereoSGBM.median(_dev(maps, cuda)).cpu().numpy()
    for n, m in enumerate(maps):
        assert np.array_equal(got[n], R.median3(m)), f'map {n}'


@pytest.mark.parametrize('name', list(K.SPECKLE))
def test_speckle_adversarial_maps(cuda, name):
    """Long parent chains (serpentines), one component per pixel, one component in all, a batch whose maps must not join,
    no valid pixel; at every window and range.  Then the fused pack into a larger disp_postp: 0 in the padding."""
    from stereotracking_amd import _lib
    from stereotracking_amd._lib import check, current_stream, ptr
    from stereotracking_amd.sgbm import StereoSGBM
    maps = K.SPECKLE[name]
    N, h, w = maps.shape
    dev = _dev(maps, cuda)
    for rg in K.SPECKLE_RANGES:
        for window in K.SPECKLE_WINDOWS:
            want = K.speckle_reference(maps, window, rg)
            out, status = StereoSGBM(speckle_window_size=window, speckle_range=rg).speckle(dev)
            assert np.array_equal(out.cpu().numpy(), want), f'window {window}, range {rg}'
            assert int(status.item()) == 0, f'window {window}, range {rg}: status'
            # the fused pack, with and without the int16 output
            H, W = h + 3, w + 17
            for with_final in (True, False):
                ws = torch.empty(2 * ((N * h * w * 4 + 255) // 256 * 256), dtype=torch.uint8, device=cuda)
                fin = torch.full_like(dev, 7)
                postp = torch.full((N, 3, H, W), -1.0, device=cuda)
                status = torch.full((1,), 9, dtype=torch.int32, device=cuda)
                check(_lib.load().st_sgbm_speckle(ptr(dev), N, h, w, window, 16 * rg, ptr(ws), ws.numel(),
                                                  ptr(fin) if with_final else None, ptr(postp), H, W, ptr(status),
                                                  current_stream()), 'st_sgbm_speckle')
                got = postp.cpu().numpy()
                for n in range(N):
                    assert np.array_equal(got[n], R.disp_postp(want[n], H, W)), f'window {window}, range {rg}: pack'
                assert not got[:, :, h:].any() and not got[:, :, :, w:].any()
                assert np.array_equal(fin.cpu().numpy(), want if with_final else np.full_like(maps, 7))
                assert int(status.item()) == 0
