"""TEST INFRASTRUCTURE: the stage-by-stage comparison of StereoSGBM (csrc/sgbm.hip) with the numpy restatement
(tests/sgbm_ref.py) that tests/test_sgbm_gpu.py and tests/test_sgbm_edges_gpu.py share."""
import numpy as np
import torch

import sgbm_ref as R


def up(v, d=32):
    return (v + d - 1) // d * d


def batch(frames, H, W, cuda, pad=114.0):
    """uint8 (3, h, w) frames -> fp32 (N, 3, H, W) on the device.  pad: a value, or a (N, 3, H, W) array whose top-left
    (h, w) the frames replace."""
    if np.ndim(pad) == 0:
        out = np.full((len(frames), 3, H, W), pad, np.float32)
    else:
        out = np.array(pad, np.float32).reshape(len(frames), 3, H, W)
    for i, f in enumerate(frames):
        out[i, :, :f.shape[1], :f.shape[2]] = f
    return torch.from_numpy(out).to(cuda)


def assert_stages_bit_exact(cuda, L, Rt, kw, refs=None, pad=114.0):
    """Every stage of N pairs (uint8 (3, h, w) lists L, Rt) under the module arguments kw equals the restatement bit for
    bit: the block-summed cost, the map before the median, the median of the GPU map, median and speckle filter on the
    restatement's own inputs, compute() into a poisoned (N, 3, H, W) output, and status 0.  -> (refs, device results)."""
    from stereotracking_amd.sgbm import StereoSGBM
    m = StereoSGBM(**kw)
    N, (h, w) = len(L), L[0].shape[1:]
    H, W = up(h), up(w)
    lb, rb = batch(L, H, W, cuda, pad), batch(Rt, H, W, cuda, pad)
    if refs is None:
        refs = [R.sgbm(a, b, stages=True, **kw) for a, b in zip(L, Rt)]
    cost, raw = m.match(lb, rb, (h, w))
    med_gpu = m.median(raw)
    med_ref_in = m.median(torch.from_numpy(np.stack([r['raw'] for r in refs])).to(cuda))
    fin, status = m.speckle(torch.from_numpy(np.stack([r['median'] for r in refs])).to(cuda))
    out = torch.full((N, 3, H, W), -1.0, device=cuda)
    m.compute(lb, rb, (h, w), out)
    torch.cuda.synchronize()
    for i, r in enumerate(refs):
        assert np.array_equal(cost[i].cpu().numpy(), r['cost']), f'pair {i}: cost'
        assert np.array_equal(raw[i].cpu().numpy(), r['raw']), f'pair {i}: map before the median'
        assert np.array_equal(med_gpu[i].cpu().numpy(), r['median']), f'pair {i}: median of the GPU map'
        assert np.array_equal(med_ref_in[i].cpu().numpy(), r['median']), f'pair {i}: median'
        assert np.array_equal(fin[i].cpu().numpy(), r['final']), f'pair {i}: speckle filter'
        assert np.array_equal(out[i].cpu().numpy(), R.disp_postp(r['final'], H, W)), f'pair {i}: disp_postp'
    assert int(status.item()) == 0 and int(m.last_status.item()) == 0, 'speckle union-find did not converge'
    return refs, dict(cost=cost, raw=raw, out=out)
