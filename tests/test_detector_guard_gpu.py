"""The detector plan and decode / NMS over a stale workspace, a NaN head buffer and inputs inside guard bands.

st_detector_workspace_bytes / st_decode_nms_workspace_bytes hand out sizes and nothing says the memory must be cleared
(HipDetector allocates both with torch.empty, INTEGRATION.md tells integrators to do the same).  Here the workspace is
filled with 0xFF (NaN as fp32, -1 as an index) and with 0x7F (3.39e38) before the forward, head_out with NaN, the inputs
stand in arenas of 0xFF bytes (guard_memory.arena) - and every tap, the head and the launch report must be what they
are over a zeroed workspace, bit for bit, under the three forced plans of plan_utils.forced_tuning (H, S, T: every
fused, chained and grouped launch path).  In a stereo context planes 1 and 2 of the disparity are NaN as well: the
context reads plane 0 with plane-summed weights (HipDetector disp_replicated).

Regions left out of the comparison: floats 6 and 7 of a head row.  include/stereotrack.h documents them as unused
padding (st_head_row_floats), the head kernels do not write them; st_decode_nms, the only reader of head rows, is run
on the poisoned head here and must give the bytes it gives on the clean one.

The residue test leaves the workspace alone between forwards: A, B, A on one context, each over what the forward
before it left behind.
"""
import pytest
import torch

import guard_memory as gm
from plan_utils import TAPS, forced_tuning
from stereotracking_amd.engine import HipDetector, RawChunk
from stereotracking_amd.synthetic import synthetic_batch, synthetic_state_dict

pytestmark = pytest.mark.gpu

# from test_detector_plan_gpu.CONFIGS: N, H, W, widen, deepen, kwargs
CONFIGS = {
    'w050_d033_1x96x160': (1, 96, 160, 0.5, 0.33, {}),
    'w0375_d033_3x224x352': (3, 224, 352, 0.375, 0.33, {}),          # feat 96: Cin tails
    'w050_d033_2x96x160_stereo': (2, 96, 160, 0.5, 0.33, dict(stereo=True)),
}
PATTERNS = (0xFF, 0x7F)          # the detector workspace holds floats only
MAX_DET = 1000                   # the 224 x 352 scenario keeps 523 boxes of one image at score_thr 0.05


def _detector(cid):
    N, H, W, widen, deepen, kw = CONFIGS[cid]
    det = HipDetector(N, H, W, widen, deepen, 1, **kw)
    # a confident head, so that decode / NMS has boxes to work on
    det.load_state_dict(synthetic_state_dict(det.param_table(), seed=0, prior_prob=0.2, logit_std=2.5))
    return det


def _inputs(cid, first=0):
    N, H, W, _, _, kw = CONFIGS[cid]
    batch = synthetic_batch(range(first, first + N), H - 16, W, 64)          # 16 padded rows
    right = synthetic_batch(range(first + 100, first + 100 + N), H - 16, W, 64)['img'] if kw.get('stereo') else None
    return batch['img'], batch['disp_postp'], right


def _frames(seed, N, h, w):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g) for _ in range(N)]


KEEP = 'keep'      # _run(fill=KEEP): the workspace as the previous forward left it


def _run(det, dev, img, disp, right, fill, raw=None):
    """One forward.  fill = None: zeroed workspace, zeroed head, plain inputs (the baseline).  fill = a byte: workspace
    filled with it, head_out NaN, every input in an arena, NaN in the disparity planes a stereo context never reads.
    fill = KEEP: the same hostile head and inputs, the workspace NOT touched - what the forward before left in it.
    raw = (left frames, right frames or None): the uint8 path.  -> ({name: CPU tensor}, launch report, arena tensors)"""
    hostile = fill is not None
    put = (lambda t: gm.arena(t.contiguous(), device=dev)) if hostile else (lambda t: t.contiguous().to(dev))
    ws = det._workspace(dev)
    if fill != KEEP:
        ws.fill_(fill if hostile else 0)
    head = torch.full((det.head_floats,), float('nan') if hostile else 0.0, dtype=torch.float32, device=dev)
    if hostile and det.stereo:
        disp = disp.clone()
        disp[:, 1:] = float('nan')
    d = put(disp)
    held = [d]
    if raw is not None:
        left = RawChunk([put(f) for f in raw[0]], 114.0)
        held += left.frames
        if det.stereo:
            rgt = RawChunk([put(f) for f in raw[1]], 114.0)
            held += rgt.frames
            det.forward_phase0_raw(left, rgt)
            det.forward_phase(1, disp=d, head_out=head)
        else:
            det.forward(left, d, head_out=head)
    elif det.stereo:
        i, r = put(img), put(right)
        held += [i, r]
        det.forward_phase(0, img=i, right=r)
        det.forward_phase(1, disp=d, head_out=head)
    else:
        i = put(img)
        held.append(i)
        det.forward(i, d, head_out=head)
    torch.cuda.synchronize()
    out = {n: det.tap(n).cpu().contiguous() for n in TAPS}
    for l, rows in enumerate(det.head_levels(head)):
        out[f'head{l}'] = rows[..., :6].cpu().contiguous()
    return out, det.launch_report(), head, held


def _assert_same(got, base, what):
    for n in base:
        gm.assert_unaffected(got[n], base[n], f'{what}: {n}')


def _decode(det, head, fill):
    """decode_nms with its workspace and the five output tensors filled with `fill` (0 / 0xFF: they hold indices)."""
    det.decode_nms(head, score_thr=0.05, max_det=MAX_DET)      # sizes the decode workspace
    det._dec_ws.fill_(fill)
    out = det.decode_buffers(MAX_DET, head.device)
    for t in out:
        t.view(torch.uint8).fill_(fill)
    res = det.decode_nms(head, score_thr=0.05, max_det=MAX_DET, out=out)
    torch.cuda.synchronize()
    return [t.cpu() for t in res]


@pytest.mark.parametrize('policy', ['H', 'S', 'T'])
@pytest.mark.parametrize('cid', list(CONFIGS))
def test_forward_is_blind_to_workspace_contents_and_guard_bands(cid, policy, cuda):
    det = _detector(cid)
    det.set_tuning(forced_tuning(det, policy))
    N, H, W = CONFIGS[cid][:3]
    img, disp, right = _inputs(cid)
    raw = (_frames(1, N, H - 16, W), _frames(2, N, H - 16, W) if det.stereo else None)
    for what, frames in (('forward', None), ('forward_raw', raw)):
        base, report, clean_head, _ = _run(det, cuda, img, disp, right, None, raw=frames)
        assert all(torch.isfinite(t).all() for t in base.values())
        assert float(base['head0'].abs().max()) > 0 and float(base['p5'].abs().max()) > 0
        clean_det = _decode(det, clean_head, 0x00)
        assert int(clean_det[4].sum()) > 0 and int(clean_det[4].max()) <= MAX_DET, 'the scenario keeps no boxes / overflows'
        for fill in PATTERNS:
            got, rep, head, held = _run(det, cuda, img, disp, right, fill, raw=frames)
            _assert_same(got, base, f'{cid} {policy} {what} over 0x{fill:02X}')
            assert rep == report, f'{what} over 0x{fill:02X}: the launch report moved'
            assert gm.bands_intact(*held), f'{what}: a guard band of an input was written'
            # the head as it stands - NaN in the padding floats of every row - through decode / NMS over a poisoned
            # decode workspace and poisoned outputs: the bytes of the clean decode
            for k, (g, b) in enumerate(zip(_decode(det, head, 0xFF), clean_det)):
                assert gm.same_bits(g, b), f'{what} over 0x{fill:02X}: decode output {k} differs'
        assert all(gm.same_bits(g, b) for g, b in zip(_decode(det, clean_head, 0xFF), clean_det))


@pytest.mark.parametrize('policy', ['H', 'S', 'T'])
@pytest.mark.parametrize('cid', ['w050_d033_1x96x160', 'w050_d033_2x96x160_stereo'])
def test_no_residue_of_the_previous_batch(cid, policy, cuda):
    """forward(A), forward(B), forward(A) on one context, the workspace left as each forward leaves it (only the first
    forward starts from a filled one): the third equals the first, and B equals a fresh context's B over a zeroed
    workspace.  Under S the chained and grouped launches keep their riders' intermediate tensors in the workspace; H and
    T run the other instances over the same residue."""
    a, b = _inputs(cid, 0), _inputs(cid, 7)
    det = _detector(cid)
    det.set_tuning(forced_tuning(det, policy))
    first, rep_a, _, _ = _run(det, cuda, *a, 0xFF)             # over poison: what it leaves is its own
    ws_after_a = det._workspace(cuda).clone()
    second, _, _, _ = _run(det, cuda, *b, KEEP)                 # over A's residue
    assert not torch.equal(det._workspace(cuda), ws_after_a), 'B left the workspace as A left it: no residue to test'
    third, rep_c, _, _ = _run(det, cuda, *a, KEEP)              # over B's residue
    fresh = _detector(cid)
    fresh.set_tuning(forced_tuning(fresh, policy))
    fresh_b, _, _, _ = _run(fresh, cuda, *b, None)
    fresh_a, _, _, _ = _run(fresh, cuda, *a, KEEP)              # and A over the fresh context's B
    _assert_same(third, first, 'A after B')
    _assert_same(second, fresh_b, 'B after A')
    _assert_same(fresh_a, first, 'A on the fresh context')
    assert rep_a == rep_c
    assert any(not torch.equal(first[n], second[n]) for n in first), 'A and B are the same batch'
