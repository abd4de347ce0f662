"""GPU: the disparity-completion model - the out_fd detector plan, DispHeadV2 on the device against the torch helper
(tests/disp_head_ref.py) in fp64, determinism, the rescale, the memory contract of the new entry points, and the
OCSORT_Disp_Completion_V2 shell.

Error rule for everything that is not a pure copy: max |gpu - fp64| <= 4 x max |fp32 CPU helper - fp64| per tap - the
factor tests/test_detector_plan_gpu.py uses for Winograd layers.  $ST_DISP_HEAD_PARITY_OUT=<file>: the measured ratios
are also written there as JSON (how profiles/disp_head_parity.json is produced)."""
import json
import os

import pytest
import torch

import disp_head_ref as ref
import guard_memory as gm
from stereotracking_amd.engine import HipDetector, HipDispHead
from stereotracking_amd.synthetic import synthetic_batch, synthetic_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_V2 = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone_disp_completion_v2.py')
CFG_DISP = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone_disp.py')
FACTOR = 4.0
RATIOS = {}


def _record(key, ratios):
    RATIOS[key] = ratios
    path = os.environ.get('ST_DISP_HEAD_PARITY_OUT')
    if path:
        with open(path, 'w') as f:
            json.dump(dict(rule='max|gpu - fp64| / max|fp32 CPU helper - fp64| per tap, bound %g' % FACTOR, cases=RATIOS), f,
                      indent=1, sort_keys=True)


def _ratio(got, r64, r32):
    """(ratio, gpu error, fp32 CPU error), all max abs against fp64."""
    e_gpu = float((got.double() - r64).abs().max())
    e_cpu = float((r32.double() - r64).abs().max())
    return (e_gpu / e_cpu if e_cpu > 0 else (0.0 if e_gpu == 0 else float('inf'))), e_gpu, e_cpu


# ---- 1. the out_fd plan ---------------------------------------------------------------------------------------------
def _run_plan(det, batch, cuda, stereo):
    if stereo:
        det.forward_phase(0, img=batch['img'].to(cuda), right=batch['right'].to(cuda))
        return det.forward_phase(1, disp=batch['disp_postp'].to(cuda))
    return det.forward(batch['img'].to(cuda), batch['disp_postp'].to(cuda))


@pytest.mark.parametrize('stereo', [False, True])
def test_out_fd_plan_is_bit_identical_and_keeps_the_disparity_features(cuda, stereo):
    N, H, W = 2, 64, 96
    batch = synthetic_batch([3, 4], H, W, 32)
    plain = HipDetector(N, H, W, 0.5, 0.33, 1, stereo=stereo)
    fd = HipDetector(N, H, W, 0.5, 0.33, 1, stereo=stereo, out_fd=True)
    sd = synthetic_state_dict(plain.param_table(), seed=21)
    plain.load_state_dict(sd)
    fd.load_state_dict(sd)
    h0 = _run_plan(plain, batch, cuda, stereo)
    h1 = _run_plan(fd, batch, cuda, stereo)
    torch.cuda.synchronize()
    for l0, l1 in zip(plain.head_levels(h0), fd.head_levels(h1)):       # the rows' written floats: cls, box, obj
        assert bool(torch.isfinite(l0[..., :6]).all()) and float(l0[..., :6].abs().max()) > 0
        assert gm.same_bits(l0[..., :6], l1[..., :6]), 'head output differs between the out_fd = 0 / 1 plans'
    fused, disp, rgb = fd.tap('stage1_fused'), fd.tap('stage1_disp'), fd.tap('stage1_rgb')
    assert tuple(disp.shape) == (N, H // 4, W // 4, 64) and rgb.shape[0] == (2 * N if stereo else N)
    assert gm.same_bits(fused, plain.tap('stage1_fused'))
    assert gm.same_bits(fused, (disp + rgb[:N]) * 0.5)
    assert float((disp - rgb[:N]).abs().max()) > 0.05        # two different branches, not one tensor twice
    # the fused tail still covers the disparity branch: conv2 + final_conv of disp_stage1 ran as one launch (56)
    descs = fd.op_descs()
    i = next(k for k, d in enumerate(descs) if 'disp_stage1.1.final_conv' in d)
    rep = fd.launch_report()
    assert rep[i] == (56, i - 1) and rep[i - 1] == (56, i - 1)
    assert descs[i + 1].startswith('avg2') and rep[i + 1][1] == i + 1


# ---- 2. the head alone --------------------------------------------------------------------------------------------
P3_PAD, P3_OFF, DF_PAD, DF_OFF = 12, 8, 8, 4


def _wide(x_nchw, pad, off, cuda, hostile=False, arena=False):
    """NCHW values as channels [off, off + C) of a wider NHWC device buffer; the other channels hold finite garbage, or
    NaN / +Inf / -Inf in turn (hostile); arena: inside guard bands.  -> (buffer, view of the slice)."""
    x = x_nchw.permute(0, 2, 3, 1).contiguous()
    c = x.shape[-1]
    g = torch.Generator().manual_seed(c + off)
    host = torch.randn(x.shape[:3] + (c + pad,), generator=g) * 3
    host[..., off:off + c] = x
    if hostile:
        gm.slack(host, off, c)
    buf = gm.arena(host, device=cuda) if arena else host.to(cuda)
    return buf, buf[..., off:off + c]


def _head_for(case, cuda, batch=None):
    N, C, h, w, cin, _ = case
    c = ref.make_case(*case)
    head = HipDispHead(batch or N, h, w, cin, C)
    head.load_state_dict(c['sd'])
    return head, c


def _nhwc(t):
    return t.permute(0, 2, 3, 1) if t.dim() == 4 else t[:, None, None, :]


@pytest.mark.parametrize('case', ref.CASES, ids=lambda c: 'N%d_C%d_%dx%d' % c[:4])
def test_head_taps_against_fp64(cuda, case):
    N, C, h, w, cin, _ = case
    head, c = _head_for(case, cuda)
    _, p3 = _wide(c['p3'], P3_PAD, P3_OFF, cuda)
    _, df = _wide(c['df'], DF_PAD, DF_OFF, cuda)
    assert p3.stride(2) == cin + P3_PAD and p3.storage_offset() == P3_OFF
    pred = head.forward_views(p3, df)
    torch.cuda.synchronize()
    taps = {n: head.tap(n).cpu() for n in ref.TAPS}
    assert tuple(pred.shape) == (N, 1, 4 * h, 4 * w) and gm.same_bits(pred.cpu().reshape(-1), taps['pred'].reshape(-1))
    # pure copies: the four replicas of the x2 upsampling hold the same bits (the ELU-ed low-resolution tensor they copy
    # is never written, so they are compared with each other, and with ELU of the raw tap by the error rule below), and
    # the concat is [upsampled | gated df]
    cat = taps['cat']
    assert tuple(cat.shape) == (N, 2 * h, 2 * w, C + 64)
    up = cat[..., :C]
    for dy, dx in ((0, 1), (1, 0), (1, 1)):
        assert gm.same_bits(up[:, dy::2, dx::2], up[:, 0::2, 0::2])
    gate = taps['gate_scale'].reshape(N, 1, 1, 64)
    assert gm.same_bits(cat[..., C:], c['df'].permute(0, 2, 3, 1) * (1 - gate))    # fp32, same operation order
    ratios = {}
    for name in ref.TAPS:
        r, e_gpu, e_cpu = _ratio(taps[name], _nhwc(c['ref64'][name]), _nhwc(c['ref32'][name]))
        ratios[name] = dict(ratio=round(r, 4), gpu_err=e_gpu, cpu_fp32_err=e_cpu)
        print(f'{case[:4]} {name}: gpu {e_gpu:.3e} cpu-fp32 {e_cpu:.3e} ratio {r:.3f}')
    # the ELU-ed low-resolution tensor behind the upsampled slice: ELU of the raw tap, in fp64
    r, e_gpu, e_cpu = _ratio(up[:, 0::2, 0::2], torch.nn.functional.elu(_nhwc(c['ref64']['dconv1_2'])),
                             torch.nn.functional.elu(_nhwc(c['ref32']['dconv1_2'])))
    ratios['elu(dconv1_2)'] = dict(ratio=round(r, 4), gpu_err=e_gpu, cpu_fp32_err=e_cpu)
    _record('head N=%d C=%d p3=%dx%d in=%d' % (N, C, h, w, cin), ratios)
    # both ReLU branches of the prediction are present on the device too
    assert float((taps['pred'] == 0).float().mean()) >= 0.10 and float((taps['pred'] > 0).float().mean()) >= 0.10
    bad = {k: v for k, v in ratios.items() if not v['ratio'] <= FACTOR}
    assert not bad, f'taps over {FACTOR} x the fp32 CPU error: {bad}'


# ---- 3. determinism and batch independence ------------------------------------------------------------------------
def test_two_runs_are_bit_equal_and_an_image_does_not_depend_on_its_batch(cuda):
    case = ref.CASES[1]                      # N = 2
    N, C, h, w, cin, _ = case
    head, c = _head_for(case, cuda)
    _, p3 = _wide(c['p3'], P3_PAD, P3_OFF, cuda)
    _, df = _wide(c['df'], DF_PAD, DF_OFF, cuda)
    runs = []
    for _ in range(2):
        head._ws = None                     # a fresh workspace each time
        pred = head.forward_views(p3, df)
        torch.cuda.synchronize()
        runs.append({n: head.tap(n).cpu().clone() for n in ref.TAPS})
        runs[-1]['out'] = pred.cpu()
    for n in runs[0]:
        assert gm.same_bits(runs[0][n], runs[1][n]), n
    one = HipDispHead(1, h, w, cin, C)
    one.load_state_dict(c['sd'])
    _, p3a = _wide(c['p3'][:1], P3_PAD, P3_OFF, cuda)
    _, dfa = _wide(c['df'][:1], DF_PAD, DF_OFF, cuda)
    pa = one.forward_views(p3a, dfa)
    torch.cuda.synchronize()
    assert gm.same_bits(one.tap('gate_scale').cpu(), runs[0]['gate_scale'][:1]), 'the gate pools across the batch'
    assert gm.same_bits(pa.cpu(), runs[0]['out'][:1])
    # and the two images of the batch got different gates
    assert not torch.equal(runs[0]['gate_scale'][0], runs[0]['gate_scale'][1])


# ---- 4. the rescale ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [(64, 96), (60, 90), (33, 50)])
def test_resize_against_fp64(cuda, size):
    g = torch.Generator().manual_seed(size[0])
    pred = torch.relu(torch.randn(2, 1, 32, 48, generator=g) * 20 + 5)      # zeros and positives, as the head yields
    head = HipDispHead(1, 4, 4, 16, 32)
    got = head.resize(pred.to(cuda), size)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (2, 1) + size
    r, e_gpu, e_cpu = _ratio(got.cpu(), ref.resize(pred.double(), size), ref.resize(pred, size))
    print(f'resize 32x48 -> {size}: gpu {e_gpu:.3e} cpu-fp32 {e_cpu:.3e} ratio {r:.3f}')
    _record('resize 32x48 -> %dx%d' % size, dict(pred=dict(ratio=round(r, 4), gpu_err=e_gpu, cpu_fp32_err=e_cpu)))
    assert r <= FACTOR


# ---- 5. the memory contract ---------------------------------------------------------------------------------------
def _nan_arena(nbytes, cuda):
    return gm.arena(torch.full((nbytes // 4,), float('nan')), device=cuda)


def test_head_entry_points_on_hostile_memory(cuda):
    """st_disp_head_forward / st_disp_head_resize with NaN / +Inf / -Inf in the channels outside the slices, inputs,
    workspace and outputs inside 0xFF guard bands, workspace and outputs pre-filled with NaN; then with every
    torch.empty (workspace, outputs) returning 0xFF bytes: bit-equal to the friendly run, bands intact, inputs unchanged."""
    case = ref.CASES[2]
    N, C, h, w, cin, _ = case
    head, c = _head_for(case, cuda)
    _, p3 = _wide(c['p3'], P3_PAD, P3_OFF, cuda)
    _, df = _wide(c['df'], DF_PAD, DF_OFF, cuda)
    base = head.forward_views(p3, df, workspace=torch.zeros(head.workspace_bytes(), dtype=torch.uint8, device=cuda))
    torch.cuda.synchronize()
    base_taps = {n: head.tap(n).cpu().clone() for n in ref.TAPS}
    base_rs = head.resize(base, (37, 51)).cpu()

    p3buf, p3h = _wide(c['p3'], P3_PAD, P3_OFF, cuda, hostile=True, arena=True)
    dfbuf, dfh = _wide(c['df'], DF_PAD, DF_OFF, cuda, hostile=True, arena=True)
    before = gm.bits(p3buf), gm.bits(dfbuf)
    ws = _nan_arena(head.workspace_bytes(), cuda)
    out = gm.arena(torch.full((N, 1, 4 * h, 4 * w), float('nan')), device=cuda)
    head.forward_views(p3h, dfh, out=out, workspace=ws.view(torch.uint8))
    rs = gm.arena(torch.full((N, 1, 37, 51), float('nan')), device=cuda)
    head.resize(out, (37, 51), out=rs)
    torch.cuda.synchronize()
    gm.assert_unaffected(out, base.cpu(), 'pred over hostile memory')
    for n in ref.TAPS:
        gm.assert_unaffected(head.tap(n), base_taps[n], f'tap {n} over hostile memory')
    gm.assert_unaffected(rs, base_rs, 'resize over hostile memory')
    assert gm.bands_intact(p3buf, dfbuf, ws, out, rs)
    assert torch.equal(gm.bits(p3buf), before[0]) and torch.equal(gm.bits(dfbuf), before[1])

    with gm.poisoned_empty(0xFF) as pe:
        head._ws = None
        got = head.forward_views(p3, df)          # workspace and output from torch.empty
        got_rs = head.resize(got, (37, 51))
        torch.cuda.synchronize()
    assert pe.device_count >= 3
    gm.assert_unaffected(got, base.cpu(), 'pred over stale memory')
    gm.assert_unaffected(got_rs, base_rs, 'resize over stale memory')
    for n in ref.TAPS:
        gm.assert_unaffected(head.tap(n), base_taps[n], f'tap {n} over stale memory')


def test_out_fd_plan_on_stale_memory(cuda):
    """The plan's new op (the branch average) and the tap it feeds, with the detector workspace and the head buffer
    handed out as 0xFF bytes."""
    N, H, W = 2, 64, 96
    batch = synthetic_batch([3, 4], H, W, 32)
    sd = None
    res = []
    for poisoned in (False, True):
        det = HipDetector(N, H, W, 0.5, 0.33, 1, out_fd=True)
        sd = sd or synthetic_state_dict(det.param_table(), seed=21)
        det.load_state_dict(sd)
        if poisoned:
            with gm.poisoned_empty(0xFF) as pe:
                head = det.forward(batch['img'].to(cuda), batch['disp_postp'].to(cuda))
            assert pe.device_count >= 2
        else:
            det._ws = torch.zeros(det.lib.st_detector_workspace_bytes(det.handle), dtype=torch.uint8, device=cuda)
            head = det.forward(batch['img'].to(cuda), batch['disp_postp'].to(cuda),
                               torch.zeros(det.head_floats, device=cuda))
        torch.cuda.synchronize()
        res.append(dict(fused=det.tap('stage1_fused').cpu().clone(), disp=det.tap('stage1_disp').cpu().clone(),
                        head=torch.cat([l[..., :6].cpu().reshape(-1) for l in det.head_levels(head)])))
    for k in res[0]:
        gm.assert_unaffected(res[1][k], res[0][k], f'{k} over stale memory')


# ---- 6. the shell ---------------------------------------------------------------------------------------------------
def _build(cfg_path, head_sd=None):
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    cfg = Config.fromfile(cfg_path)
    cfg.model.tracker['init_track_thr'] = 0.03      # random weights score low: let tracks start
    cfg.model.tracker['obj_score_thr'] = 0.02
    if head_sd is not None:
        cfg.model.detector.disparity_head['channels'] = 32
    # the heuristic launch plan: the same kernels in both models and for every batch size (a measured plan may differ
    # between two models by timing noise, and with it the fp32 summation order)
    model = MODELS.build(dict(cfg.model, autotune=False, dense_batch=2))
    sd = synthetic_state_dict(list(model.detector._table), seed=5, prior_prob=0.2, logit_std=2.5)
    if head_sd is not None:
        sd.update({'disp_head.' + k: v for k, v in head_sd.items()})
    missing = model.detector.load_state_dict(sd, strict=False)
    assert not [k for k in missing.missing_keys if not k.endswith('num_batches_tracked')]
    return model


def test_completion_shell_over_a_ragged_call(cuda):
    from stereotracking_amd.structures import TrackDataSample
    ori = (64, 96)
    head_sd = ref.random_state_dict(128, 32, seed=31)
    head_sd['reg.conv.bias'] = torch.tensor([0.4])
    fr = synthetic_batch([70, 71, 72], ori[0], ori[1], 32)

    def data():
        samples = [TrackDataSample(dict(frame_id=t, ori_shape=ori, img_shape=ori, scale_factor=(1.0, 1.0))) for t in range(3)]
        return dict(inputs=dict(img=[fr['img'][t:t + 1].to(torch.uint8) for t in range(3)],
                                disp_postp=[fr['disp_postp'][t:t + 1] for t in range(3)],
                                disp_mask=[fr['disp_mask'][t:t + 1].to(torch.uint8) for t in range(3)]),
                    data_samples=samples)

    model = _build(CFG_V2, head_sd)
    outs = model.test_step(data())              # 3 frames at dense_batch 2: chunks of 2 + 1
    torch.cuda.synchronize()
    plain = _build(CFG_DISP)
    want = plain.test_step(data())
    torch.cuda.synchronize()
    assert len(outs) == len(want) == 3
    n_tracks = 0
    for a, b in zip(outs, want):
        ta, tb = a.pred_track_instances, b.pred_track_instances
        assert ta.instances_id.tolist() == tb.instances_id.tolist()
        for k in ('bboxes', 'scores', 'labels', 'depth', 'gt_depth', 'scales'):
            assert gm.same_bits(ta[k], tb[k]), k
        assert gm.same_bits(a.pred_det_instances.bboxes, b.pred_det_instances.bboxes)
        assert 'dense_depth_map' not in b
        n_tracks += len(ta)
    assert n_tracks > 0, 'the scenario must exercise the association'
    # every map: (1, 1, h, w), and bit-equal to a batch-1 head run on that frame's taps, where the chunk's detector
    # forward left them (chunk 0 ran on context 0, chunk 1 on context 1: neither workspace has been reused)
    (runner, _), = model._dense.values()
    one = HipDispHead(1, ori[0] // 8, ori[1] // 8, 128, 32)
    one.load_state_dict(head_sd)
    for t, o in enumerate(outs):
        m = o.dense_depth_map
        assert m.is_cuda and m.dtype == torch.float32 and tuple(m.shape) == (1, 1) + ori
        det = runner.pipes[t // 2].det
        i = t % 2
        alone = one.resize(one.forward_views(det.tap('p3')[i:i + 1], det.tap('stage1_disp')[i:i + 1]), ori)
        torch.cuda.synchronize()
        assert gm.same_bits(m, alone), f'frame {t}'
        assert float((m > 0).float().mean()) > 0.05 and bool(torch.isfinite(m).all())
    assert not torch.equal(outs[0].dense_depth_map, outs[1].dense_depth_map)
    # the detector's own predict returns the pair the reference's does
    samples = [TrackDataSample(dict(frame_id=0, ori_shape=ori, img_shape=ori, scale_factor=(1.0, 1.0)))]
    res, disp = model.detector.predict(dict(img=fr['img'][:1].to(cuda), disp_postp=fr['disp_postp'][:1].to(cuda)), samples)
    torch.cuda.synchronize()
    assert len(res) == len(disp) == 1 and tuple(disp[0].shape) == (1, 1) + ori
    # (a batch-1 detector plan of its own: its tile choices, and with them the fp32 summation order, may differ from the
    # batch-2 context's, so closeness here - the bit-level statement is the one above)
    assert torch.allclose(disp[0], outs[0].dense_depth_map, rtol=1e-3, atol=1e-3)
