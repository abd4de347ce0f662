"""GPU: the left-right check of the stereo module (csrc/lr_check.hip: st_softargmin_right, st_lr_check_pack) against its
numpy restatement (tests/lrcheck_ref.py), BIT FOR BIT at every stage: the two entry points alone, the module in each of
its modes, the unchanged default, and the pipeline behind the config-built MOT shell."""
import os

import numpy as np
import pytest
import torch

import guard_memory as gm
import lrcheck_ref as R
from oracle import c_oracle
from oracle import depth as odepth
from parity_utils import rel_err
from stereotracking_amd import _lib
from stereotracking_amd._lib import check, current_stream, ptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_LR = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'stereo_yolox_s_mot_airdrone_costvolume_lrcheck.py')


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """Bit equality; NaNs must sit at the same places (their payload is the hardware's: 0 * inf differs between hosts)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def softargmin_right(V, T, cuda):
    lib = _lib.load()
    N, H, W, D = V.shape
    v = gm.device_input(np.array(V, np.float32), cuda)
    o = gm.device_output((N, H, W), cuda, float('nan'))
    check(lib.st_softargmin_right(ptr(v), N, H, W, D, T, ptr(o), current_stream()), 'st_softargmin_right')
    torch.cuda.synchronize()
    return o.cpu().numpy()


def lr_check_pack(dL, dR, s, valid_hw, lr_max_diff, cuda, want_mask=True):
    lib = _lib.load()
    N, Hl, Wl = dL.shape
    H, W = Hl * s, Wl * s
    l, r = gm.device_input(np.array(dL, np.float32), cuda), gm.device_input(np.array(dR, np.float32), cuda)
    out = gm.device_output((N, 3, H, W), cuda, float('nan'))
    mask = gm.device_output((N, 1, H, W), cuda, float('nan')) if want_mask else None
    check(lib.st_lr_check_pack(ptr(l), ptr(r), N, Hl, Wl, s, H, W, int(valid_hw[0]), int(valid_hw[1]), float(lr_max_diff),
                               ptr(out), ptr(mask), current_stream()), 'st_lr_check_pack')
    torch.cuda.synchronize()
    return out.cpu().numpy(), (mask.cpu().numpy() if want_mask else None)


# ---- st_softargmin_right: rules 2 + 3 ------------------------------------------------------------------------------------
# the scenes; one pixel; one width below and one above the 128-pixel tile; D = 12 (one partial slab, 16-byte loads),
# D = 7 (no 16-byte loads); a row that needs three tiles with 13 slabs
RIGHT_SHAPES = R.SCENE_SHAPES + [(1, 1, 16), (2, 127, 16), (2, 129, 16), (2, 33, 12), (2, 20, 7), (1, 260, 52)]


@pytest.mark.parametrize('shape', RIGHT_SHAPES)
def test_softargmin_right_bit_equal_to_restatement(shape, cuda):
    """The diagonal gather + the oracle's operation order: scene and white-noise volumes, N = 2, temperatures 32 and 1,
    W < D (every diagonal leaves the image), widths around the tile, partial tiles and slabs."""
    H, W, D = shape
    for V in (R.scene_volume(H, W, D), R.noise_volume(H, W, D)):
        for T in (32.0, 1.0):
            ref = c_oracle.softargmin(R.shear(V), T)
            got = softargmin_right(V, T, cuda)
            assert np.array_equal(bits(got), bits(ref)), (shape, T, np.abs(got - ref).max())


def test_softargmin_right_of_unaggregated_volume_is_the_right_view_matcher(cuda):
    """Without aggregation rule 2 is the cost volume with the right image as the reference: st_softargmin_right on the
    device's own left volume equals the oracle's soft-argmin of the mirrored right-reference volume."""
    lib = _lib.load()
    rng = np.random.RandomState(9)
    N, H, W, Cc, D, T = 2, 3, 150, 16, 48, 8.0
    fl = rng.normal(0, 1, (N, H, W, Cc)).astype(np.float32)
    fr = rng.normal(0, 1, (N, H, W, Cc)).astype(np.float32)
    l, r = torch.from_numpy(fl).to(cuda), torch.from_numpy(fr).to(cuda)
    vol = torch.empty(N, H, W, D, device=cuda)
    o = torch.full((N, H, W), float('nan'), device=cuda)
    check(lib.st_costvolume_softargmin(ptr(l), ptr(r), N, H, W, Cc, Cc, D, T, ptr(vol), None, current_stream()))
    check(lib.st_softargmin_right(ptr(vol), N, H, W, D, T, ptr(o), current_stream()))
    torch.cuda.synchronize()
    mirrored = c_oracle.costvolume(fr[:, :, ::-1], fl[:, :, ::-1], Cc, D)[:, :, ::-1]
    assert np.array_equal(bits(o.cpu().numpy()), bits(c_oracle.softargmin(mirrored, T)))


# ---- st_lr_check_pack: rules 4 + 5 ---------------------------------------------------------------------------------------
def assert_pack_equals_restatement(dL, dR, s, valid_hw, lr_max_diff, cuda):
    lib = _lib.load()
    c = R.check(dL, dR, s, lr_max_diff)
    ref_disp, ref_mask = R.pack(dL, c['valid'], s, valid_hw)
    got, mask = lr_check_pack(dL, dR, s, valid_hw, lr_max_diff, cuda)
    assert same(got, ref_disp)
    assert np.array_equal(bits(mask), bits(ref_mask))
    # null disp_mask: the same disparity
    got2, _ = lr_check_pack(dL, dR, s, valid_hw, lr_max_diff, cuda, want_mask=False)
    assert same(got2, got)
    # a valid pixel keeps the bits st_disp_upsample_pack writes on the same input
    N, Hl, Wl = dL.shape
    l = gm.device_input(np.array(dL, np.float32), cuda)
    up = gm.device_output((N, 3, Hl * s, Wl * s), cuda, float('nan'))
    check(lib.st_disp_upsample_pack(ptr(l), N, Hl, Wl, s, Hl * s, Wl * s, int(valid_hw[0]), int(valid_hw[1]), ptr(up),
                                    current_stream()))
    torch.cuda.synchronize()
    m = np.repeat(mask, 3, axis=1) > 0
    assert same(got[m], up.cpu().numpy()[m]) and not got[~m].any()      # (a NaN counts as any(): invalid is +0)
    return c


@pytest.mark.parametrize('shape', R.SCENE_SHAPES)
@pytest.mark.parametrize('s', [4, 1])
def test_lr_check_pack_bit_equal_to_restatement(shape, s, cuda):
    """Scenes at scale 4 (four pixels per thread) and scale 1, lr_max_diff 1 and 4 pixels, 0 and a value above D * s
    (only the pixels whose match lies outside the right image fall), the valid region cut in both directions."""
    H, W, D = shape
    sc = R.scene(shape, 1.0)
    dL, dR = sc['dL'], sc['dR']
    vhw = (H * s - (1 if H * s > 1 else 0), W * s - (3 if W * s > 3 else 0))
    for lr_max_diff in (1.0, 4.0, 0.0, float(D * s + 1)):
        c = assert_pack_equals_restatement(dL, dR, s, vhw, lr_max_diff, cuda)
        if lr_max_diff > D * s:
            assert np.array_equal(~c['valid'], c['by_xr']) and c['by_xr'].any()
    assert_pack_equals_restatement(dL, dR, s, (H * s, W * s), 1.0, cuda)


@pytest.mark.parametrize('Hl,Wl,s', [(5, 37, 1), (4, 33, 2), (3, 21, 3)])
def test_lr_check_pack_odd_widths_and_non_finite_disparities(Hl, Wl, s, cuda):
    """Output widths that are no multiple of four (one pixel per thread), and maps holding NaN / inf on either side: a
    non-finite dL is invalid, a NaN dR fails the comparison, and the invalid pixel is +0, never NaN (a VALID pixel next to
    a non-finite one interpolates it, exactly as st_disp_upsample_pack does today)."""
    rng = np.random.RandomState(Wl)
    N = 2
    dL = rng.uniform(0, 9, (N, Hl, Wl)).astype(np.float32)
    dR = (dL + rng.uniform(-0.6, 0.6, dL.shape)).astype(np.float32)
    dL[0, 1, 5], dL[1, 2, 7], dL[1, 0, 0] = np.nan, np.inf, -np.inf
    dR[0, 0, 3], dR[1, 1, 2] = np.nan, np.inf
    c = assert_pack_equals_restatement(dL, dR, s, (Hl * s - 1, Wl * s - 2), 1.0, cuda)
    assert c['valid'].any() and c['by_diff'].any() and c['by_xr'].any()


def test_lr_check_pack_is_strict_at_equality(cuda):
    V, dL, dR, v, at = R.equality_scene()
    s = R.SCENE_SCALE
    vhw = (dL.shape[1] * s, dL.shape[2] * s)
    hi = assert_pack_equals_restatement(dL, dR, s, vhw, float(v), cuda)
    lo = assert_pack_equals_restatement(dL, dR, s, vhw, float(np.nextafter(v, np.float32(0))), cuda)
    assert hi['valid'][at].all() and not lo['valid'][at].any()


# ---- through the module ---------------------------------------------------------------------------------------------------
def build_pipe(cuda, seed, **kw):
    from stereotracking_amd.pipeline import StereoDensePipeline
    from stereotracking_amd.synthetic import synthetic_state_dict
    N, H, W = 2, 88, 152                     # padded to 96 x 160 by the pipeline
    pipe = StereoDensePipeline(N, (H, W), 0.375, 0.33, 1, stereo=True, max_det=400, **kw)
    sd = synthetic_state_dict(pipe.param_table(), seed=seed, prior_prob=0.2, logit_std=2.5)
    g = torch.Generator().manual_seed(5)      # generic 3-D taps (the synthetic fan-in rule would make them tiny)
    for l in range(pipe.agg3d_layers):
        w = torch.randn(1, 1, 3, 3, 3, generator=g) * 0.1
        w[0, 0, 1, 1, 1] += 1.0
        sd[f'stereo.agg3d.{l}.weight'] = w
        sd[f'stereo.agg3d.{l}.bias'] = torch.randn(1, generator=g) * 0.02
    pipe.load_state_dict(sd, autotune=False)
    return pipe, sd, (N, H, W)


def module_run(pipe, img, right, hw, cuda, want_mask=True, disp_lr=True):
    sm = pipe.stereo_module
    N, Hp, Wp = pipe.batch, pipe.height, pipe.width
    s = 1 if sm.full_res else sm.feat_stride
    vol = torch.full((N, Hp // s, Wp // s, sm.levels), float('nan'), device=cuda)
    lr = torch.full((N, Hp // 4, Wp // 4), float('nan'), device=cuda) if disp_lr else None
    out = torch.full((N, 3, Hp, Wp), float('nan'), device=cuda)
    mask = torch.full((N, 1, Hp, Wp), float('nan'), device=cuda) if want_mask else None
    kw = dict(disp_mask=mask) if want_mask else {}
    sm.compute(pipe.det, img, right, hw, lr, out, cost_out=vol, **kw)
    torch.cuda.synchronize()
    return vol.cpu().numpy(), (lr.cpu().numpy() if disp_lr else None), out.cpu().numpy(), (mask.cpu().numpy() if want_mask else None)


@pytest.mark.parametrize('mode', ['agg', 'plain', 'fullres', 'fullres_fused_softargmin'])
def test_module_with_lr_check_equals_restatement_on_its_own_volume(mode, cuda):
    """StereoCostVolume(lr_check=True) in the default mode with one 3-D and one 2-D layer, without aggregation (the volume
    is materialised for the check), and in full_res mode with one 3-D layer - once with fuse_softargmin set, which the
    check bypasses: disp_postp and disp_mask equal the restatement applied to the module's own cost_out volume bit for
    bit, a second compute() on the same scratch gives the same bits, and compute() without cost_out / disp_mask the same
    disparity.  Without aggregation rule 1's dL is the fused kernel's own (what the module ships today; equal to the
    oracle's soft-argmin to 1e-3 only), so the restatement takes that and checks it against the oracle's."""
    from stereotracking_amd.synthetic import synthetic_batch
    D = 48 if mode == 'fullres_fused_softargmin' else 32     # 48: a level count the single-kernel form takes
    kw = dict(agg=dict(max_disp=D, agg_layers=1, agg3d_layers=1), plain=dict(max_disp=D),
              fullres=dict(max_disp=D, agg3d_layers=1, full_res=True),
              fullres_fused_softargmin=dict(max_disp=D, agg3d_layers=1, full_res=True))[mode]
    pipe, sd, (N, H, W) = build_pipe(cuda, 3, lr_check=True, lr_max_diff=4.0 if 'fullres' not in mode else 1.0, **kw)
    sm = pipe.stereo_module
    assert sm.lr_check and pipe.lr_check
    if mode == 'fullres_fused_softargmin':
        sm.fuse_softargmin = True
    batch = synthetic_batch([3, 4], H, W, D)
    img, right = batch['img'].to(cuda), batch['right'].to(cuda)
    vol, lr, out, mask = module_run(pipe, img, right, (H, W), cuda)
    s = 1 if sm.full_res else 4
    if sm.full_res:
        lr = sm.full_res_buffers(cuda, N, pipe.height // 4, pipe.width // 4)['disp'].cpu().numpy()
    oracle_dL = c_oracle.softargmin(vol, sm.temperature)
    if mode == 'plain':
        assert rel_err(lr, oracle_dL) <= 1e-3
        ref = R.restate(vol, sm.temperature, s, sm.lr_max_diff, (H, W), dL=lr)
    else:
        assert np.array_equal(bits(lr), bits(oracle_dL))
        ref = R.restate(vol, sm.temperature, s, sm.lr_max_diff, (H, W))
    assert np.array_equal(bits(out), bits(ref['disp_postp']))
    assert np.array_equal(bits(mask), bits(ref['disp_mask']))
    inside = ref['valid'][:, :(H + s - 1) // s, :(W + s - 1) // s]
    assert inside.any() and not inside.all(), 'the pair must show valid and invalid pixels'
    assert (out[:, :, H:] == 0).all() and (out[:, :, :, W:] == 0).all() and np.isfinite(out).all()
    vol2, _, out2, mask2 = module_run(pipe, img, right, (H, W), cuda)
    assert np.array_equal(bits(vol2), bits(vol)) and np.array_equal(bits(out2), bits(out))
    assert np.array_equal(bits(mask2), bits(mask))
    # nobody asks for the volume or the mask: same disparity (the no-aggregation module then writes a volume of its own)
    out3 = torch.full((N, 3, pipe.height, pipe.width), float('nan'), device=cuda)
    sm.compute(pipe.det, img, right, (H, W), None, out3)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out3.cpu().numpy()), bits(out))
    # and through run(): disp_postp is 0 exactly where disp_mask is 0
    res = pipe.run(img, right)
    torch.cuda.synchronize()
    assert np.array_equal(bits(res['disp_postp'].cpu().numpy()), bits(out))
    assert np.array_equal(bits(res['disp_mask'].cpu().numpy()), bits(mask))


@pytest.mark.parametrize('kw', [dict(agg_layers=1, agg3d_layers=1), dict(), dict(agg3d_layers=1, full_res=True)])
def test_lr_check_off_changes_nothing(kw, cuda):
    """lr_check=False and a module built without the argument give, value for value, the bits of the existing call
    sequence on the same input; run() returns no disp_mask; asking for one is an error."""
    from stereotracking_amd.synthetic import synthetic_batch
    D = 32
    base, sd, (N, H, W) = build_pipe(cuda, 3, max_disp=D, **kw)
    off, _, _ = build_pipe(cuda, 3, max_disp=D, lr_check=False, lr_max_diff=0.5, **kw)
    on, _, _ = build_pipe(cuda, 3, max_disp=D, lr_check=True, lr_max_diff=4.0, **kw)
    batch = synthetic_batch([3, 4], H, W, D)
    img, right = batch['img'].to(cuda), batch['right'].to(cuda)
    assert base.stereo_module.lr_check is False and off.stereo_module.lr_check is False
    vol_b, lr_b, out_b, _ = module_run(base, img, right, (H, W), cuda, want_mask=False)
    vol_o, lr_o, out_o, _ = module_run(off, img, right, (H, W), cuda, want_mask=False)
    assert np.array_equal(bits(vol_b), bits(vol_o)) and np.array_equal(bits(out_b), bits(out_o))
    assert np.array_equal(bits(lr_b), bits(lr_o)) or base.full_res
    # the existing call sequence on the module's own volume / left disparity
    sm = base.stereo_module
    s = 1 if sm.full_res else 4
    lib = _lib.load()
    if sm.full_res:
        dl = sm.full_res_buffers(cuda, N, base.height // 4, base.width // 4)['disp']
    else:
        dl = torch.from_numpy(lr_b).to(cuda)
    up = torch.full((N, 3, base.height, base.width), float('nan'), device=cuda)
    check(lib.st_disp_upsample_pack(ptr(dl), N, base.height // s, base.width // s, s, base.height, base.width, H, W, ptr(up),
                                    current_stream()))
    torch.cuda.synchronize()
    assert np.array_equal(bits(up.cpu().numpy()), bits(out_b))
    # the check only ever zeroes: where the mask is 1 the disparity is today's
    _, _, out_on, mask_on = module_run(on, img, right, (H, W), cuda)
    m = np.repeat(mask_on, 3, axis=1) > 0
    assert np.array_equal(bits(out_on[m]), bits(out_b[m])) and not out_on[~m].any() and m.any() and not m.all()
    res = base.run(img, right)
    assert 'disp_mask' not in res and np.array_equal(bits(res['disp_postp'].cpu().numpy()), bits(out_b))
    with pytest.raises(ValueError, match='lr_check'):
        sm.compute(base.det, img, right, (H, W), None, None, disp_mask=torch.empty(N, 1, base.height, base.width, device=cuda))


# ---- through the config-built MOT shell ---------------------------------------------------------------------------------
def test_lrcheck_config_through_the_shell_masks_the_per_box_depth(cuda):
    """configs/.../stereo_yolox_s_mot_airdrone_costvolume_lrcheck.py -> MODELS.build -> the shell's own dense pipeline on
    synthetic pairs: disp_postp is 0 exactly where disp_mask is 0, the per-box depth and scales equal oracle/depth.py on
    that MASKED map (tolerances of tests/test_stereo_depth_gpu.py), at least one box's depth differs from what the
    unmasked map gives (asserted on the oracle), and test_step runs on the same frames."""
    import math
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.pipeline import StereoDensePipeline
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.structures import TrackDataSample
    from stereotracking_amd.synthetic import synthetic_batch, synthetic_state_dict
    cfg = Config.fromfile(CFG_LR)
    for part in ('backbone', 'neck'):
        cfg.model.detector[part]['widen_factor'] = 0.375
    cfg.model.detector.bbox_head.head_module['widen_factor'] = 0.375
    cfg.model.stereo['max_disp'] = 32
    cfg.model.tracker['init_track_thr'], cfg.model.tracker['obj_score_thr'] = 0.03, 0.02
    model = MODELS.build(dict(cfg.model, autotune=False, dense_batch=2, inflight=2))
    assert model.stereo.lr_check and model.stereo.lr_max_diff == 4.0 and model.stereo.agg_layers == 2
    table = list(model.detector._table) + [('stereo.' + n, shp) for n, shp in model.stereo.param_table()]
    sd = synthetic_state_dict(table, seed=8, prior_prob=0.2, logit_std=2.5)
    model.detector.load_state_dict(sd, strict=False)
    model.stereo.load_state_dict({k[len('stereo.'):]: v for k, v in sd.items() if k.startswith('stereo.')})
    ori = (80, 160)
    runner = model.dense_runner(ori, True, 2)
    assert all(p.lr_check and p.stereo_module.lr_check and p.stereo_module.lr_max_diff == 4.0 for p in runner.pipes)
    pipe = runner.pipes[0]
    frames = [synthetic_batch([70 + t], ori[0], ori[1], 32) for t in range(2)]
    l = torch.cat([torch.nn.functional.pad(f['img'][0:1, :, :ori[0]].to(torch.uint8).float(), [0, 0, 0, 16]) for f in frames]).to(cuda)
    r = torch.cat([torch.nn.functional.pad(f['right'][0:1, :, :ori[0]].to(torch.uint8).float(), [0, 0, 0, 16]) for f in frames]).to(cuda)
    res = pipe.run(l, r)
    torch.cuda.synchronize()
    disp, mask = res['disp_postp'].cpu(), res['disp_mask'].cpu()
    assert mask.shape == (2, 1, pipe.height, pipe.width) and set(mask.unique().tolist()) == {0.0, 1.0}
    assert (mask[:, :, ori[0]:] == 0).all() and (mask[:, :, :, ori[1]:] == 0).all()
    assert torch.equal(disp[:, 0] == 0, mask[:, 0] == 0), 'a valid pixel has a positive disparity here, an invalid one 0'
    # the same pair with the check off: the unmasked map
    plain = StereoDensePipeline(2, ori, 0.375, 0.33, 1, stereo=True, max_disp=32, max_det=model.max_det, agg_layers=2)
    plain.load_state_dict(sd, autotune=False)
    unmasked = plain.disparity(l, r).cpu()
    torch.cuda.synchronize()
    m3 = mask.expand(-1, 3, -1, -1) > 0
    assert torch.equal(disp[m3], unmasked[m3])
    n_diff = 0
    for n in range(2):
        k = int(res['counts'][n])
        assert 0 < k <= pipe.max_det
        boxes = res['boxes'][n, :k].cpu()
        ref_d, ref_s, ref_sb = odepth.bbox_postp_depth(boxes, disp[n:n + 1])
        raw_d, _, _ = odepth.bbox_postp_depth(boxes, unmasked[n:n + 1])
        depth, scale, sb = res['depth'][n, :k].cpu().numpy(), res['scales'][n, :k].cpu().numpy(), res['scaled_boxes'][n, :k].cpu().numpy()
        for i in range(k):
            rd = float(ref_d[i])
            if math.isnan(rd):
                assert math.isnan(depth[i]), (n, i)
            elif rd == -1:
                assert depth[i] == -1 and scale[i] == 1.0, (n, i, depth[i])
            else:
                assert abs(depth[i] - rd) <= 1e-3 * max(1.0, abs(rd)), (n, i, depth[i], rd)
            ud = float(raw_d[i])
            if not (math.isnan(rd) and math.isnan(ud)) and not abs(rd - ud) <= 1e-3 * max(1.0, abs(ud)):
                n_diff += 1
        rs = ref_s.numpy()
        ok = ~np.isnan(rs)
        assert np.abs(scale[ok] - rs[ok]).max() <= 1e-3
        assert rel_err(sb[ok], ref_sb.numpy()[ok]) <= 1e-3
    assert n_diff >= 1, 'the masked pixels must change at least one box depth (precondition, on the oracle)'
    # the plugin surface on the same frames: same detections as the pipeline run above
    data = dict(inputs=dict(img=[f['img'][0:1, :, :ori[0]].to(torch.uint8) for f in frames],
                            right=[f['right'][0:1, :, :ori[0]].to(torch.uint8) for f in frames]),
                data_samples=[TrackDataSample(dict(frame_id=t, ori_shape=ori, img_shape=ori, scale_factor=(1.0, 1.0)))
                              for t in range(2)])
    ref_boxes = [res['boxes'][n, :int(res['counts'][n])].cpu().clone() for n in range(2)]
    outs = model.test_step(data)
    torch.cuda.synchronize()
    for n in range(2):
        assert torch.equal(outs[n].pred_det_instances.bboxes.cpu(), ref_boxes[n])


# the entry points alone (st_softargmin_right, st_lr_check_pack, st_disp_upsample_pack) on their own case tables
GUARDED = [test_softargmin_right_bit_equal_to_restatement, test_lr_check_pack_bit_equal_to_restatement,
           test_lr_check_pack_odd_widths_and_non_finite_disparities, test_lr_check_pack_is_strict_at_equality]
NAN_BY_CONTRACT = [test_lr_check_pack_odd_widths_and_non_finite_disparities]      # a valid pixel beside a NaN input is NaN


# ---- the same entry points over hostile surroundings (tests/guard_memory.py) -------------------------------------------
test_entry_points_are_blind_to_guard_bands = gm.guarded_test(GUARDED, NAN_BY_CONTRACT, doc="""Each test above twice (guard_memory.run_both): as it stands, and with the volume, both disparity maps and
    every output buffer between guard bands of 0xFF bytes (the diagonal gather's x + d past the row, the bilinear
    taps' y = -1 and x = -1 land in NaN).  The hostile run passes the test's own bit-exact bar against the restatement
    and equals the friendly run bit for bit; bands and inputs are unchanged bytewise.""")
