"""GPU: every entry point held to its row of tests/pointer_contract.py (DESIGN.md "Pointer contract").

`dispatch` rows: the entry once on 256-byte aligned buffers - held to the family's oracle at the family's bar - and
again with ONE pointer at +4, +8 and +12 bytes (byte planes: +1 .. +3), everything else aligned: the outputs are
bit-identical to the aligned run, the guard bands of every buffer are whole, and what lies outside the written slice
still holds its fill.  `required` rows: the misaligned call returns ST_ERR_INVALID, st_last_error() names the entry and
the argument, and the outputs hold their fill after a synchronise - the check stands in front of the first launch
(read in the launcher, cited in the row), so no kernel ever sees such a pointer.  Every buffer is a guard_memory.arena,
every shape the smallest that still selects the 16-byte kernel when aligned.  The convolution descriptors: one case
per instance, through test_conv_gpu.run_conv."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard_memory as gm
import lrcheck_ref as LR
import pointer_contract as pc
import rectify_ref as RR
import stereo_eval_ref as SR
import test_conv_gpu as tc
from oracle import c_oracle
from stereotracking_amd import _lib
from stereotracking_amd._lib import StConvDesc, check, current_stream, ptr

pytestmark = pytest.mark.gpu

SHIFTS = (4, 8, 12)
NAN = float('nan')


def put(host, dev, off=0):
    """`host` (numpy / tensor) on the device inside an arena, `off` bytes past a 256-byte boundary."""
    return gm.arena(torch.as_tensor(host).contiguous(), device=dev, offset_bytes=off)


def blank(shape, dev, off=0, fill=NAN, dtype=torch.float32):
    return gm.arena(torch.full(tuple(shape), fill, dtype=dtype), device=dev, offset_bytes=off)


def row(export, arg, cls):
    """The table's row of what a test exercises: the test and the table cannot drift apart silently."""
    r = pc.lookup(export, arg)
    assert r is not None and r[0] == cls and (export, arg) in pc.CASES, (export, arg, r)
    return r


def settle(*buffers):
    torch.cuda.synchronize()
    assert gm.bands_intact(*buffers), 'a guard band was written'


def np32(t):
    return t.cpu().numpy()


def same32(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def refused(lib, rc, *words):
    msg = lib.st_last_error().decode()
    assert rc == -1, f'status {rc}: {msg}'
    for w in words:
        assert w in msg, msg


def untouched(*outs):
    torch.cuda.synchronize()
    for o in outs:
        f = o.cpu().view(-1)
        assert bool(torch.isnan(f).all()) if f.is_floating_point() else bool((f == -1).all()), 'a refused call wrote an output'
    assert gm.bands_intact(*outs)


# ---- dispatch rows: the stereo module -----------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [16, 20, 112])      # the register kernel, the LDS kernel, the two-lane register kernel
def test_softargmin_volume_at_any_float_alignment(D, cuda, stlib):
    row('st_softargmin', 'cost_dev', pc.D)
    N, Hf, Wf, T = 1, 3, 37, 8.0
    cost = np.random.RandomState(D).normal(0, 1, (N, Hf, Wf, D)).astype(np.float32)
    ref = c_oracle.softargmin(cost, T)
    for off in (0,) + SHIFTS:
        c, o = put(cost, cuda, off), blank((N, Hf, Wf), cuda)
        check(stlib.st_softargmin(ptr(c), N, Hf, Wf, D, T, ptr(o), current_stream()), 'st_softargmin')
        settle(c, o)
        assert same32(np32(o), ref), f'D = {D}, volume at +{off} bytes: not the oracle\'s bits'     # = the aligned run's
        assert same32(np32(c), cost)


@pytest.mark.parametrize('want_disp', [True, False])
def test_costvolume_output_volume_at_any_float_alignment(want_disp, cuda, stlib):
    row('st_costvolume_softargmin', 'out_cost_dev', pc.D)
    N, Hf, Wf, Cc, D, T = 1, 3, 70, 8, 16, 8.0
    rng = np.random.RandomState(70)
    fl, fr = (rng.normal(0, 1, (N, Hf, Wf, Cc)).astype(np.float32) for _ in range(2))
    ref = c_oracle.costvolume(fl, fr, Cc, D)
    base = None
    for off in (0,) + SHIFTS:
        l, r = put(fl, cuda), put(fr, cuda)
        cost, disp = blank((N, Hf, Wf, D), cuda, off), (blank((N, Hf, Wf), cuda) if want_disp else None)
        check(stlib.st_costvolume_softargmin(ptr(l), ptr(r), N, Hf, Wf, Cc, Cc, D, T, ptr(cost), ptr(disp), current_stream()))
        settle(*[b for b in (l, r, cost, disp) if b is not None])
        assert same32(np32(cost), ref), f'volume at +{off} bytes: not the oracle\'s bits'
        if want_disp:
            if off == 0:
                base = np32(disp)
                err = np.abs(base - c_oracle.softargmin(ref, T)) / np.maximum(1.0, np.abs(c_oracle.softargmin(ref, T)))
                assert err.max() <= 1e-3                   # the fused soft-argmin's bar (test_stereo_depth_gpu.py)
            assert same32(np32(disp), base), f'volume at +{off} bytes: the fused disparity differs from the aligned run'


def test_disp_upsample_pack_output_at_any_float_alignment(cuda, stlib):
    row('st_disp_upsample_pack', 'disp_postp_dev', pc.D)
    N, Hf, Wf, s = 1, 6, 10, 4
    H, W, vh, vw = Hf * s, Wf * s, Hf * s - 3, Wf * s - 5
    lr = np.random.RandomState(6).uniform(0, 12, (N, Hf, Wf)).astype(np.float32)
    ref = c_oracle.disp_upsample(lr, s, vh, vw)
    for off in (0,) + SHIFTS:
        l, out = put(lr, cuda), blank((N, 3, H, W), cuda, off)
        check(stlib.st_disp_upsample_pack(ptr(l), N, Hf, Wf, s, H, W, vh, vw, ptr(out), current_stream()))
        settle(l, out)
        assert same32(np32(out), ref), f'output at +{off} bytes'


def test_softargmin_right_volume_at_any_float_alignment(cuda, stlib):
    row('st_softargmin_right', 'vol_dev', pc.D)
    H, W, D, T = 3, 33, 16, 8.0
    V = LR.scene_volume(H, W, D, N=1)
    ref = c_oracle.softargmin(LR.shear(V), T)
    for off in (0,) + SHIFTS:
        v, o = put(V, cuda, off), blank((1, H, W), cuda)
        check(stlib.st_softargmin_right(ptr(v), 1, H, W, D, T, ptr(o), current_stream()), 'st_softargmin_right')
        settle(v, o)
        assert same32(np32(o), ref), f'volume at +{off} bytes'


@pytest.mark.parametrize('which', ['disp_postp_dev', 'disp_mask_dev'])
def test_lr_check_pack_outputs_at_any_float_alignment(which, cuda, stlib):
    row('st_lr_check_pack', which, pc.D)
    N, Hl, Wl, s, diff = 1, 6, 10, 4, 2.0
    H, W, vh, vw = Hl * s, Wl * s, Hl * s - 2, Wl * s - 3
    rng = np.random.RandomState(10)
    dL = rng.uniform(0, 4, (N, Hl, Wl)).astype(np.float32)
    dR = (dL + rng.uniform(-1, 1, dL.shape)).astype(np.float32)
    ref_disp, ref_mask = LR.pack(dL, LR.check(dL, dR, s, diff)['valid'], s, (vh, vw))
    assert 0 < ref_mask.sum() < ref_mask.size
    for off in (0,) + SHIFTS:
        l, r = put(dL, cuda), put(dR, cuda)
        out = blank((N, 3, H, W), cuda, off if which == 'disp_postp_dev' else 0)
        mask = blank((N, 1, H, W), cuda, off if which == 'disp_mask_dev' else 0)
        check(stlib.st_lr_check_pack(ptr(l), ptr(r), N, Hl, Wl, s, H, W, vh, vw, diff, ptr(out), ptr(mask),
                                     current_stream()), 'st_lr_check_pack')
        settle(l, r, out, mask)
        assert same32(np32(out), ref_disp) and same32(np32(mask), ref_mask), f'{which} at +{off} bytes'


@pytest.mark.parametrize('which', ['pred_dev', 'gt_dev'])
def test_stereo_eval_maps_at_any_float_alignment(which, cuda):
    from stereotracking_amd.stereo_eval import stereo_error_stats
    row('st_stereo_eval', which, pc.D)
    N, H, W = 2, 9, 16
    pred, gt = SR.seeded_maps(3, N, 1, 1, H, W, 'disp')
    edges, taus = (0, 20, 40, 80), (0.5, 1, 2, 3)
    counts, sums, hist = SR.accumulate(pred, gt, 'disp', SR.BF, None, None, None, edges, taus)
    assert counts[..., 1].sum() > 0
    base = None
    for off in (0,) + SHIFTS:
        p, g = put(pred, cuda, off if which == 'pred_dev' else 0), put(gt, cuda, off if which == 'gt_dev' else 0)
        assert p.data_ptr() % 16 == (off if which == 'pred_dev' else 0)
        got = stereo_error_stats(p, g, 'disp', 0.25, 640, depth_edges=edges, bad_thresholds=taus)
        settle(p, g)
        if off == 0:
            base = got
            assert np.array_equal(got.counts, counts) and np.array_equal(got.hist, hist)
            assert (np.abs(got.sums - sums) <= SR.sum_bound(counts, sums)).all()
        for a, b in ((got.counts, base.counts), (got.sums, base.sums), (got.hist, base.hist)):
            assert a.tobytes() == b.tobytes(), f'{which} at +{off} bytes: differs from the aligned run'


# ---- dispatch rows: the stem's output, the rectifier's destination ---------------------------------------------------
def test_stem_output_at_any_float_alignment_and_an_odd_offset(cuda, stlib):
    row('st_stem_focus_conv', 'out_nhwc_dev', pc.D)
    N, H, W, cout = 1, 16, 24, 32
    torch.manual_seed(52)
    x = torch.rand(N, 3, H, W) * 255.0
    w = torch.randn(cout, 12, 3, 3) / 200.0
    bias = torch.randn(cout) * 0.2
    wp = torch.empty(stlib.st_stem_packed_floats(cout), dtype=torch.float32)
    bp = torch.empty(32, dtype=torch.float32)
    check(stlib.st_stem_pack_weights(ptr(w), ptr(bias), None, None, None, None, 1e-3, cout, 3, ptr(wp), ptr(bp)))
    xx = x.double()
    foc = torch.cat((xx[..., ::2, ::2], xx[..., 1::2, ::2], xx[..., ::2, 1::2], xx[..., 1::2, 1::2]), dim=1)
    ref = F.silu(F.conv2d(foc, w.double(), bias.double(), 1, 1))
    base = None
    for off, ld, ch in ((0, 40, 4), (4, 40, 4), (8, 40, 4), (12, 40, 4), (0, 40, 1), (0, 37, 4)):
        xd, wd, bd = put(x, cuda), put(wp, cuda), put(bp, cuda)
        out = blank((N, H // 2, W // 2, ld), cuda, off, fill=-777.0)
        check(stlib.st_stem_focus_conv(ptr(xd), N, H, W, 3, ptr(wd), ptr(bd), cout, ptr(out), ld, ch, 1, current_stream()))
        settle(xd, wd, bd, out)
        got = out.cpu()
        assert torch.all(got[..., :ch] == -777.0) and torch.all(got[..., ch + cout:] == -777.0), 'wrote outside its slice'
        val = got[..., ch:ch + cout].contiguous()
        if base is None:
            base = val
            tc.assert_close(val.permute(0, 3, 1, 2), ref)
        assert gm.same_bits(val, base), f'output at +{off} bytes, ld {ld}, channel offset {ch}: differs from the 16-byte stores'


@pytest.mark.parametrize('bilinear', [1, 0])
def test_rectify_destination_at_any_byte(bilinear, cuda, stlib):
    row('st_rectify_remap', 'dst_block_dev', pc.D)
    import test_rectify_gpu as tr
    P, h, w = 3, 5, 8
    rng = np.random.RandomState(58)
    host = rng.randint(0, 256, (P, h, w)).astype(np.uint8)
    qmap = tr.map_warp(h, w, h, w)
    ref = RR.remap(host, qmap, bool(bilinear), 7)
    for off in (0, 1, 2, 3):
        frame = put(host, cuda)
        maps = put(qmap[None].astype(np.int32), cuda)
        block = blank((1, P, h, w), cuda, off, fill=0x5A, dtype=torch.uint8)
        assert tr.launch(stlib, [frame], maps, [0], h, w, bilinear, 7, out_block=block, stream=current_stream()) == 0, \
            stlib.st_last_error()
        settle(frame, maps, block)
        assert np.array_equal(block.cpu().numpy()[0], ref), f'destination at +{off} bytes'


# ---- required rows ----------------------------------------------------------------------------------------------------------
def test_costvolume_refuses_misaligned_features(cuda, stlib):
    N, Hf, Wf, Cc, D = 1, 3, 70, 8, 16
    fl = np.zeros((N, Hf, Wf, Cc), np.float32)
    for arg, which in (('featL_dev', 0), ('featR_dev', 1)):
        assert row('st_costvolume_softargmin', arg, pc.R)[1] == 16
        for off in SHIFTS:
            l, r = put(fl, cuda, off if which == 0 else 0), put(fl, cuda, off if which == 1 else 0)
            cost, disp = blank((N, Hf, Wf, D), cuda), blank((N, Hf, Wf), cuda)
            rc = stlib.st_costvolume_softargmin(ptr(l), ptr(r), N, Hf, Wf, Cc, Cc, D, 1.0, ptr(cost), ptr(disp), current_stream())
            refused(stlib, rc, 'st_costvolume_softargmin', arg)
            untouched(cost, disp)


def test_feat_upsample_and_agg3d_refuse_misaligned_tensors(cuda, stlib):
    N, Hf, Wf, Cc, s = 1, 3, 5, 8, 2
    feat = np.zeros((N, Hf, Wf, Cc), np.float32)
    for arg in ('feat_dev', 'out_dev'):
        assert row('st_feat_upsample', arg, pc.R)[1] == 16
        f, o = put(feat, cuda, 4 if arg == 'feat_dev' else 0), blank((N, Hf * s, Wf * s, Cc), cuda, 4 if arg == 'out_dev' else 0)
        refused(stlib, stlib.st_feat_upsample(ptr(f), N, Hf, Wf, Cc, Cc, s, ptr(o), current_stream()), 'st_feat_upsample', '16-byte')
        untouched(o)
    w27 = (C.c_float * 27)(*([0.1] * 27))
    for arg in ('vol_in_dev', 'vol_out_dev'):
        assert row('st_volume_agg3d', arg, pc.R)[1] == 16
        v = put(np.zeros((1, 3, 5, 16), np.float32), cuda, 8 if arg == 'vol_in_dev' else 0)
        o = blank((1, 3, 5, 16), cuda, 8 if arg == 'vol_out_dev' else 0)
        refused(stlib, stlib.st_volume_agg3d(ptr(v), ptr(o), 1, 3, 5, 16, w27, 0.0, 1, current_stream()), 'st_volume_agg3d', '16-byte')
        untouched(o)


def test_box_depth_and_pack_records_refuse_misaligned_box_rows(cuda, stlib):
    N, H, W, M = 1, 8, 8, 4
    disp = put(np.full((N, 3, H, W), 4.0, np.float32), cuda)
    counts = put(np.array([2], np.int32), cuda)
    boxes_h = np.tile(np.array([1.0, 1.0, 6.0, 6.0], np.float32), (N, M, 1))
    for name, extra in (('st_box_depth', ()), ('st_box_depth_method', (2,))):
        fn = getattr(stlib, name)
        for arg in ('boxes_dev', 'out_scaled_boxes_dev'):
            assert row(name, arg, pc.R)[1] == 16
            for off in SHIFTS:
                b = put(boxes_h, cuda, off if arg == 'boxes_dev' else 0)
                depth, scale = blank((N, M), cuda), blank((N, M), cuda)
                sb = blank((N, M, 4), cuda, off if arg == 'out_scaled_boxes_dev' else 0)
                rc = fn(ptr(disp), 3 * H * W, N, H, W, ptr(b), ptr(counts), M, 0.25, 640.0, None, 0, current_stream(),
                        ptr(depth), ptr(scale), ptr(sb), *extra)
                refused(stlib, rc, 'st_box_depth', arg)
                untouched(depth, scale, sb)
    scores, depth, scales = (put(np.ones((N, M), np.float32), cuda) for _ in range(3))
    labels = put(np.zeros((N, M), np.int64), cuda)
    prior = put(np.zeros((N, M), np.int32), cuda)
    for arg in ('boxes_dev', 'scaled_boxes_dev'):
        assert row('st_pack_records', arg, pc.R)[1] == 16
        b, sb = put(boxes_h, cuda, 4 if arg == 'boxes_dev' else 0), put(boxes_h, cuda, 4 if arg == 'scaled_boxes_dev' else 0)
        rec = blank((N, M + 1, 13), cuda)
        rc = stlib.st_pack_records(ptr(b), ptr(scores), ptr(labels), ptr(depth), ptr(scales), ptr(sb), ptr(prior), ptr(counts),
                                   N, M, 2, N, ptr(rec), current_stream())
        refused(stlib, rc, 'st_pack_records', arg)
        untouched(rec)


def test_decode_nms_refuses_misaligned_rows_workspace_and_boxes(cuda, stlib):
    from stereotracking_amd._lib import StDecodeDesc
    d = StDecodeDesc()
    d.struct_size = C.sizeof(StDecodeDesc)
    d.batch, d.num_levels, d.max_det = 1, 1, 8
    d.level_h[0], d.level_w[0], d.level_stride[0], d.level_offset[0] = 2, 2, 8, 0
    d.score_thr, d.iou_thr, d.scale_x, d.scale_y, d.ori_w, d.ori_h = 0.1, 0.5, 1.0, 1.0, 16.0, 16.0
    need = stlib.st_decode_nms_workspace_bytes(C.byref(d))
    assert need > 0
    for arg, off in (('head_out_dev', 4), ('head_out_dev', 8), ('workspace_dev', 8), ('out_boxes_dev', 4), ('out_boxes_dev', 12)):
        assert row('st_decode_nms', arg, pc.R)[1] == 16
        head = put(np.zeros((1, 4, 8), np.float32), cuda, off if arg == 'head_out_dev' else 0)
        ws = blank((need + 16,), cuda, off if arg == 'workspace_dev' else 0, fill=0xFF, dtype=torch.uint8)
        boxes = blank((1, 8, 4), cuda, off if arg == 'out_boxes_dev' else 0)
        scores = blank((1, 8), cuda)
        labels, prior, count = (blank(s, cuda, fill=-1, dtype=t) for s, t in (((1, 8), torch.int64), ((1, 8), torch.int32), ((1,), torch.int32)))
        rc = stlib.st_decode_nms(C.byref(d), ptr(head), ptr(ws), need + 16 - off, current_stream(), ptr(boxes), ptr(scores),
                                 ptr(labels), ptr(prior), ptr(count))
        refused(stlib, rc, 'st_decode_nms', arg)
        untouched(boxes, scores, labels, prior, count)
        assert bool((ws.cpu() == 0xFF).all()), 'a refused call cleared its counters'


def test_focus_pack_spp_and_stem_refuse_misaligned_pointers(cuda, stlib):
    img = np.zeros((1, 3, 16, 24), np.float32)
    for arg, off in (('img_nchw_dev', 4), ('out_nhwc_dev', 4), ('out_nhwc_dev', 8)):
        row('st_focus_pack', arg, pc.R)
        x, o = put(img, cuda, off if arg == 'img_nchw_dev' else 0), blank((1, 8, 12, 12), cuda, off if arg == 'out_nhwc_dev' else 0)
        refused(stlib, stlib.st_focus_pack(ptr(x), 1, 3, 16, 24, ptr(o), current_stream()), 'focus_pack', 'aligned')
        untouched(o)
    for arg in ('x_dev', 'out_dev'):
        row('st_spp_pool', arg, pc.R)
        x, o = put(np.zeros((1, 4, 4, 8), np.float32), cuda, 4 if arg == 'x_dev' else 0), blank((1, 4, 4, 32), cuda, 4 if arg == 'out_dev' else 0)
        refused(stlib, stlib.st_spp_pool(ptr(x), 8, 0, 1, 4, 4, 8, ptr(o), 32, 0, current_stream()), 'spp_pool', '16-byte')
        untouched(o)
    wd = put(np.zeros(stlib.st_stem_packed_floats(32), np.float32), cuda)
    for arg, word in (('img_nchw_dev', 'input'), ('bias_dev', 'bias')):
        row('st_stem_focus_conv', arg, pc.R)
        x, b = put(img, cuda, 4 if arg == 'img_nchw_dev' else 0), put(np.zeros(36, np.float32), cuda, 4 if arg == 'bias_dev' else 0)
        o = blank((1, 8, 12, 32), cuda)
        refused(stlib, stlib.st_stem_focus_conv(ptr(x), 1, 16, 24, 3, ptr(wd), ptr(b), 32, ptr(o), 32, 0, 1, current_stream()),
                'stem_focus_conv', word)
        untouched(o)


# ---- the convolution descriptors -----------------------------------------------------------------------------------------
# one case per instance at N = 2, H = 5, W = 7: variant (None = st_conv1x1_chain), Cin, Cout, kernel, split allowed,
# residual allowed, the words of the refusal
CONV = {
    'tile3': (3, 32, 64, 3, True, True, None),
    'dma13': (13, 32, 64, 3, True, True, None),
    'pw41': (41, 32, 32, 1, True, True, 'pointwise conv'),
    'dc42': (42, 32, 32, 3, False, True, 'direct conv'),
    'wino43': (43, 32, 64, 3, False, True, 'winograd conv'),
    'pwr46': (46, 128, 64, 1, True, True, 'resident 1x1 conv'),
}
SHAPE = (2, 5, 7)


def _conv_inputs(name):
    variant, cin, cout, k, _, _, _ = CONV[name]
    torch.manual_seed(1000 + variant)
    N, H, W = SHAPE
    x = torch.randn(N, cin, H, W)
    w = torch.randn(cout, cin, k, k) / (cin * k * k) ** 0.5
    b = torch.randn(cout)
    res = torch.randn(N, cout, H, W)
    return variant, cout, k, x, w, b, res


@pytest.mark.parametrize('name', list(CONV))
def test_conv_slices_inside_wider_buffers(name, cuda):
    """Way 1: multiples of 4 - res_off = 8 inside res_ld = Cout + 12, out2_off = 8 with a split where the instance has
    one, up_off = 4 inside up_ld = 2 Cout + 4 on the generic tile; garbage in the slack.  Every instance takes them."""
    variant, cout, k, x, w, b, res = _conv_inputs(name)
    _, _, _, _, splits, _, _ = CONV[name]
    kw = dict(res=res, post_scale=0.5, res_ld=cout + 12, res_off=8)
    if splits:
        kw.update(split=cout // 2, out2_off=8, out2_ld=cout // 2 + 12)
    if name == 'tile3':
        kw.update(up=True, up_off=4, up_ld=2 * cout + 4)
    got, up = tc.run_conv(x, w, b, 1, k // 2, 1, cuda, variant=variant, **kw)
    ref = tc.ref_conv(x, w, b, 1, k // 2, 1, res, 0.5)
    tc.assert_close(got, ref)
    if up is not None:
        tc.assert_close(up, F.interpolate(ref, scale_factor=2, mode='nearest'))


@pytest.mark.parametrize('name', list(CONV))
def test_conv_offsets_that_are_1_mod_4(name, cuda, stlib):
    """Way 2: out1_off = 5 in out1_ld = Cout + 7, res_off = 3 in res_ld = Cout + 5.  The tile instances and the streaming
    1x1 kernel (scalar epilogue) compute the same bits as on multiples of 4; the direct, Winograd and resident
    instances refuse by name; st_conv2d_nhwc takes its tile either way."""
    variant, cout, k, x, w, b, res = _conv_inputs(name)
    words = CONV[name][6]
    odd = dict(res=res, post_scale=0.5, out1_off=5, out1_ld=cout + 7, res_off=3, res_ld=cout + 5)
    ref = tc.ref_conv(x, w, b, 1, k // 2, 1, res, 0.5)
    if words is None or variant == 41:
        base, _ = tc.run_conv(x, w, b, 1, k // 2, 1, cuda, variant=variant, res=res, post_scale=0.5)
        got, _ = tc.run_conv(x, w, b, 1, k // 2, 1, cuda, variant=variant, **odd)
        assert gm.same_bits(got.contiguous(), base.contiguous()), 'odd offsets changed the bits'
        tc.assert_close(got, ref)
    else:
        rc, _, _ = tc.run_conv(x, w, b, 1, k // 2, 1, cuda, variant=variant, want_status=True, **odd)
        refused(stlib, rc, words)
    # through st_conv2d_nhwc: a tile, bit-equal to that tile on aligned slices
    base, _ = tc.run_conv(x, w, b, 1, k // 2, 1, cuda, res=res, post_scale=0.5)
    got, _ = tc.run_conv(x, w, b, 1, k // 2, 1, cuda, **odd)
    assert gm.same_bits(got.contiguous(), base.contiguous())
    tc.assert_close(got, ref)


# what each instance does with ONE base pointer at +4 bytes: 'same' = same bits as aligned, else refused
BASES = {
    'tile3': dict(**{'in': 'refuse', 'wgt': 'refuse'}, bias='same', out1='same', out2='same', res='same', up='same'),
    'dma13': dict(**{'in': 'refuse', 'wgt': 'refuse'}, bias='same', out1='same', out2='same', res='same'),
    'pw41': dict(**{'in': 'refuse', 'wgt': 'refuse'}, bias='same', out1='same', out2='same', res='same'),
    'dc42': dict(**{'in': 'refuse', 'wgt': 'refuse'}, bias='refuse', out1='refuse', res='refuse'),
    'wino43': dict(**{'in': 'refuse'}, wino='refuse', bias='refuse', out1='refuse', res='refuse'),
    'pwr46': dict(**{'in': 'refuse', 'wgt': 'refuse'}, bias='same', out1='refuse', out2='refuse', res='refuse'),
}


@pytest.mark.parametrize('name', list(CONV))
def test_conv_each_base_pointer_at_plus_4_bytes(name, cuda, stlib):
    """Way 3.  Forced instance: the outcome BASES lists (read off the *_applicable functions and conv2d_launch).
    st_conv2d_nhwc: in_dev / wgt_dev are refused by name, every other base gives the aligned run's bits."""
    variant, cout, k, x, w, b, res = _conv_inputs(name)
    _, _, _, _, splits, _, words = CONV[name]
    for field in ('in_dev', 'wgt_dev'):
        row('st_conv2d_nhwc', f'd.{field}', pc.R)
        row('st_conv2d_nhwc_variant', f'd.{field}', pc.R)
    kw = dict(res=res, post_scale=0.5)
    if splits:
        kw.update(split=cout // 2)
    if name == 'tile3':
        kw.update(up=True)
    ref = tc.ref_conv(x, w, b, 1, k // 2, 1, res, 0.5)
    for forced in (variant, -1):
        base, base_up = tc.run_conv(x, w, b, 1, k // 2, 1, cuda, variant=forced, **kw)
        tc.assert_close(base, ref)
        outcomes = BASES[name] if forced >= 0 else dict(BASES['tile3'], **{} if name == 'tile3' else {'up': None})
        for which, outcome in outcomes.items():
            if outcome is None or which not in BASES[name]:
                continue
            rc, got, up = tc.run_conv(x, w, b, 1, k // 2, 1, cuda, variant=forced, want_status=True, shift={which: 4}, **kw)
            if outcome == 'refuse':
                msg = ('st_conv2d_nhwc',) if (forced < 0 or words is None) else (words,)
                refused(stlib, rc, *msg)
            else:
                assert rc == 0, (name, forced, which, stlib.st_last_error())
                assert gm.same_bits(got.contiguous(), base.contiguous()), f'{name} / variant {forced}: {which} at +4 bytes changed the bits'
                if up is not None:
                    assert gm.same_bits(up.contiguous(), base_up.contiguous())


def test_conv1x1_chain_pointers(cuda, stlib):
    """st_conv1x1_chain (32 -> 32 | 32 -> 32): a.in_dev at +4 bytes is refused; a.out1 / a.out2 / b.out1 at +4 bytes,
    and offsets that are 1 mod 4, take the scalar epilogue with the bits of the 16-byte one."""
    row('st_conv1x1_chain', 'a.in_dev', pc.R)
    for arg in ('a.out1_dev', 'a.out2_dev', 'b.out1_dev'):
        row('st_conv1x1_chain', arg, pc.D)
    N, H, W = SHAPE
    cin = 32
    torch.manual_seed(41)
    x = torch.randn(N, cin, H, W)
    wa, ba = torch.randn(64, cin, 1, 1) / cin ** 0.5, torch.randn(64)
    wb, bb = torch.randn(32, 32, 1, 1) / 32 ** 0.5, torch.randn(32)
    (wpa, bpa), (wpb, bpb) = tc.pack(wa, ba), tc.pack(wb, bb)
    ya = tc.ref_conv(x, wa, ba, 1, 0, 1)
    yb = F.silu(F.conv2d(ya[:, :32], wb.double(), bb.double()))

    def run(shift=None, offs=(0, 8, 4), lds=(32, 44, 36)):
        shift = shift or {}
        xin = put(x.permute(0, 2, 3, 1), cuda, shift.get('in', 0))
        wts = [put(t, cuda, shift.get(k, 0)) for t, k in ((wpa, 'wa'), (bpa, 'ba'), (wpb, 'wb'), (bpb, 'bb'))]
        main, cat, tmp = (blank((N, H, W, ld), cuda, shift.get(k, 0), fill=-777.0) for k, ld in zip(('main', 'cat', 'tmp'), lds))
        a, b = StConvDesc(), StConvDesc()
        a.in_dev = xin.data_ptr(); a.N, a.Hi, a.Wi, a.Cin, a.in_ld, a.in_off = N, H, W, cin, cin, 0
        a.wgt_dev, a.bias_dev = wts[0].data_ptr(), wts[1].data_ptr()
        a.Cout, a.KH, a.KW, a.stride, a.pad, a.act = 64, 1, 1, 1, 0, 1
        a.out1_dev = main.data_ptr(); a.out1_ld, a.out1_off, a.split = lds[0], offs[0], 32
        a.out2_dev = cat.data_ptr(); a.out2_ld, a.out2_off = lds[1], offs[1]
        b.in_dev = main.data_ptr(); b.N, b.Hi, b.Wi, b.Cin, b.in_ld, b.in_off = N, H, W, 32, 32, 0
        b.wgt_dev, b.bias_dev = wts[2].data_ptr(), wts[3].data_ptr()
        b.Cout, b.KH, b.KW, b.stride, b.pad, b.act = 32, 1, 1, 1, 0, 1
        b.out1_dev = tmp.data_ptr(); b.out1_ld, b.out1_off, b.split = lds[2], offs[2], 32
        if 'main' in shift:
            b.in_dev = 0          # ignored by the chain; its alignment is what pw_conv_applicable looks at
        if 'bin' in shift:
            b.in_dev = main.data_ptr() + shift['bin']
        rc = stlib.st_conv1x1_chain(C.byref(a), C.byref(b), current_stream())
        settle(xin, main, cat, tmp, *wts)
        outs = []
        for t, off in zip((main, cat, tmp), offs):
            h = t.cpu()
            if rc == 0:
                assert torch.all(h[..., :off] == -777.0) and torch.all(h[..., off + 32:] == -777.0), 'wrote outside a slice'
            else:
                assert torch.all(h == -777.0), 'a refused chain wrote an output'
            outs.append(h[..., off:off + 32].contiguous())
        return rc, outs

    rc, base = run()
    assert rc == 0, stlib.st_last_error()
    for got, ref in zip(base, (ya[:, :32], ya[:, 32:], yb)):
        tc.assert_close(got.permute(0, 3, 1, 2), ref)
    for shift in ({'main': 4}, {'cat': 4}, {'tmp': 4}, {'main': 8, 'cat': 12, 'tmp': 4}):
        rc, got = run(shift)
        assert rc == 0, (shift, stlib.st_last_error())
        assert all(gm.same_bits(g, b0) for g, b0 in zip(got, base)), f'{shift}: differs from the aligned run'
    rc, got = run(offs=(5, 9, 1), lds=(39, 45, 35))
    assert rc == 0 and all(gm.same_bits(g, b0) for g, b0 in zip(got, base)), 'offsets 1 mod 4 changed the bits'
    for arg, key in (('a.in_dev', 'in'), ('a.wgt_dev', 'wa'), ('b.wgt_dev', 'wb'), ('b.in_dev', 'bin')):
        row('st_conv1x1_chain', arg, pc.R)
        rc, _ = run({key: 4})
        refused(stlib, rc, 'pointwise conv')
    rc, got = run({'ba': 4, 'bb': 4})          # the biases are staged element by element
    assert rc == 0 and all(gm.same_bits(g, b0) for g, b0 in zip(got, base))


# ---- dispatch rows: raw input packing, the raw-frame stem, the fused disparity map, the JPEG planes -------------------
PACK_ARGS = {'img_u8_dev': (1, 2, 3), 'disp_u16_dev': (2, 4, 6), 'img_out_dev': SHIFTS, 'disp_postp_out_dev': SHIFTS,
             'disp_mask_out_dev': SHIFTS}


@pytest.mark.parametrize('which', list(PACK_ARGS))
def test_pack_raw_inputs_every_pointer_at_its_element_alignment(which, cuda, stlib):
    """One predicate over five pointers (4 / 8 / 16 bytes): each in turn off its vector alignment, the others on it."""
    row('st_pack_raw_inputs', which, pc.D)
    N, h, w, H, W, pad = 2, 5, 8, 6, 12, 114.0
    rng = np.random.RandomState(175)
    img = rng.randint(0, 256, (N, 3, h, w)).astype(np.uint8)
    code = rng.randint(0, 4000, (N, h, w)).astype(np.uint16)
    code[rng.rand(N, h, w) < 0.2] = 65535
    ref_img = np.full((N, 3, H, W), pad, np.float32)
    ref_img[:, :, :h, :w] = img
    ref_disp, ref_mask = np.zeros((N, 3, H, W), np.float32), np.zeros((N, 1, H, W), np.float32)
    ref_disp[:, :, :h, :w] = (np.where(code == 65535, 0, code).astype(np.float32) / np.float32(16.0))[:, None]
    ref_mask[:, 0, :h, :w] = code < 65535
    for off in (0,) + PACK_ARGS[which]:
        at = lambda name: off if name == which else 0       # noqa: E731
        i8, c16 = put(img, cuda, at('img_u8_dev')), put(code.view(np.int16), cuda, at('disp_u16_dev'))
        o_img, o_disp = blank((N, 3, H, W), cuda, at('img_out_dev')), blank((N, 3, H, W), cuda, at('disp_postp_out_dev'))
        o_mask = blank((N, 1, H, W), cuda, at('disp_mask_out_dev'))
        check(stlib.st_pack_raw_inputs(ptr(i8), ptr(c16), N, h, w, H, W, pad, ptr(o_img), ptr(o_disp), ptr(o_mask),
                                       current_stream()), 'st_pack_raw_inputs')
        settle(i8, c16, o_img, o_disp, o_mask)
        assert same32(np32(o_img), ref_img) and same32(np32(o_disp), ref_disp) and same32(np32(o_mask), ref_mask), \
            f'{which} at +{off} bytes'


def test_raw_frame_stem_output_at_any_float_alignment_and_an_odd_offset(cuda, stlib):
    row('st_stem_focus_conv_u8', 'out_dev', pc.D)
    N, h, w, H, W, cout, pad = 1, 12, 24, 16, 24, 32, 114.0
    torch.manual_seed(53)
    frame = put(torch.randint(0, 256, (3, h, w), dtype=torch.uint8), cuda)
    wgt, bias = torch.randn(cout, 12, 3, 3) / 200.0, torch.randn(cout) * 0.2
    wp = torch.empty(stlib.st_stem_packed_floats(cout), dtype=torch.float32)
    bp = torch.empty(32, dtype=torch.float32)
    check(stlib.st_stem_pack_weights(ptr(wgt), ptr(bias), None, None, None, None, 1e-3, cout, 3, ptr(wp), ptr(bp)))
    wd, bd = put(wp, cuda), put(bp, cuda)
    table = (C.c_void_p * N)(frame.data_ptr())
    # the specification: st_pack_raw_frames + st_stem_focus_conv on aligned buffers (pinned to fp64 in test_conv_gpu.py)
    x, ref = blank((N, 3, H, W), cuda), blank((N, H // 2, W // 2, cout), cuda)
    check(stlib.st_pack_raw_frames(table, N, h, w, H, W, pad, ptr(x), current_stream()))
    check(stlib.st_stem_focus_conv(ptr(x), N, H, W, 3, ptr(wd), ptr(bd), cout, ptr(ref), cout, 0, 1, current_stream()))
    settle(x, ref)
    ref = ref.cpu()
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0.1
    for off, ld, ch in ((0, 40, 4), (4, 40, 4), (8, 40, 4), (12, 40, 4), (0, 40, 1), (0, 37, 4)):
        out = blank((N, H // 2, W // 2, ld), cuda, off, fill=-777.0)
        check(stlib.st_stem_focus_conv_u8(table, N, h, w, H, W, pad, ptr(wd), ptr(bd), cout, ptr(out), ld, ch, 1, current_stream()))
        settle(frame, wd, bd, out)
        got = out.cpu()
        assert torch.all(got[..., :ch] == -777.0) and torch.all(got[..., ch + cout:] == -777.0), 'wrote outside its slice'
        assert gm.same_bits(got[..., ch:ch + cout].contiguous(), ref), f'output at +{off} bytes, ld {ld}, channel offset {ch}'


@pytest.mark.parametrize('which', ['disp_dev', 'out_dev'])
def test_disp_fuse_maps_at_any_float_alignment(which, cuda, stlib):
    """The kernel decides per address; W = 16 keeps every quad whole, so the aligned run is all 16-byte accesses."""
    import test_disp_fuse_gpu as tf
    row('st_disp_fuse', which, pc.D)
    N, Cd, H, W, ext = 2, 1, 6, 16, (5, 14)
    dense_h, disp_h = tf._dense(N, H, W), tf._disp(N, Cd, H, W, 'mixed')
    want1 = tf._resize(stlib, dense_h.to(cuda), H, W).cpu().numpy()
    plane = disp_h[:, :1].numpy()
    with np.errstate(invalid='ignore'):
        valid = plane > 0
    want2 = np.where(valid, plane, want1)
    count = (~valid)[:, 0, :ext[0], :ext[1]].reshape(N, -1).sum(1).tolist()
    for off in (0,) + SHIFTS:
        dense, disp = put(dense_h, cuda), put(disp_h, cuda, off if which == 'disp_dev' else 0)
        out = blank((N, 1, H, W), cuda, off if which == 'out_dev' else 0)
        filled = blank((N,), cuda, fill=0, dtype=torch.int32)
        assert tf._fuse(stlib, dense, disp, ext, 2, out, filled) == 0, stlib.st_last_error()
        settle(dense, disp, out, filled)
        assert tf._same(out.cpu().numpy(), want2), f'{which} at +{off} bytes'
        assert filled.cpu().tolist() == count


def test_jpeg_planes_at_any_byte(cuda):
    """Width 40: every row of an aligned plane starts on a 4-byte boundary (packed stores); +1 .. +3 takes the scalar ones."""
    import test_jpeg_gpu as tj
    from stereotracking_amd import jpeg
    row('st_jpeg_reconstruct', 'out_dev', pc.D)
    info = jpeg._info(jpeg.encode_jpeg(np.zeros((24, 40, 3), np.uint8), 90, '420'))
    rng = np.random.default_rng(77)
    coef = rng.integers(-2048, 2048, (2, int(info.coef_count))).astype(np.int16)
    quant = rng.integers(1, 256, (2, 3, 64)).astype(np.uint16)
    host = np.stack([jpeg.reconstruct_host(coef[i], quant[i], info, order='bgr', planar=True) for i in range(2)])
    work_bytes = int(jpeg._api().st_jpeg_work_bytes(C.byref(info), 2))
    for off in (0, 1, 2, 3):
        out = blank((2, 3, 24, 40), cuda, off, fill=0xFF, dtype=torch.uint8)
        work = blank((work_bytes,), cuda, fill=0xFF, dtype=torch.uint8)
        tj.device_reconstruct(info, coef, quant, cuda, out=out, work=work)
        settle(out, work)
        assert np.array_equal(out.cpu().numpy(), host), f'planes at +{off} bytes'


# ---- required rows of the fused launches, the head prediction and the detector: an aligned call that runs, then one
# pointer at +4 bytes --------------------------------------------------------------------------------------------------
def _zeros(n, dev, off=0):
    return put(torch.zeros(int(n)), dev, off)


def _desc(**kw):
    d = StConvDesc()
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_resident_chain_refuses_misaligned_weights_and_tensors(cuda, stlib):
    """st_conv1x1_chain on the resident kernel (128 -> 64 | 64, then 64 -> 64): every tensor and both weight matrices."""
    N, H, W = SHAPE

    def run(shift=None):
        shift = shift or {}
        t = {k: _zeros(n, cuda, shift.get(k, 0)) for k, n in (
            ('in', N * H * W * 128), ('wa', stlib.st_conv_packed_floats(128, 128, 1, 1)), ('ba', 128),
            ('wb', stlib.st_conv_packed_floats(64, 64, 1, 1)), ('bb', 64))}
        o = {k: blank((N, H, W, 64), cuda, shift.get(k, 0)) for k in ('main', 'cat', 'tmp')}
        a = _desc(in_dev=t['in'].data_ptr(), N=N, Hi=H, Wi=W, Cin=128, in_ld=128, wgt_dev=t['wa'].data_ptr(),
                  bias_dev=t['ba'].data_ptr(), Cout=128, KH=1, KW=1, stride=1, act=1, out1_dev=o['main'].data_ptr(), out1_ld=64,
                  split=64, out2_dev=o['cat'].data_ptr(), out2_ld=64)
        b = _desc(in_dev=o['main'].data_ptr(), N=N, Hi=H, Wi=W, Cin=64, in_ld=64, wgt_dev=t['wb'].data_ptr(),
                  bias_dev=t['bb'].data_ptr(), Cout=64, KH=1, KW=1, stride=1, act=1, out1_dev=o['tmp'].data_ptr(), out1_ld=64,
                  split=64)
        rc = stlib.st_conv1x1_chain(C.byref(a), C.byref(b), current_stream())
        settle(*t.values(), *o.values())
        return rc, o

    rc, o = run()
    assert rc == 0, stlib.st_last_error()
    assert all(bool((v.cpu() == 0).all()) for v in o.values())           # silu(0) everywhere: the pair ran
    for key in ('in', 'wa', 'wb', 'main', 'cat', 'tmp'):
        rc, o = run({key: 4})
        refused(stlib, rc, 'conv')           # not the resident pair any more, and no shape of the streaming kernel
        untouched(*o.values())


def test_fused_front_refuses_each_misaligned_pointer(cuda, stlib):
    N, H, W = 1, 6, 8
    Ho, Wo = 3, 4
    args = {'a.in_dev': 'in', 'a.wgt_dev': 'w3', 'ms.out1_dev': 'main', 'ms.out2_dev': 'cat', 'c1.out1_dev': 'tmp',
            'frag_ms_dev': 'fms', 'frag_c1_dev': 'fc1'}

    def run(shift=None):
        shift = shift or {}
        t = {k: _zeros(n, cuda, shift.get(k, 0)) for k, n in (
            ('in', N * H * W * 32), ('w3', stlib.st_conv_packed_floats(64, 32, 3, 3)), ('b3', 64), ('bm', 64), ('bc', 32),
            ('wm', stlib.st_conv_packed_floats(64, 64, 1, 1)), ('wc', stlib.st_conv_packed_floats(32, 32, 1, 1)),
            ('fms', stlib.st_front_frag_floats(64, 64)), ('fc1', stlib.st_front_frag_floats(32, 32)))}
        o = {k: blank((N, Ho, Wo, ld), cuda, shift.get(k, 0)) for k, ld in (('main', 32), ('cat', 64), ('tmp', 36))}
        a = _desc(in_dev=t['in'].data_ptr(), N=N, Hi=H, Wi=W, Cin=32, in_ld=32, wgt_dev=t['w3'].data_ptr(),
                  bias_dev=t['b3'].data_ptr(), Cout=64, KH=3, KW=3, stride=2, pad=1, act=1, post_scale=1.0, out1_ld=64, split=64)
        m = _desc(N=N, Hi=Ho, Wi=Wo, Cin=64, in_ld=64, wgt_dev=t['wm'].data_ptr(), bias_dev=t['bm'].data_ptr(), Cout=64,
                  KH=1, KW=1, stride=1, act=1, post_scale=1.0, out1_dev=o['main'].data_ptr(), out1_ld=32, split=32,
                  out2_dev=o['cat'].data_ptr(), out2_ld=64, out2_off=32)
        c = _desc(N=N, Hi=Ho, Wi=Wo, Cin=32, in_ld=32, wgt_dev=t['wc'].data_ptr(), bias_dev=t['bc'].data_ptr(), Cout=32,
                  KH=1, KW=1, stride=1, act=1, post_scale=1.0, out1_dev=o['tmp'].data_ptr(), out1_ld=36, out1_off=4, split=32)
        rc = stlib.st_conv3x3s2_csp_front(C.byref(a), C.byref(m), C.byref(c), ptr(t['fms']), ptr(t['fc1']), current_stream())
        settle(*t.values(), *o.values())
        return rc, o

    rc, o = run()
    assert rc == 0, stlib.st_last_error()
    assert bool((o['main'].cpu() == 0).all()) and bool((o['tmp'].cpu()[..., 4:] == 0).all())
    for arg, key in args.items():
        row('st_conv3x3s2_csp_front', arg, pc.R)
        rc, o = run({key: 4})
        refused(stlib, rc, 'fused front')
        untouched(*o.values())


def test_csp_tail_refuses_each_misaligned_pointer(cuda, stlib):
    N, H, W = 1, 4, 6
    args = {'conv2.in_dev': 'in', 'conv2.res_dev': 'main', 'conv2.bias_dev': 'b2', 'conv2.wgt_wino_dev': 'wino',
            'conv2.out1_dev': 'cat', 'fin.in_dev': 'cat', 'fin.out1_dev': 'out', 'fin.res_dev': 'other', 'fin.bias_dev': 'bf',
            'frag_fin_dev': 'frag'}

    def run(shift=None):
        shift = shift or {}
        t = {k: _zeros(n, cuda, shift.get(k, 0)) for k, n in (
            ('in', N * H * W * 32), ('main', N * H * W * 32), ('other', N * H * W * 64), ('b2', 32), ('bf', 64),
            ('w2', stlib.st_conv_packed_floats(32, 32, 3, 3)), ('wf', stlib.st_conv_packed_floats(64, 64, 1, 1)),
            ('wino', stlib.st_wino_packed_floats(32, 32)), ('frag', stlib.st_csp_tail_frag_floats()),
            ('cat', N * H * W * 72))}
        out = blank((N, H, W, 68), cuda, shift.get('out', 0))
        c2 = _desc(in_dev=t['in'].data_ptr(), N=N, Hi=H, Wi=W, Cin=32, in_ld=32, wgt_dev=t['w2'].data_ptr(),
                   bias_dev=t['b2'].data_ptr(), wgt_wino_dev=t['wino'].data_ptr(), Cout=32, KH=3, KW=3, stride=1, pad=1,
                   out1_dev=t['cat'].data_ptr(), out1_ld=72, out1_off=4, split=32, res_dev=t['main'].data_ptr(), res_ld=32,
                   post_scale=1.0, act=1)
        f = _desc(in_dev=t['cat'].data_ptr(), N=N, Hi=H, Wi=W, Cin=64, in_ld=72, in_off=4, wgt_dev=t['wf'].data_ptr(),
                  bias_dev=t['bf'].data_ptr(), Cout=64, KH=1, KW=1, stride=1, out1_dev=out.data_ptr(), out1_ld=68, out1_off=4,
                  split=64, res_dev=t['other'].data_ptr(), res_ld=64, post_scale=0.5, act=1)
        rc = stlib.st_conv3x3_csp_tail(C.byref(c2), C.byref(f), ptr(t['frag']), current_stream())
        settle(*t.values(), out)
        return rc, out

    rc, out = run()
    assert rc == 0, stlib.st_last_error()
    assert bool((out.cpu()[..., 4:] == 0).all())
    for arg, key in args.items():
        row('st_conv3x3_csp_tail', arg, pc.R)
        rc, out = run({key: 4})
        refused(stlib, rc, 'csp tail')
        untouched(out)


def test_winograd_group_refuses_each_misaligned_pointer(cuda, stlib):
    N, H, W = 1, 4, 6
    args = {'descs.in_dev': 'in', 'descs.out1_dev': 'out', 'descs.wgt_wino_dev': 'wino', 'descs.bias_dev': 'b'}

    def run(shift=None):
        shift = shift or {}
        keep, outs = [], []
        descs = (StConvDesc * 2)()
        for k in range(2):
            sh = shift if k == 1 else {}
            t = {n: _zeros(c, cuda, sh.get(n, 0)) for n, c in (
                ('in', N * H * W * 32), ('w', stlib.st_conv_packed_floats(64, 32, 3, 3)), ('b', 64),
                ('wino', stlib.st_wino_packed_floats(64, 32)))}
            out = blank((N, H, W, 64), cuda, sh.get('out', 0))
            for f, v in dict(in_dev=t['in'].data_ptr(), N=N, Hi=H, Wi=W, Cin=32, in_ld=32, wgt_dev=t['w'].data_ptr(),
                             bias_dev=t['b'].data_ptr(), wgt_wino_dev=t['wino'].data_ptr(), Cout=64, KH=3, KW=3, stride=1,
                             pad=1, act=1, out1_dev=out.data_ptr(), out1_ld=64, split=64).items():
                setattr(descs[k], f, v)
            keep += list(t.values())
            outs.append(out)
        rc = stlib.st_conv3x3_wino_group(descs, 2, current_stream())
        settle(*keep, *outs)
        return rc, outs

    rc, outs = run()
    assert rc == 0, stlib.st_last_error()
    assert all(bool((o.cpu() == 0).all()) for o in outs)
    for arg, key in args.items():
        row('st_conv3x3_wino_group', arg, pc.R)
        rc, outs = run({key: 4})
        refused(stlib, rc, 'winograd group')
        untouched(*outs)


def test_head_pred_refuses_misaligned_towers_and_rows(cuda, stlib):
    from stereotracking_amd._lib import StHeadPredLevel
    feat, M = 96, 4

    def run(shift=None):
        shift = shift or {}
        levels = (StHeadPredLevel * 3)()
        keep, outs = [], []
        for l in range(3):
            sh = shift if l == 1 else {}
            cls, reg = _zeros(M * feat, cuda, sh.get('cls', 0)), _zeros(M * feat, cuda, sh.get('reg', 0))
            w = [_zeros(n, cuda) for n in (stlib.st_conv_packed_floats(1, feat, 1, 1), 32, stlib.st_conv_packed_floats(5, feat, 1, 1), 32)]
            out = blank((M, 8), cuda, sh.get('out', 0))
            for f, v in dict(cls_dev=cls.data_ptr(), cls_ld=feat, reg_dev=reg.data_ptr(), reg_ld=feat, wgt_cls_dev=w[0].data_ptr(),
                             bias_cls_dev=w[1].data_ptr(), wgt_reg_dev=w[2].data_ptr(), bias_reg_dev=w[3].data_ptr(),
                             out_dev=out.data_ptr(), M=M).items():
                setattr(levels[l], f, v)
            keep += [cls, reg] + w
            outs.append(out)
        rc = stlib.st_head_pred(levels, feat, 1, current_stream())
        settle(*keep, *outs)
        return rc, outs

    rc, outs = run()
    assert rc == 0, stlib.st_last_error()
    assert all(bool((o.cpu()[:, :6] == 0).all()) for o in outs)
    for arg, key in (('levels.cls_dev', 'cls'), ('levels.reg_dev', 'reg'), ('levels.out_dev', 'out')):
        row('st_head_pred', arg, pc.R)
        rc, outs = run({key: 4})
        refused(stlib, rc, 'head_pred', '16-byte')
        untouched(*outs)


def test_detector_forward_refuses_misaligned_images_workspace_and_head(cuda):
    """run_ops' first statement, through st_detector_forward and st_detector_forward_phase (the raw-frame entries and the
    autotune reach the same statement with the same five pointers)."""
    from stereotracking_amd._lib import StError
    from stereotracking_amd.engine import HipDetector
    from stereotracking_amd.synthetic import synthetic_state_dict
    N, H, W = 1, 64, 96
    det = HipDetector(N, H, W, 0.375, 0.33, 1)
    det.load_state_dict(synthetic_state_dict(det.param_table(), seed=0))
    nws = int(det.lib.st_detector_workspace_bytes(det.handle))
    img_h = torch.rand(N, 3, H, W) * 255.0

    def run(entry, shift=None):
        shift = shift or {}
        img, disp, right = (put(img_h, cuda, shift.get(k, 0)) for k in ('img', 'disp', 'right'))
        head = blank((det.head_floats,), cuda, shift.get('head', 0))
        det._ws = blank((nws,), cuda, shift.get('ws', 0), fill=0xFF, dtype=torch.uint8)
        try:
            if entry == 'st_detector_forward':
                det.forward(img, disp, head_out=head)
            else:
                det.forward_phase(1 if ('disp' in shift or 'head' in shift) else 0, img=img, disp=disp, right=right, head_out=head)
                if not shift:
                    det.forward_phase(1, img=img, disp=disp, right=right, head_out=head)
        except StError as e:
            settle(img, disp, right, head, det._ws)
            return str(e), head
        settle(img, disp, right, head, det._ws)
        return None, head

    for entry, keys in (('st_detector_forward', dict(img_dev='img', disp_dev='disp', workspace_dev='ws', head_out_dev='head')),
                        ('st_detector_forward_phase', dict(img_dev='img', disp_dev='disp', right_dev='right', workspace_dev='ws',
                                                           head_out_dev='head'))):
        err, head = run(entry)
        assert err is None and bool(torch.isfinite(head.cpu()[:6]).all()), err
        for arg, key in keys.items():
            row(entry, arg, pc.R)
            err, head = run(entry, {key: 4})
            assert err is not None and 'st_detector_forward' in err and '16-byte' in err, (entry, arg, err)
            untouched(head)
            assert bool((det._ws.cpu() == 0xFF).all()), 'a refused forward wrote its workspace'
    det._ws = None
