"""The two launches of the detector head that have no single-layer form, on their own:

  st_conv3x3_wino_group  the grouped Winograd launch (wino_group_launch; plan instances 48 / 49): several independent
                         3x3 layers in one grid, a workgroup finding its problem by the prefix of per-problem grids
                         (each padded to a multiple of 8);
  st_head_pred           conv_cls + conv_reg + conv_obj of all three levels in one reduction launch (instance 47):
                         workgroups split across the levels by pixel share, 8 lanes per pixel.

Inside the detector both have only ever run at the map sizes of a few geometries; here the block-to-problem arithmetic
meets maps smaller than one tile block, grids that are and are not multiples of 8, and levels of 1 .. 33 pixels.
"""
import ctypes as C

import pytest
import torch

import guard_memory
from stereotracking_amd import _lib
from stereotracking_amd._lib import StConvDesc, StHeadPredLevel, check, ptr
from test_conv_gpu import assert_close, pack, ref_conv

pytestmark = pytest.mark.gpu

GUARD = -777.0


class Problem:
    """One 3x3 / stride 1 / pad 1 layer: input as a channel slice of a wider NHWC buffer (garbage around it), output at
    a channel offset inside a buffer pre-filled with GUARD.  Buffers come from the ambient guard_memory session: finite
    garbage and plain allocations, unless a guard test says otherwise."""

    def __init__(self, N, H, W, cin, cout, dev, seed, in_pad=(0, 0), out_pad=(4, 4), res=False):
        lib = _lib.load()
        self.mem = guard_memory.current()
        g = torch.Generator().manual_seed(seed)
        self.shape = (N, H, W, cin, cout)
        self.x = torch.randn(N, cin, H, W, generator=g) + 0.5
        self.w = torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5)
        self.b = torch.randn(cout, generator=g) * 0.1
        self.in_off, self.in_ld = in_pad[0], in_pad[0] + cin + in_pad[1]
        self.out_off, self.out_ld = out_pad[0], out_pad[0] + cout + out_pad[1]
        xin = torch.randn(N, H, W, self.in_ld, generator=g) * 3.0
        xin[..., self.in_off:self.in_off + cin] = self.x.permute(0, 2, 3, 1)
        wp, bp = pack(self.w, self.b)
        wino = torch.empty(lib.st_wino_packed_floats(cout, cin), dtype=torch.float32)
        check(lib.st_wino_pack_weights(ptr(wp), cout, cin, ptr(wino)), 'st_wino_pack_weights')
        self.dev = dev
        self.xin = self.mem.input(xin, dev, self.in_off, cin)
        self.wp, self.bp, self.wino = wp.to(dev), bp.to(dev), wino.to(dev)
        self.res = self.mem.input(torch.randn(N, H, W, cout, generator=g), dev) if res else None

    def out_buffer(self):
        N, H, W, _, _ = self.shape
        return self.mem.output((N, H, W, self.out_ld), self.dev, GUARD)

    def desc(self, out):
        N, H, W, cin, cout = self.shape
        d = StConvDesc()
        d.in_dev = self.xin.data_ptr(); d.N, d.Hi, d.Wi, d.Cin, d.in_ld, d.in_off = N, H, W, cin, self.in_ld, self.in_off
        d.wgt_dev, d.bias_dev, d.wgt_wino_dev = self.wp.data_ptr(), self.bp.data_ptr(), self.wino.data_ptr()
        d.Cout, d.KH, d.KW, d.stride, d.pad = cout, 3, 3, 1, 1
        d.out1_dev = out.data_ptr(); d.out1_ld, d.out1_off, d.split = self.out_ld, self.out_off, cout
        if self.res is not None:
            d.res_dev = self.res.data_ptr(); d.res_ld, d.res_off = cout, 0
        d.post_scale, d.act = 1.0, 1
        return d

    def check_output(self, out, what):
        cout = self.shape[4]
        o = out.cpu()
        assert torch.all(o[..., :self.out_off] == GUARD) and torch.all(o[..., self.out_off + cout:] == GUARD), \
            f'{what}: wrote outside its channel slice'
        return o[..., self.out_off:self.out_off + cout].permute(0, 3, 1, 2)


def group_array(descs):
    arr = (StConvDesc * len(descs))()
    for i, d in enumerate(descs):
        arr[i] = d
    return arr


# (N, H, W, Cin, Cout, input (off, tail) padding, output (off, tail) padding); one tile block = 8 x 16 output pixels,
# workgroups per problem = N * ceil(H / 8) * ceil(W / 16) * Cout / 64
GROUPS = {
    # 2 + 2 workgroups: a map under one tile block whose grid is padded 2 -> 8, then single pixels
    'n2_3x5_and_1x1': [(1, 3, 5, 128, 128, (0, 0), (4, 4)), (2, 1, 1, 32, 64, (32, 0), (0, 8))],
    # the head's first tower depth at the smallest test geometry: 16, 4, 4 workgroups (the first already a multiple of 8)
    'n3_tower_12x20_6x10_3x5': [(1, 12, 20, 128, 256, (0, 128), (4, 4)), (1, 6, 10, 128, 256, (0, 0), (0, 0)),
                                (1, 3, 5, 128, 256, (32, 0), (8, 0))],
    # six problems: exactly one tile block (1 workgroup), 8 workgroups (no padding ids) between ragged ones (12, 4, 18, 2),
    # three cin (1, 3, 4 K-chunks), three cout, N = 3
    'n6_mixed': [(1, 8, 16, 96, 64, (0, 0), (4, 4)), (2, 16, 32, 32, 64, (0, 32), (0, 0)),
                 (3, 9, 17, 128, 64, (64, 64), (4, 0)), (1, 3, 5, 96, 256, (0, 0), (0, 4)),
                 (1, 23, 40, 32, 128, (32, 32), (128, 0)), (1, 1, 1, 128, 128, (0, 0), (4, 4))],
}


@pytest.mark.parametrize('name', list(GROUPS))
def test_grouped_winograd_launch_equals_separate_launches(name, stlib, cuda):
    """Every output of st_conv3x3_wino_group is BIT-IDENTICAL to st_conv2d_nhwc_variant(d, 43) on the same descriptor:
    the group kernel instantiates wino_conv3x3_body<2, 2, false, false>, which is what variant 43 launches for Cout % 64
    == 0, Cin % 32 == 0 without a residual (wino_conv_launch: cbn = 2, no K tail) - true of every problem here.  Guard
    bands around the output slices stay untouched, and each result is within 1e-4 of scale of fp64."""
    probs = [Problem(N, H, W, cin, cout, cuda, 1000 * k + H * W + cin, ip, op)
             for k, (N, H, W, cin, cout, ip, op) in enumerate(GROUPS[name])]
    stream = _lib.current_stream()
    grouped = [p.out_buffer() for p in probs]
    check(stlib.st_conv3x3_wino_group(group_array([p.desc(o) for p, o in zip(probs, grouped)]), len(probs), stream),
          'st_conv3x3_wino_group')
    torch.cuda.synchronize()
    for k, (p, og) in enumerate(zip(probs, grouped)):
        alone = p.out_buffer()
        d = p.desc(alone)
        check(stlib.st_conv2d_nhwc_variant(C.byref(d), stream, 43), 'variant 43')
        torch.cuda.synchronize()
        got, ref = p.check_output(og, f'problem {k} grouped'), p.check_output(alone, f'problem {k} alone')
        assert torch.equal(got, ref), f'problem {k} {p.shape}: grouped launch differs from its own launch'
        assert_close(got, ref_conv(p.x, p.w, p.b, 1, 1, 1))


def test_grouped_winograd_launch_refuses_what_it_cannot_run(stlib, cuda):
    ok = [Problem(1, 6, 10, 32, 64, cuda, 5), Problem(1, 3, 5, 32, 64, cuda, 6)]
    bad = {'residual': Problem(1, 6, 10, 32, 64, cuda, 7, res=True), 'Cout = 96': Problem(1, 6, 10, 32, 96, cuda, 8),
           'Cin = 48': Problem(1, 6, 10, 48, 64, cuda, 9)}
    cases = {'n = 1': ok[:1], 'n = 7': [ok[0]] * 7}
    cases.update({k: [ok[0], p] for k, p in bad.items()})
    for what, probs in cases.items():
        outs = [p.out_buffer() for p in probs]
        rc = stlib.st_conv3x3_wino_group(group_array([p.desc(o) for p, o in zip(probs, outs)]), len(probs),
                                         _lib.current_stream())
        torch.cuda.synchronize()
        assert rc == -1, f'{what}: accepted'
        assert b'winograd group' in stlib.st_last_error(), what
        assert all(torch.all(o == GUARD) for o in outs), f'{what}: refused but something was launched'
    assert stlib.st_conv3x3_wino_group(None, 2, None) == -1
    # the same two layers that were refused next to a bad one do run together
    outs = [p.out_buffer() for p in ok]
    check(stlib.st_conv3x3_wino_group(group_array([p.desc(o) for p, o in zip(ok, outs)]), 2, _lib.current_stream()))
    torch.cuda.synchronize()
    for p, o in zip(ok, outs):
        assert_close(p.check_output(o, 'pair'), ref_conv(p.x, p.w, p.b, 1, 1, 1))


# ---- st_head_pred ----------------------------------------------------------------------------------------------------
class HeadLevel:
    """One level: both tower outputs as channel slices [cls | reg] of ONE wider buffer (ld = 2 feat + 8, the way the plan
    keeps [cls_feat0 | reg_feat0]), or as two tensors of their own; head rows pre-filled with GUARD, 3 rows past M.
    Buffers come from the ambient guard_memory session, as for Problem."""

    def __init__(self, feat, M, dev, seed, shared):
        g = torch.Generator().manual_seed(seed)
        self.mem = guard_memory.current()
        self.M, self.feat = M, feat
        self.xc = torch.randn(M, feat, generator=g) + 1.5          # non-zero mean: a dropped lane or channel quad shows
        self.xr = torch.randn(M, feat, generator=g) - 1.0
        self.wc = torch.randn(1, feat, 1, 1, generator=g) / feat ** 0.5
        self.wr = torch.randn(5, feat, 1, 1, generator=g) / feat ** 0.5
        self.bc, self.br = torch.randn(1, generator=g), torch.randn(5, generator=g)
        if shared:
            ld = 2 * feat + 8
            buf = torch.randn(M, ld, generator=g) * 5.0
            buf[:, 4:4 + feat], buf[:, 4 + feat:4 + 2 * feat] = self.xc, self.xr
            self.cls = self.reg = self.mem.input(buf, dev, 4, 2 * feat)
            self.cls_ld = self.reg_ld = ld
            self.cls_off, self.reg_off = 4, 4 + feat
        else:
            self.cls = self.mem.input(self.xc, dev)
            self.reg = self.mem.input(self.xr, dev)
            self.cls_ld = self.reg_ld = feat
            self.cls_off = self.reg_off = 0
        (wcp, bcp), (wrp, brp) = pack(self.wc, self.bc), pack(self.wr, self.br)
        self.wcp, self.bcp, self.wrp, self.brp = wcp.to(dev), bcp.to(dev), wrp.to(dev), brp.to(dev)
        self.dev = dev

    def rows(self):
        return self.mem.output((self.M + 3, 8), self.dev, GUARD)

    def level(self, out):
        return StHeadPredLevel(self.cls.data_ptr(), self.cls_ld, self.cls_off, self.reg.data_ptr(), self.reg_ld,
                               self.reg_off, self.wcp.data_ptr(), self.bcp.data_ptr(), self.wrp.data_ptr(),
                               self.brp.data_ptr(), out.data_ptr(), self.M)

    def ref64(self):
        c = self.xc.double() @ self.wc.double().view(1, -1).t() + self.bc.double()
        r = self.xr.double() @ self.wr.double().view(5, -1).t() + self.br.double()
        return torch.cat([c, r], 1)

    def unfused(self, lib):
        """The pair of st_conv2d_nhwc launches the plan uses when the fused launch does not apply (feat 192, several
        classes): 1x1, no activation, into the same 8-float rows."""
        out = self.rows()
        for src, ld, off, wp, bp, cout, col in ((self.cls, self.cls_ld, self.cls_off, self.wcp, self.bcp, 1, 0),
                                                (self.reg, self.reg_ld, self.reg_off, self.wrp, self.brp, 5, 1)):
            d = StConvDesc()
            d.in_dev = src.data_ptr(); d.N, d.Hi, d.Wi, d.Cin, d.in_ld, d.in_off = 1, 1, self.M, self.feat, ld, off
            d.wgt_dev, d.bias_dev = wp.data_ptr(), bp.data_ptr()
            d.Cout, d.KH, d.KW, d.stride, d.pad = cout, 1, 1, 1, 0
            d.out1_dev = out.data_ptr(); d.out1_ld, d.out1_off, d.split = 8, col, cout
            d.post_scale, d.act = 1.0, 0
            check(lib.st_conv2d_nhwc(C.byref(d), _lib.current_stream()), 'st_conv2d_nhwc')
        return out


def levels_array(levels, outs):
    arr = (StHeadPredLevel * 3)()
    for i, (L, o) in enumerate(zip(levels, outs)):
        arr[i] = L.level(o)
    return arr


@pytest.mark.parametrize('feat,Ms,shared', [
    (96, (15, 8, 1), True),            # every level under 32 pixels: one workgroup each, partial pixel groups
    (128, (33, 15, 1), True),          # 33 = one pixel into a second workgroup's share
    (256, (1, 33, 8), False),          # the smallest level first; towers in tensors of their own
    (128, (240, 60, 15), True),        # 12x20 / 6x10 / 3x5 maps of a 96x160 input
    (256, (33, 33, 33), True),
    (96, (2772, 693, 165), False),     # 3 x (28x44 | 14x22 | 7x11): odd maps, N = 3
    (128, (8 * 14720, 8 * 3680, 8 * 920), True),   # the shipped geometry: 2048-workgroup budget split 1560 : 390 : 98
])
def test_head_pred_matches_fp64_and_the_unfused_convs(feat, Ms, shared, stlib, cuda):
    levels = [HeadLevel(feat, M, cuda, 31 * feat + M + l, shared) for l, M in enumerate(Ms)]
    outs = [L.rows() for L in levels]
    check(stlib.st_head_pred(levels_array(levels, outs), feat, 1, _lib.current_stream()), 'st_head_pred')
    torch.cuda.synchronize()
    for l, (L, o) in enumerate(zip(levels, outs)):
        got = o.cpu()
        assert torch.all(got[:L.M, 6:] == GUARD), f'level {l}: wrote the padding floats of a head row'
        assert torch.all(got[L.M:] == GUARD), f'level {l}: wrote rows past M'
        ref = L.ref64()
        assert_close(got[:L.M, :6], ref)
        two = L.unfused(stlib)
        torch.cuda.synchronize()
        assert_close(got[:L.M, :6], two.cpu()[:L.M, :6].double(), tol=2e-5)


def test_head_pred_refuses_other_heads(stlib, cuda):
    for feat, nc in ((128, 2), (192, 1), (64, 1)):
        levels = [HeadLevel(feat, 15, cuda, feat + l, True) for l in range(3)]
        outs = [L.rows() for L in levels]
        assert stlib.st_head_pred(levels_array(levels, outs), feat, nc, _lib.current_stream()) == -1, (feat, nc)
        assert b'head_pred' in stlib.st_last_error()
        torch.cuda.synchronize()
        assert all(torch.all(o == GUARD) for o in outs)
    levels = [HeadLevel(128, 15, cuda, l, True) for l in range(3)]
    outs = [L.rows() for L in levels]
    arr = levels_array(levels, outs)
    arr[1].M = 0
    assert stlib.st_head_pred(arr, 128, 1, _lib.current_stream()) == -1          # an empty level
    arr[1].M, arr[2].reg_off = 15, 128 + 12
    assert stlib.st_head_pred(arr, 128, 1, _lib.current_stream()) == -1          # slice runs past its row
    torch.cuda.synchronize()
    assert all(torch.all(o == GUARD) for o in outs)
    assert stlib.st_head_pred(None, 128, 1, None) == -1
