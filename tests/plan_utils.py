"""Deterministic launch plans for the detector tests (test infrastructure; host code only, no GPU needed).

The detector's fast paths exist only in a TUNED plan (`Op::tuned`, csrc/detector.cpp): the chained resident 1x1 pair
needs both ops tuned to 46, a grouped Winograd launch needs every op of its run tuned to 43 / 44.  An autotuned plan is
whatever the timing search picked on one machine on one day; `forced_tuning` instead derives a tuning vector from the
op SHAPES by the documented applicability rules of each instance (include/stereotrack.h section 1, the `*_applicable`
functions of csrc/), so that a test runs the same plan everywhere and can say beforehand which launches it must see.
"""
import re
from collections import Counter, namedtuple

import torch

from oracle.torch_model import head_to_rows

PlanOp = namedtuple('PlanOp', 'kind k stride N H W cin cout res up split name')

_CONV = re.compile(r'conv k(\d+) s(\d+) N=(\d+)x(\d+) Hi=(\d+) Wi=(\d+) Cin=(\d+) Cout=(\d+)((?: \+\w+)*)  (\S+)$')
_STEM = re.compile(r'stem focus\+conv6x6 s2 input=\d+ N=(\d+) Hi=(\d+) Wi=(\d+) Cin=(\d+) Cout=(\d+)  (\S+)$')
_SPP = re.compile(r'spp_pool N=(\d+) H=(\d+) W=(\d+) C=(\d+)$')
_PRED = re.compile(r'head conv_cls \+ conv_reg \+ conv_obj, 3 levels \((\d+)x(\d+), .*\) N=(\d+) Cin=(\d+)  (\S+)$')

TAPS = ('stage1_rgb', 'stage1_fused', 'stage2', 'stage3', 'stage4', 'p3_inner', 'p3', 'p4', 'p5')


def plan_ops(det):
    """The ops of a HipDetector's launch plan, parsed from st_detector_op_desc: a list of PlanOp
    (kind in {'conv', 'stem', 'spp', 'pred', 'focus'}; N of a conv = images per launch, sub-batch groups not counted)."""
    ops = []
    for text in det.op_descs():
        m = _CONV.match(text)
        if m:
            k, s, n, _, h, w, cin, cout = (int(v) for v in m.groups()[:8])
            flags = m.group(9)
            ops.append(PlanOp('conv', k, s, n, h, w, cin, cout, '+res' in flags, '+up' in flags, '+split' in flags,
                              m.group(10)))
            continue
        m = _STEM.match(text)
        if m:
            n, h, w, cin, cout = (int(v) for v in m.groups()[:5])
            ops.append(PlanOp('stem', 6, 2, n, h, w, cin, cout, False, False, False, m.group(6)))
            continue
        m = _SPP.match(text)
        if m:
            n, h, w, c = (int(v) for v in m.groups())
            ops.append(PlanOp('spp', 0, 1, n, h, w, c, 4 * c, False, False, False, 'spp_pool'))
            continue
        m = _PRED.match(text)
        if m:
            h, w, n, cin = (int(v) for v in m.groups()[:4])
            ops.append(PlanOp('pred', 1, 1, n, h, w, cin, 6, False, False, False, m.group(5)))
            continue
        assert text.startswith('focus_pack'), f'unparsed op description: {text!r}'
        ops.append(PlanOp('focus', 0, 1, 0, 0, 0, 3, 12, False, False, False, 'focus_pack'))
    return ops


# ---- applicability of the special instances, from the op shape alone (every plan tensor is 16-byte aligned with
# ---- channel strides / offsets that are multiples of 4, so only the shape rules of the *_applicable functions remain)
def wino_shape(o):
    """43 (and 44 when Cout % 64 == 0): wino_conv_applicable / wino_shape_ok of csrc/wino_conv.hip."""
    return (o.kind == 'conv' and o.k == 3 and o.stride == 1 and o.cin >= 16 and o.cin % 4 == 0 and
            (o.cout % 32 == 0 or 32 < o.cout < 64) and o.cout % 4 == 0 and not o.split and not o.up)


def direct_shape(o):
    """42: dc_conv_applicable of csrc/direct_conv.hip."""
    return (o.kind == 'conv' and o.k == 3 and o.stride == 1 and o.cin in (32, 48, 64) and o.cout in (32, 48, 64) and
            not o.split and not o.up)


def resident_shape(o):
    """46: pwr_conv_applicable of csrc/pointwise_resident.hip (a split store of the plan is always Cout / 2)."""
    return (o.kind == 'conv' and o.k == 1 and o.stride == 1 and not o.up and
            (o.cin, o.cout) in ((64, 64), (128, 64), (128, 128), (256, 128)))


def streaming_shape(o):
    """41: pw_conv_applicable of csrc/pointwise_conv.hip."""
    return o.kind == 'conv' and o.k == 1 and o.stride == 1 and not o.up and o.cin in (32, 64) and 1 <= o.cout <= 64


# implicit-GEMM tiles of policy T: the LDS-DMA instances, then the tiles of the committed plan; value = the tile's
# cout extent, which must divide the padded Cout (conv_variant_valid of csrc/conv_igemm.hip)
_T_TILES = ((12, 128), (13, 64), (15, 32), (18, 64), (0, 128), (3, 64), (7, 128), (19, 128))


def tile_valid(variant, cout):
    bn = dict(_T_TILES)[variant]
    return ((cout + 31) // 32 * 32) % bn == 0


def forced_tuning(det, policy):
    """A tuning vector for det.set_tuning (one int per op), from the op shapes alone:
      'H'  all -1: the heuristic plan (what autotune=False runs);
      'S'  43 on every Winograd-shaped 3x3, 46 on every resident-shaped 1x1, 41 on the remaining narrow 1x1: the plan
           in which the chained 46 pairs and both grouped Winograd launches of the head happen;
      'T'  the alternates: 42 where the direct 3x3 kernel applies, else 44 (Cout % 64 == 0) / 43 on Winograd shapes;
           every other conv gets an implicit-GEMM tile out of _T_TILES, rotating with the op index over the valid ones
           (the 32-cout tile 15 is valid for every Cout, so there always is one)."""
    assert policy in ('H', 'S', 'T'), policy
    out = []
    for i, o in enumerate(plan_ops(det)):
        v = -1
        if o.kind != 'conv' or policy == 'H':
            pass
        elif policy == 'S':
            v = 43 if wino_shape(o) else 46 if resident_shape(o) else 41 if streaming_shape(o) else -1
        elif direct_shape(o):
            v = 42
        elif wino_shape(o):
            v = 44 if o.cout % 64 == 0 else 43
        else:
            for r in range(len(_T_TILES)):
                cand = _T_TILES[(i + r) % len(_T_TILES)][0]
                if tile_valid(cand, o.cout):
                    v = cand
                    break
        out.append(v)
    return out


def summarise(report):
    """HipDetector.launch_report() -> Counter of LAUNCHES: key '<instance>' for a launch of its own, '<instance>+<r>'
    for a launch that also computed r following ops (its riders); the implicit-GEMM tiles 0..21 count as 'tile', ops
    without an instance (SPP pooling, focus packing) as 'other'.  Every rider must name an earlier op as its owner and
    report the instance that run_ops gives riders (49 behind a 48, the owner's own instance otherwise)."""
    riders = Counter()
    for i, (variant, owner) in enumerate(report):
        assert 0 <= owner <= i, f'op {i} has no launch: owner {owner}'
        if owner != i:
            riders[owner] += 1
            head = report[owner][0]
            assert report[owner][1] == owner and variant == (49 if head == 48 else head), (i, variant, owner, head)
    out = Counter()
    for i, (variant, owner) in enumerate(report):
        if owner != i:
            continue
        name = 'other' if variant < 0 else 'tile' if variant < 40 else str(variant)
        out[name + (f'+{riders[i]}' if riders[i] else '')] += 1
    return out


def oracle_taps(ora, batch, right=None):
    """One forward of an OracleDetector (any dtype) with hooks -> {tap name: (N,C,H,W) tensor} for the names of
    st_detector_tap, plus 'head0..2' = the head rows (N, h*w, 6) per level.  `right`: the right images of a stereo
    context, whose stage-1 features follow the left ones in 'stage1_rgb' (phase 0 runs over 2N images)."""
    got, hooks = {}, []

    def keep(name):
        return lambda mod, inp, out: got.__setitem__(name, out.detach())

    bb, neck = ora.backbone, ora.neck
    for i in (1, 2, 3, 4):
        hooks.append(getattr(bb, f'stage{i}').register_forward_hook(keep('stage1_rgb' if i == 1 else f'stage{i}')))
    hooks.append(bb.stage2.register_forward_pre_hook(lambda mod, inp: got.__setitem__('stage1_fused', inp[0].detach())))
    hooks.append(neck.top_down_layers[1].register_forward_hook(keep('p3_inner')))
    for i in range(3):
        hooks.append(neck.out_layers[i].register_forward_hook(keep(f'p{3 + i}')))
    try:
        with torch.no_grad():
            rows = head_to_rows(*ora(batch))
            taps = dict(got)
            if right is not None:
                taps['stage1_rgb'] = torch.cat([taps['stage1_rgb'], bb.stage1_features(right)], 0)
    finally:
        for h in hooks:
            h.remove()
    for l, r in enumerate(rows):
        taps[f'head{l}'] = r
    return taps
