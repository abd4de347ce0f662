"""The weight ring of the Winograd kernel (wino_conv.hip: wino_conv3x3_body<.., RING = true>) at the smallest shapes at
which its hand-counted waits can go wrong.

The ring issues a slot's weight load three slots (12 MFMAs) ahead, into named registers, and counts every s_waitcnt
itself: the count in front of a slot is (younger weight loads in flight) + (window-DMA loads issued behind that slot's
load), it differs between the wave that issues 5 window pieces and the three that issue 6, and it runs down to 0 where
the stream ends - in the middle of a chunk for a K tail.  A wrong count reads a register before its load has landed:
wrong numbers on some waves of some launches, so every case is checked against fp64, against the implicit-GEMM kernel,
between the 64- and the 32-cout instance, and between two launches.  Arithmetic is untouched by the schedule: in the
tools build (ST_LIBRARY = the ablation library) every case must also equal the schedule before the ring bit for bit.
"""
import ctypes as C
import os

import pytest
import torch

from stereotracking_amd import _lib
from stereotracking_amd._lib import check
from test_conv_gpu import assert_close, ref_conv, run_conv
from test_head_kernels_gpu import Problem, group_array

pytestmark = pytest.mark.gpu


def ablation_library():
    """The condition the persistent form's (variant 57) check uses: the tools build is the selected library."""
    return 'ablation' in os.path.basename(os.environ.get('ST_LIBRARY', ''))


class parent_schedule:
    """Tools build only: every Winograd launch inside the block runs the K loop as it was before the ring."""

    def __enter__(self):
        os.environ['ST_WINO_SCHED'] = 'parent'

    def __exit__(self, *exc):
        del os.environ['ST_WINO_SCHED']


# cin, cout, (N, H, W), residual, in_ld, in_off
CASES = [
    (16, 32, (1, 5, 5), False, None, 0),        # half a K-chunk: the ring runs past the last step inside the prologue
    (32, 64, (1, 5, 5), False, None, 0),        # one K-chunk, 64 couts: the same
    (64, 64, (1, 9, 17), True, None, 0),        # two chunks: one window DMA in flight over one chunk boundary
    (256, 64, (1, 9, 9), False, None, 0),       # eight chunks: steady state
    (36, 48, (1, 9, 17), False, None, 0),       # K tail, g_last = 1 (Cin % 32 = 4), padded cout block
    (40, 48, (1, 9, 17), False, None, 0),       # K tail, g_last = 1 (Cin % 32 = 8)
    (48, 48, (1, 9, 17), False, None, 0),       # K tail, g_last = 2: the aggregation convs
    (52, 48, (1, 9, 17), False, None, 0),       # K tail, g_last = 3
    (128, 256, (1, 9, 17), False, 160, 32),     # four cout blocks sharing a window, input = a channel slice
    (64, 96, (1, 12, 20), False, None, 0),      # three 32-cout blocks: the CBN = 1 ring
]


@pytest.mark.parametrize('cin,cout,shape,res,in_ld,in_off', CASES)
def test_weight_ring_matches_reference_and_every_other_instance(cin, cout, shape, res, in_ld, in_off, cuda):
    N, H, W = shape
    g = torch.Generator().manual_seed(cin * 1000 + cout + H)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5)
    b = torch.randn(cout, generator=g) * 0.1
    r = torch.randn(N, cout, H, W, generator=g) if res else None
    kw = dict(res=r, post_scale=0.5 if res else 1.0, in_ld=in_ld, in_off=in_off)
    ref = ref_conv(x, w, b, 1, 1, 1, r, 0.5 if res else 1.0)
    got, _ = run_conv(x, w, b, 1, 1, 1, cuda, variant=43, **kw)
    assert_close(got, ref)                                    # fp64 conv2d, 1e-4 of the output scale
    base, _ = run_conv(x, w, b, 1, 1, 1, cuda, variant=4, **kw)
    assert_close(got, base.double(), tol=2e-5)                # the implicit-GEMM kernel on the same packed weights
    again, _ = run_conv(x, w, b, 1, 1, 1, cuda, variant=43, **kw)
    assert torch.equal(again, got), 'two launches of the same case differ'
    narrow = None
    if cout % 64 == 0:                                        # the same layout computed by 32-cout workgroups
        narrow, _ = run_conv(x, w, b, 1, 1, 1, cuda, variant=44, **kw)
        assert torch.equal(narrow, got), 'variant 44 differs from variant 43'
    if ablation_library():
        with parent_schedule():
            before, _ = run_conv(x, w, b, 1, 1, 1, cuda, variant=43, **kw)
            assert torch.equal(before, got), 'variant 43: the ring differs from the schedule before it'
            if narrow is not None:
                before, _ = run_conv(x, w, b, 1, 1, 1, cuda, variant=44, **kw)
                assert torch.equal(before, narrow), 'variant 44: the ring differs from the schedule before it'


def test_weight_ring_grouped_launch_equals_single_launches(stlib, cuda):
    """Six 128 -> 128 problems (12x20, 6x10, 3x5, twice each) through st_conv3x3_wino_group: bit-identical to the six
    single launches (and, in the tools build, to the grouped launch on the schedule before the ring)."""
    maps = [(12, 20), (6, 10), (3, 5)] * 2
    probs = [Problem(1, H, W, 128, 128, cuda, 4000 + 10 * k + H) for k, (H, W) in enumerate(maps)]
    stream = _lib.current_stream()

    def grouped_launch():
        outs = [p.out_buffer() for p in probs]
        check(stlib.st_conv3x3_wino_group(group_array([p.desc(o) for p, o in zip(probs, outs)]), len(probs), stream),
              'st_conv3x3_wino_group')
        torch.cuda.synchronize()
        return [p.check_output(o, f'problem {k} grouped') for k, (p, o) in enumerate(zip(probs, outs))]

    grouped = grouped_launch()
    for k, p in enumerate(probs):
        alone = p.out_buffer()
        d = p.desc(alone)
        check(stlib.st_conv2d_nhwc_variant(C.byref(d), stream, 43), 'variant 43')
        torch.cuda.synchronize()
        assert torch.equal(grouped[k], p.check_output(alone, f'problem {k} alone')), \
            f'problem {k} {p.shape}: grouped launch differs from its own launch'
        assert_close(grouped[k], ref_conv(p.x, p.w, p.b, 1, 1, 1))
    if ablation_library():
        with parent_schedule():
            before = grouped_launch()
        for k in range(len(probs)):
            assert torch.equal(before[k], grouped[k]), f'problem {k}: the ring differs from the schedule before it'
