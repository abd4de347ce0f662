"""The conv kernels over non-finite channel slack and inside guard bands.

Every parity test of test_conv_gpu.py, test_wino_ring_gpu.py and test_head_kernels_gpu.py builds its buffers through
guard_memory's ambient session.  Here each of them runs twice on its OWN case table: as it always has (finite garbage
in the unused channels, plain allocations), and with NaN / +Inf / -Inf in every channel outside the input slice and
the input, the residual and every GUARD-filled output buffer inside an arena of 0xFF bytes (NaN as fp32).  A kernel that
loads past its K tail, outside its channel slice, a halo row before the buffer or a K-chunk past its end and multiplies
by a zero weight or a zero mask computes 0 * NaN = NaN in the second run.

Asserted per case (guard_memory.run_both): every output buffer of the hostile run is finite (GUARD columns included) and
BIT-IDENTICAL to the friendly run's; guard bands, inputs and slack are unchanged bytewise; and the test's own
assertions - fp64 parity at its own tolerance, output guard columns, bit-identity between instances - hold in both.
"""
import pytest
import torch

import guard_memory
import test_conv_gpu as tc
import test_head_kernels_gpu as th
import test_wino_ring_gpu as tw

pytestmark = pytest.mark.gpu

FUNCTIONS = [
    tc.test_conv_matches_torch,                                   # CASES
    tc.test_conv_all_tile_variants,                               # tiles 0..21
    tc.test_conv_pointwise_instances_of_all_tile_variants,        # K tail 72, slice of ld 80
    tc.test_conv_split_stores_whole_tile_and_mixed,
    tc.test_conv_upsampled_store_coordinates,
    tc.test_conv_lds_dma_variants_zero_fill_and_ragged,           # LDS-DMA variants 12, 13, 15, 18
    tc.test_conv_epilogue_residual_scale_split_upsample,
    tc.test_conv_no_act_and_input_slice,
    tc.test_spp_pool_matches_torch_maxpool,                       # st_spp_pool
    tc.test_fused_focus_stem_matches_torch,                       # st_stem_focus_conv (planes 1, 2 NaN when planes = 1)
    tc.test_fused_stem_raw_uint8_frames_equal_pack_then_stem,     # st_stem_focus_conv_u8
    tc.test_pointwise_streaming_kernel_matches_torch,             # 41
    tc.test_chained_pointwise_pair_matches_torch,                 # st_conv1x1_chain
    tc.test_direct_conv3x3_kernel_matches_torch,                  # 42
    tc.test_winograd_conv_matches_direct_convolution,             # 43 / 44
    tc.test_fused_stage1_front_matches_separate_convolutions,     # st_conv3x3s2_csp_front
    tc.test_resident_pointwise_kernel_matches_torch,              # 46
    tc.test_chained_resident_pointwise_pair_matches_torch,
    tc.test_csp_tail_fused_kernel_matches_the_two_launches,       # st_conv3x3_csp_tail
    tw.test_weight_ring_matches_reference_and_every_other_instance,   # Cin 16, 36, 40, 48, 52
    tw.test_weight_ring_grouped_launch_equals_single_launches,
    th.test_grouped_winograd_launch_equals_separate_launches,     # GROUPS
    th.test_head_pred_matches_fp64_and_the_unfused_convs,         # st_head_pred
]


def _runs(fn, kw):
    """Not the one table entry its own test skips: an LDS-DMA tile that does not divide the padded Cout."""
    return fn is not tc.test_conv_lds_dma_variants_zero_fill_and_ragged or tc.lds_dma_tile_divides(kw['variant'], kw['case'][4])


test_kernel_is_blind_to_slack_and_guard_bands = guard_memory.guarded_test(FUNCTIONS, applies=_runs)


@pytest.mark.parametrize('masked', [False, True])
def test_run_both_tells_a_multiplied_load_from_a_masked_one_on_the_device(masked, cuda):
    """The harness on the device, on a stand-in for the bug class (torch ops, not a kernel of the library): a 1x1 conv
    over channels [4, 28) of an ld = 40 buffer that walks a whole 32-wide K-chunk with zero weights behind channel 24.
    Loading the chunk and multiplying passes the friendly run and fails the hostile one; masking the load passes both."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 3, 5, 24, generator=g)
    w = torch.zeros(6, 32)
    w[:, :24] = torch.randn(6, 24, generator=g)

    def conv():
        mem = guard_memory.current()
        buf = torch.randn(1, 3, 5, 40, generator=torch.Generator().manual_seed(2)) * 3.0
        buf[..., 4:28] = x
        xin = mem.input(buf, cuda, 4, 24)
        out = mem.output((1, 3, 5, 6), cuda)
        a = xin[..., 4:36]
        if masked:
            a = torch.where(torch.arange(32, device=cuda) < 24, a, torch.zeros((), device=cuda))
        out.copy_(a @ w.to(cuda).t())

    if masked:
        assert guard_memory.run_both(conv) == 1
    else:
        with pytest.raises(AssertionError, match='non-finite'):
            guard_memory.run_both(conv)


@pytest.mark.parametrize('reads_outside', [False, True])
def test_run_both_sees_a_max_reduction_that_reads_outside_its_map(reads_outside, cuda):
    """Why st_spp_pool's buffers stand between +Inf images (Session.framed): a max over a window that runs one row into
    the next image drops a NaN band but not a +Inf frame."""
    x = torch.randn(2, 4, 5, 3, generator=torch.Generator().manual_seed(3))

    def pool():
        mem = guard_memory.current()
        xin = mem.framed(x, cuda)
        out = mem.output((2, 4, 5, 3), cuda)
        rows = xin.reshape(8, 5, 3)
        if reads_outside and mem.framed_buffers:      # the row after each row; the last map row's comes from the frame
            nxt = mem.framed_buffers[-1][0].reshape(16, 5, 3)[5:13]
        elif reads_outside:                           # friendly run: the model owns nothing behind the map
            nxt = torch.cat([rows[1:], rows[-1:]])
        else:
            nxt = torch.cat([rows[1:4], rows[3:4], rows[5:], rows[-1:]])      # clamped inside each image
        out.copy_(torch.fmax(rows, nxt).reshape(2, 4, 5, 3))                  # fmax drops a NaN, as fmaxf does

    if reads_outside:
        with pytest.raises(AssertionError, match='non-finite'):
            guard_memory.run_both(pool)
    else:
        assert guard_memory.run_both(pool) == 1
