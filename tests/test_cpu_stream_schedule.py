"""CPU: the bookkeeping of the stream-schedule harness (tests/stream_schedule.py, tests/test_stream_schedule_gpu.py).

 - the header parse finds the stream parameter of every export the binding declares;
 - COVER assigns every stream-taking export the package calls to the scenario of the GPU file that forces its
   ordering (that file asserts the Recorder really saw it there); a new stream-taking export the package calls and
   COVER lacks fails HERE;
 - the wrapper mechanics on a fake handle: restore on exit, the position of the stream argument, the refusal of the
   legacy stream and of a stream that is not the current one."""
import ctypes as C

import pytest

import stream_schedule as ss
from stereotracking_amd import _lib

# entry points that wait for the device BY CONTRACT: no delayed run, no non-blocking assertion
EXEMPT = {
    'st_detector_autotune': 'times kernels between events and synchronises by design (engine.HipDetector.autotune)',
    'st_batched_tracker_get_states': 'copies the track states to the host and synchronises by contract '
                                     '(include/stereotrack.h section 8)',
}

# stream-taking exports the package never calls: inside the product they are internal launches of st_detector_forward*
INTERNAL = ('st_conv3x3_wino_group', 'st_conv1x1_chain', 'st_conv3x3s2_csp_front', 'st_conv3x3_csp_tail',
            'st_focus_pack', 'st_stem_focus_conv', 'st_stem_focus_conv_u8', 'st_spp_pool', 'st_head_pred')

# entry point -> the scenario of tests/test_stream_schedule_gpu.py that calls it under delays
COVER = {
    # P: InflightPipelines.submit
    'st_detector_forward': 'P/mono',
    'st_decode_nms': 'P/mono',
    'st_box_depth': 'P/mono',
    'st_detector_forward_phase': 'P/costvolume_lrcheck',
    'st_conv2d_nhwc_variant': 'P/costvolume_lrcheck',
    'st_softargmin': 'P/costvolume_lrcheck',
    'st_softargmin_right': 'P/costvolume_lrcheck',
    'st_lr_check_pack': 'P/costvolume_lrcheck',
    'st_sgbm_f32': 'P/sgbm',
    'st_costvolume_softargmin': 'P/costvolume',
    'st_disp_upsample_pack': 'P/costvolume',
    'st_volume_agg3d': 'P/costvolume_agg3d',
    'st_conv2d_nhwc': 'P/fullres_agg3d',
    'st_feat_upsample': 'P/fullres_agg3d',
    'st_costvolume_agg3d': 'P/fullres_agg3d',
    'st_costvolume_agg3d_softargmin': 'P/fullres_single_kernel',
    'st_box_depth_method': 'P/median_depth',
    # Q: a sequence.py run through the RawFrameUploader's copy stream
    'st_pack_raw_inputs': 'Q/packed',
    # E: single-stream users on a side stream
    'st_pack_raw_frames': 'E/datasets',
    'st_resize_planes': 'E/datasets',
    'st_mot_similarity': 'E/mot_eval',
    'st_mot_walk': 'E/mot_eval',
    'st_mot_hota_match': 'E/mot_eval',
    'st_mot_hota_accumulate': 'E/mot_eval',
    'st_mot_kitti_preprocess': 'E/kitti',
    'st_mot_challenge_preprocess': 'E/motchallenge',
    'st_mot_file_round': 'E/motchallenge',
    'st_coco_prepare': 'E/coco',
    'st_coco_match': 'E/coco',
    'st_coco_accumulate': 'E/coco',
    'st_tracklet_interpolate': 'E/tracklets',
    'st_tracklet_gsi': 'E/tracklets',
    'st_aflink_gate': 'E/aflink',
    'st_aflink_transform': 'E/aflink',
    'st_aflink_score': 'E/aflink',
    'st_aflink_run': 'E/aflink',
    'st_batched_tracker_run': 'E/batched_tracker',
    'st_sgbm_match_f32': 'E/sgbm_stages',
    'st_sgbm_median': 'E/sgbm_stages',
    'st_sgbm_speckle': 'E/sgbm_stages',
    'st_cmc_front_u8': 'E/cmc',
    'st_cmc_front_f32': 'E/cmc',
    'st_cmc_flow': 'E/cmc',
    'st_cmc_mesh_fit': 'E/cmc',
    'st_cmc_fit': 'E/cmc',
    'st_cmc_estimate': 'E/cmc',
    'st_cmc_ecc_front_f32': 'E/cmc',
    'st_cmc_ecc_prepare': 'E/cmc',
    'st_cmc_ecc_step': 'E/cmc',
    # H: the shell's test_step
    'st_detector_forward_raw': 'H/disp/inflight2_queue1',
    'st_pack_records': 'H/disp/inflight2_queue1',
    'st_detector_forward_phase0_raw': 'H/costvolume_lrcheck/inflight2_queue1',
    'st_rectify_remap': 'H/sgbm_rectify/inflight2_queue1',
    'st_sgbm_u8': 'H/sgbm_rectify/inflight2_queue1',
    'st_disp_head_forward': 'H/completion_v2_fused/inflight2_queue1',
    'st_disp_head_resize': 'H/completion_v2_fused/inflight2_queue1',
    'st_disp_fuse': 'H/completion_v2_fused/inflight2_queue1',
    'st_cmc_ecc_front_u8': 'H/disp_ecc/inflight2_queue1',
    'st_cmc_ecc_estimate': 'H/disp_ecc/inflight2_queue1',
    'st_stereo_eval': 'H/sgbm_dispeval/inflight2_queue1',
    # M: MultiStreamTracker
    'st_stream_gather': 'M/step',
    'st_batched_tracker_step': 'M/step',
    'st_stream_unscale': 'M/step',
    'st_stream_record': 'M/step',
    # by contract
    'st_detector_autotune': 'exempt',
    'st_batched_tracker_get_states': 'exempt',
}

# entry points that MAY return after waiting for the device, each with the line that waits or copies synchronously
BLOCKING = {}


def test_header_parse_finds_the_stream_parameter_of_every_binding_entry():
    exports = ss.exports_with_stream()
    assert len(exports) == 75
    # every export of the header that takes a stream is bound, and its stream argument is a void pointer there
    for name, pos in exports.items():
        assert name in _lib._PROTOS, name
        args = _lib._PROTOS[name][1]
        assert pos < len(args) and args[pos] is C.c_void_p, (name, pos)
    # ... and the parse misses none: the binding's view of the same header, by parameter NAME
    with open(ss.HEADER) as f:
        decls = dict(ss._declarations(f.read()))
    for name in _lib._PROTOS:
        assert name in decls, f'{name} is bound but its declaration was not parsed'
        params = decls[name]
        assert len(params) == len(_lib._PROTOS[name][1]) or params == ['void'], (name, params)
        takes = [i for i, p in enumerate(params) if 'st_stream_t' in p]
        assert (takes == [exports[name]]) if name in exports else not takes, name
    # a few positions by hand (first, middle, last argument)
    assert exports['st_conv2d_nhwc'] == 1 and exports['st_conv2d_nhwc_variant'] == 1
    assert exports['st_detector_forward_phase0_raw'] == 8 and exports['st_pack_records'] == 13
    assert exports['st_stream_unscale'] == 5


def test_cover_names_every_stream_entry_point_the_package_calls():
    used = ss.package_used()
    assert len(used) == 66
    assert set(INTERNAL) == set(ss.exports_with_stream()) - set(used)
    assert set(EXEMPT) <= set(used) and len(EXEMPT) == 2
    missing = sorted(set(used) - set(COVER))
    assert not missing, f'stream-taking exports the package calls without a scenario in COVER: {missing}'
    stale = sorted(set(COVER) - set(used))
    assert not stale, f'COVER names exports the package does not call: {stale}'
    for name, where in COVER.items():
        assert (where == 'exempt') == (name in EXEMPT), name
    assert not set(BLOCKING) & set(EXEMPT) and set(BLOCKING) <= set(COVER)
    assert all(isinstance(r, str) and ':' in r for r in BLOCKING.values()), 'every exemption cites file:line'


def test_a_new_stream_export_the_package_calls_fails_the_cover_check(tmp_path):
    """The check above has teeth: a header with one more stream-taking export, named by a package module."""
    header = tmp_path / 'stereotrack.h'
    with open(ss.HEADER) as f:
        header.write_text(f.read() + '\nint st_brand_new(const float* x_dev, int n,\n   st_stream_t stream, float* out);\n')
    pkg = tmp_path / 'pkg'
    pkg.mkdir()
    (pkg / 'new.py').write_text('check(lib.st_brand_new(ptr(x), n, current_stream(), ptr(out)))\n')
    (pkg / '_lib.py').write_text("'st_never_called_elsewhere'\n")
    used = ss.package_used(str(header), str(pkg))
    assert used == {'st_brand_new': 2}
    assert set(used) - set(COVER) == {'st_brand_new'}


# ---- the wrapper on a fake handle ----------------------------------------------------------------------------------
class FakeHandle:
    def __init__(self):
        self.log = []
        self.st_first = lambda *a: self.log.append(('st_first', a)) or 0
        self.st_last = lambda *a: self.log.append(('st_last', a)) or 7
        self.st_other = lambda *a: self.log.append(('st_other', a)) or 0


POSITIONS = {'st_first': 0, 'st_last': 2}


def test_wrapper_restores_the_handle_logs_the_stream_and_refuses_stream_0():
    h = FakeHandle()
    first, last, other = h.st_first, h.st_last, h.st_other
    current = [0x1000]
    with ss.Recorder(h, POSITIONS, current=lambda: current[0]) as rec:
        assert h.st_first is not first and h.st_last is not last and h.st_other is other
        assert h.st_first(C.c_void_p(0x1000), 5) == 0
        assert h.st_last(1, 2, 0x1000) == 7                  # the wrapped function's result comes back
        h.st_other(None)
        assert rec.calls == [('st_first', 0x1000), ('st_last', 0x1000)]
        assert [n for n, _ in h.log] == ['st_first', 'st_last', 'st_other']
        with pytest.raises(ss.StreamViolation, match='legacy'):
            h.st_last(1, 2, None)                            # ctypes passes None as NULL: the legacy stream
        with pytest.raises(ss.StreamViolation, match='legacy'):
            h.st_first(C.c_void_p(0), 5)
        with pytest.raises(ss.StreamViolation, match='not the current stream'):
            h.st_last(0x1000, 2, 0x2000)                     # the stream is argument 2, not argument 0
        current[0] = 0x2000
        assert h.st_last(0x1000, 2, 0x2000) == 7
        with pytest.raises(ss.StreamViolation, match='argument 2'):
            h.st_last(1, 2)
        assert len(h.log) == 4                               # a refused call never reaches the library
        assert rec.entries() == ['st_first', 'st_last'] and rec.streams() == [0, 0x1000, 0x2000]
    assert h.st_first is first and h.st_last is last and h.st_other is other


def test_wrapper_restores_the_handle_when_the_body_raises():
    h = FakeHandle()
    first = h.st_first
    with pytest.raises(RuntimeError):
        with ss.Recorder(h, POSITIONS, current=lambda: 1):
            raise RuntimeError('scenario failed')
    assert h.st_first is first
    with pytest.raises(KeyError):
        ss.Delayed(h, ['st_other'], 1.0, POSITIONS)


def test_delayed_brackets_only_the_chosen_entries():
    """_before / _after run around the chosen entry only, in order: delay + marker, the real call, the query."""
    h = FakeHandle()
    order = []

    class Probe(ss.Delayed):
        def _before(self, name, stream):
            if name in self.delayed:
                order.append(('before', name, stream))
                return 'marker'

        def _after(self, name, token):
            if token is not None:
                order.append(('after', name, token, len(h.log)))

    with Probe(h, ['st_last'], 50.0, POSITIONS) as d:
        d.current = lambda: 0x30
        h.st_first(0x30)
        h.st_last(0, 0, 0x30)
    assert order == [('before', 'st_last', 0x30), ('after', 'st_last', 'marker', 2)]


def test_delay_length_rule():
    assert ss.delay_length(0.0) == 50.0 and ss.delay_length(0.010) == 50.0
    assert ss.delay_length(0.040) == 80.0 and ss.delay_length(1.0) == 500.0


def test_differences_sees_bits_shapes_types_and_missing_paths():
    import numpy as np
    import torch
    a = dict(x=torch.tensor([1.0, float('nan')]), y=[np.arange(3), 2.5], z='s')
    b = dict(x=torch.tensor([1.0, float('nan')]), y=[np.arange(3), 2.5], z='s')
    assert ss.same_results(a, b)                              # a NaN equals itself: bits are compared
    assert ss.differences(dict(x=torch.tensor([0.0])), dict(x=torch.tensor([-0.0]))) == ['.x']
    b = dict(a, y=[np.arange(3).astype(np.int32), 2.5])
    assert ss.differences(a, b) == ['.y[0]']
    assert ss.differences(a, dict(a, w=1)) == ['.w']
    assert ss.differences(dict(a, y=[np.arange(3)]), a) == ['.y.len', '.y[1]']
    assert ss.differences(dict(v=0.0), dict(v=-0.0)) == ['.v']
