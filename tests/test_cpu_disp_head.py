"""CPU: the disparity-completion model's host side - parameter tables, config, constructor restrictions, the out_fd
plan's op list, and the conditions the GPU tests' inputs must meet."""
import ctypes as C
import os

import pytest
import torch

import disp_head_ref as ref
from stereotracking_amd import _lib
from stereotracking_amd.engine import HipDetector, HipDispHead

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_V2 = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone_disp_completion_v2.py')
CFG_DISP = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone_disp.py')


@pytest.mark.parametrize('in_channels,channels', [(128, 256), (16, 32), (24, 96)])
def test_param_table_equals_the_helper_state_dict(in_channels, channels):
    table = HipDispHead(1, 4, 4, in_channels, channels).param_table()
    sd = {k: tuple(v.shape) for k, v in ref.RefDispHead(in_channels, channels).state_dict().items()
          if not k.endswith('num_batches_tracked')}
    assert dict(table) == sd and len(table) == len(sd)
    for key in ('dconv1_1.conv.weight', 'dconv1_1.bn.running_var', 'cbam.ChannelGate.mlp.1.weight',
                'cbam.ChannelGate.mlp.3.bias', 'reg.conv.weight', 'reg.conv.bias'):
        assert key in sd
    # the registry module holds the same keys, num_batches_tracked included, so a checkpoint loads strictly
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd import detectors  # noqa: F401
    mod = MODELS.build(dict(type='DispHeadV2', in_channels=in_channels, channels=channels, in_index=0))
    assert set(mod.state_dict()) == set(ref.RefDispHead(in_channels, channels).state_dict())


def test_new_config_parses_and_builds():
    from stereotracking_amd import mot
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    cfg = Config.fromfile(CFG_V2)
    base = Config.fromfile(CFG_DISP)
    assert cfg.model.type == 'OCSORT_Disp_Completion_V2' and cfg.model.detector.backbone['out_fd'] is True
    assert dict(cfg.model.tracker) == dict(base.model.tracker)
    assert dict(cfg.model.detector.test_cfg) == dict(base.model.detector.test_cfg)
    model = MODELS.build(dict(cfg.model))
    assert isinstance(model, mot.OCSORT_Disp_Completion_V2) and isinstance(model, mot.OCSORT_Disparity)
    det = model.detector
    assert det.out_fd and det.head_config() == dict(in_channels=128, channels=256, bn_eps=0.001)
    # the detector's own table is the plain disparity detector's; the head's keys live under disp_head.
    plain = MODELS.build(dict(base.model)).detector
    assert det._table == plain._table
    keys = set(model.state_dict())
    assert 'detector.disp_head.dconv2_1.bn.running_mean' in keys and 'detector.disp_head.reg.conv.bias' in keys
    assert {k for k in keys if not k.startswith('detector.disp_head.')} == set(MODELS.build(dict(base.model)).state_dict())
    assert model._runner_extras() == dict(disp_head=det.head_config())


@pytest.mark.parametrize('kwargs,word', [
    (dict(in_index=-1), 'in_index'), (dict(in_index=1), 'in_index'), (dict(channels=48), 'channels'),
    (dict(in_channels=6), 'in_channels'), (dict(out_channels=2), 'out_channels'),
    (dict(norm_cfg=dict(type='GN', num_groups=8)), 'norm'), (dict(act_cfg=dict(type='ReLU')), 'act'),
    (dict(input_transform='resize_concat'), 'input_transform'), (dict(align_corners=True), 'align_corners')])
def test_unsupported_head_arguments_raise_naming_the_argument(kwargs, word):
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd import detectors  # noqa: F401
    cfg = dict(type='DispHeadV2', in_channels=128, channels=256, in_index=0)
    MODELS.build(dict(cfg))
    with pytest.raises(NotImplementedError, match=word):
        MODELS.build(dict(cfg, **kwargs))


def _old_config_struct():
    class Old(C.Structure):       # StDetectorConfig as it was before out_fd
        _fields_ = _lib.StDetectorConfig._fields_[:-1]
    assert _lib.StDetectorConfig._fields_[-1][0] == 'out_fd'
    return Old


def _descs(lib, handle):
    buf = C.create_string_buffer(512)
    out = []
    for i in range(lib.st_detector_num_ops(handle)):
        assert lib.st_detector_op_desc(handle, i, buf, 512) == 0
        out.append(buf.value.decode())
    return out


@pytest.mark.parametrize('stereo', [0, 1])
def test_out_fd_plan_is_the_old_plan_plus_one_op(stlib, stereo):
    Old = _old_config_struct()
    plain = HipDetector(2, 64, 96, 0.5, 0.33, 1, stereo=bool(stereo), out_fd=False)
    fd = HipDetector(2, 64, 96, 0.5, 0.33, 1, stereo=bool(stereo), out_fd=True)
    want = plain.op_descs()
    assert len(want) == (72 if stereo else 71)      # the plan's op count before out_fd existed
    # a caller compiled against the old struct: the same bytes (out_fd sits in the old tail padding), or a struct_size
    # that stops in front of the field
    for size in (C.sizeof(Old), _lib.StDetectorConfig.out_fd.offset):
        cfg = Old(size, 0.5, 0.33, 1, 2, 64, 96, 1e-3, stereo, stereo, 0)
        h = C.c_void_p()
        assert stlib.st_detector_create(C.cast(C.byref(cfg), C.POINTER(_lib.StDetectorConfig)), C.byref(h)) == 0
        assert _descs(stlib, h) == want
        assert stlib.st_detector_workspace_bytes(h) == stlib.st_detector_workspace_bytes(plain.handle)
        stlib.st_detector_destroy(h)
    got = fd.op_descs()
    assert len(got) == len(want) + 1
    new = [i for i, d in enumerate(got) if d.startswith('avg2')]
    assert len(new) == 1
    i = new[0]
    assert 'disp_stage1.1.final_conv' in got[i - 1] and '+res' not in got[i - 1] and '+res' in want[i - 1]
    assert got[:i - 1] == want[:i - 1] and got[i + 1:] == want[i:]
    assert fd.param_table() == plain.param_table()
    # a tuning plan of the other plan's length is refused as a whole, never applied shifted by one
    with pytest.raises(_lib.StError, match='expected'):
        fd.set_tuning([0] * len(want))
    assert fd.get_tuning() == [-1] * len(got)
    with pytest.raises(_lib.StError, match='expected'):
        plain.set_tuning([0] * len(got))
    assert plain.get_tuning() == [-1] * len(want)


def test_out_fd_without_a_disparity_branch_is_an_error(stlib):
    with pytest.raises(ValueError, match='out_fd'):
        HipDetector(1, 64, 96, 0.5, 0.33, 1, rgb_only=True, out_fd=True)
    cfg = _lib.StDetectorConfig(C.sizeof(_lib.StDetectorConfig), 0.5, 0.33, 1, 1, 64, 96, 1e-3, 0, 0, 1, 1)
    h = C.c_void_p()
    assert stlib.st_detector_create(C.byref(cfg), C.byref(h)) == -1 and b'out_fd' in stlib.st_last_error()
    cfg.rgb_only, cfg.out_fd = 0, 2
    assert stlib.st_detector_create(C.byref(cfg), C.byref(h)) == -1 and b'out_fd' in stlib.st_last_error()
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd import detectors  # noqa: F401
    assert MODELS.build(dict(type='YOLOXCSPDarknet_Disparity_V1_MMYOLO', out_fd=True, widen_factor=0.5,
                             deepen_factor=0.33)).out_fd is True
    # the completion detector needs the flag: the head reads the features it keeps
    from stereotracking_amd.config import Config
    det = dict(Config.fromfile(CFG_V2).model.detector)
    det['backbone'] = dict(det['backbone'], out_fd=False)
    with pytest.raises(ValueError, match='out_fd'):
        MODELS.build(det)


def test_head_create_refuses_bad_configs(stlib):
    h = C.c_void_p()
    good = dict(batch=1, p3_height=4, p3_width=4, in_channels=16, channels=32)
    for bad in (dict(channels=48), dict(in_channels=6), dict(batch=0), dict(p3_width=0)):
        k = dict(good, **bad)
        cfg = _lib.StDispHeadConfig(C.sizeof(_lib.StDispHeadConfig), k['batch'], k['p3_height'], k['p3_width'],
                                    k['in_channels'], k['channels'], 1e-3)
        assert stlib.st_disp_head_create(C.byref(cfg), C.byref(h)) == -1, bad
    cfg = _lib.StDispHeadConfig(8, 1, 4, 4, 16, 32, 1e-3)
    assert stlib.st_disp_head_create(C.byref(cfg), C.byref(h)) == -1 and b'struct_size' in stlib.st_last_error()


@pytest.mark.parametrize('case', ref.CASES)
def test_inputs_of_the_gpu_tests_exercise_both_branches(case):
    """For the seeds the GPU tests use: the fp64 prediction has at least 10 % exact zeros and 10 % positives (ReLU), and
    at least 20 % of the pre-ELU values are negative."""
    c = ref.make_case(*case)
    pred = c['ref64']['pred']
    assert (pred == 0).double().mean() >= 0.10 and (pred > 0).double().mean() >= 0.10
    assert (c['ref64']['pre_elu'] < 0).double().mean() >= 0.20
    g = c['ref64']['gate_scale']
    assert 0.02 < float(g.min()) and float(g.max()) < 0.98 and float(g.std()) > 0.01     # the gate is not saturated
