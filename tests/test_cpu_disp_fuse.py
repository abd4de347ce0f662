"""CPU: the depth_source option's host side - refusals before anything is built, the new config, the ABI entry, and the
conditions the inputs of tests/test_disp_depth_source_gpu.py must meet (asserted from numpy alone)."""
import numpy as np
import pytest
import torch

import disp_fuse_inputs as S
from stereotracking_amd import _lib
from stereotracking_amd.config import Config
from stereotracking_amd.registry import MODELS


def _model_cfg(path=S.CFG_V2):
    from stereotracking_amd import mot  # noqa: F401
    return dict(Config.fromfile(path).model, autotune=False)


def test_a_bad_depth_source_raises_value_error():
    for bad in ('dense', 'FUSED', '', None, 2):
        with pytest.raises(ValueError, match='depth_source'):
            MODELS.build(dict(_model_cfg(), depth_source=bad))
    for good in ('input', 'completed', 'fused'):
        assert MODELS.build(dict(_model_cfg(), depth_source=good)).depth_source == good
    assert MODELS.build(_model_cfg()).depth_source == 'input'


def test_the_plain_shell_has_no_head_to_read():
    cfg = _model_cfg(S.CFG_V2.replace('_completion_v2', ''))
    assert MODELS.build(dict(cfg, depth_source='input')).depth_source == 'input'
    with pytest.raises(ValueError, match='depth_source'):
        MODELS.build(dict(cfg, depth_source='fused'))


def test_stereo_eval_map_depth_needs_a_depth_source():
    with pytest.raises(ValueError, match="map='depth'"):
        MODELS.build(dict(_model_cfg(), stereo_eval=dict(map='depth')))
    with pytest.raises(ValueError, match="map='depth'"):
        MODELS.build(dict(_model_cfg(), stereo_eval=dict(map='depth'), depth_source='input'))
    with pytest.raises(ValueError, match='map'):
        MODELS.build(dict(_model_cfg(), stereo_eval=dict(map='completed'), depth_source='fused'))
    m = MODELS.build(dict(_model_cfg(), stereo_eval=dict(map='depth', boxes='gt'), depth_source='fused'))
    assert m.stereo_eval_map == 'depth' and m.stereo_eval['boxes'] == 'gt'
    m = MODELS.build(dict(_model_cfg(), stereo_eval=dict(), depth_source='fused'))
    assert m.stereo_eval_map == 'input' and 'map' not in m.stereo_eval


def test_a_pipeline_with_depth_source_but_no_head_raises():
    from stereotracking_amd.pipeline import StereoDensePipeline, depth_source_code
    for src in ('completed', 'fused'):
        with pytest.raises(ValueError, match='disp_head'):
            StereoDensePipeline(2, S.ORI, stereo=False, depth_source=src)
    with pytest.raises(ValueError, match='depth_source'):
        StereoDensePipeline(2, S.ORI, stereo=False, depth_source='holes', disp_head=dict(in_channels=128, channels=32))
    assert [depth_source_code(k) for k in ('input', 'completed', 'fused')] == [0, 1, 2]


def test_the_sharded_driver_refuses_the_option():
    from stereotracking_amd.sequence import track_gathered
    model = MODELS.build(dict(_model_cfg(), depth_source='fused'))
    with pytest.raises(NotImplementedError, match='depth_source'):
        track_gathered(torch.zeros(1, 2, 8), None, 1, model.tracker, model)


def test_new_config_parses_and_builds():
    from stereotracking_amd import mot
    cfg, base = Config.fromfile(S.CFG_FUSED), Config.fromfile(S.CFG_V2)
    assert cfg.model.depth_source == 'fused' and 'depth_source' not in base.model
    assert {k: v for k, v in dict(cfg.model).items() if k != 'depth_source'} == dict(base.model)
    model = MODELS.build(dict(cfg.model, autotune=False))
    assert isinstance(model, mot.OCSORT_Disp_Completion_V2) and model.depth_source == 'fused'
    assert model._runner_extras() == dict(disp_head=model.detector.head_config(), depth_source='fused')
    assert set(model.state_dict()) == set(MODELS.build(dict(base.model, autotune=False)).state_dict())


def test_abi_declares_the_entry_and_refuses_null_pointers(stlib):
    assert hasattr(stlib, 'st_disp_fuse') and 'st_disp_fuse' in _lib._PROTOS
    assert stlib.st_disp_fuse(None, None, 256, 1, 16, 16, 16, 16, 1, None, None, None) != 0
    assert b'st_disp_fuse' in stlib.st_last_error()


@pytest.mark.parametrize('seeds', [S.SEEDS_SHELL, S.SEEDS_LONG] + list(S.SEEDS_STREAMS), ids=lambda s: f'seeds{s[0]}_{len(s)}')
def test_inputs_of_the_gpu_tests_have_holes_that_matter(seeds):
    """Per frame: every gt box has its centre pixel on a hole; at least one of them keeps a valid pixel (where `center`
    reads 1.6e8 m) and at least one is all hole (where every estimator returns -1); the punch made a difference;
    between 10 % and 90 % of the extent is invalid; the all-valid variant has no hole."""
    fr, whole, valid = S.frames(seeds), S.frames(seeds, holes=False), S.frames(seeds, all_valid=True)
    for t in range(len(seeds)):
        plane, boxes = fr['disp'][t, 0], fr['boxes'][t]
        assert plane.shape == S.ORI and len(boxes) == S.GT_PER_FRAME
        assert (boxes[:, 0] >= 0).all() and (boxes[:, 2] <= S.ORI[1]).all() and (boxes[:, 3] <= S.ORI[0]).all()
        centre_invalid, any_valid = S.box_classes(plane, boxes)
        assert centre_invalid.all() and (centre_invalid & any_valid).sum() >= 1 and (~any_valid).sum() >= 1
        assert S.box_classes(whole['disp'][t, 0], boxes)[0].sum() < len(boxes), 'the holes were there before the punch'
        assert 0.10 <= S.invalid_fraction(plane) <= 0.90, S.invalid_fraction(plane)
        assert S.invalid_fraction(valid['disp'][t, 0]) == 0.0
        assert np.array_equal(fr['disp'][t, 0], fr['disp'][t, 1]) and np.array_equal(fr['disp'][t, 0], fr['disp'][t, 2])
        depth = fr['depth'][t, 0]
        assert np.isfinite(depth).all() and 0 < depth.min() and depth.max() <= 160.0


def test_conditioned_head_weights():
    sd = S.head_weights()
    assert float(sd['reg.conv.bias']) == 8.0 and float(sd['reg.conv.weight'].abs().max()) < 0.05
