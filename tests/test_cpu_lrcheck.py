"""CPU: the left-right check of the stereo module - with the numpy restatement alone (tests/lrcheck_ref.py) what makes each
scene able to tell a right kernel from a wrong one; the constructor, the new config and the C entry points' argument
checks.  tests/test_lrcheck_gpu.py runs the same scenes on the device."""
import os

import numpy as np
import pytest

import lrcheck_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort')


def test_shear_is_the_right_view_cost_volume():
    """Rule 2 without aggregation: the sheared left volume equals the cost volume computed with the RIGHT image as the
    reference, cost_R[x'][d] = (1/C) sum_c R[x'][c] L[x'+d][c] (products commute; same c-ascending fmaf chain)."""
    from oracle import c_oracle
    rng = np.random.RandomState(3)
    N, H, W, Cc, D = 1, 2, 21, 8, 12
    fl = rng.normal(0, 1, (N, H, W, Cc)).astype(np.float32)
    fr = rng.normal(0, 1, (N, H, W, Cc)).astype(np.float32)
    VR = R.shear(c_oracle.costvolume(fl, fr, Cc, D))
    # the oracle correlates its first argument at x with the second at x - d: mirror both images in x
    mirrored = c_oracle.costvolume(fr[:, :, ::-1], fl[:, :, ::-1], Cc, D)[:, :, ::-1]
    assert np.array_equal(VR.view(np.uint32), np.ascontiguousarray(mirrored).view(np.uint32))


@pytest.mark.parametrize('shape', R.SCENE_SHAPES)
@pytest.mark.parametrize('lr_max_diff', R.SCENE_MAX_DIFFS)
def test_scene_preconditions(shape, lr_max_diff):
    """Every scene the GPU tests use has valid pixels, pixels that fall by their difference, pixels whose match lies
    outside the right image, and an invalid share between 10 % and 90 %: a kernel that ignores any clause fails on it."""
    sc = R.scene(shape, lr_max_diff)
    valid, by_xr, by_diff = sc['valid'], sc['by_xr'], sc['by_diff']
    assert np.isfinite(sc['dL']).all() and np.isfinite(sc['dR']).all()
    assert valid.any()
    assert by_xr.any()
    if not (tuple(shape) == (4, 12, 16) and lr_max_diff > 1.0):   # twelve columns: both planes agree to within a level
        assert by_diff.any()
    assert np.array_equal(~valid, by_xr | by_diff)
    share = 1.0 - valid.mean()
    assert 0.10 <= share <= 0.90, share
    # rule 5: 0 exactly where the mask is 0, today's value where it is 1
    from oracle import c_oracle
    s = R.SCENE_SCALE
    u = c_oracle.disp_upsample(sc['dL'], s, shape[0] * s, shape[1] * s)
    m = sc['disp_mask'][:, 0] > 0
    assert np.array_equal(sc['disp_postp'][:, 0][m].view(np.uint32), u[:, 0][m].view(np.uint32))
    assert not sc['disp_postp'][:, :, ~m[0]][0].any() and not np.signbit(sc['disp_postp']).any()


def test_equality_scene_flips_exactly_the_pixels_at_the_threshold():
    """lr_max_diff equal to an observed difference: those pixels are valid (the test is <=); at the next float below it
    exactly they fall.  A kernel testing < instead of <= differs on them."""
    V, dL, dR, v, at = R.equality_scene()
    assert at.any() and v > 0
    hi = R.check(dL, dR, R.SCENE_SCALE, v)['valid']
    lo = R.check(dL, dR, R.SCENE_SCALE, np.nextafter(v, np.float32(0)))['valid']
    assert hi[at].all() and not lo[at].any()
    assert np.array_equal(hi & ~lo, at)


def test_check_rule_clauses_on_hand_made_maps():
    dL = np.array([[[0.0, 1.49, 2.5, np.nan, 1.0, np.inf]]], np.float32)
    dR = np.array([[[0.0, 1.0, 9.0, 3.0, 1.25, 0.0]]], np.float32)
    c = R.check(dL, dR, 4, 1.0)
    # x=0: r=0, xr=0, diff 0 -> valid.  x=1: r=1, xr=0, |1.49-0|*4 > 1.  x=2: r=3, xr=-1.  x=3: NaN.  x=4: r=1, xr=3,
    # |1-3|*4 > 1.  x=5: inf.
    assert c['valid'][0, 0].tolist() == [True, False, False, False, False, False]
    assert c['by_xr'][0, 0].tolist() == [False, False, True, False, False, False]
    assert c['by_diff'][0, 0].tolist() == [False, True, False, False, True, False]
    # a NaN on the right side fails the comparison; a huge lr_max_diff leaves only xr < 0 and non-finite pixels invalid
    dRn = dR.copy()
    dRn[0, 0, 0] = np.nan
    assert not R.check(dL, dRn, 4, 1e9)['valid'][0, 0, 0]
    assert R.check(dL, dR, 4, 1e9)['valid'][0, 0].tolist() == [True, True, False, False, True, False]


@pytest.mark.parametrize('bad', [-1.0, -0.0001, float('nan'), float('inf'), 'x', None])
def test_constructor_refuses_bad_lr_max_diff(bad):
    from stereotracking_amd.stereo import StereoCostVolume
    with pytest.raises(ValueError, match='lr_max_diff'):
        StereoCostVolume(lr_check=True, lr_max_diff=bad)


def test_default_module_has_the_check_off_and_the_positional_order_is_kept():
    from stereotracking_amd.stereo import StereoCostVolume
    m = StereoCostVolume()
    assert m.lr_check is False and m.lr_max_diff == 1.0
    m = StereoCostVolume(64, 4, 16.0, 1, 1, False, 8, 64, True, 0.0)     # appended after feat_channels
    assert m.lr_check is True and m.lr_max_diff == 0.0 and m.agg_layers == 1 and m.agg3d_layers == 1
    assert m.param_table() == StereoCostVolume(64, 4, 16.0, 1, 1).param_table()     # the check has no parameters


def test_lrcheck_config_parses_and_builds_the_shell():
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    cfg = Config.fromfile(os.path.join(CFG_DIR, 'stereo_yolox_s_mot_airdrone_costvolume_lrcheck.py'))
    base = Config.fromfile(os.path.join(CFG_DIR, 'stereo_yolox_s_mot_airdrone_costvolume.py'))
    assert cfg.model.stereo.type == 'StereoCostVolume' and cfg.model.stereo.lr_check is True
    assert cfg.model.stereo.lr_max_diff == 4.0
    assert {k: v for k, v in cfg.model.stereo.items() if not k.startswith('lr_')} == dict(base.model.stereo)
    assert cfg.model.detector == base.model.detector and cfg.model.tracker == base.model.tracker
    model = MODELS.build(cfg.model)
    assert model.stereo.lr_check is True and model.stereo.lr_max_diff == 4.0
    assert model.stereo.lr_max_diff == model.stereo.feat_stride        # one level
    assert MODELS.build(base.model).stereo.lr_check is False
    assert sorted(model.state_dict()) == sorted(MODELS.build(base.model).state_dict())


def test_entry_points_check_their_arguments_before_touching_the_device(stlib):
    """Both calls validate first: null pointers, a negative or NaN lr_max_diff and an output that is not scale x the
    level map are refused with ST_ERR_INVALID and a message naming the entry point."""
    import ctypes as C
    one = C.c_void_p(16)
    assert stlib.st_softargmin_right(None, 1, 1, 1, 16, 1.0, None, None) != 0
    assert b'st_softargmin_right' in stlib.st_last_error()
    assert stlib.st_softargmin_right(one, 1, 1, 0, 16, 1.0, one, None) != 0
    assert stlib.st_lr_check_pack(None, None, 1, 1, 1, 4, 4, 4, 4, 4, 1.0, None, None, None) != 0
    assert b'st_lr_check_pack' in stlib.st_last_error()
    for bad in (-1.0, float('nan')):
        assert stlib.st_lr_check_pack(one, one, 1, 1, 1, 4, 4, 4, 4, 4, bad, one, None, None) != 0
        assert b'lr_max_diff' in stlib.st_last_error()
    assert stlib.st_lr_check_pack(one, one, 1, 1, 1, 4, 4, 5, 4, 4, 1.0, one, None, None) != 0
    assert stlib.st_lr_check_pack(one, one, 1, 1, 1, 4, 4, 4, 5, 4, 1.0, one, None, None) != 0
