"""CPU: known answers of the per-box depth estimators' numpy restatement (tests/depth_methods_ref.py), which
tests/test_depth_methods_gpu.py holds the kernel to, and the validation of the depth_extraction / depth_method option."""
import ctypes as C
import os

import numpy as np
import pytest

import depth_methods_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort')


def _map(values, H=8, W=8, fill=0.0):
    """(H, W) depth map, `values` written row-major from the top-left corner, the rest `fill` (invalid at 0)."""
    d = np.full(H * W, fill, np.float32)
    d[:len(values)] = values
    return d.reshape(H, W)


def test_median_odd_and_even():
    d = _map([5.0, 1.0, 3.0], W=3)
    v, s = R.extract_depth(d, [[0, 0, 3, 1]], 'median')
    assert v[0] == np.float32(3.0)
    d = _map([4.0, 1.0, 2.0, 3.0], W=4)
    v, _ = R.extract_depth(d, [[0, 0, 4, 1]], 'median')
    assert v[0] == np.float32(2.5)
    d = _map([9.0, 0.0, 200.0, 1.0, 3.0, 2.0], W=6)            # invalid pixels are not counted: n = 4
    v, _ = R.extract_depth(d, [[0, 0, 6, 1]], 'median')
    assert v[0] == np.float32(2.5)


def test_truncated_mean_bounds_and_single_pixel_nan():
    vals = np.arange(1, 21, dtype=np.float32)                   # n = 20: s[2:18] = 3..18
    v, _ = R.extract_depth(_map(vals, H=4, W=5), [[0, 0, 5, 4]], 'truncated_mean')
    assert v[0] == np.float32(np.mean(np.arange(3, 19)))
    v, _ = R.extract_depth(_map([7.0, 9.0], W=2), [[0, 0, 2, 1]], 'truncated_mean')
    assert v[0] == np.float32(7.0)                              # n = 2: s[0:1]
    v, s = R.extract_depth(_map([7.0], W=1, H=1), [[0, 0, 1, 1]], 'truncated_mean')
    assert np.isnan(v[0]) and np.isnan(s[0])                    # n = 1: s[0:0], s[:-1] empty -> NaN, scale NaN


def test_mean_is_the_float64_mean():
    vals = np.float32([0.1, 0.2, 0.3, 149.9, 0.0, 150.0, -3.0])  # 0, 150 and negatives are not valid
    v, _ = R.extract_depth(_map(vals, H=1, W=7), [[0, 0, 7, 1]], 'mean')
    assert v[0] == np.float32(np.sum(vals[:4], dtype=np.float64) / 4)


def test_center_reads_the_raw_map_and_wraps():
    d = _map([1.0] * 64)
    d[3, 4] = 500.0                                             # invalid value at the centre is still taken
    v, s = R.extract_depth(d, [[2, 2, 7, 5]], 'center')        # cx = 9 // 2 = 4, cy = 7 // 2 = 3
    assert v[0] == np.float32(500.0) and s[0] == np.float32(3.0)
    d[3, 5], d[3, 6], d[3, 4] = 2.0, 3.0, 4.0
    v, _ = R.extract_depth(d, [[-12, 2, 7, 5]], 'center')      # cx = -5 // 2 = -3 (floor, not -2) -> 5 after the wrap
    assert v[0] == np.float32(2.0)
    v, _ = R.extract_depth(d, [[-12.9, 2, 6.9, 5]], 'center')  # truncation first: (-12 + 6) // 2 = -3, not -4
    assert v[0] == np.float32(2.0)


def test_center_out_of_range_is_the_stated_deviation():
    d = _map([30.0] * 64)
    v, s = R.extract_depth(d, [[0, 0, 8, 30]], 'center')        # cy = 15 >= H: numpy raises IndexError
    assert v[0] == np.float32(-1.0) and s[0] == np.float32(1.0)
    v, s = R.extract_depth(d, [[-30, 0, 4, 4]], 'center')       # cx = -13 -> -5 after one wrap: still out
    assert v[0] == np.float32(-1.0) and s[0] == np.float32(1.0)


@pytest.mark.parametrize('method', R.METHODS)
def test_discard_rules(method):
    d = np.full((4, 900), 10.0, np.float32)
    v, s = R.extract_depth(d, [[0, 0, 801, 4]], method)         # w > 800
    assert v[0] == np.float32(-1.0) and s[0] == np.float32(1.0)
    v, s = R.extract_depth(d, [[0, 0, 800, 4]], method)         # w == 800 is kept
    assert v[0] == np.float32(10.0)
    d[:] = 0.0
    v, s = R.extract_depth(d, [[0, 0, 10, 4]], method)          # no valid pixel
    assert v[0] == np.float32(-1.0) and s[0] == np.float32(1.0)
    v, s = R.extract_depth(d, [[5, 2, 3, 4]], method)           # empty window
    assert v[0] == np.float32(-1.0) and s[0] == np.float32(1.0)


def test_scale_clamps_at_d_20_and_sqrt_1200():
    assert R.scale_of(20.0) == np.float32(1.0)                  # 400 / 400
    assert R.scale_of(10.0) == np.float32(1.0)
    assert R.scale_of(25.0) == np.float32(625.0 / 400.0)
    d = np.float32(34.64)                                       # just below sqrt(1200) = 34.641...
    dd = np.float32(d * d)
    assert R.scale_of(d) == np.float32(float(dd) / 400.0) and R.scale_of(d) < np.float32(3.0)
    assert R.scale_of(np.float32(34.65)) == np.float32(3.0)
    assert R.scale_of(1e20) == np.float32(3.0)                  # d * d overflows to inf in fp32: min(inf, 3.)
    assert np.isnan(R.scale_of(np.nan))


def test_scale_bbox_about_the_centre():
    b = R.scale_bbox([[10, 20, 30, 60]], [2.0])
    assert b.tolist() == [[0.0, 0.0, 40.0, 80.0]]


# ---- the option ------------------------------------------------------------------------------------------------
def test_depth_method_codes_match_the_header():
    from stereotracking_amd.pipeline import DEPTH_METHODS, depth_method_code
    hdr = open(os.path.join(ROOT, 'include', 'stereotrack.h')).read()
    for name, code in DEPTH_METHODS.items():
        assert f'ST_DEPTH_{name.upper()} = {code}' in hdr
        assert depth_method_code(name) == code
    assert set(DEPTH_METHODS) == {'reference', *R.METHODS}
    for bad in ('Median', 'trimmed', '', None, 3):
        with pytest.raises(ValueError, match='unknown depth extraction method'):
            depth_method_code(bad)


def test_model_rejects_an_unknown_depth_extraction():
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.registry import MODELS
    with pytest.raises(ValueError, match='unknown depth extraction method'):
        MODELS.build(dict(type='OCSORT_Disparity', depth_extraction='mode'))
    assert MODELS.build(dict(type='OCSORT_Disparity')).depth_extraction == 'reference'
    for m in R.METHODS:
        assert MODELS.build(dict(type='OCSORT_Disparity', depth_extraction=m)).depth_extraction == m


def test_median_config_parses():
    from stereotracking_amd.config import Config
    cfg = Config.fromfile(os.path.join(CFG_DIR, 'yolox_s_mmyolo_mot_airdrone_disp_median.py'))
    base = Config.fromfile(os.path.join(CFG_DIR, 'yolox_s_mmyolo_mot_airdrone_disp.py'))
    assert cfg.model.depth_extraction == 'median'
    assert 'depth_extraction' not in base.model
    assert cfg.model.tracker == base.model.tracker and cfg.model.detector == base.model.detector


def test_abi_refuses_an_unknown_method(stlib):
    from stereotracking_amd._lib import ST_OK
    p = C.c_void_p(256)       # never dereferenced: the method is checked before anything is launched
    for bad in (-1, 5, 99):
        rc = stlib.st_box_depth_method(p, 64, 1, 8, 8, p, p, 4, 0.25, 640.0, None, 0, None, p, p, p, bad)
        assert rc != ST_OK
        assert b'unknown method' in stlib.st_last_error()
