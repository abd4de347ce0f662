"""GPU: the default per-box depth estimator (csrc/box_depth.hip, box_depth_kernel behind st_box_depth) against its numpy
restatement (tests/depth_methods_ref.py, rules R1-R5 and R14-R19) on the crafted inputs of tests/box_depth_cases.py:
every cnt and segment bound, ties at the bounds, the strict comparisons, every radix level of the 7-rank select, the
window geometry (LDS cache boundary, streamed windows, wraps, clamps) and the scale's clamps.

The -1 and NaN decisions are the restatement's.  Finite depths are within 1 float32 ulp of it (R11: both accumulate
in float64 and round once; only the order of the float64 sum differs).  The scale is exactly scale_of_default of the
DEVICE depth, the scaled boxes are exactly scale_bbox of the device scale, rows past min(count, max_det) are 0.
tests/test_cpu_box_depth_ref.py shows that these inputs notice each of 12 plausible errors."""
import numpy as np
import pytest
import torch

import guard_memory as gm
import box_depth_cases as B
import depth_methods_ref as R

pytestmark = pytest.mark.gpu


def run_default(case, cuda, maps=None, is_depth=None, via_method=False):
    """st_box_depth (or st_box_depth_method with method 0) on a case -> numpy depth (N, M), scale (N, M), boxes."""
    from stereotracking_amd import _lib
    from stereotracking_amd._lib import check, current_stream, ptr
    maps = case.maps if maps is None else maps
    is_depth = case.is_depth if is_depth is None else is_depth
    N, Cc, H, W = maps.shape
    M = case.boxes.shape[1]
    dev_map = gm.device_planes(maps.copy(), cuda)            # channel 0 is the map: the others are never read
    boxes = gm.device_input(case.boxes.copy(), cuda)
    counts = gm.device_input(case.counts.copy(), cuda)
    d = gm.device_output((N, M), cuda, 7.0)                   # poisoned: every row must be written
    s = gm.device_output((N, M), cuda, 7.0)
    b = gm.device_output((N, M, 4), cuda, 7.0)
    base = (-1.0, 1.0) if is_depth else (0.25, 640.0)
    args = (ptr(dev_map), Cc * H * W, N, H, W, ptr(boxes), ptr(counts), M, *base, None, 0, current_stream(), ptr(d),
            ptr(s), ptr(b))
    lib = _lib.load()
    if via_method:
        check(lib.st_box_depth_method(*args, 0), 'st_box_depth_method')
    else:
        check(lib.st_box_depth(*args), 'st_box_depth')
    torch.cuda.synchronize()
    return d.cpu().numpy(), s.cpu().numpy(), b.cpu().numpy()


def assert_case(case, got, ref=None):
    """The kernel's rows against the restatement -> the largest distance of a finite depth, in ulps of the reference."""
    gd_all, gs_all, gb_all = got
    ref = B.reference(case) if ref is None else ref
    worst = 0.0
    for n, (rd, rs, traces) in enumerate(ref):
        k = len(rd)
        gd, gs, gb = gd_all[n, :k], gs_all[n, :k], gb_all[n, :k]
        where = f'{case.name} image {n}'

        def rows(mask):
            return [(int(i), gd[i], rd[i], traces[i][:5]) for i in np.flatnonzero(mask)[:5]]
        bad = (gd == -1) != (rd == -1)
        assert not bad.any(), f'{where}: -1 decisions (box, got, want, (cnt, n, a, b, fallback)): {rows(bad)}'
        bad = np.isnan(gd) != np.isnan(rd)
        assert not bad.any(), f'{where}: NaN decisions: {rows(bad)}'
        fin = np.isfinite(rd) & (rd != -1)
        assert np.isfinite(gd[fin]).all(), f'{where}: {rows(fin & ~np.isfinite(gd))}'
        ulps = np.zeros(k)
        ulps[fin] = np.abs(gd[fin].astype(np.float64) - rd[fin]) / np.spacing(np.abs(rd[fin])).astype(np.float64)
        worst = max(worst, float(ulps.max(initial=0.0)))
        assert not (ulps > 1).any(), f'{where}: beyond 1 ulp: {rows(ulps > 1)}'
        want_s = np.asarray([np.float32(1.0) if t.cnt is None else R.scale_of_default(v) for v, t in zip(gd, traces)],
                            np.float32)
        assert np.array_equal(gs, want_s, equal_nan=True), f'{where}: scale: {rows(~((gs == want_s) | np.isnan(gs)))}'
        assert np.array_equal(gb, R.scale_bbox(case.boxes[n, :k], gs), equal_nan=True), f'{where}: scaled boxes'
        assert np.array_equal(np.isnan(gb).all(axis=1), np.isnan(rd)) and \
            np.array_equal(np.isnan(gb).any(axis=1), np.isnan(rd)), f'{where}: NaN rows of the scaled boxes'
        assert not gd_all[n, k:].any() and not gs_all[n, k:].any() and not gb_all[n, k:].any(), \
            f'{where}: rows past min(count, max_det) are not 0'
    return worst


@pytest.mark.parametrize('builder', B.BUILDERS)
def test_default_estimator_matches_the_restatement(builder, cuda):
    worst = 0.0
    for case in B.cases(builder):
        got = run_default(case, cuda)
        worst = max(worst, assert_case(case, got))
        again = run_default(case, cuda)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), f'{case.name}: two runs differ'
    print(f'\nbox depth default, {builder}: largest distance {worst:.3f} ulp')


def test_method_zero_is_the_default_kernel(cuda):
    case, = B.tie_maps()
    a, b = run_default(case, cuda), run_default(case, cuda, via_method=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize('builder', ['tie_maps', 'near_depth'])
def test_disparity_and_gt_depth_input_agree(builder, cuda):
    """The same depths through both front ends: the disparity maps, and their float32 depths (R1) as a gt-depth map.
    Going from disparity to depth keeps the depths equal by construction (160 / depth would not round-trip); each run
    is held to the one restatement, and their -1 / NaN decisions are the same."""
    case, = B.cases(builder)
    assert not case.is_depth
    depth = case.maps.copy()
    depth[:, 0] = B.depth_maps(case)
    from_disp, from_depth = run_default(case, cuda), run_default(case, cuda, maps=depth, is_depth=True)
    assert_case(case, from_disp)
    assert_case(case, from_depth)
    assert np.array_equal(from_disp[0] == -1, from_depth[0] == -1)
    assert np.array_equal(np.isnan(from_disp[0]), np.isnan(from_depth[0]))
    assert (from_disp[0] > 0).any()


GUARDED = [test_default_estimator_matches_the_restatement, test_method_zero_is_the_default_kernel]
NAN_BY_CONTRACT = GUARDED                                   # a NaN depth is one of the estimator's decisions


# ---- the same entry points over hostile surroundings (tests/guard_memory.py) -------------------------------------------
test_entry_points_are_blind_to_guard_bands = gm.guarded_test(GUARDED, NAN_BY_CONTRACT, doc="""st_box_depth twice on every crafted case (guard_memory.run_both): as it stands, and with the disparity map
    between guard bands of 0xFF bytes and NaN in its planes 1 and 2 (windows that wrap, clamp or touch the last row must
    not leave channel 0).  The hostile run passes the 1-ulp bar against the restatement and equals the friendly run bit
    for bit; bands, maps, boxes and counts are unchanged bytewise.""")
