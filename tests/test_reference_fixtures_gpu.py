"""GPU: the kernels against outputs RECORDED FROM THE REFERENCE'S OWN CODE (tests/golden/reference/, written on a
development machine by tests/golden/make_reference_golden.py; the reference tree itself is never read here).

Every other GPU test holds a kernel to a specification of ours.  Here each kernel meets the reference's recorded
output under exactly the bar its existing test applies against our specification; the bar is quoted at the assertion
and named by the test it comes from.  tests/test_cpu_reference_fixtures.py holds the specifications themselves to the
same files."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import aflink_cases  # noqa: E402
import aflink_ref  # noqa: E402
import depth_methods_ref as R  # noqa: E402
import guard_memory as gm  # noqa: E402
import tracklets_ref as tr  # noqa: E402
from kalman_ref import LoopKalmanFilter  # noqa: E402
from stereotracking_amd import _lib  # noqa: E402
from stereotracking_amd._lib import check, current_stream, ptr  # noqa: E402
from stereotracking_amd.aflink import AppearanceFreeLink  # noqa: E402
from stereotracking_amd.batched_assoc import BatchedGpuTracker  # noqa: E402
from stereotracking_amd.tracklets import InterpolateTracklets  # noqa: E402
from tracker_state_utils import run_states, state_differences  # noqa: E402

pytestmark = pytest.mark.gpu
REF_DIR = os.path.join(HERE, 'golden', 'reference')
_FAMILIES = {}


def family(name):
    if name not in _FAMILIES:
        with np.load(os.path.join(REF_DIR, name + '.npz')) as z:
            _FAMILIES[name] = {k: z[k] for k in z.files}
    return _FAMILIES[name]


def by_frame_then_id(rows):
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))]


# ================================================================================================================= depth
def depth_inputs(tag, cuda, rows_past_count=0):
    """One recorded map as (1, 3, H, W) (planes 1 and 2 unread) + its boxes, padded by rows the count excludes."""
    z = family('depth')
    disp, boxes = z[f'{tag}/disp'], z[f'{tag}/boxes']
    k = len(boxes)
    padded = np.concatenate([boxes, np.tile(np.float32([[5, 5, 60, 60]]), (rows_past_count, 1))])[None]
    dev_map = gm.device_planes(np.repeat(disp[None, None], 3, 1), cuda)
    return z, dev_map, gm.device_input(padded, cuda), gm.device_input(np.asarray([k], np.int32), cuda), k


def check_box_depth(tag, cuda):
    z, dev_map, boxes, counts, k = depth_inputs(tag, cuda, rows_past_count=5)
    _, _, H, W = dev_map.shape
    M = boxes.shape[1]
    depth, scale, sb = (gm.device_output(s, cuda, -7.0) for s in ((1, M), (1, M), (1, M, 4)))
    check(_lib.load().st_box_depth(ptr(dev_map), 3 * H * W, 1, H, W, ptr(boxes), ptr(counts), M, float(z['baseline']),
                                   float(z['focal_length']), None, 0, current_stream(), ptr(depth), ptr(scale), ptr(sb)))
    torch.cuda.synchronize()
    depth, scale, sb = depth.cpu().numpy()[0], scale.cpu().numpy()[0], sb.cpu().numpy()[0]
    ref_d = z[f'{tag}/values'].astype(np.float32)
    ref_s, ref_sb = z[f'{tag}/postp_scales'], z[f'{tag}/postp_scaled_boxes']
    # the bar of test_stereo_depth_gpu.py::test_box_depth_matches_reference_semantics: decisions exact, floats within
    # 1e-3 * max(1, |ref|), rows past the count zero
    for i in range(k):
        if np.isnan(ref_d[i]):
            assert np.isnan(depth[i]), (tag, i)
        elif ref_d[i] == -1:
            assert depth[i] == -1 and scale[i] == 1.0, (tag, i, depth[i])
        else:
            assert abs(depth[i] - ref_d[i]) <= 1e-3 * max(1.0, abs(ref_d[i])), (tag, i, depth[i], ref_d[i])
    ok = ~np.isnan(ref_s)
    assert np.array_equal(np.isnan(scale[:k]), ~ok)
    assert np.abs(scale[:k][ok] - ref_s[ok]).max() <= 1e-3
    assert np.abs(sb[:k][ok] - ref_sb[ok]).max() <= 1e-3 * max(np.abs(ref_sb[ok]).max(), 1e-30)
    assert np.all(depth[k:] == 0.0) and np.all(scale[k:] == 0.0) and np.all(sb[k:] == 0.0)
    fin = np.isfinite(ref_d) & (ref_d != -1)
    ulps = np.abs(depth[:k][fin].astype(np.float64) - ref_d[fin]) / np.spacing(np.abs(ref_d[fin])).astype(np.float64)
    print(f'st_box_depth {tag}: {int(fin.sum())} estimated boxes, largest distance from the recorded reference '
          f'{ulps.max():.2f} ulp, {int((ref_d == -1).sum())} x -1, {int(np.isnan(ref_d).sum())} x NaN')
    return depth[:k]


@pytest.mark.parametrize('tag', ['small', 'big'])
def test_box_depth_against_the_recorded_reference(tag, cuda):
    """st_box_depth against OCSORT_Disparity.bbox_postp_depth of the reference: the 160 x 256 map with holes and its 48
    boxes (every crafted edge of test_box_depth_matches_reference_semantics) and the 736 x 1280 map with the two
    w > 800 boxes."""
    got = check_box_depth(tag, cuda)
    assert (got == -1).sum() >= 2 and (got > 0).sum() >= 2


def check_depth_method(method, tag, cuda):
    from test_depth_methods_gpu import run_method
    z, dev_map, boxes, counts, k = depth_inputs(tag, cuda, rows_past_count=3)
    gd, gs, gb = run_method(dev_map, boxes, counts, method, float(z['baseline']), float(z['focal_length']))
    gd, gs, gb = gd[0], gs[0], gb[0]
    rd = z[f'{tag}/{method}/values'].astype(np.float32)
    rs = z[f'{tag}/{method}/scales'].astype(np.float32)
    where = f'{tag} {method}'
    # the bar of tests/test_depth_methods_gpu.py::assert_matches, the recorded reference in the restatement's place
    assert np.array_equal(np.isnan(gd[:k]), np.isnan(rd)), f'{where}: NaN decisions differ'
    assert np.array_equal(gd[:k] == -1, rd == -1) and np.array_equal(np.isnan(gs[:k]), np.isnan(rs)), f'{where}: -1 decisions'
    if method in ('median', 'center'):
        assert np.array_equal(gd[:k], rd, equal_nan=True), f'{where}: depth not bit-exact'
        assert np.array_equal(gs[:k], rs, equal_nan=True), f'{where}: scale not bit-exact'
    else:   # fp64 sums in another order: within 1 fp32 ulp; the scale follows the value
        fin = np.isfinite(rd)
        ulps = np.abs(gd[:k][fin].astype(np.float64) - rd[fin]) / np.spacing(np.abs(rd[fin])).astype(np.float64)
        print(f'st_box_depth_method {where}: largest distance from the recorded reference {ulps.max():.2f} ulp')
        assert np.all(np.abs(gd[:k][fin] - rd[fin]) <= np.spacing(np.abs(rd[fin]))), f'{where}: mean beyond 1 ulp'
        est = (rd != -1) & fin
        want = np.where(est, [R.scale_of(v) for v in gd[:k]], rs).astype(np.float32)
        assert np.array_equal(gs[:k], want, equal_nan=True), f'{where}: scale of the value'
    assert np.array_equal(gb[:k], R.scale_bbox(z[f'{tag}/boxes'], gs[:k]), equal_nan=True), f'{where}: scaled boxes'
    assert not gd[k:].any() and not gs[k:].any() and not gb[k:].any(), 'rows past the count are not 0'


@pytest.mark.parametrize('tag', ['small', 'big'])
@pytest.mark.parametrize('method', R.METHODS)
def test_depth_methods_against_the_recorded_reference(method, tag, cuda):
    """st_box_depth_method against extract_depth wrapped by each decorator of depth_extraction_comparison.py."""
    check_depth_method(method, tag, cuda)


def test_box_depth_on_the_recorded_map_is_blind_to_guard_bands(cuda):
    """The small recorded case twice (guard_memory.run_both): as it stands, and between guard bands with NaN in the
    unread planes.  NaN rows are in the contract (an empty corner slice): outputs compared as bits."""
    gm.run_both(check_box_depth, 'small', cuda, finite=False)
    gm.run_both(check_depth_method, 'median', 'small', cuda, finite=False)


# =============================================================================================================== tracker
def tracker_pairs():
    return [str(p) for p in family('tracker')['pairs']]


def tracker_case(pair):
    z = family('tracker')
    stream, cname = pair.split('/')
    return z, z[f'{stream}/detections'], z[f'{stream}/frame_ids'], json.loads(str(z['configs']))[cname]


def device_tracker_run(pair, cuda, max_dets=32, max_tracks=64):
    """One recorded stream through a BatchedGpuTracker of one sequence -> (fixture-layout rows, header, track states).
    Inputs through the ambient guard session, the rows of every step recorded as outputs."""
    _, det, fids, cfg = tracker_case(pair)
    trk = BatchedGpuTracker(1, max_tracks=max_tracks, max_dets=max_dets, device=cuda, **cfg)
    out = []
    for s, fid in enumerate(fids):
        d = det[det[:, 0] == s]
        k = len(d)
        assert k <= max_dets
        dets = np.zeros((1, max_dets, 8), np.float32)
        dets[0, :k, 0:4] = d[:, 1:5]
        dets[0, :k, 4], dets[0, :k, 6], dets[0, :k, 7] = d[:, 5], d[:, 6], d[:, 7]
        rows, ids, n = trk.step(gm.device_input(np.asarray([fid], np.int32), cuda), gm.device_input(dets, cuda),
                                gm.device_input(np.asarray([k], np.int32), cuda))
        m = int(n.cpu()[0])
        gm.current().track(rows[0, :m].clone())
        r, i = rows.cpu().double().numpy()[0], ids.cpu().numpy()[0]
        out += [[s, int(i[j]), *r[j, 0:4], r[j, 4], r[j, 6], r[j, 7]] for j in range(m)]
    hdr, states = trk.sequence_state(0)
    return np.asarray(out, np.float64).reshape(-1, 9), hdr, states


def check_tracker_rows(pair, cuda):
    from test_batched_assoc_gpu import assert_same_bits
    z = family('tracker')
    got, hdr, states = device_tracker_run(pair, cuda)
    # the bar of tests/test_batched_assoc_gpu.py (assert_same_bits): ids per step, then every row bit for bit
    assert_same_bits(got, z[f'{pair}/np1/rows'], f'{pair}: device vs the recorded reference tracker')
    return hdr, states


@pytest.mark.parametrize('pair', tracker_pairs())
def test_batched_tracker_rows_and_state_against_the_recorded_reference(pair, cuda):
    """BatchedGpuTracker.step against OCSORTTracker_Disparity.track of the reference, frame by frame: ids, boxes,
    scores, depth and scales on the bits.  Then the per-track state after the last frame: the live ids and the tentative
    flags are the recorded ones; mean and covariance by the rule of tests/test_tracker_state_gpu.py - the device
    evaluates the filter as the loops of the native tracker do, so it is held, field for field on the bits
    (tracker_state_utils.state_differences), to the Python backend driven by tests/kalman_ref.LoopKalmanFilter on the
    recorded stream - and to the RECORDED mean and covariance within rtol 1e-9 / atol 1e-9 and rtol 1e-9 / atol 1e-12,
    the bar of test_cpu_tracker_oracle.py::test_product_tracker_reproduces_the_oracle_frame_by_frame."""
    z, det, fids, cfg = tracker_case(pair)
    hdr, states = check_tracker_rows(pair, cuda)
    ids = z[f'{pair}/np1/ids']
    assert hdr['n_tracks'] == len(ids) and hdr['status'] == 0
    assert [t['id'] for t in states] == ids.tolist()
    assert [bool(t['tentative']) for t in states] == z[f'{pair}/np1/tentative'].tolist()
    loop = run_states(det, fids, cfg, 'python', LoopKalmanFilter())[-1][3]
    diff = state_differences(states, loop)
    assert not diff, f'{pair}: {len(diff)} fields differ from the loop-filter tracker\n' + '\n'.join(diff[:12])
    means = np.asarray([t['mean'] for t in states], np.float64).reshape(-1, 8)
    covs = np.asarray([t['cov'] for t in states], np.float64).reshape(-1, 8, 8)
    want_m, want_c = z[f'{pair}/np1/means'], z[f'{pair}/np1/covs']
    # the recorded state itself: the bar that holds loop-form to numpy-form Kalman state in
    # test_cpu_tracker_oracle.py::test_product_tracker_reproduces_the_oracle_frame_by_frame
    assert means.shape == want_m.shape and covs.shape == want_c.shape
    for tid, m, c, wm, wc in zip(ids, means, covs, want_m, want_c):
        assert np.allclose(m, wm, rtol=1e-9, atol=1e-9), f'{pair}: mean of track {tid} is off the recorded reference'
        assert np.allclose(c, wc, rtol=1e-9, atol=1e-12), f'{pair}: covariance of track {tid} is off the recorded reference'
    scale = np.sqrt(np.einsum('nii,njj->nij', want_c, want_c))
    print(f'{pair}: device state vs the recorded reference: largest |cov - ref| / sqrt(P_ii P_jj) '
          f'{(np.abs(covs - want_c) / scale).max():.3e}, largest |mean - ref| {np.abs(means - want_m).max():.3e}')


def test_batched_tracker_on_a_recorded_stream_is_blind_to_guard_bands(cuda):
    gm.run_both(check_tracker_rows, 'occlusion/defaults', cuda)


# ============================================================================================================= tracklets
@pytest.mark.parametrize('mm', ['5_20', '2_4'])
def test_tracklet_interpolate_equals_the_recorded_reference(mm, cuda):
    """st_tracklet_interpolate against InterpolateTracklets.forward of the reference on every linear scenario: equality,
    after ordering the reference's rows by (frame, id) (its own order is an unstable argsort on the frame)."""
    z = family('tracklets')
    names = [str(n) for n in z['linear_names'] if str(n).split('/')[1] == mm]
    mn, mx = (int(v) for v in mm.split('_'))
    assert len(names) == 5
    got = InterpolateTracklets(mn, mx, backend='device').forward_many([z[n + '/rows'] for n in names], device=cuda)
    for n, g in zip(names, got):
        want = by_frame_then_id(z[n + '/out'])
        assert g.shape == want.shape and g.dtype == want.dtype and np.array_equal(g, want), n


def test_tracklet_gsi_against_the_recorded_reference(cuda):
    """st_tracklet_gsi on the rows the reference smoothed: frames, ids and scores equal the recorded ones; the smoothed
    coordinates meet tracklets_ref.gsi_tolerance against the committed truth - the bar of
    tests/test_tracklets_gpu.py::test_gsi_meets_the_truth_tolerance, which the recorded reference output meets too."""
    z, cases = family('tracklets'), tr.gsi_cases()
    for name in (str(n) for n in z['gsi_names']):
        case = cases[name]
        rows, ref_out = z[f'gsi/{name}/rows'], by_frame_then_id(z[f'gsi/{name}/out'])
        out = InterpolateTracklets(use_gsi=True, smooth_tau=int(case['tau']), backend='device').forward_many(
            [rows], device=cuda)[0]
        assert out.shape == ref_out.shape and np.array_equal(out[:, [0, 1, 6]], ref_out[:, [0, 1, 6]])
        tol = tr.gsi_tolerance(case)
        err = float(np.abs(out[:, 2:6].T - case['truth']).max())
        ref_err = float(np.abs(ref_out[:, 2:6].T - case['truth']).max())
        print(f'gsi {name}: device err {err:.3e}, recorded reference err {ref_err:.3e}, tol {tol:.3e}, device vs '
              f'recorded {float(np.abs(out[:, 2:6] - ref_out[:, 2:6]).max()):.3e}')
        assert err <= tol and ref_err <= tol


# ================================================================================================================ aflink
def test_aflink_run_against_the_recorded_reference(cuda):
    """st_aflink_run (AppearanceFreeLink(backend='device')) against AppearanceFreeLink.forward of the reference with the
    recorded seeded weights.  Bars of tests/test_aflink_gpu.py: the candidates' inputs bit-equal (here: to what the
    reference fed its network); confidences |conf - conf64| <= 4 ref_err + 2^-23 and the threshold decisions equal
    (test_score_of_all_candidates_against_fp64), the decisions here being the recorded reference's; the linked rows
    equal (test_forward_many_equals_the_host...), except the row kept where two linked tracks share a frame, which the
    reference leaves to an unstable sort."""
    z = family('aflink')
    sd = aflink_cases.recipe_state_dict(int(z['seed']))
    sd['classifier.fc2.weight'], sd['classifier.fc2.bias'] = torch.from_numpy(z['fc2_weight']), torch.from_numpy(z['fc2_bias'])
    assert aflink_cases.state_dict_sha256(sd) == str(z['state_dict_sha256'])
    thr = float(z['threshold'])
    link = AppearanceFreeLink(sd, confidence_threshold=thr, backend='device')
    sets = [z[f'set{s}/rows'] for s in range(4)]   # set 3 = set 0 under its own ids
    linked = link.forward_many(sets, device=cuda)
    for s, rows in enumerate(sets):
        stages = link.device_stages([rows], device=cuda)
        x, conf = stages['x'], stages['conf']
        rec = {np.ascontiguousarray(a[:, :3]).tobytes() + np.ascontiguousarray(b[:, :3]).tobytes(): c
               for a, b, c in zip(z[f'set{s}/x1'], z[f'set{s}/x2'], z[f'set{s}/conf'])}
        keys = [np.ascontiguousarray(x[k, 0]).tobytes() + np.ascontiguousarray(x[k, 1]).tobytes() for k in range(len(x))]
        assert len(keys) == len(rec) and set(keys) == set(rec), f'set {s}: gate / transform differ from the reference'
        want = np.asarray([rec[k] for k in keys], np.float32)
        conf64, _ = aflink_ref.scores(sd, x, torch.float64)
        conf32, _ = aflink_ref.scores(sd, x, torch.float32)
        ref_err = float(np.abs(conf32.astype(np.float64) - conf64).max())
        err = float(np.abs(conf.astype(np.float64) - conf64).max())
        print(f'aflink set {s}: {len(x)} pairs, device vs fp64 {err:.3e} = {err / ref_err:.2f} ref_err, device vs recorded '
              f'reference {float(np.abs(conf - want).max()):.3e}')
        assert err <= 4 * ref_err + 2.0 ** -23
        assert np.array_equal(conf >= thr, want >= thr)
        if s == 3:      # the reference relabels by matrix index there: ours = set 0's, ids mapped back
            back = dict(zip(sets[0][:, 1], rows[:, 1]))
            want_rows = linked[0].copy()
            want_rows[:, 1] = [back[i] for i in want_rows[:, 1]]
            assert np.array_equal(linked[3], by_frame_then_id(want_rows))
            continue
        got, ref_rows = linked[s], z[f'set{s}/linked']
        assert got.shape == ref_rows.shape and np.array_equal(got[:, :2], ref_rows[:, :2]), f'set {s}: (frame, id) keys'
        differ = np.flatnonzero((got != ref_rows).any(1))
        assert len(differ) <= len(rows) - len(ref_rows)
        for r in differ:          # a frame two linked tracks share: both choices are input rows of that frame
            frame = rows[rows[:, 0] == got[r, 0]]
            assert all(any(np.array_equal(np.delete(c, 1), np.delete(row, 1)) for c in frame) for row in (got[r], ref_rows[r]))


# =============================================================================================================== loading
@pytest.mark.parametrize('size', ['50x70', '48x72'])
def test_pack_raw_inputs_against_the_recorded_loader(size, cuda):
    """st_pack_raw_inputs against LoadDisparityFromFile._post_processing_v2 of the reference (uint16 codes, 65535 holes):
    bit exact, as tests/test_stereo_depth_gpu.py::test_pack_raw_inputs_matches_reference_pipeline; the padding is 0."""
    from stereotracking_amd.mot import pack_raw_inputs
    z = family('loading')
    code = z[f'{size}/codes']
    h, w = code.shape
    out = pack_raw_inputs(disp_u16=gm.device_input(code[None].view(np.int16), cuda))
    torch.cuda.synchronize()
    disp, mask = out['disp_postp'].cpu().numpy(), out['disp_mask'].cpu().numpy()
    want = z[f'{size}/c3/postp']
    assert disp.shape[:2] == (1, 3) and disp.shape[2] >= h and disp.shape[3] >= w
    for c in range(3):
        assert np.array_equal(disp[0, c, :h, :w].view(np.uint32), want[:, :, c].view(np.uint32))
    assert not disp[:, :, h:].any() and not disp[:, :, :, w:].any()
    assert np.array_equal(mask[0, 0, :h, :w], (code < 65535).astype(np.float32))
