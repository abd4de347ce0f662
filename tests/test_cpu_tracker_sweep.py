"""CPU: the host-side validation of the tracker-option sweep - sweep.grid, BatchedGpuTracker(options=...) and
TrackerSweep before anything is launched.  It relies on st_batched_tracker_create_multi touching no device (its
refusals come before any device call, and the option sets reach the device with the first launch), as
MultiStreamTracker._check_tracker_options relies on st_batched_tracker_create."""
import ctypes as C

import numpy as np
import pytest

from stereotracking_amd import _lib
from stereotracking_amd.batched_assoc import BatchedGpuTracker
from stereotracking_amd.sweep import TrackerSweep, grid, records_to_detections
from stereotracking_amd import records as R

ERR_INVALID = -1          # ST_ERR_INVALID of include/stereotrack.h


def test_grid_order_and_unknown_keys():
    g = grid(dict(vel_delta_t=1), match_iou_thr=[0.1, 0.3], num_tentatives=[1, 2, 3])
    assert len(g) == 6 and all(o['vel_delta_t'] == 1 for o in g)
    assert [(o['match_iou_thr'], o['num_tentatives']) for o in g] == \
        [(0.1, 1), (0.1, 2), (0.1, 3), (0.3, 1), (0.3, 2), (0.3, 3)]           # the last keyword varies fastest
    assert grid() == [{}] and grid(dict(num_tentatives=2)) == [dict(num_tentatives=2)]
    assert grid(dict(num_tentatives=2), num_tentatives=[5]) == [dict(num_tentatives=5)]
    with pytest.raises(ValueError, match='match_iou'):
        grid(match_iou=[0.1])
    with pytest.raises(ValueError, match='retain'):
        grid(dict(retain=3), match_iou_thr=[0.1])


def test_options_of_the_wrong_length_or_name_raise():
    with pytest.raises(ValueError, match='3 option sets for a batch of 4'):
        BatchedGpuTracker(4, max_tracks=8, max_dets=8, device='cuda:0', options=[{}] * 3)
    with pytest.raises(ValueError, match=r'options\[1\].*iou_thr'):
        BatchedGpuTracker(2, max_tracks=8, max_dets=8, device='cuda:0', options=[{}, dict(iou_thr=0.3)])


def test_a_refused_member_is_named():
    """vel_delta_t = 9 > the observation window (ST_TRACK_WINDOW - 1 = 7) in member 2 of 4: refused by the library
    before any device call, the member index in the message; through the C ABI and through the class."""
    opts = [{}, dict(vel_delta_t=7), dict(vel_delta_t=9), {}]
    with pytest.raises(_lib.StError, match=r'member 2: vel_delta_t must be in \[0, 7\]'):
        BatchedGpuTracker(4, max_tracks=8, max_dets=8, device='cuda:0', options=opts)
    lib = _lib.load()
    base = dict(obj_score_thr=0.3, init_track_thr=0.7, weight_iou_with_det_scores=True, match_iou_thr=0.3,
                num_tentatives=3, vel_consist_weight=0.2, vel_delta_t=3, num_frames_retain=10)
    cfgs = (_lib.StTrackerConfig * 3)(*[_lib.tracker_config(**dict(base, **o)) for o in ({}, {}, dict(num_tentatives=0))])
    h = C.c_void_p()
    assert lib.st_batched_tracker_create_multi(cfgs, 3, 8, 8, C.byref(h)) != _lib.ST_OK and not h
    assert b'member 2' in lib.st_last_error()
    assert lib.st_batched_tracker_create_multi(cfgs, 2, 8, 8, C.byref(h)) == _lib.ST_OK and h     # members 0, 1 are fine
    assert lib.st_batched_tracker_state_bytes(h) > 0
    # run refuses before any launch: null pointers (video_of among them), V / F <= 0, a bad frame range
    one = C.c_void_p(8)        # never dereferenced: every call below is refused on its arguments
    args = lambda **kw: [kw.get(k, one) for k in ('frame_ids', 'dets', 'counts', 'video_of')] + \
        [kw.get('V', 1), kw.get('F', 4), kw.get('f_begin', 0), kw.get('f_end', 4)] + [one] * 6 + [None]
    for bad in (dict(video_of=None), dict(dets=None), dict(V=0), dict(F=0), dict(f_begin=-1), dict(f_begin=2, f_end=2),
                dict(f_end=5)):
        assert lib.st_batched_tracker_run(h, *args(**bad)) == ERR_INVALID, bad
    assert lib.st_batched_tracker_run(None, *args()) == ERR_INVALID
    lib.st_batched_tracker_destroy(h)


def video(F=5, m=4, most=3):
    counts = np.full(F, most, np.int32)
    return dict(frame_ids=np.arange(F), dets=np.ones((F, m, 8), np.float32), counts=counts)


def test_tracker_sweep_validation_and_member_order():
    with pytest.raises(ValueError, match='no option sets'):
        TrackerSweep([])
    with pytest.raises(ValueError, match='unknown tracker options'):
        TrackerSweep([dict(thr=1)])
    sweep = TrackerSweep(grid(num_tentatives=[1, 2, 3]), max_dets=3, device='cuda:0')
    with pytest.raises(ValueError, match='no videos'):
        sweep.run()
    with pytest.raises(ValueError, match='4 detections > max_dets = 3'):
        sweep.add_video(**video(most=4))
    with pytest.raises(ValueError, match='5 detections, dets has 4 rows'):
        sweep.add_video(**video(most=5))
    with pytest.raises(ValueError):
        sweep.add_video()
    with pytest.raises(ValueError):
        sweep.add_video(np.zeros((5, 5, 13), np.float32), dets=np.zeros((5, 4, 8), np.float32))
    assert sweep.add_video(**video()) == 0 and sweep.add_video(**video(F=7)) == 1
    V = 2
    members = sweep.members()
    assert members == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]
    assert all(members[k * V + v] == (k, v) for k in range(3) for v in range(V))
    fids, dets, counts, M = sweep._stacked()                    # ragged lengths: padded with count -1
    assert fids.shape == (2, 7) and dets.shape == (2, 7, 3, 8) and M == 3
    assert counts[0].tolist() == [3] * 5 + [-1] * 2 and counts[1].tolist() == [3] * 7


def test_records_to_detections_follows_the_tracker_column_rule():
    """[depth-scaled box, score, label, depth, scale] from a 13-column frame record, the count from the header row, -1
    for batch padding; 8-column records (no scaled box) and an overfull frame are refused."""
    rec = np.arange(3 * 4 * 13, dtype=np.float32).reshape(3, 4, 13)
    rec[:, R.REC_HEADER] = 0
    rec[:, R.REC_HEADER, R.REC_CAP] = 3
    rec[0, R.REC_HEADER, [R.REC_COUNT, R.REC_VALID]] = 2, 1
    rec[2, R.REC_HEADER, [R.REC_COUNT, R.REC_VALID]] = 3, 1
    dets, counts = records_to_detections(rec)
    assert counts.tolist() == [2, -1, 3] and dets.shape == (3, 3, 8)
    assert np.array_equal(dets[..., 0:4], rec[:, 1:, 8:12]) and np.array_equal(dets[..., 4:8], rec[:, 1:, 4:8])
    with pytest.raises(ValueError, match='scaled box'):
        records_to_detections(rec[..., :8])
    rec[2, R.REC_HEADER, R.REC_COUNT] = 4
    with pytest.raises(ValueError, match='4 detections kept'):
        records_to_detections(rec)
