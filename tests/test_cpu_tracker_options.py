"""CPU: the product tracker (native C++ routine and the pure-Python restatement) against the ORACLE tracker across the
option sets and stream shapes of tests/golden/tracker_options.npz: vel_delta_t 0 / 1 / 7, num_tentatives 1 / 5,
num_frames_retain 1 / 2, vel_consist_weight 0 / 1, weight_iou_with_det_scores, a high match_iou_thr; NaN rows as
extract_depth emits them, the area-100 boundary, zero-width boxes, negative coordinates, frame-id gaps, empty frames,
mid-stream frame-0 resets and a one-object stream.  The host tracker is the spec of the batched GPU association
(tests/test_batched_assoc_gpu.py holds the device to the same fixture), so it is held to the oracle here first."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))

from make_golden import (SHIPPED_TRACKER, TRACKER_OPTIONS, nan_detection_row, run_oracle_steps,  # noqa: E402
                         tracker_option_streams)
from stereotracking_amd.motion import KalmanFilter  # noqa: E402
from stereotracking_amd.structures import InstanceData, TrackDataSample  # noqa: E402
from stereotracking_amd.trackers import OCSORTTracker_Disparity  # noqa: E402

FIXTURE = os.path.join(HERE, 'golden', 'tracker_options.npz')
STREAMS = np.load(FIXTURE)['streams'].tolist()
PAIRS = [(s, c) for s in STREAMS for c in TRACKER_OPTIONS]


@pytest.fixture(scope='module')
def golden():
    return np.load(FIXTURE)


class _Model:
    motion = KalmanFilter()


def run_product_steps(det, frame_ids, backend, **cfg):
    """The product tracker over a stream of steps (tests/golden/make_golden.run_oracle_steps' convention: step s feeds
    det[det[:, 0] == s] with frame id frame_ids[s], -1 = no call) -> rows [s, id, box (4), score, depth, scale]."""
    trk = OCSORTTracker_Disparity(backend=backend, **cfg)
    out = []
    for s, fid in enumerate(frame_ids):
        if fid < 0:
            continue
        d = det[det[:, 0] == s]
        smp = TrackDataSample(dict(frame_id=int(fid)))
        smp.pred_det_instances = InstanceData(
            bboxes=torch.from_numpy(d[:, 1:5].copy()), scores=torch.from_numpy(d[:, 5].copy()),
            labels=torch.zeros(len(d), dtype=torch.long), scales=torch.from_numpy(d[:, 7].copy()),
            depth=torch.from_numpy(d[:, 6].copy()))
        r = trk.track(_Model(), None, None, smp)
        for i in range(len(r.instances_id)):
            out.append([s, int(r.instances_id[i]), *r.bboxes[i].tolist(), float(r.scores[i]), float(r.depth[i]),
                        float(r.scales[i])])
    return np.asarray(out, np.float64).reshape(-1, 9)


def assert_rows_equal(got, ref, what):
    """ids exact per step, every float equal (NaN rows: NaN in the same places)."""
    assert got.shape == ref.shape, f'{what}: {got.shape} vs {ref.shape}'
    for s in np.unique(ref[:, 0]):
        a, b = got[got[:, 0] == s], ref[ref[:, 0] == s]
        assert a[:, 1].tolist() == b[:, 1].tolist(), f'{what} step {int(s)}: track ids differ\n{a[:, 1]}\n{b[:, 1]}'
    assert np.array_equal(got, ref, equal_nan=True), f'{what}: boxes / scores / depth / scales differ'


def test_fixture_configs_and_streams_are_the_generators(golden):
    pytest.importorskip('oracle.tracker')     # the generator reads the oracle tracker's Kalman prediction (forks)
    assert json.loads(str(golden['configs'])) == json.loads(json.dumps(TRACKER_OPTIONS, sort_keys=True))
    assert STREAMS == sorted(tracker_option_streams())
    for name, (det, fids) in tracker_option_streams().items():
        assert np.array_equal(golden[f'{name}__detections'], det, equal_nan=True), name
        assert np.array_equal(golden[f'{name}__frame_ids'], fids), name
    assert os.path.getsize(FIXTURE) < 1 << 20


@pytest.mark.parametrize('stream', STREAMS)
def test_fixture_equals_a_live_oracle_run(stream, golden):
    pytest.importorskip('oracle.tracker')     # the reference-tracker restatement stays in the build container
    det, fids = golden[f'{stream}__detections'], golden[f'{stream}__frame_ids']
    for cname, cfg in TRACKER_OPTIONS.items():
        rows, nan_live, sentinel = run_oracle_steps(det, fids, probe=True, **cfg)
        key = f'{stream}__{cname}__'
        assert np.array_equal(rows, golden[key + 'tracks'], equal_nan=True), cname
        assert np.array_equal(nan_live, golden[key + 'nan_live']) and np.array_equal(sentinel, golden[key + 'sentinel'])


@pytest.mark.parametrize('backend', ['native', 'python'])
@pytest.mark.parametrize('stream,cname', PAIRS)
def test_product_tracker_equals_the_oracle_fixture(stream, cname, backend, golden):
    det, fids = golden[f'{stream}__detections'], golden[f'{stream}__frame_ids']
    ref = golden[f'{stream}__{cname}__tracks']
    got = run_product_steps(det, fids, backend, **TRACKER_OPTIONS[cname])
    assert_rows_equal(got, ref, f'{backend} {stream} {cname}')


def test_every_option_set_changes_some_stream(golden):
    """Each option set moves the rows of at least one stream away from the shipped set's: every option has teeth."""
    for cname in TRACKER_OPTIONS:
        if cname == 'shipped':
            continue
        moved = [s for s in STREAMS
                 if not np.array_equal(golden[f'{s}__{cname}__tracks'], golden[f'{s}__shipped__tracks'], equal_nan=True)]
        assert moved, f'{cname} gives the shipped rows on every stream'


def test_streams_reach_the_edges(golden):
    """The streams hold what they claim: NaN rows that live on as confirmed NaN tracks inside association, row scans
    that meet the 1e6 sentinel, area exactly 100 and one ulp above, zero width, negative box sums, frame-id gaps,
    empty frames, mid-stream frame-0 resets and a one-object stream."""
    box, dep, scl = nan_detection_row()
    assert np.isnan(box).all() and np.isnan(dep) and np.isnan(scl)
    nan_det = golden['nan__detections']
    nan_rows = nan_det[np.isnan(nan_det[:, 1:5]).all(1)]
    assert np.isnan(nan_rows[:, 6:8]).all()
    assert (nan_rows[nan_rows[:, 0] == 0, 5] > SHIPPED_TRACKER['init_track_thr']).any()       # confirmed at frame 0
    later = nan_rows[nan_rows[:, 0] > 0, 5]
    assert (later > SHIPPED_TRACKER['init_track_thr']).any() and (later < SHIPPED_TRACKER['init_track_thr']).any()
    ref = golden['nan__shipped__tracks']
    assert np.isnan(ref[ref[:, 0] == 0, 2:6]).all(1).any()                                    # a NaN track is born
    for cname in TRACKER_OPTIONS:
        assert golden[f'nan__{cname}__nan_live'].sum() > 0 and golden[f'nan__{cname}__sentinel'].sum() > 0, cname
    assert golden['nan__shipped__nan_live'].sum() >= 20                     # lives on for many frames (retain 30)
    b = golden['boundary__detections']
    area = (b[:, 3] - b[:, 1]) * (b[:, 4] - b[:, 2])
    assert (area == np.float32(100)).sum() >= 10 and ((area > 100) & (area < np.float32(100.001))).sum() >= 10
    assert (b[:, 3] == b[:, 1]).any() and (b[:, 1:5].sum(1) < 0).any() and (b[:, 1] < 0).any()
    assert (golden['gaps__frame_ids'] < 0).sum() >= 5
    er = golden['empty_reset__frame_ids']
    assert (er == 0).sum() == 3
    present = set(golden['empty_reset__detections'][:, 0].astype(int).tolist())
    assert {8, 9, 20, 40} - present == {8, 9, 20, 40}
    single = golden['single__detections']
    assert np.bincount(single[:, 0].astype(int)).max() <= 2
