"""GPU: the device backend of the MOT evaluation (csrc/mot_eval.hip, stereotracking_amd/mot_eval.py) against the host
backend of stereotracking_amd/metrics.py on the same rows (scenarios: tests/mot_eval_cases.py).

Integer outputs must be equal.  Float outputs must agree within 1e-9 * max(1, |ref|): the only operations that are not
bit-equal are fp64 sums of at most about 1e5 terms in [0, 1] taken in another order, an error of at most
N * 2^-53, about 1e-11.  Where the device is specified to be bit-equal (the IoU matrices, HOTA's potential) the
intermediate arrays are compared for equality."""
import numpy as np
import pytest
import torch

import mot_eval_cases as cases
from stereotracking_amd import metrics as M
from stereotracking_amd import mot_eval
from stereotracking_amd.structures import InstanceData, TrackDataSample

pytestmark = pytest.mark.gpu
TOL = 1e-9


def host_intermediates(gt_rows, pred_rows):
    """metrics.hota's pass 1 restated for the check of the intermediates: the IoU matrix of every frame, potential."""
    p = mot_eval.pack_sequences([gt_rows], [pred_rows])
    g, pr = p['gt_rows'], p['pred_rows']
    potential = np.zeros((int(p['seq_ng'][0]), int(p['seq_nt'][0])))
    sims = []
    eps = np.finfo(float).eps
    for f in range(len(p['frame_no'])):
        a = g[p['frame_gt_off'][f]:p['frame_gt_off'][f + 1]]
        b = pr[p['frame_pred_off'][f]:p['frame_pred_off'][f + 1]]
        sim = M.box_iou_xywh(a[:, 2:6], b[:, 2:6])
        sims.append(sim)
        if len(a) and len(b):
            den = sim.sum(0)[None, :] + sim.sum(1)[:, None] - sim
            siou = np.zeros_like(sim)
            m = den > eps
            siou[m] = sim[m] / den[m]
            potential[a[:, 1].astype(int)[:, None], b[:, 1].astype(int)[None, :]] += siou
    return sims, potential


@pytest.mark.parametrize('name', sorted(cases.SCENARIOS))
def test_device_scores_equal_the_host_backend(cuda, name):
    gt, pred = cases.scenario(name)
    ref = cases.host_reference(name)
    packed = mot_eval.pack_sequences(gt, pred)
    got = mot_eval.evaluate_packed(packed, 0.5, device=cuda, return_arrays=True)
    assert packed['videos'] == sorted(ref) and len(got) == len(ref)
    for v, r in zip(packed['videos'], got):
        cases.assert_same_scores(r, ref[v], TOL, where=(name, v))
        sims, potential = host_intermediates(gt.get(v, []), pred.get(v, []))
        assert len(sims) == len(r['arrays']['sim'])
        for f, (a, b) in enumerate(zip(r['arrays']['sim'], sims)):
            assert a.shape == b.shape and np.array_equal(a, b), (name, v, f)
        assert np.array_equal(r['arrays']['hota_potential'], potential), (name, v)


def test_scenario_facts_on_the_device(cuda):
    """What the scenarios are built for, read from the device's own results."""
    r = mot_eval.evaluate_packed(mot_eval.pack_sequences(*cases.scenario('clear_continuity')), 0.5, device=cuda)[0]['clear_identity']
    assert (r['TP'], r['IDSW'], r['Frag'], r['PT'], r['ML']) == (13, 1, 1, 1, 1) and r['MT'] == 2
    packed = mot_eval.pack_sequences(*cases.scenario('empty_kinds'))
    res = dict(zip(packed['videos'], mot_eval.evaluate_packed(packed, 0.5, device=cuda)))
    assert res['mixed']['clear_identity']['IDSW'] == 0 and res['mixed']['clear_identity']['Frag'] == 0
    assert res['zero']['clear_identity']['TP'] == 0 and res['nogt']['clear_identity']['FP'] == 2
    assert res['nopred']['hota']['HOTA_FN'].tolist() == [3.0] * 19 and res['nopred']['hota']['LocA'].tolist() == [1.0] * 19
    t = mot_eval.evaluate_packed(mot_eval.pack_sequences(*cases.scenario('thresholds')), 0.5, device=cuda)[0]
    assert t['clear_identity']['TP'] == 1 and t['hota']['HOTA_TP'].tolist() == [4, 4, 3] + [2] * 6 + [1] + [0] * 9


def test_single_sequence_call_forms(cuda):
    gt, pred = cases.scenario('random_b1')
    ref = cases.host_reference('random_b1')['solo']
    got = dict(clear_identity=M.clear_identity(gt['solo'], pred['solo'], 0.5, backend='device'),
               hota=M.hota(gt['solo'], pred['solo'], backend='device'))
    cases.assert_same_scores(got, ref, TOL)
    other = M.clear_identity(gt['solo'], pred['solo'], 0.85, backend='device')       # iou_thr reaches the device
    href = M.clear_identity(gt['solo'], pred['solo'], 0.85)
    cases.assert_same_scores(dict(clear_identity=other, hota=None), dict(clear_identity=href, hota=None), TOL)
    assert other['TP'] < got['clear_identity']['TP']


def test_frame_above_the_limit_is_refused_naming_the_frame(cuda):
    lim = mot_eval.max_frame_objects()
    assert lim >= 256
    gt, pred = cases.limit_frame(lim + 1)
    packed = mot_eval.pack_sequences(gt, pred)
    assert packed['max_frame_objects'] == lim + 1
    with pytest.raises(ValueError, match=r"video 'limit', frame 2"):
        mot_eval.evaluate_packed(packed, 0.5, device=cuda)


def test_bad_inputs_reach_the_status_word(cuda):
    gt, pred = cases.scenario('random_b3')
    packed = mot_eval.pack_sequences(gt, pred)
    f = int(packed['seq_frame_off'][1]) + 4                      # a frame of video 'b'
    frame = int(packed['frame_no'][f])
    nan = dict(packed, pred_rows=packed['pred_rows'].copy())
    nan['pred_rows'][packed['frame_pred_off'][f] + 1, 4] = np.nan
    with pytest.raises(ValueError, match=rf"non-finite box: video 'b', frame {frame}\b"):
        mot_eval.evaluate_packed(nan, 0.5, device=cuda)
    dup = dict(packed, gt_rows=packed['gt_rows'].copy())
    r = packed['frame_gt_off'][f]
    dup['gt_rows'][r + 2, 1] = dup['gt_rows'][r, 1]             # pack_sequences refuses this; the device must as well
    with pytest.raises(ValueError, match=rf"twice in one frame: video 'b', frame {frame}\b"):
        mot_eval.evaluate_packed(dup, 0.5, device=cuda)
    with pytest.raises(ValueError, match=rf"video 'b', frame {frame}\b"):       # the same without the HOTA stages
        mot_eval.evaluate_packed(nan, 0.5, ('CLEAR', 'Identity'), cuda)


def _fill(metrics, seed0=0):
    """Three videos through process(); the depth filter drops some prediction and ground-truth rows."""
    for video, seed in (('v0', seed0), ('v1', seed0 + 1), ('v2', seed0 + 2)):
        rng = np.random.RandomState(seed)
        base = torch.tensor([[10., 10, 44, 40], [200., 100, 240, 141], [400., 50, 433, 82], [30., 30, 66, 64]])
        for t in range(8):
            boxes = (base + torch.tensor([3.0 * t, 1.0 * t, 3.0 * t, 1.0 * t]) +
                     torch.from_numpy(rng.normal(0, 2.0, (4, 4))).float())
            ids = torch.tensor([0, 1, 2 if t < 4 else 7, 3])
            keep = [0, 1, 2, 3] if t != 5 else [0, 2, 3]
            depth = torch.tensor([20.0, 30.0, 95.0 if t == 2 else 40.0, -1.0 if t == 6 else 50.0])
            s = TrackDataSample(dict(frame_id=t))
            s.pred_track_instances = InstanceData(bboxes=boxes[keep], scores=torch.full((len(keep),), 0.9),
                                                  labels=torch.zeros(len(keep), dtype=torch.long), depth=depth[keep],
                                                  instances_id=ids[keep])
            gt = [dict(instance_id=k, bbox=(base[k] + torch.tensor([3.0 * t, 1.0 * t, 3.0 * t, 1.0 * t])).tolist(),
                       location=[0, 0, 90.0 if (k == 1 and t == 3) else 20.0]) for k in range(4)]
            metrics.process(video, s, gt)
    return metrics


def _assert_results_equal(got, ref):
    assert set(got) == set(ref) == {'per_video', 'combined'}
    assert set(got['per_video']) == set(ref['per_video'])
    for d, r in [(got['combined'], ref['combined'])] + [(got['per_video'][v], ref['per_video'][v]) for v in ref['per_video']]:
        assert set(d) == set(r)
        for k in r:
            if k in cases.INT_KEYS:
                assert d[k] == r[k], (k, d[k], r[k])
            else:
                assert abs(d[k] - r[k]) <= TOL * max(1.0, abs(r[k])), (k, d[k], r[k])


def test_mot_drone_metrics_device_backend_equals_host(cuda):
    ref = _fill(M.MOTDroneMetrics(depth_thr=80)).evaluate()
    m = _fill(M.MOTDroneMetrics(depth_thr=80, backend='device'))
    assert sum(len(v) for v in m.pred.values()) < 3 * (8 * 4 - 1) and sum(len(v) for v in m.gt.values()) < 3 * 8 * 4
    got = m.evaluate()
    _assert_results_equal(got, ref)
    assert ref['combined']['IDSW'] > 0 and 'HOTA' in got['combined'] and 'LocA' in got['combined']
    # without 'HOTA' in the metric list: no HOTA key, and the HOTA stages are not launched
    ref2 = _fill(M.MOTDroneMetrics(depth_thr=80, metric=('CLEAR', 'Identity'))).evaluate()
    before = dict(mot_eval.LAUNCHES)
    got2 = _fill(M.MOTDroneMetrics(depth_thr=80, metric=('CLEAR', 'Identity'), backend='device')).evaluate()
    _assert_results_equal(got2, ref2)
    assert not any(k in got2['combined'] for k in ('HOTA', 'DetA', 'AssA', 'LocA'))
    assert not any('HOTA' in d for d in got2['per_video'].values())
    assert mot_eval.LAUNCHES['st_mot_walk'] == before['st_mot_walk'] + 1
    assert mot_eval.LAUNCHES['st_mot_similarity'] == before['st_mot_similarity'] + 1
    for k in ('st_mot_hota_match', 'st_mot_hota_accumulate'):
        assert mot_eval.LAUNCHES[k] == before.get(k, 0) and before.get(k, 0) > 0


def _raw_outputs(packed, cuda):
    """Every result array of one evaluate_packed call as bytes: the device's intermediates and all result values."""
    parts = []
    for r in mot_eval.evaluate_packed(packed, 0.5, device=cuda, return_arrays=True):
        arr = r['arrays']
        parts += [np.concatenate([s.ravel() for s in arr['sim']] + [np.zeros(0)]).tobytes(), arr['hota_potential'].tobytes(),
                  arr['id_potential'].tobytes(), arr['gt_count'].tobytes(), arr['tr_count'].tobytes()]
        for d in (r['clear_identity'], r['hota']):
            parts += [np.asarray(d[k], dtype=np.float64).tobytes() for k in sorted(d)]
    return b''.join(parts)


def test_two_runs_give_identical_bytes(cuda):
    packed = mot_eval.pack_sequences(*cases.scenario('random_b3'))
    a, b = _raw_outputs(packed, cuda), _raw_outputs(packed, cuda)
    assert len(a) > 10000 and a == b


def _dets(frames_of, t, M_, cuda):
    """The step's tracker input of B sequences (frames_of[b][t]: detection rows, or None = no frame)."""
    B = len(frames_of)
    dets, counts = np.zeros((B, M_, 8), np.float32), np.full(B, -1, np.int32)
    for b in range(B):
        d = frames_of[b][t]
        if d is None:
            continue
        k = len(d)
        dets[b, :k, 0:4] = d[:, 1:5]
        dets[b, :k, 4], dets[b, :k, 6], dets[b, :k, 7] = d[:, 5], d[:, 6], d[:, 7]
        counts[b] = k
    return torch.from_numpy(dets).to(cuda), torch.from_numpy(counts).to(cuda)


def test_sweep_helper_one_batched_run_of_four_sequences(cuda):
    """ONE BatchedGpuTracker of B = 4 on four different drops of a detection stream (one sequence lacks a frame, one
    ends early: n = -1), every step through ONE TrackCollector, the collector handed to evaluate_sweep: equal to the
    host backend on the collected rows.  The stream's boxes are depth-scaled with scales up to 3 and the ground truth
    is in image space, so the scores also show that the collector scales the boxes back: an object detected in nine
    frames of ten is matched (concentric boxes of scale s have IoU 1 / s^2, below 0.5 from s = 1.42 on)."""
    from stereotracking_amd.batched_assoc import BatchedGpuTracker
    T, M_ = 24, 32
    stream, gt = cases.detection_stream_with_gt(seed=51, T=T, K=6)
    frames_of = cases.thinned_streams(stream, T)
    trk = BatchedGpuTracker(4, max_tracks=32, max_dets=M_, device=cuda)
    col = mot_eval.TrackCollector()
    for t in range(T):
        dets, counts = _dets(frames_of, t, M_, cuda)
        rows, ids, n = trk.step(torch.full((4,), t, dtype=torch.int32, device=cuda), dets, counts)
        col.add([t] * 4, rows, ids, n)
    frames, rows, ids, n = col.to_host()
    assert frames.shape == n.shape == (T, 4) and rows.shape == (T, 4, M_, 8) and ids.shape == (T, 4, M_)
    assert n[10, 2] == -1 and (n[18:, 3] == -1).all() and (n[:, 0] >= 0).all()
    assert float(rows[..., 7].max()) > 2.0                                    # scales that matter
    preds = col.prediction_rows()
    assert len(preds) == 4 and not np.any(preds[2][:, 0] == 10) and preds[3][:, 0].max() <= 17
    got = mot_eval.evaluate_sweep(col, gt, 0.5, device=cuda)
    ref = mot_eval.evaluate_sweep(preds, gt, 0.5, backend='host')
    for b in range(4):
        cases.assert_same_scores(got[b], ref[b], TOL, where=b)
    c0 = got[0]['clear_identity']
    assert c0['TP'] > 0.7 * len(gt) and c0['MOTP'] > 0.85, c0
    assert len({(r['clear_identity']['TP'], r['clear_identity']['IDSW']) for r in got}) >= 3
    # per-sequence ground truth: the same scores
    again = mot_eval.evaluate_sweep(col, [gt] * 4, 0.5, device=cuda)
    assert [r['clear_identity'] for r in again] == [r['clear_identity'] for r in got]


def test_sweep_helper_four_tracker_settings(cuda):
    """Four tracker settings on one synthetic detection stream of 24 frames: the device scores of the collected rows
    equal the host backend's on the same rows, and the settings do not all score alike.  The tracker takes ONE option
    set per instance, so different settings cannot share a batch: four instances, their rows scored together as
    B = 4 prediction sets against one ground truth."""
    from stereotracking_amd.batched_assoc import BatchedGpuTracker
    T, M_ = 24, 32
    stream, gt = cases.detection_stream_with_gt(seed=51, T=T, K=6)
    frames_of = cases.thinned_streams(stream, T)[:1]
    settings = [dict(match_iou_thr=0.3, init_track_thr=0.7), dict(match_iou_thr=0.6, init_track_thr=0.7),
                dict(match_iou_thr=0.3, init_track_thr=0.9), dict(match_iou_thr=0.05, init_track_thr=0.4)]
    preds = []
    for opt in settings:
        trk = BatchedGpuTracker(1, max_tracks=32, max_dets=M_, device=cuda, **opt)
        col = mot_eval.TrackCollector()
        for t in range(T):
            dets, counts = _dets(frames_of, t, M_, cuda)
            col.add([t], *trk.step(torch.tensor([t], dtype=torch.int32, device=cuda), dets, counts))
        preds += col.prediction_rows()
    assert len(preds) == 4 and all(len(p) > 20 for p in preds)
    got = mot_eval.evaluate_sweep(preds, gt, 0.5, device=cuda)
    ref = mot_eval.evaluate_sweep(preds, gt, 0.5, backend='host')
    for b in range(4):
        cases.assert_same_scores(got[b], ref[b], TOL, where=b)
    keys = [(r['clear_identity']['TP'], r['clear_identity']['FP'], r['clear_identity']['IDSW']) for r in got]
    assert len(set(keys)) >= 2, keys
