"""CPU: the host side of the device MOT evaluation (stereotracking_amd/mot_eval.py): pack_sequences against hand-written
answers, the `backend` keyword, and the precondition of the GPU tests - on every scenario of tests/mot_eval_cases.py
the host scorer alone does not depend on how assignment ties break."""
import numpy as np
import pytest
import torch

import mot_eval_cases as cases
from stereotracking_amd import metrics as M
from stereotracking_amd import mot_eval
from stereotracking_amd.structures import InstanceData, TrackDataSample


def test_pack_sequences_frame_union_id_compaction_and_ragged_offsets():
    gt = {'v': [[7, 10 ** 6, 1, 2, 3, 4, 1.0], [2, 3, 5, 6, 7, 8, 1.0], [7, 7, 9, 10, 11, 12, 1.0], [2, 7, 0, 0, 1, 1, 1.0]],
          'w': [[5, 1, 0, 0, 2, 2, 1.0]]}
    pred = {'v': [[4, 50, 1, 1, 1, 1, 0.9], [7, 40, 2, 2, 2, 2, 0.9]],
            'w': [[5, 9, 0, 0, 2, 2, 0.9], [5, 8, 1, 1, 2, 2, 0.9], [6, 9, 3, 3, 2, 2, 0.9]]}
    p = mot_eval.pack_sequences(gt, pred)
    assert p['videos'] == ['v', 'w']
    assert p['frame_no'].tolist() == [2, 4, 7, 5, 6] and p['frame_seq'].tolist() == [0, 0, 0, 1, 1]
    assert p['seq_frame_off'].tolist() == [0, 3, 5]
    assert p['gt_ids'][0].tolist() == [3, 7, 10 ** 6] and p['tr_ids'][0].tolist() == [40, 50]
    # rows sorted by frame, the order inside a frame kept; ids 3, 7, 10^6 -> 0, 1, 2
    assert p['gt_rows'].tolist() == [[2, 0, 5, 6, 7, 8], [2, 1, 0, 0, 1, 1], [7, 2, 1, 2, 3, 4], [7, 1, 9, 10, 11, 12],
                                     [5, 0, 0, 0, 2, 2]]
    assert p['pred_rows'][:, :2].tolist() == [[4, 1], [7, 0], [5, 1], [5, 0], [6, 1]]
    assert p['frame_gt_off'].tolist() == [0, 2, 2, 4, 5, 5] and p['frame_pred_off'].tolist() == [0, 0, 1, 2, 4, 5]
    assert p['frame_pair_off'].tolist() == [0, 0, 0, 2, 4, 4]
    assert p['seq_ng'].tolist() == [3, 1] and p['seq_nt'].tolist() == [2, 2]
    assert p['seq_gid_off'].tolist() == [0, 3, 4] and p['seq_tid_off'].tolist() == [0, 2, 4]
    assert p['seq_mat_off'].tolist() == [0, 6, 8] and p['max_frame_objects'] == 2
    assert p['gt_rows'].dtype == np.float64 and p['frame_pair_off'].dtype == np.int64


def test_pack_sequences_empty_videos_of_each_kind():
    p = mot_eval.pack_sequences({'g': [[1, 1, 0, 0, 1, 1]], 'z': [], 'p': []}, {'p': [[3, 2, 0, 0, 1, 1]], 'z': [], 'g': []})
    assert p['videos'] == ['g', 'p', 'z']
    assert p['seq_frame_off'].tolist() == [0, 1, 2, 2] and p['frame_no'].tolist() == [1, 3]
    assert p['seq_ng'].tolist() == [1, 0, 0] and p['seq_nt'].tolist() == [0, 1, 0]
    assert p['frame_gt_off'].tolist() == [0, 1, 1] and p['frame_pred_off'].tolist() == [0, 0, 1]
    assert p['seq_mat_off'].tolist() == [0, 0, 0, 0] and p['frame_pair_off'].tolist() == [0, 0, 0]
    lists = mot_eval.pack_sequences([[[1, 1, 0, 0, 1, 1]]], [[]])          # two lists: videos 0 .. B - 1
    assert lists['videos'] == [0] and len(lists['pred_rows']) == 0
    nothing = mot_eval.pack_sequences({}, {})
    assert nothing['videos'] == [] and nothing['gt_rows'].shape == (0, 6) and nothing['seq_frame_off'].tolist() == [0]


def test_pack_sequences_refuses_an_id_twice_in_one_frame():
    rows = [[1, 4, 0, 0, 1, 1], [2, 4, 0, 0, 1, 1], [2, 9, 5, 5, 1, 1], [2, 4, 7, 7, 1, 1]]
    with pytest.raises(ValueError, match=r"video 'clip'.*id 4 .*frame 2"):
        mot_eval.pack_sequences({'clip': rows}, {'clip': []})
    with pytest.raises(ValueError, match=r"video 'clip'.*prediction id 4 .*frame 2"):
        mot_eval.pack_sequences({'clip': []}, {'clip': rows})


@pytest.mark.parametrize('name', sorted(cases.SCENARIOS))
def test_host_scores_do_not_depend_on_how_ties_break(name):
    """The precondition of the GPU tests: rows shuffled and all ids relabelled in reverse order (every matrix scipy
    sees is permuted) - the host backend returns the same integers and floats within 1e-12."""
    gt, pred = cases.scenario(name)
    ref = cases.host_reference(name)
    gt2 = {v: cases.shuffled_and_relabelled(r, 7) for v, r in gt.items()}
    pred2 = {v: cases.shuffled_and_relabelled(r, 8) for v, r in pred.items()}
    got = cases.host_scores(gt2, pred2)
    assert sorted(got) == sorted(ref)
    for v in ref:
        cases.assert_same_scores(got[v], ref[v], 1e-12, where=(name, v))


def test_scenarios_hold_what_they_are_built_for():
    r = cases.host_reference('clear_continuity')['bonus']['clear_identity']
    assert r['IDSW'] == 1 and r['Frag'] == 1 and r['MT'] >= 1 and r['PT'] == 1 and r['ML'] == 1
    assert r['TP'] == 5 + 3 + 5                      # gt 1 keeps its partner in every frame: no switch to the newcomer
    r = cases.host_reference('empty_kinds')['mixed']['clear_identity']
    assert r['IDSW'] == 0 and r['Frag'] == 0          # a reset at the gt-only or prediction-only frame would change both
    t = cases.host_reference('thresholds')['thr']
    assert t['clear_identity']['TP'] == 1 and M.HOTA_ALPHAS[9] == 0.5 and M.HOTA_ALPHAS[2] == 0.15000000000000002
    assert t['hota']['HOTA_TP'].tolist() == [4, 4, 3] + [2] * 6 + [1] + [0] * 9
    for name in ('random_b1', 'random_b3'):
        tot = [v['clear_identity'] for v in cases.host_reference(name).values()]
        assert sum(r['IDSW'] for r in tot) > 0 and sum(r['FN'] for r in tot) > 0 and sum(r['FP'] for r in tot) > 0
    # 'contested': in the first frame neither the row maxima nor the column maxima of CLEAR's score are an assignment
    gt, pred = cases.scenario('contested')
    gt2, pred2 = cases.scenario('contested_shapes')
    gt, pred = dict(gt, **gt2), dict(pred, **pred2)
    assert len(gt) == 8
    for v in gt:
        g = np.array([r[2:6] for r in gt[v] if r[0] == 1])
        p = np.array([r[2:6] for r in pred[v] if r[0] == 1])
        sim = M.box_iou_xywh(g, p)
        for w in (np.where(sim >= 0.5, sim, 0.0), sim):
            rows, cols = w.argmax(1)[w.max(1) > 0], w.argmax(0)[w.max(0) > 0]        # the positive maxima only
            assert len(set(rows.tolist())) < len(rows) and len(set(cols.tolist())) < len(cols), v
    assert cases.host_reference('contested')['long_chain']['clear_identity']['TP'] > 100
    stream, gt = cases.detection_stream_with_gt()
    assert len(gt) == 24 * 6 and stream.shape[1] == 8


def _fill(metrics):
    for video, seed in (('a', 0), ('b', 1)):
        rng = np.random.RandomState(seed)
        for t in range(4):
            boxes = torch.tensor([[10. + 3 * t, 10, 40 + 3 * t, 40], [200., 100, 240, 140]]) + float(rng.randint(0, 3))
            s = TrackDataSample(dict(frame_id=t))
            s.pred_track_instances = InstanceData(bboxes=boxes, scores=torch.full((2,), 0.9), labels=torch.zeros(2, dtype=torch.long),
                                                  depth=torch.tensor([20.0, 95.0 if t == 2 else 30.0]),
                                                  instances_id=torch.tensor([0, 1 if t < 2 else 5]))
            metrics.process(video, s, [dict(instance_id=k, bbox=boxes[k].tolist(), location=[0, 0, 20.0]) for k in range(2)])
    return metrics


def test_backend_keyword_is_validated():
    with pytest.raises(ValueError, match='backend'):
        M.MOTDroneMetrics(backend='gpu')
    with pytest.raises(ValueError, match='backend'):
        M.clear_identity([], [], backend='cuda')
    with pytest.raises(ValueError, match='backend'):
        M.hota([], [], backend=None)
    with pytest.raises(ValueError, match='backend'):
        mot_eval.evaluate_sweep([[]], [[]], backend='numpy')
    assert M.MOTDroneMetrics().backend == 'host' and M.MOTDroneMetrics(backend='device').backend == 'device'


def test_default_backend_is_the_host_scorer_through_both_call_forms():
    gt, pred = cases.scenario('random_b1')
    a, b = M.clear_identity(gt['solo'], pred['solo']), M.clear_identity(gt['solo'], pred['solo'], 0.5, backend='host')
    assert a == b == cases.host_reference('random_b1')['solo']['clear_identity']
    ha, hb = M.hota(gt['solo'], pred['solo']), M.hota(gt['solo'], pred['solo'], backend='host')
    assert set(ha) == set(hb) and all(np.array_equal(ha[k], hb[k]) for k in ha)
    ra, rb = _fill(M.MOTDroneMetrics()).evaluate(), _fill(M.MOTDroneMetrics(backend='host')).evaluate()
    assert ra == rb and ra['combined']['IDSW'] > 0 and 'HOTA' in ra['combined']


def test_device_backend_without_a_device_raises_at_evaluate(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    m = _fill(M.MOTDroneMetrics(backend='device'))       # construction and process() need no device
    with pytest.raises(RuntimeError, match='CUDA'):
        m.evaluate()
    with pytest.raises(RuntimeError, match='CUDA'):
        M.clear_identity([[1, 1, 0, 0, 1, 1]], [[1, 1, 0, 0, 1, 1]], backend='device')
    with pytest.raises(RuntimeError, match='CUDA'):
        M.hota([[1, 1, 0, 0, 1, 1]], [[1, 1, 0, 0, 1, 1]], backend='device')
    with pytest.raises(RuntimeError, match='CUDA'):
        mot_eval.evaluate_packed(mot_eval.pack_sequences(*cases.scenario('thresholds')))
