"""CPU: MOTDroneMetrics(protocol='trackeval') on the host - a known answer for every rule of the protocol, the rounding
of metrics.motchallenge_file_rows against Python's own formatting on values where rint(x * 1000) / 1000 is wrong, the
write -> read -> 'rows' invariant, and the precondition of the GPU comparison (no tied optimum on the generators).
Inputs and the independent restatement: tests/motchallenge_ref.py."""
import os

import numpy as np
import pytest

import motchallenge_ref as ref
from stereotracking_amd import metrics as M
from stereotracking_amd import mot_eval
from stereotracking_amd.config import Config
from stereotracking_amd.registry import METRICS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone_disp_eval_trackeval.py')


def metric(gt, pred, video='v', **kw):
    m = M.MOTDroneMetrics(**kw)
    m.gt[video] = [list(r) for r in np.asarray(gt, dtype=np.float64).reshape(-1, 9)]
    m.pred[video] = [list(r) for r in np.asarray(pred, dtype=np.float64).reshape(-1, 7)]
    return m


def counts(gt, pred, **kw):
    r = metric(gt, pred, **kw).evaluate()['combined']
    return int(r['TP']), int(r['FP']), int(r['FN'])


# three well separated places; a prediction sits on each
BOX = ([100.0, 100.0, 40.0, 80.0], [300.0, 100.0, 40.0, 80.0], [500.0, 100.0, 40.0, 80.0])
PRED = [[1, 10 + k] + [v + 0.25 for v in b] + [0.9] for k, b in enumerate(BOX)]


def gt_row(k, cls, conf=1):
    return [1, k + 1] + BOX[k] + [conf, cls, 1.0]


# ---- known answers, one per rule ---------------------------------------------------------------------------------------
def test_truncated_ground_truth_turns_a_miss_into_a_match():
    gt = [[1, 1, 13.9, 0, 10.9, 10, 1, 1, 1.0]]
    pred = [[1, 1, 10, 0, 10, 10, 0.9]]
    assert M.box_iou_xywh(np.array([[13.9, 0, 10.9, 10]]), np.array([[10.0, 0, 10, 10]]))[0, 0] == pytest.approx(61 / 148)
    assert counts(gt, pred) == (0, 1, 1) == counts(gt, pred, protocol='rows')
    assert counts(gt, pred, protocol='trackeval') == (1, 0, 0)
    g, _ = M.motchallenge_file_rows(gt, pred)
    assert g.tolist() == [[1, 1, 13, 0, 10, 10, 1, 1]]
    assert M.box_iou_xywh(g[:, 2:6], np.array([[10.0, 0, 10, 10]]))[0, 0] == pytest.approx(70 / 130)


def test_prediction_on_a_distractor_is_removed_and_one_on_a_zero_marked_pedestrian_is_a_false_positive():
    gt = [gt_row(0, 8), gt_row(1, 1, conf=0), gt_row(2, 1)]
    assert counts(gt, PRED) == (3, 0, 0)
    assert counts(gt, PRED, protocol='trackeval') == (1, 1, 0)
    g, p = M.motchallenge_file_rows(gt, PRED)
    gk, pk = M.motchallenge_preprocess(g, p, 'MOT17')
    assert gk.tolist() == [False, False, True] and pk.tolist() == [False, True, True]


def test_ground_truth_of_another_class_is_dropped_and_its_prediction_kept():
    gt = [gt_row(0, 3), gt_row(2, 1)]
    assert counts(gt, PRED, protocol='trackeval') == (1, 2, 0)
    gk, pk = M.motchallenge_preprocess(*M.motchallenge_file_rows(gt, PRED), 'MOT17')
    assert gk.tolist() == [False, True] and pk.all()


def test_mot15_removes_nothing_and_keeps_every_class():
    gt = [gt_row(0, 8), gt_row(1, 1, conf=0), gt_row(2, 1)]
    gk, pk = M.motchallenge_preprocess(*M.motchallenge_file_rows(gt, PRED), 'MOT15')
    assert gk.tolist() == [True, False, True] and pk.all()
    assert counts(gt, PRED, protocol='trackeval', benchmark='MOT15') == (2, 1, 0)


def test_non_mot_vehicle_is_a_distractor_under_mot20_only():
    gt = [gt_row(0, 6), gt_row(2, 1)]
    assert M.motchallenge_preprocess(*M.motchallenge_file_rows(gt, PRED), 'MOT20')[1].tolist() == [False, True, True]
    assert M.motchallenge_preprocess(*M.motchallenge_file_rows(gt, PRED), 'MOT17')[1].tolist() == [True, True, True]
    assert counts(gt, PRED, protocol='trackeval', benchmark='MOT20') == (1, 1, 0)
    assert counts(gt, PRED, protocol='trackeval', benchmark='MOT17') == (1, 2, 0)
    for b in ('MOT16', 'DanceTrack'):
        assert M.motchallenge_distractors(b) == (2, 7, 8, 12)
    assert sorted(M.motchallenge_distractors('MOT20')) == [2, 6, 7, 8, 12]


def test_every_distractor_class_removes_its_prediction():
    for cls in range(1, 14):
        gk, pk = M.motchallenge_preprocess(*M.motchallenge_file_rows([gt_row(0, cls)], PRED[:1]), 'MOT17')
        assert pk.tolist() == [cls not in (2, 7, 8, 12)] and gk.tolist() == [cls == 1]


def test_the_match_threshold_is_trackevals_constant_not_iou_thr():
    gt = [[1, 1, 100, 100, 40, 80, 1, 8, 1.0]]
    pred = [[1, 5, 112.0, 100, 40, 80, 0.9]]            # IoU 28 / 52 = 0.538: a match at 0.5, none at iou_thr = 0.7
    assert counts(gt, pred, protocol='trackeval', iou_thr=0.7) == (0, 0, 0)
    pred = [[1, 5, 115.0, 100, 40, 80, 0.9]]            # IoU 25 / 55 = 0.4545: no match, the prediction stays
    assert counts(gt, pred, protocol='trackeval', iou_thr=0.3) == (0, 1, 0)


def test_class_outside_the_table_raises():
    with pytest.raises(ValueError, match='class 14'):
        metric([gt_row(0, 14)], PRED, protocol='trackeval').evaluate()
    with pytest.raises(ValueError, match='class 0'):
        M.motchallenge_preprocess([gt_row(0, 0)[:8]], PRED, 'MOT15')
    metric([gt_row(0, 14)], PRED).evaluate()            # 'rows' never looks at the class


def test_non_finite_value_raises_naming_video_and_row():
    gt = [gt_row(0, 1), gt_row(1, 1)]
    gt[1][3] = float('nan')
    with pytest.raises(ValueError, match=r"non-finite value: video 'cam3', ground-truth row 1\b"):
        metric(gt, PRED, video='cam3', protocol='trackeval').evaluate()
    pred = [list(r) for r in PRED]
    pred[2][6] = float('inf')
    with pytest.raises(ValueError, match=r"non-finite value: video 'cam3', prediction row 2\b"):
        metric([gt_row(0, 1)], pred, video='cam3', protocol='trackeval').evaluate()


def test_arguments_are_checked_and_the_default_is_rows():
    m = M.MOTDroneMetrics()
    assert (m.protocol, m.benchmark) == ('rows', 'MOT17')
    with pytest.raises(ValueError, match='protocol'):
        M.MOTDroneMetrics(protocol='files')
    with pytest.raises(ValueError, match='benchmark'):
        M.MOTDroneMetrics(benchmark='MOT18')
    with pytest.raises(ValueError, match='protocol'):
        mot_eval.evaluate_sweep([np.zeros((0, 6))], np.zeros((0, 6)), backend='host', protocol='files')


# ---- rounding ------------------------------------------------------------------------------------------------------------
def test_file_rows_equal_python_formatting_where_rint_is_wrong():
    x = ref.adversarial_values()
    assert len(x) == 20000 and (x < 0).sum() > 5000
    want = ref.round3_ref(x)
    naive = np.rint(x * 1000.0) / 1000.0
    assert int((naive != want).sum()) >= 1000          # the set has teeth: the one-line rounding fails on these
    pred = np.zeros((len(x) // 5, 7))
    pred[:, 2:] = x.reshape(-1, 5)
    _, got = M.motchallenge_file_rows(np.zeros((0, 9)), pred)
    assert np.array_equal(got[:, 2:].ravel(), want)
    # truncation toward zero, and the columns it applies to
    g, p = M.motchallenge_file_rows([[1.9, 2.9, 13.9, -0.5, -1.5, 1e9 + 0.5, 0.9, 1.9, 0.123456]], [[3.9, -7.9, 0.0625, 0.1875, 2.5, -0.0625, 0.99951]])
    assert g.tolist() == [[1, 2, 13, 0, -1, 1e9, 0, 1]]
    assert p.tolist() == [[3, -7, 0.062, 0.188, 2.5, -0.062, 1.0]]        # 62.5 and 187.5 are exact ties: to the even one


def test_file_rows_equal_the_independent_line_formatting():
    for v, (gt, pred) in ref.videos().items():
        g, p = M.motchallenge_file_rows(gt, pred, video=v)
        rg, rp = ref.file_rows_ref(gt, pred)
        assert np.array_equal(g, rg) and np.array_equal(p, rp), v
        assert (g[:, 2:6] != gt[:, 2:6]).any() and (p[:, 2:6] != pred[:, 2:6]).any()


# ---- the files ---------------------------------------------------------------------------------------------------------
def _filled(**kw):
    m = M.MOTDroneMetrics(**kw)
    for v, (gt, pred) in ref.videos().items():
        m.gt[v] = [list(r) for r in gt]
        m.pred[v] = [list(r) for r in pred]
    return m


def assert_same_result(a, b, tol=0.0):
    assert set(a['per_video']) == set(b['per_video'])
    for x, y in [(a['combined'], b['combined'])] + [(a['per_video'][v], b['per_video'][v]) for v in b['per_video']]:
        assert set(x) == set(y)
        for k in y:
            assert abs(x[k] - y[k]) <= tol * max(1.0, abs(y[k])), (k, x[k], y[k])


@pytest.mark.parametrize('benchmark', ['MOT17', 'MOT20', 'MOT15'])
def test_scoring_the_rows_equals_scoring_the_written_files(tmp_path, benchmark):
    """The main invariant: protocol='trackeval' on the in-memory rows == the files written, read back, preprocessed and
    scored by the 'rows' scorers."""
    m = _filled(protocol='trackeval', benchmark=benchmark)
    got = m.evaluate()
    m.write_motchallenge(str(tmp_path))
    back = M.MOTDroneMetrics.read_motchallenge(str(tmp_path))
    assert sorted(back.gt) == sorted(back.pred) == sorted(ref.videos()) and back.protocol == 'rows'
    kept = M.MOTDroneMetrics()
    for v in back.gt:
        assert np.asarray(back.gt[v]).shape[1] == 9 and np.asarray(back.pred[v]).shape[1] == 7
        gk, pk = M.motchallenge_preprocess(back.gt[v], back.pred[v], benchmark)
        rg, rp, _ = ref.preprocess_ref(np.asarray(back.gt[v])[:, :8], back.pred[v], benchmark)
        assert np.array_equal(gk, rg) and np.array_equal(pk, rp)
        kept.gt[v] = np.asarray(back.gt[v])[gk]
        kept.pred[v] = np.asarray(back.pred[v])[pk]
    assert_same_result(got, kept.evaluate())
    rows = _filled().evaluate()
    assert rows['combined']['TP'] != got['combined']['TP'] or rows['combined']['FP'] != got['combined']['FP']
    # and read_motchallenge carries the arguments through
    again = M.MOTDroneMetrics.read_motchallenge(str(tmp_path), protocol='trackeval', benchmark=benchmark)
    assert_same_result(again.evaluate(), got)      # reading and rounding again changes nothing


def test_default_protocol_scores_the_rows_as_before():
    got = _filled().evaluate()
    for v, (gt, pred) in ref.videos().items():
        want = M.clear_identity(gt, pred, 0.5)
        assert all(got['per_video'][v][k] == want[k] for k in want)
        assert got['per_video'][v]['HOTA'] == float(M.hota(gt, pred)['HOTA'].mean())


# ---- the generators of the GPU comparison -------------------------------------------------------------------------------
def test_generators_fire_the_rules_without_a_tie():
    total = dict(removed=0, matched=0, ties=0, frames=0)
    dropped = 0
    inputs = dict(ref.videos(), crowd=ref.crowd(64, 64), crowd_ws=ref.crowd(65, 70), crowd_small=ref.crowd(3, 5),
                  sparse=ref.frame(64, 64, classes=[(1, 2, 7, 8, 12, 6)[i % 6] for i in range(64)]))
    for name, (gt, pred) in inputs.items():
        g, p = M.motchallenge_file_rows(gt, pred)
        for benchmark in ('MOT17', 'MOT20'):
            gk, pk, stats = ref.preprocess_ref(g, p, benchmark)
            hk, hp = M.motchallenge_preprocess(g, p, benchmark)
            assert np.array_equal(gk, hk) and np.array_equal(pk, hp), (name, benchmark)
            assert stats['ties'] == 0, (name, benchmark, stats)
            for k in total:
                total[k] += stats[k]
            dropped += int((~gk).sum())
    assert total['removed'] > 100 and total['matched'] > 400 and dropped > 100


# ---- sweeps, registry, config ------------------------------------------------------------------------------------------
def test_evaluate_sweep_host_carries_the_protocol():
    vids = list(ref.videos().values())
    gts, preds = [g for g, _ in vids], [p[:, :6] for _, p in vids]
    got = mot_eval.evaluate_sweep(preds, gts, backend='host', protocol='trackeval', benchmark='MOT20')
    for (g, p), r in zip(vids, got):
        fg, fp = M.motchallenge_file_rows(g, np.column_stack([p[:, :6], np.ones(len(p))]))
        gk, pk = M.motchallenge_preprocess(fg, fp, 'MOT20')
        assert r['clear_identity'] == M.clear_identity(fg[gk], fp[pk], 0.5)
    # ground truth without conf / class columns: every row is a marked pedestrian
    six = mot_eval.evaluate_sweep(preds, [g[:, :6] for g in gts], backend='host', protocol='trackeval')
    for (g, p), r in zip(vids, six):
        fg, fp = ref.file_rows_ref(np.column_stack([g[:, :6], np.ones((len(g), 3))]), np.column_stack([p[:, :6], np.ones(len(p))]))
        assert r['clear_identity'] == M.clear_identity(fg, fp, 0.5)


def test_registry_and_config_accept_the_protocol():
    m = METRICS.build(dict(type='mmtrack.MOTDroneMetrics', protocol='trackeval', benchmark='MOT20', depth_thr=80))
    assert isinstance(m, M.MOTDroneMetrics) and (m.protocol, m.benchmark) == ('trackeval', 'MOT20')
    cfg = Config.fromfile(CFG)
    assert cfg.val_evaluator == cfg.test_evaluator and len(cfg.test_evaluator) == 2
    assert dict(cfg.test_evaluator[0])['type'] == 'mmdet.CocoMetric'
    m = METRICS.build(dict(cfg.test_evaluator[1]))
    assert isinstance(m, M.MOTDroneMetrics) and (m.protocol, m.benchmark, m.depth_thr, m.backend) == ('trackeval', 'MOT17', 80, 'host')


def test_abi_declares_the_two_entries(stlib):
    import ctypes as C
    from stereotracking_amd import _lib
    for name in ('st_mot_file_round', 'st_mot_challenge_workspace_bytes', 'st_mot_challenge_preprocess'):
        assert hasattr(stlib, name) and name in _lib._PROTOS
    args = _lib.StMotChallengeArgs()
    args.struct_size = C.sizeof(_lib.StMotChallengeArgs)
    assert stlib.st_mot_challenge_workspace_bytes(C.byref(args)) == 256
    args.struct_size -= 4
    assert stlib.st_mot_challenge_workspace_bytes(C.byref(args)) == 0
    assert stlib.st_mot_challenge_preprocess(C.byref(args), None) == -1 and b'struct_size' in stlib.st_last_error()
