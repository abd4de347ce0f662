"""GPU: the device stage of KITTI's preprocessing (st_mot_kitti_preprocess in csrc/mot_eval.hip, behind
mot_eval.kitti_keep_masks) against metrics.kitti_preprocess on the same rows, byte for byte, and MOTKittiMetrics'
device backend against its host backend.  Inputs: tests/kitti_eval_cases.py; tests/test_cpu_kitti_metrics.py proves that
the generator makes every rule fire and has no tied optimum.

Masks must be equal.  Scores: integers equal, floats within 1e-9 * max(1, |ref|), the bound of
tests/test_mot_eval_gpu.py (the scoring stages' fp64 sums of at most about 1e5 terms in [0, 1] taken in another order)."""
import numpy as np
import pytest

import kitti_eval_cases as cases
from stereotracking_amd import metrics as M
from stereotracking_amd import mot_eval
from stereotracking_amd.kitti_metrics import MOTKittiMetrics

pytestmark = pytest.mark.gpu
TOL = 1e-9
INT_KEYS = ('TP', 'FN', 'FP', 'IDSW', 'Frag', 'MT', 'PT', 'ML', 'IDTP', 'IDFN', 'IDFP')


def host_masks(sequences, classes):
    out = []
    for s in sequences:
        pairs = [M.kitti_preprocess(s[0], s[1], s[2], cid, dis) for cid, dis in classes]
        out.append((np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])))
    return out


def assert_masks_equal(got, ref, where):
    assert len(got) == len(ref)
    for k, ((gk, pk), (rg, rp)) in enumerate(zip(got, ref)):
        assert gk.dtype == bool and pk.dtype == bool and gk.shape == rg.shape and pk.shape == rp.shape, (where, k)
        assert np.array_equal(gk, rg), (where, k, 'gt', np.nonzero(gk != rg))
        assert np.array_equal(pk, rp), (where, k, 'pred', np.nonzero(pk != rp))


def test_masks_equal_the_host_on_the_generator(cuda):
    sequences = list(cases.random_sequences().values())
    assert len(sequences) == 3
    got = mot_eval.kitti_keep_masks(sequences, cases.BOTH, device=cuda)
    ref = host_masks(sequences, cases.BOTH)
    assert_masks_equal(got, ref, 'generator')
    removed = sum(int(((s[1][:, 2] == cid) & ~pk[c]).sum()) for s, (_, pk) in zip(sequences, got) for c, (cid, _) in enumerate(cases.BOTH))
    assert removed > 100 and sum(int(pk.sum()) for _, pk in got) > 100
    # rows in another order: the masks follow the rows
    rng = np.random.RandomState(5)
    perms = [[rng.permutation(len(rows)) for rows in s] for s in sequences]
    shuffled = [tuple(rows[o] for rows, o in zip(s, po)) for s, po in zip(sequences, perms)]
    again = mot_eval.kitti_keep_masks(shuffled, cases.BOTH, device=cuda)
    for (gk, pk), (rg, rp), po in zip(again, ref, perms):
        assert np.array_equal(gk, rg[:, po[0]]) and np.array_equal(pk, rp[:, po[1]])


def test_masks_equal_the_host_on_the_rule_frames(cuda):
    s = cases.rule_sequence()
    got = mot_eval.kitti_keep_masks([s], cases.BOTH, device=cuda)
    assert_masks_equal(got, host_masks([s], cases.BOTH), 'rules')
    # and the known answers themselves, frame by frame
    for k, (name, (one, cls, gt_keep, pred_keep)) in enumerate(sorted(cases.rule_frames().items())):
        c = list(cases.CLASSES).index(cls)
        assert got[0][0][c][s[0][:, 0] == k].tolist() == gt_keep, name
        assert got[0][1][c][s[1][:, 0] == k].tolist() == pred_keep, name


def test_masks_equal_the_host_on_the_edge_frames(cuda):
    s = cases.edge_sequence()
    big_g = int(((s[0][:, 0] == 4) & np.isin(s[0][:, 2], (cases.CAR, cases.VAN))).sum())
    big_p = int(((s[1][:, 0] == 4) & (s[1][:, 2] == cases.CAR)).sum())
    assert (big_g, big_p) == (70, 66) and big_g * big_p > 64 * 64
    got = mot_eval.kitti_keep_masks([s], cases.BOTH, device=cuda)
    ref = host_masks([s], cases.BOTH)
    assert_masks_equal(got, ref, 'edges')
    car = got[0][1][0]
    assert int(car[s[1][:, 0] == 4].sum()) == 33        # the chain: 66 matches, every second one on a van
    assert int(car[s[1][:, 0] == 5].sum()) + int(car[s[1][:, 0] == 6].sum()) >= 2
    # one class evaluated alone, either of them
    for c, cls in enumerate(cases.BOTH):
        alone = mot_eval.kitti_keep_masks([s], [cls], device=cuda)
        assert alone[0][0].shape[0] == 1
        assert np.array_equal(alone[0][0][0], ref[0][0][c]) and np.array_equal(alone[0][1][0], ref[0][1][c])
    # sequences without rows of a kind, and an empty one, beside an ordinary one
    empty = cases.seq([], [], [])
    no_pred = (s[0], np.zeros((0, 8)), s[2])
    no_gt = (np.zeros((0, 9)), s[1], np.zeros((0, 5)))
    mixed = [no_pred, empty, no_gt, cases.tie_sequence()[0]]
    assert_masks_equal(mot_eval.kitti_keep_masks(mixed, cases.BOTH, device=cuda), host_masks(mixed, cases.BOTH), 'mixed')


def _assert_results_equal(got, ref):
    assert set(got) == set(ref) == {'per_class', 'summary'}
    assert set(got['summary']) == set(ref['summary']) and list(got['per_class']) == list(ref['per_class'])
    for k, r in ref['summary'].items():
        assert abs(got['summary'][k] - r) <= TOL * max(1.0, abs(r)), (k, got['summary'][k], r)
    for cls in ref['per_class']:
        g, r = got['per_class'][cls], ref['per_class'][cls]
        assert set(g['per_video']) == set(r['per_video'])
        for d, e in [(g['combined'], r['combined'])] + [(g['per_video'][v], r['per_video'][v]) for v in r['per_video']]:
            assert set(d) == set(e)
            for k in e:
                if k in INT_KEYS:
                    assert d[k] == e[k], (cls, k, d[k], e[k])
                else:
                    assert abs(d[k] - e[k]) <= TOL * max(1.0, abs(e[k])), (cls, k, d[k], e[k])


def _filled(**kw):
    m = MOTKittiMetrics(**kw)
    for v, s in cases.random_sequences().items():
        cases.fill(m, v, s)
    return m


def test_device_backend_equals_host_and_launches_every_stage_once(cuda):
    ref = _filled().evaluate()
    m = _filled(backend='device')
    before = dict(mot_eval.LAUNCHES)
    got = m.evaluate()
    _assert_results_equal(got, ref)
    for k in ('st_mot_kitti_preprocess', 'st_mot_similarity', 'st_mot_walk', 'st_mot_hota_match', 'st_mot_hota_accumulate'):
        assert mot_eval.LAUNCHES[k] == before.get(k, 0) + 1, k       # 3 videos x 2 classes: one launch of every stage
    assert ref['summary']['TP_car'] > 50 and ref['summary']['TP_pedestrian'] > 50
    assert ref['summary']['FP_car'] > 0 and ref['summary']['IDSW_car'] + ref['summary']['IDSW_pedestrian'] > 0
    assert 0.0 < got['summary']['HOTA_car'] < 1.0
    # without HOTA: the HOTA stages are not launched
    ref2 = _filled(metric=['CLEAR', 'Identity'], classes_eval=['pedestrian']).evaluate()
    before = dict(mot_eval.LAUNCHES)
    got2 = _filled(metric=['CLEAR', 'Identity'], classes_eval=['pedestrian'], backend='device').evaluate()
    _assert_results_equal(got2, ref2)
    assert mot_eval.LAUNCHES['st_mot_kitti_preprocess'] == before['st_mot_kitti_preprocess'] + 1
    assert mot_eval.LAUNCHES['st_mot_hota_match'] == before['st_mot_hota_match']
    assert not any(k.startswith('HOTA') for k in got2['summary'])


def test_frame_above_the_limit_is_refused_naming_video_and_frame(cuda):
    lim = mot_eval.max_frame_objects()
    ok = cases.limit_sequence(lim)
    assert_masks_equal(mot_eval.kitti_keep_masks([ok], cases.BOTH, device=cuda), host_masks([ok], cases.BOTH), 'at the limit')
    over = cases.limit_sequence(lim + 1)
    with pytest.raises(ValueError, match=r"more rows of one class in one frame.*video 'long', frame 3\b"):
        mot_eval.kitti_keep_masks([cases.tie_sequence()[0], over], cases.BOTH, device=cuda, videos=['short', 'long'])
    # the other class's rows do not count: lim + 1 car predictions are fine for pedestrian alone
    alone = mot_eval.kitti_keep_masks([over], [cases.CLASSES['pedestrian']], device=cuda)
    assert not alone[0][1].any() and not alone[0][0].any()


def test_nan_box_reaches_the_status_word(cuda):
    sequences = [tuple(a.copy() for a in s) for s in cases.random_sequences().values()]
    row = int(np.nonzero(sequences[1][1][:, 0] == 7)[0][0])
    sequences[1][1][row, 5] = np.nan
    with pytest.raises(ValueError, match=r"non-finite box: video 'k1', frame 7\b"):
        mot_eval.kitti_keep_masks(sequences, cases.BOTH, device=cuda, videos=list(cases.random_sequences()))
    sequences[1][1][row, 5] = 100.0
    sequences[2][2][0, 1] = np.inf                             # an ignore region
    frame = int(sequences[2][2][0, 0])
    with pytest.raises(ValueError, match=rf"non-finite box: video 'k2', frame {frame}\b"):
        mot_eval.kitti_keep_masks(sequences, cases.BOTH, device=cuda, videos=list(cases.random_sequences()))


def test_two_runs_give_identical_bytes(cuda):
    sequences = list(cases.random_sequences().values()) + [cases.edge_sequence()]

    def run():
        return b''.join(a.tobytes() + b.tobytes() for a, b in mot_eval.kitti_keep_masks(sequences, cases.BOTH, device=cuda))
    a, b = run(), run()
    assert len(a) > 2000 and a == b


def test_degenerate_boxes_follow_the_eps_rules(cuda):
    s, expect = cases.degenerate_sequence()
    got = mot_eval.kitti_keep_masks([s], cases.BOTH, device=cuda)
    assert_masks_equal(got, host_masks([s], cases.BOTH), 'degenerate')
    assert got[0][1][0].tolist() == expect and got[0][0][0].tolist() == [True, True]


def test_tie_frame_removes_the_same_set_in_every_optimum(cuda):
    s, expect = cases.tie_sequence()
    got = mot_eval.kitti_keep_masks([s], cases.BOTH, device=cuda)
    assert got[0][1][0].tolist() == expect
    assert_masks_equal(got, host_masks([s], cases.BOTH), 'tie')
    swapped = (s[0], s[1][[1, 0, 2]], s[2])                      # the twins in the other order
    assert mot_eval.kitti_keep_masks([swapped], cases.BOTH, device=cuda)[0][1][0].tolist() == expect
