"""GPU: the device path of MOTDroneMetrics(protocol='trackeval') - st_mot_file_round and st_mot_challenge_preprocess
(csrc/mot_eval.hip, include/stereotrack.h section 21) against the host specification (metrics.motchallenge_file_rows /
motchallenge_preprocess) and Python's own formatting.  Inputs: tests/motchallenge_ref.py; tests/
test_cpu_motchallenge_protocol.py proves that the generators have no tied optimum.

Rounded values and masks must be equal.  Scores: integers equal, floats within 1e-9 * max(1, |ref|), the device-vs-host
bar of DESIGN.md section 15 (tests/test_mot_eval_gpu.py)."""
import numpy as np
import pytest
import torch

import guard_memory as gm
import motchallenge_ref as ref
from stereotracking_amd import metrics as M
from stereotracking_amd import mot_eval

pytestmark = pytest.mark.gpu
TOL = 1e-9
INT_KEYS = ('TP', 'FN', 'FP', 'IDSW', 'Frag', 'MT', 'PT', 'ML', 'IDTP', 'IDFN', 'IDFP')
T, R3, CP = mot_eval.FILE_TRUNCATE, mot_eval.FILE_ROUND3, mot_eval.FILE_COPY


def device_round(x, modes, cuda, in_place=False):
    rows = torch.from_numpy(np.array(x, dtype=np.float64)).to(cuda)
    out = rows if in_place else torch.empty_like(rows)
    status = torch.empty(8, dtype=torch.int32, device=cuda)
    mot_eval.file_round(rows, modes, out, status)
    return out.cpu().numpy(), status.cpu().numpy()


# ---- st_mot_file_round ---------------------------------------------------------------------------------------------------
def test_round3_equals_python_formatting_on_the_adversarial_set(cuda):
    x = ref.adversarial_values()
    want = ref.round3_ref(x)
    assert len(x) == 20000 and int((np.rint(x * 1000.0) / 1000.0 != want).sum()) >= 1000
    got, status = device_round(x.reshape(-1, 5), (R3,) * 5, cuda)
    assert not status.any()
    bad = np.nonzero(got.ravel() != want)[0]                 # == : the sign of a zero is not compared
    assert len(bad) == 0, (len(bad), x[bad[:5]].tolist(), got.ravel()[bad[:5]].tolist(), want[bad[:5]].tolist())
    again, _ = device_round(x.reshape(-1, 5), (R3,) * 5, cuda, in_place=True)
    assert again.tobytes() == got.tobytes()
    # exact ties go to the even neighbour; the largest magnitudes below the limit
    edge = np.array([[0.0625, 0.1875, -0.0625, 2.5, np.nextafter(2.0 ** 43, 0)], [0.0005, 1.0005, -2.0 ** 42 - 0.0625, 0.0, -0.0004]])
    got, status = device_round(edge, (R3,) * 5, cuda)
    assert not status.any() and np.array_equal(got.ravel(), ref.round3_ref(edge.ravel()))
    assert got[0, :3].tolist() == [0.062, 0.188, -0.062]


def test_truncation_and_the_column_modes(cuda):
    x = np.array([[13.9, -0.5, -1.5, 1e9 + 0.5, 7.0, np.nan], [-13.9, 0.5, 1.5, -1e9 - 0.5, 2.0 ** 43, np.inf]])
    got, status = device_round(x, (T, T, T, T, T, CP), cuda)
    assert not status.any()
    assert got[:, :5].tolist() == [[13, 0, -1, 1e9, 7], [-13, 0, 1, -1e9, 2.0 ** 43]]
    assert not np.signbit(got[0, 1]) and np.isnan(got[0, 5]) and np.isinf(got[1, 5])          # a copied column is not checked
    gt, pred = ref.videos()['v0']
    g, sg = device_round(gt[:, :8], (T,) * 8, cuda)
    p, sp = device_round(pred, (T, T) + (R3,) * 5, cuda)
    hg, hp = M.motchallenge_file_rows(gt, pred)
    assert not sg.any() and not sp.any() and np.array_equal(g, hg) and np.array_equal(p, hp)


def test_status_names_the_first_offending_row(cuda):
    x = np.arange(40, dtype=np.float64).reshape(10, 4) + 0.4321
    bad = x.copy()
    bad[7, 2], bad[4, 3] = np.nan, np.inf
    got, status = device_round(bad, (T, T, R3, R3), cuda)
    assert status[0] == 1 and 10 - status[1] == 4 and status[2] == 0
    assert np.array_equal(got[:4], M.motchallenge_file_rows(np.zeros((0, 9)), np.column_stack([x, x[:, :3]]))[1][:4, :4])
    big = x.copy()
    big[6, 3], big[8, 2], big[2, 0] = 2.0 ** 43, -2.0 ** 50, 2.0 ** 60          # column 0 truncates: no limit there
    got, status = device_round(big, (T, T, R3, R3), cuda)
    assert status[0] == 2 and 10 - status[2] == 6 and status[1] == 0 and got[2, 0] == 2.0 ** 60
    both = bad.copy()
    both[9, 2] = 2.0 ** 44
    _, status = device_round(both, (T, T, R3, R3), cuda)
    assert status[0] == 3 and 10 - status[1] == 4 and 10 - status[2] == 9
    # through the product call: a ValueError naming the video and the row as it was passed
    gt, pred = (a.copy() for a in ref.videos()['v1'])
    pred[5, 4] = 2.0 ** 43
    with pytest.raises(ValueError, match=r"2\^43 or more.*video 'b', prediction row 5\b"):
        mot_eval.motchallenge_keep_masks([ref.videos()['v0'][0], gt], [ref.videos()['v0'][1], pred], device=cuda, videos=['a', 'b'])
    pred[5, 4] = np.nan
    with pytest.raises(ValueError, match=r"non-finite value: video 'b', prediction row 5\b"):
        mot_eval.motchallenge_keep_masks([ref.videos()['v0'][0], gt], [ref.videos()['v0'][1], pred], device=cuda, videos=['a', 'b'])


# ---- st_mot_challenge_preprocess -------------------------------------------------------------------------------------------
def host_masks(gts, preds, benchmark):
    out = []
    for g, p in zip(gts, preds):
        out.append(M.motchallenge_preprocess(*M.motchallenge_file_rows(g, p), benchmark))
    return out


def assert_masks_equal(got, want, where):
    assert len(got) == len(want)
    for k, ((gk, pk), (rg, rp)) in enumerate(zip(got, want)):
        assert gk.dtype == bool and pk.dtype == bool and gk.shape == rg.shape and pk.shape == rp.shape, (where, k)
        assert np.array_equal(gk, rg), (where, k, 'gt', np.nonzero(gk != rg))
        assert np.array_equal(pk, rp), (where, k, 'pred', np.nonzero(pk != rp))


ALL_CLASSES = [(1, 2, 7, 8, 12, 6, 3, 13)[i % 8] for i in range(64)]


def shape_sequence():
    """Frames 1 .. 8: 1 x 1, 3 x 5, 64 x 64 (every class), a crowded 64 x 64, 65 x 70 (the workspace path), no ground
    truth, no predictions, a crowded 3 x 5."""
    none_g, none_p = np.zeros((0, 9)), np.zeros((0, 7))
    return ref.stack(ref.frame(1, 1, classes=[8]), ref.frame(3, 5, classes=[1, 7, 12], conf=[0, 1, 1]),
                     ref.frame(64, 64, classes=ALL_CLASSES, conf=[i % 5 != 0 for i in range(64)]), ref.crowd(64, 64),
                     ref.crowd(65, 70), (none_g, ref.frame(0, 4)[1]), (ref.frame(4, 0)[0], none_p), ref.crowd(3, 5))


@pytest.mark.parametrize('benchmark', ['MOT17', 'MOT20', 'MOT15'])
def test_masks_equal_the_host_on_every_shape(cuda, benchmark):
    gt, pred = shape_sequence()
    sizes = [(int((gt[:, 0] == f).sum()), int((pred[:, 0] == f).sum())) for f in range(1, 9)]
    assert sizes == [(1, 1), (3, 5), (64, 64), (64, 64), (65, 70), (0, 4), (4, 0), (3, 5)]
    got = mot_eval.motchallenge_keep_masks([gt], [pred], benchmark, device=cuda)
    want = host_masks([gt], [pred], benchmark)
    assert_masks_equal(got, want, benchmark)
    gk, pk = got[0]
    if benchmark == 'MOT15':                                  # do_preproc off
        assert pk.all() and np.array_equal(gk, gt[:, 6] != 0)
    else:
        assert not pk[pred[:, 0] == 1].any()                  # the 1 x 1 frame: a prediction on a class-8 box
        removed = ~pk[pred[:, 0] == 3]
        assert int(removed.sum()) >= (40 if benchmark == 'MOT20' else 32) - 8       # every distractor class fires
        assert int((~pk[pred[:, 0] == 5]).sum()) >= 15 and pk[pred[:, 0] == 6].all()
        assert np.array_equal(gk, (gt[:, 6] != 0) & (gt[:, 7] == 1))
    # rows in another order: the masks follow the rows
    rng = np.random.RandomState(3)
    og, op_ = rng.permutation(len(gt)), rng.permutation(len(pred))
    again = mot_eval.motchallenge_keep_masks([gt[og]], [pred[op_]], benchmark, device=cuda)
    assert np.array_equal(again[0][0], want[0][0][og]) and np.array_equal(again[0][1], want[0][1][op_])


def test_two_packed_sequences_and_empty_ones(cuda):
    a, b = ref.video(7, 6, 6, classes=(1, 8, 1, 2, 1, 12), zero_marked=(4,)), ref.video(8, 6, 5, classes=(7, 1, 1, 8, 6))
    assert len(np.unique(a[0][:, 0])) == len(np.unique(b[0][:, 0])) == 6
    before = dict(mot_eval.LAUNCHES)
    got = mot_eval.motchallenge_keep_masks([a[0], b[0]], [a[1], b[1]], device=cuda)
    assert mot_eval.LAUNCHES['st_mot_challenge_preprocess'] == before.get('st_mot_challenge_preprocess', 0) + 1
    assert mot_eval.LAUNCHES['st_mot_file_round'] == before.get('st_mot_file_round', 0) + 2
    want = host_masks([a[0], b[0]], [a[1], b[1]], 'MOT17')
    assert_masks_equal(got, want, 'two sequences')
    assert sum(int((~pk).sum()) for _, pk in got) >= 10
    alone = mot_eval.motchallenge_keep_masks([b[0]], [b[1]], device=cuda)
    assert_masks_equal(alone, want[1:], 'alone')
    e9, e7 = np.zeros((0, 9)), np.zeros((0, 7))
    mixed = ([a[0], e9, e9, b[0][:, :6]], [e7, e7, a[1], b[1][:, :6]])         # 6-column rows: conf 1, class 1, score 1
    assert_masks_equal(mot_eval.motchallenge_keep_masks(*mixed, device=cuda), host_masks(*mixed, 'MOT17'), 'mixed')
    assert mot_eval.motchallenge_keep_masks([], [], device=cuda) == []


def test_frame_above_the_limit_sets_bit_8(cuda):
    lim = mot_eval.max_frame_objects()
    assert lim == 256
    ok = ref.stack(ref.frame(2, 2), ref.frame(lim, lim))
    assert_masks_equal(mot_eval.motchallenge_keep_masks([ok[0]], [ok[1]], device=cuda), host_masks([ok[0]], [ok[1]], 'MOT17'),
                       'at the limit')
    over = ref.stack(ref.frame(2, 2), ref.frame(2, 2), ref.frame(3, lim + 1))
    with pytest.raises(ValueError, match=r"more rows in one frame.*video 'long', frame 3\b"):
        mot_eval.motchallenge_keep_masks([ok[0], over[0]], [ok[1], over[1]], device=cuda, videos=['short', 'long'])


def test_class_outside_the_table_raises_on_the_device_path_too(cuda):
    gt, pred = (a.copy() for a in ref.videos()['v0'])
    gt[3, 7] = 14
    with pytest.raises(ValueError, match=r"video 'x'.*row 3 has class 14"):
        mot_eval.motchallenge_keep_masks([gt], [pred], device=cuda, videos=['x'])


def test_two_runs_give_identical_bytes(cuda):
    gt, pred = shape_sequence()

    def run():
        return b''.join(a.tobytes() + b.tobytes() for a, b in mot_eval.motchallenge_keep_masks([gt], [pred], device=cuda))
    a, b = run(), run()
    assert len(a) == len(gt) + len(pred) and a == b


# ---- end to end ----------------------------------------------------------------------------------------------------------
def assert_results_equal(got, want):
    assert set(got['per_video']) == set(want['per_video'])
    for d, e in [(got['combined'], want['combined'])] + [(got['per_video'][v], want['per_video'][v]) for v in want['per_video']]:
        assert set(d) == set(e)
        for k in e:
            if k in INT_KEYS:
                assert d[k] == e[k], (k, d[k], e[k])
            else:
                assert abs(d[k] - e[k]) <= TOL * max(1.0, abs(e[k])), (k, d[k], e[k])


def _filled(**kw):
    m = M.MOTDroneMetrics(**kw)
    for v, (gt, pred) in ref.videos().items():
        m.gt[v] = [list(r) for r in gt]
        m.pred[v] = [list(r) for r in pred]
    return m


@pytest.mark.parametrize('benchmark', ['MOT17', 'MOT15'])
def test_device_backend_equals_host_under_the_protocol(cuda, benchmark):
    want = _filled(protocol='trackeval', benchmark=benchmark).evaluate()
    before = dict(mot_eval.LAUNCHES)
    got = _filled(protocol='trackeval', benchmark=benchmark, backend='device').evaluate()
    assert_results_equal(got, want)
    for k in ('st_mot_challenge_preprocess', 'st_mot_similarity', 'st_mot_walk', 'st_mot_hota_match', 'st_mot_hota_accumulate'):
        assert mot_eval.LAUNCHES[k] == before.get(k, 0) + 1, k      # 3 videos: one launch of every stage
    rows = _filled(backend='device').evaluate()
    assert rows['combined']['TP'] != got['combined']['TP'] or rows['combined']['FP'] != got['combined']['FP']
    assert want['combined']['TP'] > 50 and want['combined']['FP'] > 0 and 0.0 < got['combined']['HOTA'] < 1.0
    no_hota = _filled(protocol='trackeval', benchmark=benchmark, backend='device', metric=['CLEAR', 'Identity']).evaluate()
    assert_results_equal(no_hota, _filled(protocol='trackeval', benchmark=benchmark, metric=['CLEAR', 'Identity']).evaluate())


def test_sweep_scores_under_the_protocol(cuda):
    from stereotracking_amd.sweep import TrackerSweep
    from test_tracker_sweep_gpu import M as MAX_DETS, MAX_TRACKS, SWEEP_VIDEOS, add_arrays, sweep_options, sweep_video
    videos = [sweep_video(*v) for v in SWEEP_VIDEOS[:2]]
    options = sweep_options()[:3]
    sweep = TrackerSweep(options, max_tracks=MAX_TRACKS, max_dets=MAX_DETS, device=cuda)
    add_arrays(sweep, videos)
    res = sweep.run()
    gts = []
    for _, _, gt in videos:       # object 1 a distractor, object 2 zero-marked, object 3 of another class
        cls = np.where(gt[:, 1] == 1, 8, np.where(gt[:, 1] == 3, 3, 1))
        gts.append(np.column_stack([gt, np.where(gt[:, 1] == 2, 0, 1), cls, np.ones(len(gt))]))
    dev = res.scores(gts, backend='device', protocol='trackeval')
    host = res.scores(gts, backend='host', protocol='trackeval')
    plain = res.scores(gts, backend='host')
    assert len(dev) == len(host) == 3
    for k, (d, h, p) in enumerate(zip(dev, host, plain)):
        assert d['overflowed'] is False and d['status'] == h['status'] == [0, 0]
        for key, want in h.items():
            if key in ('status', 'overflowed'):
                continue
            if key in INT_KEYS:
                assert d[key] == want, (k, key, d[key], want)
            else:
                assert abs(d[key] - want) <= TOL * max(1.0, abs(want)), (k, key, d[key], want)
        assert h['TP'] < p['TP'] and h['TP'] > 20


# ---- the memory contract ---------------------------------------------------------------------------------------------------
def test_file_round_writes_its_cells_only(cuda):
    """Rows and outputs inside 0xFF guard bands (a NaN as fp64): the outputs equal the plain run's, the bands survive."""
    x = ref.adversarial_values()[:5000].reshape(-1, 5)
    want, _ = device_round(x, (R3,) * 5, cuda)
    rows = gm.arena(torch.from_numpy(np.array(x)), device=cuda)
    out = gm.arena(torch.full(x.shape, float('nan'), dtype=torch.float64), device=cuda)
    status = gm.arena(torch.full((8,), -1, dtype=torch.int32), device=cuda)
    mot_eval.file_round(rows, (R3,) * 5, out, status)
    torch.cuda.synchronize()
    assert gm.bands_intact(rows, out, status)
    gm.assert_unaffected(out, torch.from_numpy(want), 'rounded rows')
    assert not status.cpu().numpy().any() and torch.equal(gm.bits(rows), gm.bits(torch.from_numpy(np.array(x))))


def test_both_kernels_over_stale_memory(cuda):
    """Workspace, status words, keep bytes and the rounded rows come from torch.empty: filled with 0x00, then with 0xFF
    (NaN as fp64), the masks and the scores are the same bytes."""
    from test_stale_memory_gpu import over_stale_memory
    gt, pred = shape_sequence()
    want = host_masks([gt], [pred], 'MOT17')
    host = _filled(protocol='trackeval').evaluate()

    def stage():
        masks = mot_eval.motchallenge_keep_masks([gt], [pred], device=cuda)
        assert_masks_equal(masks, want, 'stale')
        got = _filled(protocol='trackeval', backend='device').evaluate()
        assert_results_equal(got, host)
        return dict(masks=masks, scores=got)
    over_stale_memory(stage)
