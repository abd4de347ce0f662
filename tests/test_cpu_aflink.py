"""CPU: AppearanceFreeLink's host backend (stereotracking_amd/aflink.py, the executable specification of csrc/aflink.hip):
the gate, the transform and the linking logic on known answers, the decided error cases, the whole forward against the
restatement of tests/aflink_ref.py, the preconditions the generator of tests/aflink_cases.py owes the decision
comparisons, the checkpoint names, and the wiring into the registries, MOTDroneMetrics and evaluate_sweep."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aflink_cases as cases  # noqa: E402
import aflink_ref as ref  # noqa: E402
import tracklets_ref  # noqa: E402
from stereotracking_amd import _lib, aflink  # noqa: E402
from stereotracking_amd import metrics as M  # noqa: E402
from stereotracking_amd import mot_eval  # noqa: E402
from stereotracking_amd.aflink import AFLinkModel, AppearanceFreeLink, link_from_scores  # noqa: E402
from stereotracking_amd.registry import TASK_UTILS  # noqa: E402


def track(tid, frames, x, y, score=0.9):
    """Rows of one track standing at (x, y) (scalars or per-frame arrays), boxes of 10 x 20."""
    f = np.asarray(frames, np.float64)
    x, y = np.broadcast_to(np.asarray(x, np.float64), f.shape), np.broadcast_to(np.asarray(y, np.float64), f.shape)
    return np.column_stack([f, np.full(len(f), float(tid)), x, y, x + 10, y + 20, np.full(len(f), score)])


def test_registry_names():
    assert TASK_UTILS.get('AppearanceFreeLink') is AppearanceFreeLink
    assert TASK_UTILS.get('mmtrack.AppearanceFreeLink') is AppearanceFreeLink
    built = TASK_UTILS.build(dict(type='mmtrack.AppearanceFreeLink', checkpoint=None, spatial_threshold=50))
    assert isinstance(built, AppearanceFreeLink) and built.spatial_threshold == 50 and built.backend == 'host'
    assert built.temporal_threshold == (0, 30) and built.confidence_threshold == 0.95 and not built.model.training


def reference_tree_keys():
    """The state-dict names of the reference's module tree (aflink.py:17-115), written out from its constructors."""
    bn = ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')
    keys = []
    for m in (1, 2):
        for block in range(4):
            keys.append(f'TemporalModule_{m}.{block}.conv.weight')
            keys += [f'TemporalModule_{m}.{block}.{name}.{k}' for name in ('bnf', 'bnx', 'bny') for k in bn]
        keys.append(f'FusionBlock_{m}.conv.weight')
        keys += [f'FusionBlock_{m}.bn.{k}' for k in bn]
    return keys + [f'classifier.{fc}.{k}' for fc in ('fc1', 'fc2') for k in ('weight', 'bias')]


def test_checkpoint_names_shapes_and_round_trip(tmp_path):
    sd = AFLinkModel().state_dict()
    assert sorted(sd) == sorted(reference_tree_keys())
    assert tuple(sd['TemporalModule_2.3.conv.weight'].shape) == (256, 128, 7, 1)
    assert tuple(sd['FusionBlock_1.conv.weight'].shape) == (256, 256, 1, 3)
    assert tuple(sd['classifier.fc1.weight'].shape) == (128, 512) and tuple(sd['classifier.fc2.weight'].shape) == (2, 128)
    want = cases.case()['state_dict']
    path = str(tmp_path / 'aflink.pth')
    torch.save(dict(state_dict={'module.' + k: v for k, v in want.items()}, meta=dict(epoch=20)), path)
    got = AppearanceFreeLink(path).model.state_dict()
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert all(torch.equal(AppearanceFreeLink(want).model.state_dict()[k], want[k]) for k in want)
    with pytest.raises(RuntimeError, match='remote'):
        AppearanceFreeLink('https://example.invalid/aflink.pth')
    torch.save(dict(state_dict={'backbone.weight': torch.zeros(3)}), path)
    with pytest.raises(RuntimeError, match='does not hold the link network'):
        AppearanceFreeLink(path)
    packed = aflink.pack_weights(want)
    assert packed.dtype == np.float32 and packed.size == int(_lib.load().st_aflink_packed_floats())


# ---------------------------------------------------------------------- gate
@pytest.mark.parametrize('dt,kept', [(-1, False), (0, True), (30, True), (31, False)])
def test_gate_temporal_ends_are_inclusive(dt, kept):
    rows = np.concatenate([track(1, [3, 10], 0, 0), track(2, [10 + dt, 50], 45, 60)])
    t = aflink.build_tracks(rows)
    i, j = list(t['ids']).index(1), list(t['ids']).index(2)
    flags = aflink.gate(t['info'])
    assert bool(flags[i, j]) == kept and not flags[j, i] and not flags[i, i] and not flags[j, j]
    assert np.array_equal(flags, ref.gate_flags(ref.tracks(rows)[2]))


def test_gate_distance_75_is_kept_and_the_next_one_dropped():
    up = np.nextafter(75.0, np.inf)
    assert np.sqrt(45.0 ** 2 + 60.0 ** 2) == 75.0 and np.sqrt(0.0 ** 2 + up ** 2) == up > 75.0
    rows = np.concatenate([track(1, [0, 1], 0, 0), track(2, [2, 3], 45, 60), track(3, [2, 3], 0, up), track(4, [2, 3], -45, -60)])
    t = aflink.build_tracks(rows)
    assert list(t['ids']) == [1, 2, 3, 4]
    flags = aflink.gate(t['info'])
    assert flags[0].tolist() == [False, True, False, True]
    assert np.array_equal(flags, ref.gate_flags(ref.tracks(rows)[2]))
    assert not aflink.gate(t['info'], (0, 30), 74.99).any() and aflink.gate(t['info'], (0, 30), up)[0, 2]


# ---------------------------------------------------------------------- transform
@pytest.mark.parametrize('ni,nj', [(1, 1), (29, 31), (30, 30), (31, 29), (1, 40)])
def test_transform_lengths_and_pads(ni, nj):
    rng = np.random.default_rng(ni * 100 + nj)
    a = np.column_stack([99000.0 + np.arange(ni), rng.uniform(50, 300, ni), rng.uniform(50, 300, ni)])
    b = np.column_stack([99000.0 + ni + 3 + np.arange(nj), rng.uniform(50, 300, nj), rng.uniform(50, 300, nj)])
    xa, xb = aflink.transform(a, b)
    assert xa.shape == xb.shape == (30, 3) and xa.dtype == xb.dtype == np.float32
    wa, wb = ref.transform64(a, b)
    assert np.array_equal(xa, wa.astype(np.float32)) and np.array_equal(xb, wb.astype(np.float32))
    both = np.concatenate([xa, xb])
    assert both.max() <= 1.0 and both.min() >= -1.0
    if ni < 30:          # the zero pads take part: they are the minimum of every (positive) column, so they map to -1
        assert np.all(np.abs(xa[:30 - ni] + 1.0) < 1e-6) and np.array_equal(xa[30 - ni:], wa[30 - ni:].astype(np.float32))
    else:                # i's LAST 30 rows, j's FIRST 30: the frame column rises by one per row
        lo = 0.0 if nj < 30 else a[ni - 30, 0]
        hi = b[min(nj, 30) - 1, 0]
        assert xa[0, 0] == np.float32((a[ni - 30, 0] - (hi + lo) / 2) / ((hi - lo) / 2 + 1e-5))
    if nj < 30:
        assert np.all(np.abs(xb[nj:] + 1.0) < 1e-6)
    if ni >= 30 and nj >= 30:          # no pads: frames near 1e5 spread over [-1, 1]
        assert abs(both[:, 0].max() - 1.0) < 1e-6 and abs(both[:, 0].min() + 1.0) < 1e-6


def test_transform_constant_column_and_known_values():
    a = np.column_stack([np.arange(30.0), np.full(30, 12.5), np.arange(30.0) * 2])
    b = np.column_stack([30.0 + np.arange(30.0), np.full(30, 12.5), 60.0 + np.arange(30.0) * 2])
    xa, xb = aflink.transform(a, b)
    assert np.all(xa[:, 1] == 0) and np.all(xb[:, 1] == 0)                   # a constant column becomes 0
    # column 0: min 0, max 59: (v - 29.5) / (29.5 + 1e-5)
    assert xa[0, 0] == np.float32((0 - 29.5) / (29.5 + 1e-5)) and xb[29, 0] == np.float32((59 - 29.5) / (29.5 + 1e-5))
    assert xb[0, 2] == np.float32((60 - 59.0) / (59.0 + 1e-5))
    # a one-row pair: 29 zero rows in front of i, 29 behind j; the pads are the minimum
    xa, xb = aflink.transform(np.array([[7.0, 4.0, 8.0]]), np.array([[9.0, 2.0, 8.0]]))
    assert xa[29].tolist() == [np.float32((7 - 4.5) / (4.5 + 1e-5)), np.float32((4 - 2.0) / (2.0 + 1e-5)),
                               np.float32((8 - 4.0) / (4.0 + 1e-5))]
    assert xb[0, 0] == np.float32((9 - 4.5) / (4.5 + 1e-5)) and xa[0, 0] == np.float32((0 - 4.5) / (4.5 + 1e-5)) == xb[1, 0]


# ---------------------------------------------------------------------- linking, no network
def three_tracks(ids):
    return np.concatenate([track(ids[0], [0, 1], 0, 0), track(ids[1], [4, 5], 5, 5), track(ids[2], [8, 9], 9, 9)])


def test_link_chain_in_both_index_orders():
    rows = three_tracks((10, 20, 30))
    out = link_from_scores(rows, [(0, 1), (1, 2)], np.float32([0.99, 0.98]))
    assert out.shape == (6, 7) and set(out[:, 1]) == {10.0} and out[:, 0].tolist() == [0, 1, 4, 5, 8, 9]
    assert np.array_equal(out[:, 2:], rows[:, 2:])                         # the other columns are carried through
    # the links found in descending index order: the reference's two loops end at the LAST track's id
    out = link_from_scores(rows, [(2, 1), (1, 0)], np.float32([0.99, 0.98]))
    assert set(out[:, 1]) == {30.0}
    for pairs, conf in (([(0, 1), (1, 2)], [0.99, 0.98]), ([(2, 1), (1, 0)], [0.99, 0.98]), ([(0, 2)], [0.5])):
        assert np.array_equal(link_from_scores(rows, pairs, np.float32(conf)), ref.link(rows, pairs, np.float32(conf), 0.95))
    assert np.array_equal(link_from_scores(rows, [(0, 2)], np.float32([0.5])), rows)      # below the threshold: no link
    assert set(link_from_scores(rows, [(0, 2)], np.float32([0.5]), confidence_threshold=0.5)[:, 1]) == {10.0, 20.0}


def test_link_threshold_is_compared_in_fp64_and_cost_is_fp32():
    rows = three_tracks((1, 2, 3))
    c = np.float32(0.95)                                                    # 0.949999988079071 < 0.95
    assert float(c) < 0.95
    assert np.array_equal(link_from_scores(rows, [(0, 1)], [c]), rows)
    assert set(link_from_scores(rows, [(0, 1)], [np.nextafter(c, np.float32(1))])[:, 1]) == {1.0, 3.0}


def test_link_contested_pair_takes_the_cheaper_link():
    rows = three_tracks((1, 2, 3))
    out = link_from_scores(rows, [(0, 2), (1, 2)], np.float32([0.99, 0.96]))
    assert out[:, 1].tolist() == [1, 1, 2, 2, 1, 1]
    out = link_from_scores(rows, [(0, 2), (1, 2)], np.float32([0.96, 0.99]))
    assert out[:, 1].tolist() == [1, 1, 2, 2, 2, 2]


def test_link_dt_zero_keeps_the_first_row_of_the_shared_frame():
    a, b = track(1, [3, 5], 0, 0, score=0.7), track(2, [5, 6], 4, 4, score=0.8)
    out = link_from_scores(np.concatenate([a, b]), [(0, 1)], np.float32([0.99]))
    assert out[:, 0].tolist() == [3, 5, 6] and set(out[:, 1]) == {1.0} and out[1, 6] == 0.7 and out[1, 2] == 0.0
    out = link_from_scores(np.concatenate([b, a]), [(0, 1)], np.float32([0.99]))       # b's row of frame 5 comes first
    assert out[:, 0].tolist() == [3, 5, 6] and set(out[:, 1]) == {1.0} and out[1, 6] == 0.8 and out[1, 2] == 4.0


def test_link_uses_ids_not_matrix_indices():
    rows = three_tracks((7, 3, 100))          # track order by first frame: 7, 3, 100 = indices 0, 1, 2
    out = link_from_scores(rows, [(0, 1)], np.float32([0.99]))
    assert out[:, 1].tolist() == [7, 7, 7, 7, 100, 100]        # id 3 takes id 7; comparing index 1 with the ids finds nothing
    out = link_from_scores(rows, [(1, 2)], np.float32([0.99]))
    assert out[:, 1].tolist() == [7, 7, 3, 3, 3, 3]
    tie = np.concatenate([track(9, [0, 1], 0, 0), track(4, [0, 1], 50, 50)])
    assert list(aflink.build_tracks(tie)['ids']) == [4, 9]     # the same first frame: by id


# ---------------------------------------------------------------------- whole forward
def test_empty_one_track_and_two_tracks():
    link = AppearanceFreeLink(None)
    for empty in (np.zeros((0, 7)), [], np.zeros((0, 9))):
        out = link.forward(empty)
        assert out.shape == (0, 7) and out.dtype == np.float64
    one = track(5, [4], 1, 2)
    assert np.array_equal(link.forward(one), one)                           # a single row is a track and is kept
    two = np.concatenate([track(8, [0, 1, 2], 0, 0), track(5, [4, 5], 3, 3)])
    assert np.array_equal(link.forward(two), two)                           # initialised weights: far below 0.95
    out = AppearanceFreeLink(None, confidence_threshold=0.0).forward(two[[3, 0, 4, 1, 2]])
    assert out[:, 0].tolist() == [0, 1, 2, 4, 5] and set(out[:, 1]) == {8.0}
    far = np.concatenate([track(8, [0, 1, 2], 0, 0), track(5, [4, 5], 300, 3)])
    assert np.array_equal(AppearanceFreeLink(None, confidence_threshold=0.0).forward(far),
                          far[np.lexsort((far[:, 1], far[:, 0]))])
    assert [len(o) for o in link.forward_many([two, np.zeros((0, 7)), one])] == [5, 0, 1]
    wide = np.column_stack([two, np.zeros((5, 2))])                         # further columns are dropped
    assert np.array_equal(link.forward(wide), two)


def test_input_errors():
    link = AppearanceFreeLink(None)
    ok = track(1, [0, 1, 2], 0, 0)
    for col, val, what in ((0, 1.5, 'not integral'), (1, 0.25, 'not integral'), (0, np.nan, 'not integral')):
        bad = ok.copy()
        bad[1, col] = val
        with pytest.raises(ValueError, match=f'AppearanceFreeLink.*{what}'):
            link.forward(bad)
    with pytest.raises(ValueError, match='AppearanceFreeLink.*strictly increasing'):
        link.forward(ok[[0, 2, 1]])
    for col, val in ((2, np.nan), (3, np.inf)):
        bad = ok.copy()
        bad[2, col] = val
        with pytest.raises(ValueError, match='AppearanceFreeLink.*non-finite'):
            link.forward(bad)
    bad = ok.copy()
    bad[0, 4] = np.nan                                                       # c2 takes no part
    assert np.array_equal(link.forward(bad), bad, equal_nan=True)
    with pytest.raises(ValueError, match='rows must be'):
        link.forward(np.zeros((4, 6)))
    with pytest.raises(ValueError, match='backend'):
        AppearanceFreeLink(None, backend='gpu')
    m = AFLinkModel()
    with pytest.raises(RuntimeError, match='evaluation'):
        m(torch.zeros(1, 1, 30, 3), torch.zeros(1, 1, 30, 3))


def test_device_backend_without_a_device_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    link = AppearanceFreeLink(None, backend='device')
    with pytest.raises(RuntimeError, match='no CUDA'):                      # no fallback to the host backend
        link.forward(np.concatenate([track(1, [0, 1], 0, 0), track(2, [3, 4], 1, 1)]))
    with pytest.raises(RuntimeError, match='no CUDA'):
        link.forward_many([np.zeros((0, 7))])


def test_generator_preconditions():
    """What the decision comparisons (host against restatement here, device against host on the GPU) rest on: the
    confidences spread, the threshold splits them, and no fp64 confidence is near enough to the threshold for any
    correct fp32 evaluation to land on the other side."""
    c = cases.case()
    conf, thr, err = c['conf64'], c['threshold'], c['ref_err']
    print(f'candidates {len(conf)}, ref_err {err:.3e}, logit_err {c["logit_err"]:.3e}, threshold {thr:.6f}, '
          f'passing {np.mean(conf >= thr):.3f}, nearest {np.abs(conf - thr).min():.3e}')
    assert 0 < err < 1e-4
    assert conf.min() < 0.2 and conf.max() > 0.8
    assert 0.25 <= np.mean(conf >= thr) <= 0.75
    assert np.abs(conf - thr).min() > 32 * err


def test_host_forward_equals_the_restatement():
    c = cases.case()
    link = AppearanceFreeLink(c['state_dict'], confidence_threshold=c['threshold'])
    t = aflink.build_tracks(c['rows'])
    pairs = np.argwhere(aflink.gate(t['info']))
    assert np.array_equal(pairs, c['pairs']) and list(t['ids']) == ref.tracks(c['rows'])[1]
    conf = link.score_host(t['info'], pairs)
    assert conf.dtype == np.float32 and np.abs(conf - c['conf64']).max() <= 4 * c['ref_err'] + 2.0 ** -23
    got = link.forward(c['rows'])
    want = ref.forward(c['rows'], c['state_dict'], threshold=c['threshold'])
    assert got.shape == want.shape and np.array_equal(got, want)
    assert len(np.unique(got[:, 1])) < len(np.unique(c['rows'][:, 1]))      # links were made
    key = got[:, 0] * 1e8 + got[:, 1]
    assert np.all(np.diff(key) > 0)                                         # ascending frame, then id; no duplicates


# ---------------------------------------------------------------------- evaluators
def fragmented_videos():
    """'gap' of tests/tracklets_ref.py with its predicted track cut in two ids (5, then 6 from frame 7 on)."""
    vids = tracklets_ref.metric_videos()
    pred, gt = vids['gap']
    pred = pred.copy()
    pred[(pred[:, 1] == 5) & (pred[:, 0] >= 7), 1] = 6
    return dict(gap=(pred, gt), plain=vids['plain'])


def test_an_instance_works_in_the_metric_and_the_dict_is_still_refused():
    link = AppearanceFreeLink(None, confidence_threshold=0.0, spatial_threshold=30)
    vids = fragmented_videos()

    def run(**kw):
        m = M.MOTDroneMetrics(metric=['CLEAR', 'Identity'], **kw)
        for v, (pred, gt) in vids.items():
            tracklets_ref.feed_metric(m, v, pred, gt)
        return m.evaluate(distributed=False)
    base, post = run(), run(postprocess_tracklet_cfg=[link])
    assert base['per_video']['gap']['IDSW'] == 1 and post['per_video']['gap']['IDSW'] == 0
    assert post['per_video']['gap']['TP'] == base['per_video']['gap']['TP']
    assert repr(post['per_video']['plain']) == repr(base['per_video']['plain'])
    for t in ('AppearanceFreeLink', 'mmtrack.AppearanceFreeLink'):
        with pytest.raises(NotImplementedError, match='AppearanceFreeLink'):
            M.MOTDroneMetrics(postprocess_tracklet_cfg=[dict(type=t, checkpoint=None)])


def test_an_instance_works_in_evaluate_sweep():
    link = AppearanceFreeLink(None, confidence_threshold=0.0, spatial_threshold=30)
    vids = fragmented_videos()

    def xywh(r):
        r = np.array(r, dtype=np.float64)
        r[:, 4:6] -= r[:, 2:4]
        return r
    preds, gts = [xywh(vids[v][0]) for v in ('gap', 'plain')], [xywh(vids[v][1]) for v in ('gap', 'plain')]
    got = mot_eval.evaluate_sweep(preds, gts, backend='host', postprocess=[link])
    want = mot_eval.evaluate_sweep([link.forward(p) for p in preds], gts, backend='host')
    raw = mot_eval.evaluate_sweep(preds, gts, backend='host')
    assert repr(got) == repr(want)
    assert raw[0]['clear_identity']['IDSW'] == 1 and got[0]['clear_identity']['IDSW'] == 0
