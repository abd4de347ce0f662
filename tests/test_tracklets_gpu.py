"""GPU: the device backend of InterpolateTracklets (csrc/tracklet_post.hip, stereotracking_amd/tracklets.py) against the
host backend (the specification) and the committed mpmath truth (tests/golden/gsi_truth.npz; scenarios and the tolerance:
tests/tracklets_ref.py).

Filled rows are specified bit-equal to the host's: array_equal.  Smoothed coordinates are another correct fp64 evaluation
of an ill-conditioned system: max |device - truth| <= max(4 * ref_err, n * ulp(max |y|)), ref_err = scikit-learn's own
distance from the truth.  Measured on an MI355X (device err / ref_err): see DESIGN.md section 17."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mot_eval_cases as mcases  # noqa: E402
import tracklets_ref as ref  # noqa: E402
from stereotracking_amd import metrics as M  # noqa: E402
from stereotracking_amd import mot_eval, tracklets  # noqa: E402
from stereotracking_amd.tracklets import InterpolateTracklets  # noqa: E402

pytestmark = pytest.mark.gpu
GSI = ref.gsi_cases()
NAMES = sorted(GSI)
TAUS = sorted({int(c['tau']) for c in GSI.values()})


def _device(tau=10, **kw):
    return InterpolateTracklets(use_gsi=True, smooth_tau=tau, backend='device', **kw)


@pytest.fixture(scope='module')
def gsi_alone(cuda):
    """Every fixture case through the device backend in a call of its own, computed once (treat as read-only)."""
    return {n: _device(int(GSI[n]['tau'])).forward_many([ref.gsi_rows(GSI[n])], device=cuda)[0] for n in NAMES}


@pytest.mark.parametrize('mn,mx', [(5, 20), (2, 4)])
def test_linear_rows_equal_the_host_backend(cuda, mn, mx):
    sc = ref.linear_scenarios(mn, mx)
    names = sorted(sc)
    host = InterpolateTracklets(mn, mx)
    got = InterpolateTracklets(mn, mx, backend='device').forward_many([sc[n] for n in names] + [np.zeros((0, 7))], device=cuda)
    assert got[-1].shape == (0, 7)
    for n, g in zip(names, got):
        want = host.forward(sc[n])
        assert g.shape == want.shape and np.array_equal(g, want), n
    one = InterpolateTracklets(mn, mx, backend='device').forward(sc['gaps'])
    assert np.array_equal(one, host.forward(sc['gaps']))


@pytest.mark.parametrize('name', NAMES)
def test_gsi_meets_the_truth_tolerance(gsi_alone, name):
    case, out = GSI[name], gsi_alone[name]
    rows = ref.gsi_rows(case)
    host = InterpolateTracklets(use_gsi=True, smooth_tau=int(case['tau'])).forward(rows)
    assert out.shape == host.shape and np.array_equal(out[:, [0, 1, 6]], host[:, [0, 1, 6]])
    err = float(np.abs(out[:, 2:6].T - case['truth']).max())
    tol = ref.gsi_tolerance(case)
    print(f'{name}: n {len(rows)} device err {err:.3e} ref_err {float(case["ref_err"]):.3e} tol {tol:.3e}')
    assert err <= tol


def test_gsi_is_deterministic_and_batch_invariant(cuda, gsi_alone):
    for tau in TAUS:
        names = [n for n in NAMES if int(GSI[n]['tau']) == tau]
        sets = [ref.gsi_rows(GSI[n]) for n in names]
        among = _device(tau).forward_many(sets, device=cuda)
        again = _device(tau).forward_many(sets, device=cuda)
        rev = _device(tau).forward_many(sets[::-1], device=cuda)[::-1]
        # the cases as tracks of ONE set (ids 1 ..), so that they share a launch's sorted track list in another order
        one = _device(tau).forward_many([np.concatenate([ref.gsi_rows(GSI[n], tid=i + 1) for i, n in enumerate(names)])],
                                        device=cuda)[0]
        for i, n in enumerate(names):
            assert np.array_equal(among[i], gsi_alone[n]), n
            assert np.array_equal(again[i], gsi_alone[n]), n
            assert np.array_equal(rev[i], gsi_alone[n]), n
            mine = one[one[:, 1] == i + 1]
            assert np.array_equal(mine[:, [0, 2, 3, 4, 5, 6]], gsi_alone[n][:, [0, 2, 3, 4, 5, 6]]), n


def _mixed_tracks():
    """40 tracks of 3 .. 256 rows in 4 sets, some with gaps that are filled."""
    rng = np.random.default_rng(7)
    lengths = [3, 256, 129, 128, 17, 200, 64, 5, 6, 255] + rng.integers(3, 257, 30).tolist()
    sets = [[] for _ in range(4)]
    for i, n in enumerate(lengths):
        frames = np.arange(1, n + 1)
        if n > 40 and i % 3 == 0:
            frames = np.concatenate([frames[:20], frames[20:n - 6] + 6])       # a gap of 7: 6 rows are filled back in
        sets[i % 4].append(ref.track(i + 1, frames, seed=i))
    return [np.concatenate(s) for s in sets], lengths


def test_several_launches_equal_one_launch(cuda):
    sets, lengths = _mixed_tracks()
    assert len(lengths) == 40 and min(lengths) == 3 and max(lengths) == 256
    it = _device()
    tracklets.LAUNCHES.clear()
    single = it.forward_many(sets, device=cuda)
    assert tracklets.LAUNCHES['st_tracklet_gsi'] == 1 and tracklets.LAUNCHES['st_tracklet_interpolate'] == 1
    slot = 257 * 256 * 8
    tracklets.LAUNCHES.clear()
    split = it.forward_many(sets, device=cuda, workspace_budget=2 * slot + 4096)
    assert tracklets.LAUNCHES['st_tracklet_gsi'] >= 3 and tracklets.LAUNCHES['st_tracklet_interpolate'] == 1
    for a, b in zip(single, split):
        assert np.array_equal(a, b)
    host = InterpolateTracklets().forward_many(sets)
    for a, h in zip(single, host):
        assert np.array_equal(a[:, [0, 1, 6]], h[:, [0, 1, 6]])
    with pytest.raises(ValueError, match='budget'):
        it.forward_many(sets, device=cuda, workspace_budget=slot - 1)


def test_track_above_the_limit_is_refused_before_any_launch(cuda):
    lim = tracklets.max_track_rows()
    assert lim >= 512
    rows = np.concatenate([ref.track(3, np.arange(1, 40)), ref.track(12, np.arange(1, lim + 2))])
    tracklets.LAUNCHES.clear()
    with pytest.raises(ValueError, match=rf'id 12 .*{lim + 1} rows'):
        _device().forward(rows)
    # filling counts: lim rows + 1 filled
    gap = np.concatenate([np.arange(1, 100), np.arange(101, lim + 2)])
    with pytest.raises(ValueError, match=rf'{lim + 1} rows'):
        _device().forward(ref.track(5, gap))
    assert sum(tracklets.LAUNCHES.values()) == 0
    out = InterpolateTracklets(backend='device').forward(rows)        # the linear part has no limit
    assert len(out) == 39 + lim + 1


def test_longest_supported_track(cuda):
    """A track of st_tracklet_max_rows() rows (the global-workspace path at its largest, every thread owning two rows)
    against its own mpmath truth (tests/golden/gsi_truth_long.npz), with the tolerance rule of the other cases."""
    case = ref.gsi_long_case()
    assert len(case['frames']) == tracklets.max_track_rows() == 512
    rows = ref.gsi_rows(case)
    out = _device().forward_many([rows], device=cuda)[0]
    assert np.array_equal(out[:, [0, 1, 6]], rows[:, [0, 1, 6]])
    err = float(np.abs(out[:, 2:6].T - case['truth']).max())
    tol = ref.gsi_tolerance(case)
    print(f'n512: device err {err:.3e} ref_err {float(case["ref_err"]):.3e} tol {tol:.3e}')
    assert err <= tol


def _metric(**kw):
    m = M.MOTDroneMetrics(ignore_depth=True, **kw)
    for v, (pred, gt) in ref.metric_videos().items():
        ref.feed_metric(m, v, pred, gt)
    return m


def test_metric_device_equals_host_with_linear_interpolation(cuda):
    got = _metric(backend='device', postprocess_tracklet_cfg=[dict(type='InterpolateTracklets')]).evaluate(distributed=False)
    want = _metric(backend='host', postprocess_tracklet_cfg=[dict(type='InterpolateTracklets')]).evaluate(distributed=False)
    assert set(got['per_video']) == set(want['per_video'])
    for v in want['per_video']:
        g, w = got['per_video'][v], want['per_video'][v]
        assert set(g) == set(w)
        for k in w:
            if k in mcases.INT_KEYS:
                assert g[k] == w[k], (v, k)
            else:
                assert abs(g[k] - w[k]) <= 1e-9 * max(1.0, abs(w[k])), (v, k, g[k], w[k])
    assert got['per_video']['gap']['TP'] == 12 and got['per_video']['gap']['FP'] == 0
    for k, w in want['combined'].items():
        assert abs(got['combined'][k] - w) <= 1e-9 * max(1.0, abs(w)), k


def test_metric_with_gsi_scores_the_rows_of_forward_many(cuda):
    tracklets.LAUNCHES.clear()
    m = _metric(backend='device', postprocess_tracklet_cfg=[dict(type='InterpolateTracklets', use_gsi=True)])
    got = m.evaluate(distributed=False)
    assert tracklets.LAUNCHES['st_tracklet_interpolate'] == 1         # all videos in one forward_many call
    videos = sorted(m.pred)
    rows = _device().forward_many([np.asarray(m.pred[v], dtype=np.float64) for v in videos], device=cuda)
    packed = mot_eval.pack_sequences({v: m.gt[v] for v in videos}, dict(zip(videos, rows)))
    direct = dict(zip(packed['videos'], mot_eval.evaluate_packed(packed, 0.5, device=cuda)))
    for v in videos:
        for k, w in direct[v]['clear_identity'].items():
            assert got['per_video'][v][k] == w, (v, k)
        assert got['per_video'][v]['HOTA'] == float(direct[v]['hota']['HOTA'].mean())


def test_evaluate_sweep_with_postprocess_on_the_device(cuda):
    vids = ref.metric_videos()
    def xywh(r):
        r = np.array(r, dtype=np.float64)
        r[:, 4:6] -= r[:, 2:4]
        return r
    preds, gts = [xywh(vids['gap'][0]), xywh(vids['plain'][0])], [xywh(vids['gap'][1]), xywh(vids['plain'][1])]
    got = mot_eval.evaluate_sweep(preds, gts, device=cuda, postprocess=InterpolateTracklets(backend='device'))
    want = mot_eval.evaluate_sweep(preds, gts, backend='host', postprocess=InterpolateTracklets())
    for g, w in zip(got, want):
        mcases.assert_same_scores(g, w, 1e-9)
