"""CPU: what a track KNOWS - the float64 Kalman mean and covariance, the `saved` filter observation-centric recovery
restores, the observation window, the last observation and the velocity direction - pinned for the native host tracker
(csrc/ocsort_tracker.cpp, read through st_tracker_get_states) against the pure-Python backend, field for field, on the
bits, after every step.  The other tracker tests observe ids and rows only, and rows are the detections passed through:
a filter that is wrong in its fifth digit passes them all ("Per-track state": the table of wrong filters
that reproduce all 72 fixture pairs).

Three links make the chain:
  1. native == Python backend driven by tests/kalman_ref.LoopKalmanFilter (the loops of ocsort_tracker.cpp as Python
     floats: IEEE float64, no contraction), exactly, on the 72 stream x option pairs of tests/golden/tracker_options.npz
     and on synthetic streams with an occlusion and duplicates;
  2. the loop filter is a correct filter: every initiate / predict / update call of a shipped-options run against
     mpmath at 50 digits, its error at most 4 x that of motion.KalmanFilter (the numpy / scipy restatement of reference
     mmtrack/models/motion/kalman_filter.py:60-189);
  3. the comparison has teeth (the five wrong filters that pass every row test are each rejected) and the streams reach
     the paths (recovery with saved != kf, long predictions, removal, resets, NaN states, full windows).
tests/test_tracker_state_gpu.py holds the device tracker to the same native state."""
import numpy as np
import pytest

from kalman_ref import LoopKalmanFilter
from stereotracking_amd.motion import KalmanFilter
from stereotracking_amd.synthetic import synthetic_detection_stream
from stereotracking_amd.trackers import OCSORTTracker_Disparity
from tracker_state_utils import (OPTION_CONFIGS, OPTION_STREAMS, PAIRS, SHIPPED, assert_states_equal, option_stream,
                                 run_states, state_differences)

SYNTHETIC = {
    'occlusion_dup': (dict(seed=100, T=48, K=6, occlusion=(1, 10, 16), duplicates=True), 'shipped'),
    'occlusion_long': (dict(seed=104, T=36, K=5, occlusion=(0, 8, 20), duplicates=False), 'vel_delta_t_7'),
    'dup_tentatives_1': (dict(seed=107, T=30, K=7, occlusion=(2, 12, 14), duplicates=True), 'num_tentatives_1'),
}

_NATIVE = {}


def native_trace(stream, cname):
    """The native tracker's state after every step of a fixture pair, computed once."""
    if (stream, cname) not in _NATIVE:
        det, fids = option_stream(stream)
        _NATIVE[stream, cname] = run_states(det, fids, OPTION_CONFIGS[cname])
    return _NATIVE[stream, cname]


def assert_traces_equal(got, ref, what):
    assert len(got) == len(ref)
    for (s, fid, ids, states, nxt), (s2, fid2, ids2, states2, nxt2) in zip(got, ref):
        assert (s, fid) == (s2, fid2)
        assert ids == ids2 and nxt == nxt2, f'{what} step {s}: ids {ids} vs {ids2}, next id {nxt} vs {nxt2}'
        assert_states_equal(states, states2, f'{what} step {s} (frame id {fid})')


# ---- 1. native == Python backend with the loop filter, exactly -------------------------------------------------------
@pytest.mark.parametrize('stream,cname', PAIRS)
def test_native_state_equals_the_python_backend_on_the_fixture(stream, cname):
    det, fids = option_stream(stream)
    py = run_states(det, fids, OPTION_CONFIGS[cname], 'python', LoopKalmanFilter())
    ref = native_trace(stream, cname)
    assert sum(len(r[3]) for r in ref) > 20
    assert_traces_equal(py, ref, f'{stream} / {cname}: Python backend vs native')


@pytest.mark.parametrize('name', sorted(SYNTHETIC))
def test_native_state_equals_the_python_backend_on_synthetic_streams(name):
    kw, cname = SYNTHETIC[name]
    kw = dict(kw)
    det = synthetic_detection_stream(kw.pop('seed'), **kw)
    fids = np.arange(kw['T'])
    cfg = OPTION_CONFIGS[cname]
    ref = run_states(det, fids, cfg)
    assert any(not t['tracked'] for r in ref for t in r[3]), 'the occlusion loses no track'
    assert_traces_equal(run_states(det, fids, cfg, 'python', LoopKalmanFilter()), ref, f'{name}: Python vs native')


def test_native_state_refuses_a_window_longer_than_the_struct():
    from stereotracking_amd._lib import StError
    det, fids = option_stream('single')
    with pytest.raises(StError, match='window of 9 observations'):
        run_states(det, fids[:12], dict(SHIPPED, vel_delta_t=8))
    trk = OCSORTTracker_Disparity(backend='python', **dict(SHIPPED, vel_delta_t=8))
    with pytest.raises(ValueError, match='window'):
        trk.track_states()


def test_native_state_keeps_the_older_accessor():
    """native_state() (st_tracker_get_track) reports the same tracks as track_states()."""
    det, fids = option_stream('occlusion')
    trk = OCSORTTracker_Disparity(backend='native', **SHIPPED)
    from tracker_state_utils import sample
    for s in range(20):
        trk.track(None, None, None, sample(det, s, fids[s]))
    old, new = trk.native_state(), trk.track_states()
    assert len(old) == len(new) > 2
    for o, n in zip(old, new):
        assert (o['id'], o['tentative'], o['tracked'], o['last_frame']) == \
            (n['id'], n['tentative'], n['tracked'], n['last_frame'])
        assert np.array_equal(o['mean'], n['mean']) and np.array_equal(o['covariance'], n['cov'])


# ---- 2. the loop filter is a correct filter ---------------------------------------------------------------------------
class RecordingFilter(KalmanFilter):
    """motion.KalmanFilter that keeps the float64 inputs of every call."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def initiate(self, measurement):
        self.calls.append(('initiate', (np.array(measurement, np.float64),)))
        return super().initiate(measurement)

    def predict(self, mean, covariance):
        self.calls.append(('predict', (np.array(mean, np.float64), np.array(covariance, np.float64))))
        return super().predict(mean, covariance)

    def update(self, mean, covariance, measurement, bbox_score=0.):
        self.calls.append(('update', (np.array(mean, np.float64), np.array(covariance, np.float64),
                                      np.array(measurement, np.float64))))
        return super().update(mean, covariance, measurement)


def mp_truth(kind, args):
    """The call in mpmath at 50 digits -> (mean (8,), cov (8, 8)) as mpf."""
    import mpmath as mp
    mp.mp.dps = 50
    wp, wv = mp.mpf(1) / 20, mp.mpf(1) / 160
    dec = lambda s: mp.mpf(s)  # noqa: E731  (the decimal constants of the reference, not their float64 roundings)
    H = mp.matrix(4, 8)
    F = mp.eye(8)
    for i in range(4):
        H[i, i] = 1
        F[i, i + 4] = 1
    if kind == 'initiate':
        m = [mp.mpf(float(v)) for v in args[0]]
        h = m[3]
        std = [2 * wp * h, 2 * wp * h, dec('1e-2'), 2 * wp * h, 10 * wv * h, 10 * wv * h, dec('1e-5'), 10 * wv * h]
        return mp.matrix(m + [0] * 4), mp.diag([s * s for s in std])
    mean = mp.matrix([mp.mpf(float(v)) for v in args[0]])
    cov = mp.matrix([[mp.mpf(float(v)) for v in row] for row in args[1]])
    h = mean[3]
    if kind == 'predict':
        std = [wp * h, wp * h, dec('1e-2'), wp * h, wv * h, wv * h, dec('1e-5'), wv * h]
        return F * mean, F * cov * F.T + mp.diag([s * s for s in std])
    z = mp.matrix([mp.mpf(float(v)) for v in args[2]])
    std = [wp * h, wp * h, dec('1e-1'), wp * h]
    S = H * cov * H.T + mp.diag([s * s for s in std])
    K = cov * H.T * mp.inverse(S)
    return mean + K * (z - H * mean), cov - K * S * K.T


def scaled_errors(got, truth):
    """max over the elements of |x - truth| / scale: mean[i] by max(|truth_i|, sqrt(P_ii)), cov[i][j] by
    sqrt(P_ii P_jj), P = the true covariance."""
    import mpmath as mp
    tm, tc = truth
    worst = mp.mpf(0)
    for i in range(8):
        sd = mp.sqrt(tc[i, i])
        worst = max(worst, abs(mp.mpf(float(got[0][i])) - tm[i]) / max(abs(tm[i]), sd))
        for j in range(8):
            worst = max(worst, abs(mp.mpf(float(got[1][i, j])) - tc[i, j]) / mp.sqrt(tc[i, i] * tc[j, j]))
    return float(worst)


@pytest.fixture(scope='module')
def filter_calls():
    """Every filter call (float64 inputs) of the Python backend with the shipped options on the six streams; identical
    calls once."""
    rec, seen, calls = RecordingFilter(), set(), []
    for stream in OPTION_STREAMS:
        det, fids = option_stream(stream)
        run_states(det, fids, SHIPPED, 'python', rec)
    for kind, args in rec.calls:
        key = (kind,) + tuple(a.tobytes() for a in args)
        if key not in seen:
            seen.add(key)
            calls.append((kind, args))
    return calls


def test_loop_filter_error_against_mpmath_is_within_4x_of_numpy(filter_calls):
    """Per function: max scaled error of the loop filter <= 4 x that of motion.KalmanFilter, both against mpmath at 50
    digits, over every recorded call with finite inputs (4 = the project's margin for another correct operation
    order).  Measured (the test prints them): initiate 70 calls 3.25e-16 / 3.25e-16 (bit-equal to numpy;
    the residue is the decimal 1e-2 / 1e-5 against their float64 roundings), predict 1342 calls 3.45e-16 / 3.45e-16,
    update 1354 calls 2.85e-15 (loops) / 3.57e-15 (numpy), ratio 0.80."""
    loop, ref = LoopKalmanFilter(), KalmanFilter()
    worst = {k: [0.0, 0.0] for k in ('initiate', 'predict', 'update')}
    used = {k: 0 for k in worst}
    skipped = []
    for n, (kind, args) in enumerate(filter_calls):
        if not all(np.isfinite(a).all() for a in args):
            skipped.append(n)
            continue
        truth = mp_truth(kind, args)
        a, b = getattr(loop, kind)(*args), getattr(ref, kind)(*args)
        if kind == 'initiate':    # squares only: the same single operations in numpy
            assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
            assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
        worst[kind][0] = max(worst[kind][0], scaled_errors(a, truth))
        worst[kind][1] = max(worst[kind][1], scaled_errors(b, truth))
        used[kind] += 1
    # skipped = exactly the calls with a non-finite input (the NaN stream's), and they are a small part
    assert skipped == [n for n, (_, args) in enumerate(filter_calls) if not all(np.isfinite(a).all() for a in args)]
    assert 0 < len(skipped) < len(filter_calls) // 4
    assert used['initiate'] > 30 and used['predict'] > 300 and used['update'] > 300, used
    for kind, (e_loop, e_np) in worst.items():
        ratio = e_loop / e_np if e_np else float('inf') if e_loop else 0.0
        print(f'{kind}: {used[kind]} calls, max scaled error loop {e_loop:.3e}, numpy {e_np:.3e}, ratio {ratio:.3f}')
        assert e_loop <= 4 * e_np, f'{kind}: loop filter {e_loop:.3e} > 4 x numpy {e_np:.3e}'
        assert e_np < 1e-12, f'{kind}: the numpy filter itself is {e_np:.3e} from the truth'


# ---- 3a. the comparison has teeth --------------------------------------------------------------------------------------
class _Cov73(LoopKalmanFilter):
    def update(self, mean, covariance, measurement, bbox_score=0.):
        m, c = super().update(mean, covariance, measurement)
        c[7, 3] *= 0.9
        return m, c


class _Init66(LoopKalmanFilter):
    def initiate(self, measurement):
        m, c = super().initiate(measurement)
        c[6, 6] *= 100
        return m, c


class _UpdateFp32(LoopKalmanFilter):
    def update(self, mean, covariance, measurement, bbox_score=0.):
        m, c = super().update(mean, covariance, measurement)
        return m.astype(np.float32).astype(np.float64), c.astype(np.float32).astype(np.float64)


WRONG_FILTERS = {
    'velocity noise weight x 1.001': lambda: LoopKalmanFilter(w_vel=1.001 / 160),
    'aspect process std 1e-2 -> 2e-2': lambda: LoopKalmanFilter(predict_aspect_std=2e-2),
    'update: cov[7][3] x 0.9': _Cov73,
    'initiate: cov[6][6] x 100': _Init66,
    'update: mean and covariance rounded to fp32': _UpdateFp32,
}


@pytest.mark.parametrize('name', sorted(WRONG_FILTERS))
def test_a_wrong_filter_is_rejected(name):
    """Each of the five filters that reproduce the rows of all 72 fixture pairs gives a state that differs
    from the native tracker's on a fixture stream - and here the rows still agree up to that step."""
    det, fids = option_stream('occlusion')
    ref = native_trace('occlusion', 'shipped')
    got = run_states(det, fids, SHIPPED, 'python', WRONG_FILTERS[name]())
    first = next((k for k, (g, r) in enumerate(zip(got, ref)) if state_differences(g[3], r[3])), None)
    assert first is not None, f'{name}: the state equals the native tracker\'s on every step'
    assert all(g[2] == r[2] for g, r in zip(got[:first + 1], ref)), 'ids already differ: not a blind spot'
    fields = {d.split()[2].rstrip(':') for d in state_differences(got[first][3], ref[first][3])}
    assert fields <= {'mean', 'cov', 'saved_mean', 'saved_cov'}, fields


# ---- 3b. the streams reach the paths ------------------------------------------------------------------------------------
def _by_id(states):
    return {t['id']: t for t in states}


def reached_paths():
    """Which state transitions the native tracker goes through on the 72 fixture pairs (read from its state)."""
    hit = {k: set() for k in ('smooth_gap_1', 'smooth_gap_2plus', 'lost_predicted_3plus', 'removed_at_retain',
                              'tentative_dropped', 'frame0_reset', 'nan_lives_on', 'full_window_shifted')}
    for stream, cname in PAIRS:
        cfg = OPTION_CONFIGS[cname]
        trace = native_trace(stream, cname)
        for (s0, f0, _, st0, _), (s1, f1, ids1, st1, nxt1) in zip(trace, trace[1:]):
            before, after = _by_id(st0), _by_id(st1)
            if f1 == 0:
                if before:
                    assert all(t['last_frame'] == 0 and t['n_fed'] == 1 for t in st1) and nxt1 == len(ids1)
                    hit['frame0_reset'].add((stream, cname))
                continue
            for tid, t in before.items():
                a = after.get(tid)
                if a is None:
                    if t['tentative']:
                        hit['tentative_dropped'].add((stream, cname))
                    elif f1 - t['last_frame'] >= cfg['num_frames_retain']:
                        hit['removed_at_retain'].add((stream, cname))
                    continue
                if not t['tracked'] and a['tracked']:
                    # recovered: online_smooth restored `saved` and ran `trailing_none` virtual updates; at restore
                    # time the filter had been predicted since, so saved != kf
                    assert a['last_frame'] == f1 and t['trailing_none'] >= 1
                    # (the covariance always grows in a predict; a mean with zero velocity stays)
                    assert not np.array_equal(t['saved_cov'], t['cov']) or np.isnan(t['cov']).any()
                    assert np.array_equal(t['saved_cov'], a['saved_cov'], equal_nan=True)
                    hit['smooth_gap_1' if t['trailing_none'] == 1 else 'smooth_gap_2plus'].add((stream, cname))
                if not t['tracked'] and not a['tracked'] and a['trailing_none'] >= 3 and \
                        not np.array_equal(t['mean'][:4], a['mean'][:4], equal_nan=True):
                    hit['lost_predicted_3plus'].add((stream, cname))
                if np.isnan(t['mean']).any() and np.isnan(a['mean']).any():
                    hit['nan_lives_on'].add((stream, cname))
                if a['win_len'] == cfg['vel_delta_t'] + 1 and a['n_obs'] > a['win_len']:
                    hit['full_window_shifted'].add((stream, cfg['vel_delta_t']))
    return hit


def test_the_streams_reach_the_paths():
    hit = reached_paths()
    for path in ('smooth_gap_1', 'smooth_gap_2plus', 'lost_predicted_3plus', 'removed_at_retain', 'tentative_dropped',
                 'frame0_reset', 'nan_lives_on'):
        assert hit[path], f'no fixture pair reaches {path}'
    assert {v for _, v in hit['full_window_shifted']} >= {0, 1, 3, 7}
