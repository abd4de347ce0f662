"""GPU: the per-track state of the batched device tracker (csrc/batched_assoc.hip, read back through
st_batched_tracker_get_states) against the native host tracker's (st_tracker_get_states), field for field, on the bits,
after EVERY step: float64 Kalman mean / covariance, the `saved` filter, the observation window, the last observation,
the velocity direction, every counter and flag (the rule: tests/tracker_state_utils.py).  The host state is itself held
to the Python backend and to mpmath by tests/test_cpu_tracker_state.py.  tests/test_batched_assoc_gpu.py compares the
same two trackers through ids and rows only, which a filter wrong in its fifth digit passes ("Per-track
state"); here the one-wave kf_predict / kf_update, online_smooth's restore of `saved` and push_obs's window shift are
pinned on their numbers."""
import numpy as np
import pytest
import torch

from stereotracking_amd.batched_assoc import BatchedGpuTracker
from stereotracking_amd.synthetic import synthetic_detection_stream
from stereotracking_amd.trackers import OCSORTTracker_Disparity
from tracker_state_utils import (OPTION_CONFIGS, OPTION_STREAMS, SHIPPED, assert_states_equal, option_stream, run_states,
                                 sample, state_differences)

pytestmark = pytest.mark.gpu

STRESS = dict(SHIPPED, obj_score_thr=0.02, init_track_thr=0.05)


def drive(streams, cfg, cuda, max_dets=32, max_tracks=64, read=True):
    """Streams [(det, frame_ids)] through ONE BatchedGpuTracker in lockstep (a step without a frame for a sequence is a
    padding slot, count -1), a native host tracker per sequence beside it.  After every step, for every sequence: ids
    and rows equal the host's; with read=True the device state equals the host tracker's, the header agrees, and a
    sequence that sat the step out holds the state it held before.  -> (per sequence [(step, ids, rows)], number of
    track states compared, steps sat out)."""
    B = len(streams)
    dev = BatchedGpuTracker(B, max_tracks=max_tracks, max_dets=max_dets, device=cuda, **cfg)
    host = [OCSORTTracker_Disparity(backend='native', **cfg) for _ in range(B)]
    out = [[] for _ in range(B)]
    last = [None] * B
    compared = sat_out = 0
    for s in range(max(len(f) for _, f in streams)):
        fid = np.zeros(B, np.int32)
        counts = np.full(B, -1, np.int32)
        dets = np.zeros((B, max_dets, 8), np.float32)
        for b, (det, fids) in enumerate(streams):
            if s >= len(fids) or fids[s] < 0:
                continue
            d = det[det[:, 0] == s]
            k = len(d)
            assert k <= max_dets
            fid[b], counts[b] = fids[s], k
            dets[b, :k, 0:4] = d[:, 1:5]
            dets[b, :k, 4], dets[b, :k, 6], dets[b, :k, 7] = d[:, 5], d[:, 6], d[:, 7]
        rows, ids, n = dev.step(torch.from_numpy(fid).to(cuda), torch.from_numpy(dets).to(cuda),
                                torch.from_numpy(counts).to(cuda))
        rows, ids, n = rows.cpu().numpy(), ids.cpu().numpy(), n.cpu().numpy()
        for b, (det, fids) in enumerate(streams):
            what = f'sequence {b} step {s}'
            if counts[b] < 0:
                assert n[b] == -1
                if read and last[b] is not None:
                    now = dev.sequence_state(b)
                    assert now[0] == last[b][0] and not state_differences(now[1], last[b][1]), \
                        f'{what}: the sequence sat the step out and its state changed'
                    sat_out += 1
                continue
            r = host[b].track(None, None, None, sample(det, s, fids[s]))
            m = int(n[b])
            assert ids[b, :m].tolist() == [int(i) for i in r.instances_id], f'{what}: ids differ'
            out[b].append((s, ids[b, :m].copy(), rows[b, :m].copy()))
            if not read:
                continue
            ref = host[b].track_states()
            hdr, got = dev.sequence_state(b)
            assert hdr == dict(n_tracks=len(ref), next_id=int(host[b].num_tracks), status=0), f'{what}: header {hdr}'
            assert_states_equal(got, ref, f'{what} (frame id {fids[s]}): device vs native host tracker')
            if fids[s] == 0:   # frame id 0 empties the sequence: what lives now was born in this very step
                assert hdr['next_id'] == m == len(got) and all(t['last_frame'] == 0 and t['n_fed'] == 1 for t in got)
            last[b] = (hdr, got)
            compared += len(got)
    return out, compared, sat_out


def peak_track_slots(det, fids, cfg):
    """Track slots the device needs: max over steps of (tracks alive before the step + ids started in it)."""
    peak, alive, nxt = 0, 0, 0
    for _, fid, ids, states, next_id in run_states(det, fids, cfg):
        if fid == 0:
            alive, nxt = 0, 0
        peak = max(peak, alive + sum(i >= nxt for i in ids))
        alive, nxt = len(states), next_id
    return peak


@pytest.mark.parametrize('cname', sorted(OPTION_CONFIGS))
def test_fixture_batch_state_equals_the_host_tracker(cname, cuda):
    """The six streams of tests/golden/tracker_options.npz as ONE batch under each option set (72 pairs): NaN tracks
    that live on, recoveries over gaps of 1 and more (`saved` restored), frame-id gaps, frame-0 resets mid-stream,
    windows of 1 / 2 / 4 / 8 observations.  The gap stream sits steps out: its state must not move."""
    _, compared, sat_out = drive([option_stream(s) for s in OPTION_STREAMS], OPTION_CONFIGS[cname], cuda)
    assert compared > 6 * 48 and sat_out >= 5


def short_sequences():
    return [(synthetic_detection_stream(100 + s, T=48 - (s % 5) * 6, K=4 + s % 4,
                                        occlusion=(1, 10 + s % 7, 16 + s % 7), duplicates=(s % 2 == 0)),
             np.arange(48 - (s % 5) * 6, dtype=np.int32)) for s in range(24)]


def test_many_short_sequences_state_equals_the_host_tracker(cuda):
    """The 24 sequences of test_batched_assoc_gpu.test_many_short_sequences_equal_the_host_tracker (lengths 24 .. 48,
    an occlusion each, duplicates in every other one; max_tracks 64)."""
    _, compared, sat_out = drive(short_sequences(), SHIPPED, cuda, max_dets=32, max_tracks=64)
    assert compared > 24 * 20 * 3 and sat_out > 24


@pytest.mark.parametrize('max_dets,K,dup', [(1, 1, False), (65, 65, False), (130, 120, True)])
def test_capacities_state_equals_the_host_tracker(max_dets, K, dup, cuda):
    """max_dets 1 / 65 / 130 with max_tracks at exactly the peak the stream needs (1, 65, 121: lane loops over tracks
    with a partial last round, the compaction of the track slots after removals)."""
    det = synthetic_detection_stream(300 + K, T=24, K=K, occlusion=(0, 8, 12), duplicates=dup)
    if max_dets == 1:
        det = det[np.unique(det[:, 0], return_index=True)[1]]
    fids = np.arange(24, dtype=np.int32)
    for cname in ('shipped', 'num_tentatives_1'):
        cfg = OPTION_CONFIGS[cname]
        peak = peak_track_slots(det, fids, cfg)
        assert peak % 64 != 0 and peak > max_dets - 16
        _, compared, _ = drive([(det, fids)], cfg, cuda, max_dets=max_dets, max_tracks=peak)
        assert compared >= 24 * min(K, max_dets) // 2


def test_dense_sequence_state_equals_the_host_tracker(cuda):
    """300 objects, 12 frames, the stress thresholds (hundreds of live tracks: every lane round of the Kalman loops)."""
    rng = np.random.RandomState(7)
    T, n_det = 12, 300
    pos = rng.uniform([20, 20], [1260, 700], (n_det, 2))
    vel = rng.uniform(-2, 2, (n_det, 2))
    size = rng.uniform(12, 60, (n_det, 2))
    score = rng.uniform(0.01, 0.9, n_det) ** 2
    rows = []
    for t in range(T):
        p = pos + vel * t + rng.normal(0, 0.5, (n_det, 2))
        keep = rng.uniform(size=n_det) > 0.1
        b = np.concatenate([p - size / 2, p + size / 2], 1)[keep].astype(np.float32)
        sc = (score[keep] + rng.normal(0, 0.005, keep.sum())).clip(0.011, 0.99).astype(np.float32)
        for i in np.argsort(-sc, kind='stable'):
            rows.append([t, *b[i], sc[i], 20.0, 1.5])
    stream = np.asarray(rows, np.float32)
    out, compared, _ = drive([(stream, np.arange(T, dtype=np.int32))], STRESS, cuda, max_dets=512, max_tracks=1024)
    assert max(len(i) for _, i, _ in out[0]) > 150 and compared > T * 150


def test_reading_state_does_not_change_the_following_steps(cuda):
    """The same batch with and without the reads between the steps: the same ids and rows, bit for bit."""
    streams = [option_stream(s) for s in OPTION_STREAMS]
    with_reads, compared, _ = drive(streams, SHIPPED, cuda, read=True)
    without, none, _ = drive(streams, SHIPPED, cuda, read=False)
    assert compared > 0 and none == 0
    for a, b in zip(with_reads, without):
        assert len(a) == len(b) > 10
        for (s, ids, rows), (s2, ids2, rows2) in zip(a, b):
            assert s == s2 and np.array_equal(ids, ids2) and np.array_equal(rows.view(np.uint32), rows2.view(np.uint32))


def test_empty_frame_zero_and_an_overflow(cuda):
    """Frame id 0 empties a sequence even with no detection; an overflowed sequence reports its sticky status and no
    tracks (its slots are not a state any more) while its neighbour carries on; the read leaves the buffer alone."""
    trk = BatchedGpuTracker(2, max_tracks=4, max_dets=8, device=cuda, **dict(SHIPPED, init_track_thr=0.1))
    dets = torch.zeros(2, 8, 8, device=cuda)
    for k in range(8):
        dets[:, k, 0:4] = torch.tensor([20.0 * k, 10.0, 20.0 * k + 15, 40.0], device=cuda)
        dets[:, k, 4] = 0.9
    zero, one = (torch.full((2,), v, dtype=torch.int32, device=cuda) for v in (0, 1))
    trk.step(zero, dets, torch.tensor([3, 2], dtype=torch.int32, device=cuda))
    hdr, tracks = trk.sequence_state(0)
    assert hdr == dict(n_tracks=3, next_id=3, status=0) and [t['id'] for t in tracks] == [0, 1, 2]
    assert all(not t['tentative'] and t['tracked'] and t['win_len'] == 1 and t['n_obs'] == 1 for t in tracks)
    assert all(not t['saved_mean'].any() and not t['saved_cov'].any() for t in tracks)       # no saved filter yet
    # sequence 1 starts 8 tracks > max_tracks = 4: sticky status 1, no tracks; sequence 0 goes on
    trk.step(one, dets, torch.tensor([3, 8], dtype=torch.int32, device=cuda), check_status=False)
    before = trk.state.clone()
    assert trk.sequence_state(1) == (dict(n_tracks=0, next_id=trk.sequence_state(1)[0]['next_id'], status=1), [])
    hdr, tracks = trk.sequence_state(0)
    assert hdr == dict(n_tracks=3, next_id=3, status=0) and all(t['n_fed'] == 2 and t['last_frame'] == 1 for t in tracks)
    assert torch.equal(trk.state, before)
    trk.step(one + 1, dets, torch.tensor([3, 2], dtype=torch.int32, device=cuda), check_status=False)
    assert trk.sequence_state(1)[0]['status'] == 1 and trk.sequence_state(1)[1] == []
    # frame id 0 with no detection at all: both sequences empty, ids start over
    trk.step(zero, dets, torch.zeros(2, dtype=torch.int32, device=cuda))
    for b in range(2):
        assert trk.sequence_state(b) == (dict(n_tracks=0, next_id=0, status=0), [])
