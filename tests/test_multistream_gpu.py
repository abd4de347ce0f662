"""GPU: MultiStreamTracker (stereotracking_amd/multistream.py, csrc/stream_track.hip) against the single-video shell.

The yardstick is `model.test_step` on each stream's frames run ALONE (tests/test_config2_oracle_gpu.py and
tests/test_batched_assoc_gpu.py tie that path to the oracle fixtures): over the ticks every stream must receive EQUAL
results - the bits of every float field, list equality on ids, labels and prior_idx, same order - with the same model,
the same frame ids and one and the same launch plan (dense_batch = the chunk size of the multi-stream run;
tests/test_shell_gpu.py:274-277 says why bit equality is a property of one plan).  Equality, not a tolerance: every
stage is bit-reproducible per frame, the batched tracker's rows equal the host tracker's, the unscale is specified
operation by operation.  Nothing under oracle/tracker.py and nothing of the reference tree is read here."""
import json
import os
import time

import numpy as np
import pytest
import torch

from stereotracking_amd.multistream import MultiStreamTracker, StreamOverflow
from stereotracking_amd.structures import TrackDataSample
from stereotracking_amd.synthetic import synthetic_batch
from parity_utils import write_record
from test_shell_gpu import CFG, CFG_STEREO, build_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORI = (80, 160)
FLOAT_FIELDS = ('bboxes', 'scores', 'scales', 'depth', 'gt_depth')
# the tiny models run with lowered score gates (build_model): a frame starts a few hundred tracks, not the shipped ~10
TINY_MAX_TRACKS = 512


# ---- inputs ----------------------------------------------------------------------------------------------------------
def tiny_frames(seeds, cuda, png):
    """One input dict per seed, as a dataset yields a frame: un-padded uint8 images; the stereo config takes left /
    right, the PNG-disparity config the disparity, its mask and a depth map (so that gt_depth differs from depth)."""
    uniq = sorted(set(seeds))
    fr = synthetic_batch(uniq, ORI[0], ORI[1], 32)
    made = {}
    for i, s in enumerate(uniq):
        f = dict(img=fr['img'][i:i + 1, :, :ORI[0]].to(torch.uint8).to(cuda))
        if png:
            f['disp_postp'] = fr['disp_postp'][i:i + 1, :, :ORI[0]].to(cuda)
            f['disp_mask'] = fr['disp_mask'][i:i + 1, :, :ORI[0]].to(torch.uint8).to(cuda)
            f['depth_postp'] = (fr['disp_postp'][i:i + 1, :, :ORI[0]] * 0.75 + 2.0).to(cuda)
        else:
            f['right'] = fr['right'][i:i + 1, :, :ORI[0]].to(torch.uint8).to(cuda)
        made[s] = f
    return [made[s] for s in seeds]


def make_data(frames, metas):
    keys = frames[0].keys()
    return dict(inputs={k: [f[k] for f in frames] for k in keys},
                data_samples=[TrackDataSample(dict(m, ori_shape=ORI, img_shape=ORI, scale_factor=(1.0, 1.0))) for m in metas])


class Schedule:
    """streams[s] = list of (tick, frame id, frame): what stream s shows and when."""

    def __init__(self, streams):
        self.streams = streams
        self.num_ticks = 1 + max(t for st in streams for t, _, _ in st)

    def ticks(self, leave_out=lambda s, t: False):
        """-> per tick (data, [(stream, index into streams[stream])])."""
        for t in range(self.num_ticks):
            present = [(s, i) for s, st in enumerate(self.streams) for i, (tt, _, _) in enumerate(st)
                       if tt == t and not leave_out(s, t)]
            if not present:
                continue
            # not in stream order: the slot of a stream changes from tick to tick
            present = present[t % len(present):] + present[:t % len(present)]
            frames = [self.streams[s][i][2] for s, i in present]
            metas = [dict(stream=s, frame_id=self.streams[s][i][1]) for s, i in present]
            yield make_data(frames, metas), present

    def alone(self, model):
        """model.test_step on each stream's frames alone (one call per stream, the stream's own frame ids)."""
        outs = []
        for st in self.streams:
            data = make_data([f for _, _, f in st], [dict(frame_id=fid) for _, fid, _ in st])
            outs.append(model.test_step(data))
            torch.cuda.synchronize()
        return outs


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_same_sample(got, ref, what):
    dg, dr = got.pred_det_instances, ref.pred_det_instances
    assert set(dg.keys()) == set(dr.keys()) == {'bboxes', 'scores', 'labels', 'prior_idx'}, what
    for k in ('bboxes', 'scores'):
        assert dg[k].dtype == dr[k].dtype and dg[k].shape == dr[k].shape and torch.equal(bits(dg[k]), bits(dr[k])), (what, k)
    for k in ('labels', 'prior_idx'):
        assert dg[k].dtype == dr[k].dtype == torch.int64 and dg[k].tolist() == dr[k].tolist(), (what, k)
    tg, tr = got.pred_track_instances, ref.pred_track_instances
    assert set(tg.keys()) == set(tr.keys()) >= set(FLOAT_FIELDS) | {'labels', 'instances_id'}, what
    assert tg.instances_id.dtype == tr.instances_id.dtype == torch.int64
    assert tg.instances_id.tolist() == tr.instances_id.tolist(), (what, 'instances_id')
    assert tg.labels.dtype == tr.labels.dtype and tg.labels.tolist() == tr.labels.tolist(), (what, 'labels')
    for k in FLOAT_FIELDS:
        assert tg[k].dtype == tr[k].dtype and tg[k].shape == tr[k].shape, (what, k)
        assert tg[k].device == tr[k].device
        assert torch.equal(bits(tg[k]), bits(tr[k])), (what, k, tg[k], tr[k])
    for k in ('frame_id', 'ori_shape', 'batch_input_shape', 'pad_shape'):
        assert got.metainfo.get(k) == ref.metainfo.get(k), (what, k)


def run_and_compare(mst, sched, ref, use_run=False, leave_out=lambda s, t: False):
    """Drive the schedule through step() (or run()); every returned sample equals the alone run's.  -> samples seen."""
    plan = list(sched.ticks(leave_out))
    if use_run:
        results = list(mst.run(d for d, _ in plan))
    else:
        results = [mst.step(d) for d, _ in plan]
    torch.cuda.synchronize()
    seen = 0
    for (data, present), outs in zip(plan, results):
        assert len(outs) == len(present)
        for (s, i), o, given in zip(present, outs, data['data_samples']):
            assert o is given and o.metainfo['stream'] == s              # the samples given, in the order given
            assert_same_sample(o, ref[s][i], f'stream {s} frame {i}')
            seen += 1
    return seen


def assert_scenario_tracks(ref):
    """Inputs that track nothing prove nothing: every stream produced tracks, some stream handed out an id > 0, and
    some track outlived a missed detection (present, absent in a later frame of its video, present again)."""
    print('track rows per frame:', [[len(o.pred_track_instances) for o in outs] for outs in ref])
    assert all(sum(len(o.pred_track_instances) for o in outs) > 0 for outs in ref)
    assert max(int(o.pred_track_instances.instances_id.max()) for outs in ref for o in outs
               if len(o.pred_track_instances)) > 0
    outlived = False
    for outs in ref:
        start = 0
        for j in range(1, len(outs) + 1):      # videos of a slot: split where the frame id restarts at 0
            if j == len(outs) or outs[j].metainfo['frame_id'] == 0:
                sets = [set(o.pred_track_instances.instances_id.tolist()) for o in outs[start:j]]
                for a in range(len(sets)):
                    for b in range(a + 1, len(sets)):
                        for c in range(b + 1, len(sets)):
                            outlived |= bool((sets[a] & sets[c]) - sets[b])
                start = j
    assert outlived, 'no track of the scenario outlived a missed detection'


def video(seeds, frames_of, start_tick=0, first_id=0, skip=()):
    """A video shown from `start_tick`, one frame per tick; ticks in `skip` are missed (the frame ids jump)."""
    fr = frames_of(seeds)
    return [(start_tick + k, first_id + k, fr[k]) for k in range(len(seeds)) if start_tick + k not in skip]


# A frame shown several times keeps its tracks matched; another frame in between is a missed detection for them.
A, B_, C_, D_ = [11, 11, 11, 11, 12, 11, 11, 11, 11, 13, 11, 11], [21, 21, 21, 22, 21, 21, 21, 21, 21], \
    [31, 31, 31, 31, 32], [41, 41, 41, 42, 42, 41, 41, 41, 43, 41, 41, 41]


def ragged_schedule(frames_of):
    """S = 4 over 12 ticks: lengths 12 / 9 / 5 (+ a second video) / 12; stream 1 is absent for ticks 4-6 and returns
    (its frame ids jump), slot 2's video ends after 5 frames and a new one starts with frame_id 0 at tick 6."""
    return Schedule([video(A, frames_of),
                     video([21, 21, 21, 21, 0, 0, 0, 21, 22, 21, 21, 21], frames_of, skip=(4, 5, 6)),
                     video(C_, frames_of) + video([33, 33, 33, 34, 33, 33], frames_of, start_tick=6),
                     video(D_, frames_of)])


# ---- 1. lockstep equals each video alone ----------------------------------------------------------------------------
@pytest.mark.parametrize('config', ['stereo', 'png'])
def test_lockstep_equals_each_video_alone(config, cuda):
    png = config == 'png'
    model, _, _ = build_model(CFG if png else CFG_STEREO, cuda, autotune=False)
    model.dense_batch = 4
    sched = ragged_schedule(lambda seeds: tiny_frames(seeds, cuda, png))
    assert [len(s) for s in sched.streams] == [12, 9, 11, 12] and sched.num_ticks == 12
    ref = sched.alone(model)
    assert_scenario_tracks(ref)
    if png:      # the depth map is not the disparity's depth: the gt column is a column of its own
        assert any(not torch.equal(bits(o.pred_track_instances.depth), bits(o.pred_track_instances.gt_depth))
                   for outs in ref for o in outs)
    mst = MultiStreamTracker(model, streams=4, max_tracks=TINY_MAX_TRACKS)
    assert mst.chunk == 4
    assert run_and_compare(mst, sched, ref) == 44


# ---- 2. run() equals step() -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('inflight', [1, 2, 3])
@pytest.mark.parametrize('queue_depth', [1, 2])
def test_run_equals_step(inflight, queue_depth, cuda):
    model, _, _ = build_model(CFG_STEREO, cuda, autotune=False)
    model.dense_batch, model.inflight, model.queue_depth = 4, inflight, queue_depth
    sched = ragged_schedule(lambda seeds: tiny_frames(seeds, cuda, False))
    mst = MultiStreamTracker(model, streams=4, max_tracks=TINY_MAX_TRACKS)
    stepped = [mst.step(d) for d, _ in sched.ticks()]
    torch.cuda.synchronize()
    assert len(model.dense_runner(ORI, True, 4)) == inflight
    ran = list(mst.run(d for d, _ in sched.ticks()))          # every stream restarts at frame_id 0: same tracker, reset
    torch.cuda.synchronize()
    assert len(ran) == len(stepped) == 12
    n_tracks = 0
    for t, (a, b) in enumerate(zip(ran, stepped)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x.metainfo['stream'] == y.metainfo['stream']
            assert_same_sample(x, y, f'tick {t} stream {x.metainfo["stream"]}')
            n_tracks += len(x.pred_track_instances)
    assert n_tracks > 0
    # and both equal the alone runs
    assert run_and_compare(mst, sched, sched.alone(model), use_run=True) == 44


# ---- 3. S larger than the dense batch -------------------------------------------------------------------------------
def test_more_streams_than_the_dense_batch(cuda):
    model, _, _ = build_model(CFG_STEREO, cuda, autotune=False)
    model.dense_batch, model.inflight = 4, 2
    fo = lambda seeds: tiny_frames(seeds, cuda, False)     # noqa: E731
    sched = Schedule([video(A[:8], fo), video(B_[:8], fo, skip=(5,)), video(C_ + C_[:3], fo), video(D_[:8], fo),
                      video([51, 51, 51, 52, 51, 51], fo, start_tick=2), video([61, 61, 61, 61, 62, 61, 61], fo, start_tick=1)])
    ref = sched.alone(model)
    assert all(sum(len(o.pred_track_instances) for o in outs) > 0 for outs in ref)
    mst = MultiStreamTracker(model, streams=6, max_tracks=TINY_MAX_TRACKS)
    assert (mst.chunk, mst.max_chunks) == (4, 2)            # two chunks per tick, one association step
    seen = run_and_compare(mst, sched, ref)
    assert seen == sum(len(s) for s in sched.streams)
    runner = model.dense_runner(ORI, True, 4)
    assert runner.batch == 4 and len(model._dense) == 1     # ONE launch plan served the alone runs and the ticks
    assert run_and_compare(mst, sched, ref, use_run=True) == seen


# ---- 4. full size ---------------------------------------------------------------------------------------------------
def test_full_size_eight_streams_equal_each_sequence_alone(cuda):
    """The two configs[2] sequences (tests/golden/config2_sequence.npz, regenerated from their seeds) as eight streams:
    four start offsets of each, so that in every tick the streams stand at different frames.  Shipped thresholds, the
    committed tuning plan, dense_batch = 8, max_dets = the fixture's max_det.  The per-stream row counts and the tick
    time are written as the record multistream_config2.json, where parity_utils.write_record keeps the suite's records
    (a record, not an assertion)."""
    from test_config2_oracle_gpu import GOLD, SEQUENCES, build, frames_u8
    g = np.load(GOLD)
    T, H, W = int(g['T']), int(g['H']), int(g['W'])
    model = build({}, g)
    assert model.dense_batch == 8 and model.autotune
    seqs, ref = [], []
    for name, (_, smooth) in SEQUENCES.items():
        left, right = frames_u8(g, cuda, smooth)
        seqs.append((left, right))
        samples = [TrackDataSample(dict(frame_id=t, ori_shape=(H, W), img_shape=(H, W), scale_factor=(1.0, 1.0)))
                   for t in range(T)]
        ref.append(model.test_step(dict(inputs=dict(img=left, right=right), data_samples=samples)))
        torch.cuda.synchronize()
    assert all(sum(len(o.pred_track_instances) for o in outs) > 0 for outs in ref)
    offsets = (0, 3, 7, 13)
    mst = MultiStreamTracker(model, streams=8, max_dets=int(g['max_det']))
    assert mst.chunk == 8 and mst.max_dets == int(g['max_det'])
    rows = [dict(sequence=list(SEQUENCES)[s // 4], offset=offsets[s % 4], detections=0, tracks=0) for s in range(8)]
    tick_ms = []
    for k in range(T + max(offsets)):
        present = [(s, k - offsets[s % 4]) for s in range(8) if 0 <= k - offsets[s % 4] < T]
        present = present[k % len(present):] + present[:k % len(present)]
        data = dict(inputs=dict(img=[seqs[s // 4][0][f] for s, f in present], right=[seqs[s // 4][1][f] for s, f in present]),
                    data_samples=[TrackDataSample(dict(stream=s, frame_id=f, ori_shape=(H, W), img_shape=(H, W),
                                                       scale_factor=(1.0, 1.0))) for s, f in present])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = mst.step(data)
        torch.cuda.synchronize()
        tick_ms.append((time.perf_counter() - t0) * 1e3)
        assert len(outs) == len(present)
        for (s, f), o in zip(present, outs):
            assert_same_sample(o, ref[s // 4][f], f'tick {k} stream {s} frame {f}')
            rows[s]['detections'] += len(o.pred_det_instances)
            rows[s]['tracks'] += len(o.pred_track_instances)
    full = [ms for k, ms in enumerate(tick_ms) if k >= max(offsets) and k < T]        # ticks with all 8 streams present
    rec = dict(what='MultiStreamTracker.step, 8 streams (2 configs[2] sequences x 4 start offsets), 1280x720, D=192, '
                    'dense_batch 8, shipped thresholds; every stream equal to model.test_step on its sequence alone',
               frames_per_stream=T, streams=rows, ticks=len(tick_ms),
               tick_sync_ms=dict(first=tick_ms[0], median_full_ticks=float(np.median(full)), max_full_ticks=max(full)))
    print(json.dumps(rec))
    write_record('multistream_config2.json', rec)


# ---- 5. overflow is surfaced per stream -----------------------------------------------------------------------------
def track_slots_per_step(model, frames):
    """Track slots the device tracker needs at every step of a video: tracks alive before the step + ids started in it,
    from the native host tracker behind model.test_step (tests/test_batched_assoc_gpu.py::peak_track_slots)."""
    need = []
    for fid, f in enumerate(frames):
        trk = model.tracker
        alive = 0 if fid == 0 else len(trk.native_state())
        first_new = 0 if fid == 0 else int(trk.num_tracks)
        out = model.test_step(make_data([f], [dict(frame_id=fid)]))[0]
        need.append(alive + int((out.pred_track_instances.instances_id >= first_new).sum()))
    return need


def test_overflow_is_surfaced_per_stream(cuda):
    """max_tracks below what ONE stream needs.  The scenario is built from the alone path: of a pool of still videos
    the one that needs the most track slots in its first 3 frames is stream 1's, the two that need the fewest are the
    others', and max_tracks is one less than stream 1 needs.  Stream 1 is left out after its overflow and restarts at
    tick 3 (frame_id 0) with a video that fits.  This reads a status word the kernel already writes; it provokes
    nothing on the device."""
    model, _, _ = build_model(CFG_STEREO, cuda, autotune=False)
    model.dense_batch = 3
    pool = list(range(70, 78))
    frames = dict(zip(pool, tiny_frames(pool, cuda, False)))
    need = {s: track_slots_per_step(model, [frames[s]] * 7) for s in pool}
    print('track slots per step:', need)
    big = max(pool, key=lambda s: max(need[s][:3]))
    small, small2 = sorted((s for s in pool if s != big), key=lambda s: max(need[s]))[:2]
    cap = max(need[big][:3]) - 1
    assert 0 < max(need[small]) <= cap and max(need[small2]) <= cap, (cap, need)      # the others fit, stream 1 does not
    t_over = next(i for i, v in enumerate(need[big][:3]) if v > cap)
    fo = lambda seeds: [frames[s] for s in seeds]     # noqa: E731
    sched = Schedule([video([small] * 7, fo), video([big] * 3, fo) + video([small2] * 4, fo, start_tick=3),
                      video([small2] * 7, fo)])
    ref = sched.alone(model)
    mst = MultiStreamTracker(model, streams=3, max_tracks=cap)
    plan = list(sched.ticks(leave_out=lambda s, t: s == 1 and t_over < t < 3))    # the poisoned stream is left out
    assert len(plan) == 7
    for t, (data, present) in enumerate(plan):
        if t == t_over:
            with pytest.raises(StreamOverflow, match='max_tracks') as exc:
                mst.step(data)
            e = exc.value
            assert e.streams == [1] and e.status == [1] and f'max_tracks={cap}' in str(e)
            outs = e.results
            present = [(s, i) for s, i in present if s != 1]
        else:
            outs = mst.step(data)
        assert len(outs) == len(present) and any(s == 1 for s, _ in present) == (t < t_over or t >= 3)
        for (s, i), o in zip(present, outs):
            assert_same_sample(o, ref[s][i], f'tick {t} stream {s}')
    # a stream that is NOT left out keeps reporting its sticky status until it restarts, and the others keep their results
    mst2 = MultiStreamTracker(model, streams=3, max_tracks=cap)
    for t, (data, present) in enumerate(sched.ticks()):
        if t_over <= t < 3:
            with pytest.raises(StreamOverflow) as exc:
                mst2.step(data)
            assert exc.value.streams == [1] and exc.value.status == [1]
            outs, present = exc.value.results, [(s, i) for s, i in present if s != 1]
        else:
            outs = mst2.step(data)
        assert len(outs) == len(present)
        for (s, i), o in zip(present, outs):
            assert_same_sample(o, ref[s][i], f'sticky: tick {t} stream {s}')


# ---- 6. empty frames and thin ticks ---------------------------------------------------------------------------------
def test_frames_without_detections(cuda):
    """A score threshold nothing passes: empty containers with the right shapes, keys and dtypes (what
    test_shell_gpu.py::test_frames_without_detections_and_ragged_calls checks for the shell), full and thin ticks."""
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.synthetic import synthetic_state_dict
    cfg = Config.fromfile(CFG_STEREO)
    for part in ('backbone', 'neck'):
        cfg.model.detector[part]['widen_factor'] = 0.375
    cfg.model.detector.bbox_head.head_module['widen_factor'] = 0.375
    cfg.model.stereo['max_disp'] = 32
    cfg.model.detector.test_cfg['score_thr'] = 0.9999
    mst = MODELS.build(dict(type='MultiStreamTracker', streams=5, max_tracks=16,
                            model=dict(cfg.model, autotune=False, dense_batch=4, inflight=2)))
    model = mst.model
    table = list(model.detector._table) + [('stereo.' + n, shp) for n, shp in model.stereo.param_table()]
    sd = synthetic_state_dict(table, seed=5)
    model.detector.load_state_dict(sd, strict=False)
    model.stereo.load_state_dict({k[len('stereo.'):]: v for k, v in sd.items() if k.startswith('stereo.')})
    fr = tiny_frames(list(range(60, 65)), cuda, False)
    for t, streams in enumerate(([0, 1, 2, 3, 4], [3], [4, 0])):
        outs = mst.step(make_data([fr[s] for s in streams], [dict(stream=s, frame_id=t) for s in streams]))
        torch.cuda.synchronize()
        assert [o.metainfo['stream'] for o in outs] == streams
        for o in outs:
            det, trk = o.pred_det_instances, o.pred_track_instances
            assert len(det) == 0 and len(trk) == 0
            assert tuple(det.bboxes.shape) == (0, 4) and det.bboxes.dtype == torch.float32
            assert tuple(det.scores.shape) == (0,) and det.labels.dtype == det.prior_idx.dtype == torch.int64
            assert set(trk.keys()) >= {'bboxes', 'labels', 'scores', 'scales', 'depth', 'gt_depth', 'instances_id'}
            assert tuple(trk.bboxes.shape) == (0, 4) and tuple(trk.depth.shape) == (0,)
            assert trk.instances_id.dtype == trk.labels.dtype == torch.int64
            assert o.metainfo['batch_input_shape'] == (96, 160) and o.metainfo['pad_shape'] == ORI


def test_ticks_with_a_single_present_stream(cuda):
    """Thin ticks: S = 4 with ONE stream present per tick (the dense chunk is padded, three slots reach the tracker with
    count -1), the streams taking turns; equal to the alone runs."""
    model, _, _ = build_model(CFG_STEREO, cuda, autotune=False)
    model.dense_batch = 4
    fo = lambda seeds: tiny_frames(seeds, cuda, False)     # noqa: E731
    vids = [A[:6], B_[:6], D_[:6], [81, 81, 81, 82, 81, 81]]
    # stream s shows frame k of its video at tick 4 k + s
    sched = Schedule([[(4 * k + s, k, f) for k, f in enumerate(fo(v))] for s, v in enumerate(vids)])
    ref = sched.alone(model)
    assert all(sum(len(o.pred_track_instances) for o in outs) > 0 for outs in ref)
    mst = MultiStreamTracker(model, streams=4, max_tracks=TINY_MAX_TRACKS)
    plan = list(sched.ticks())
    assert len(plan) == 24 and all(len(p) == 1 for _, p in plan)
    assert run_and_compare(mst, sched, ref) == 24


# ---- 7. ragged chunks through the cast-and-pad branch ---------------------------------------------------------------
def test_ragged_chunks_without_the_raw_stem(cuda, monkeypatch):
    """raw_stem off, S = 3 over dense_batch = 2: a tick of three frames ends in a ragged chunk, padded by repeating its
    frame, and every chunk is cast + padded in a pass of its own (shell_inputs.chunk_inputs' second branch, which the
    other tests here, with the raw stem on, never reach).  Stream 1 is absent in tick 2.  Equal to the alone runs."""
    from stereotracking_amd.shell_inputs import RawFrames
    calls = dict(chunk=0, raw_chunk=0)
    for name in calls:
        def spy(self, *args, _name=name, _orig=getattr(RawFrames, name)):
            calls[_name] += 1
            return _orig(self, *args)
        monkeypatch.setattr(RawFrames, name, spy)
    model, _, _ = build_model(CFG_STEREO, cuda, autotune=False)
    model.dense_batch, model.raw_stem = 2, False
    fo = lambda seeds: tiny_frames(seeds, cuda, False)     # noqa: E731
    sched = Schedule([video(A[:4], fo), video(B_[:4], fo, skip=(2,)), video(D_[:4], fo)])
    assert sched.num_ticks == 4 and [len(s) for s in sched.streams] == [4, 3, 4]
    ref = sched.alone(model)
    assert all(sum(len(o.pred_track_instances) for o in outs) > 0 for outs in ref)
    mst = MultiStreamTracker(model, streams=3, max_tracks=TINY_MAX_TRACKS)
    assert (mst.chunk, mst.max_chunks) == (2, 2)
    calls.update(chunk=0, raw_chunk=0)
    assert run_and_compare(mst, sched, ref) == 11
    # 3 + 3 + 2 + 3 frames = 2 + 2 + 1 + 2 chunks, left and right converted for each; no chunk went to the stems raw
    assert calls == dict(chunk=14, raw_chunk=0)
