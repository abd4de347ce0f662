"""CPU suite: MultiStreamTracker's construction and per-tick validation errors (all raised on the host, before a device
is touched), and its resolution from a config.  The device path is held to the single-video shell in
tests/test_multistream_gpu.py; the ABI test of test_cpu_oracle_and_abi.py covers the st_stream_* exports."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from stereotracking_amd import _lib, mot  # noqa: F401
from stereotracking_amd.config import Config
from stereotracking_amd.multistream import MultiStreamTracker, StreamOverflow
from stereotracking_amd.registry import MODELS
from stereotracking_amd.structures import TrackDataSample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_STEREO = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'stereo_yolox_s_mot_airdrone_costvolume.py')
ORI = (80, 160)


def model_cfg(**tracker):
    cfg = Config.fromfile(CFG_STEREO)
    for part in ('backbone', 'neck'):
        cfg.model.detector[part]['widen_factor'] = 0.375
    cfg.model.detector.bbox_head.head_module['widen_factor'] = 0.375
    cfg.model.stereo['max_disp'] = 32
    cfg.model.tracker.update(tracker)
    return dict(cfg.model, autotune=False, dense_batch=4)


def tick(streams, frame_ids=None, ori=None):
    n = len(streams)
    frame_ids = frame_ids or [0] * n
    ori = ori or [ORI] * n
    samples = [TrackDataSample(dict(stream=s, frame_id=f, ori_shape=o, scale_factor=(1.0, 1.0)))
               for s, f, o in zip(streams, frame_ids, ori)]
    frames = [torch.zeros(1, 3, *o, dtype=torch.uint8) for o in ori]
    return dict(inputs=dict(img=frames, right=[f.clone() for f in frames]), data_samples=samples)


def test_builds_from_a_config_and_takes_its_options_from_the_wrapped_model():
    mst = MODELS.build(dict(type='MultiStreamTracker', model=model_cfg(), streams=6, max_tracks=32))
    assert isinstance(mst, MultiStreamTracker)
    assert type(mst.model).__name__ == 'OCSORT_Disparity'
    assert mst.chunk == 4 and mst.max_chunks == 2            # S = 6 over dense_batch = 4: two chunks per tick
    assert mst.max_dets == mst.model.max_det and mst.max_tracks == 32
    trk = mst.model.tracker
    assert mst.tracker_options == {k: getattr(trk, k) for k in mst.tracker_options}
    assert set(mst.tracker_options) == {'obj_score_thr', 'init_track_thr', 'weight_iou_with_det_scores',
                                        'match_iou_thr', 'num_tentatives', 'vel_consist_weight', 'vel_delta_t',
                                        'num_frames_retain'}
    built = MODELS.build(model_cfg())
    assert MultiStreamTracker(built, streams=2).model is built and MultiStreamTracker(built, streams=2).chunk == 2
    assert issubclass(StreamOverflow, RuntimeError)


def test_construction_errors():
    with pytest.raises(NotImplementedError, match='OCSORT_Disparity'):
        MultiStreamTracker(model_cfg(cmc=dict(method='glme_affine')), streams=4)
    with pytest.raises(ValueError, match='refuses'):
        MultiStreamTracker(model_cfg(vel_delta_t=9), streams=4)       # the device tracker keeps 8 observations
    with pytest.raises(ValueError, match='streams'):
        MultiStreamTracker(model_cfg(), streams=0)
    with pytest.raises(ValueError, match='streams'):
        MultiStreamTracker(model_cfg(), streams=129)
    with pytest.raises(ValueError, match='max_dets'):
        MultiStreamTracker(model_cfg(), streams=4, max_dets=100000)
    with pytest.raises(TypeError):
        MultiStreamTracker(object(), streams=4)


def test_tick_validation_errors_are_raised_without_a_device():
    mst = MultiStreamTracker(model_cfg(), streams=4)
    with pytest.raises(ValueError, match='empty tick'):
        mst.step(dict(inputs=dict(img=[], right=[]), data_samples=[]))
    with pytest.raises(ValueError, match=r'outside \[0, 4\)'):
        mst.step(tick([0, 4]))
    with pytest.raises(ValueError, match='outside'):
        mst.step(tick([-1]))
    with pytest.raises(ValueError, match='twice'):
        mst.step(tick([1, 2, 1]))
    with pytest.raises(NotImplementedError, match='uniform ori_shape'):
        mst.step(tick([0, 1], ori=[ORI, (96, 160)]))
    with pytest.raises(KeyError, match='stream'):
        mst.step(dict(inputs=dict(img=[torch.zeros(1, 3, *ORI, dtype=torch.uint8)]),
                      data_samples=[TrackDataSample(dict(frame_id=0, ori_shape=ORI))]))
    with pytest.raises(ValueError, match='frame_id'):
        mst.step(tick([0], frame_ids=[-3]))
    with pytest.raises(ValueError, match='at most one frame per stream'):
        mst.step(tick([0, 1, 2, 3, 0]))
    assert mst._dev is None and mst._pending == 0            # nothing was built or launched
    # run() validates the same way, tick by tick
    with pytest.raises(ValueError, match='twice'):
        list(mst.run([tick([0, 0])]))


def test_host_tensors_are_refused_there_is_no_host_fallback():
    cfg = model_cfg()
    cfg['data_preprocessor'] = dict(cfg['data_preprocessor'], device='cpu')     # the frames stay on the host
    mst = MultiStreamTracker(cfg, streams=4)
    with pytest.raises(RuntimeError, match='HIP path only: inputs must be CUDA tensors'):
        mst.step(tick([0, 1]))
    assert mst._dev is None


def test_tick_record_layout_matches_the_header(stlib):
    """The byte layout multistream.py reads the page-locked record with is the one include/stereotrack.h declares."""
    src = open(os.path.join(ROOT, 'include', 'stereotrack.h')).read()
    for name, val in (('ST_STREAM_MAX_STREAMS', 128), ('ST_STREAM_HDR_INTS', 4), ('ST_STREAM_ROW_FLOATS', 10),
                      ('ST_STREAM_DET_FLOATS', 8)):
        assert f'#define {name} {val}\n' in src
    S, T, M = 6, 50, 70
    assert stlib.st_stream_record_bytes(S, T, M) == 8 * S * T + 4 * S * 4 + 4 * S * T * 10 + 4 * S * M * 8
    assert stlib.st_stream_record_bytes(0, T, M) == 0
    assert C.sizeof(_lib.StStreamTick) == 6 * 4 + 2 * C.sizeof(C.c_void_p)


def test_stream_entries_validate_a_tick_on_the_host(stlib):
    """st_stream_* refuse a malformed tick before they launch (ST_ERR_INVALID = -1; no device is needed to get there)."""
    def call(streams, chunk, chunks, slots):
        sl = np.asarray(slots, np.int32)
        fid = np.zeros(max(streams, 1), np.int32)
        t = _lib.StStreamTick(C.sizeof(_lib.StStreamTick), streams, chunk, chunks, 16, 16, sl.ctypes.data, fid.ctypes.data)
        return stlib.st_stream_unscale(C.byref(t), None, None, None, None, None)
    assert call(4, 2, 2, [0, 1, 1, -1]) == -1 and b'twice' in stlib.st_last_error()
    assert call(4, 2, 2, [0, 7, -1, -1]) == -1 and b'names stream 7' in stlib.st_last_error()
    assert call(129, 2, 2, [0, 1, 2, 3]) == -1
    assert call(4, 64, 3, [0] * 192) == -1
    assert call(4, 2, 2, [0, 1, 2, 3]) == -1 and b'null pointer' in stlib.st_last_error()   # a valid tick, null buffers
