"""GPU: st_rectify_remap (csrc/rectify.hip) bit for bit against the numpy restatement (tests/rectify_ref.py) over sizes,
plane / frame counts, map selections and map kinds; nearest mode; the status of refused calls; the memory contract
(tests/guard_memory.py arenas); then through the MOT shell and MultiStreamTracker on the SGBM config."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import guard_memory as gm
import rectify_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


# ---- maps ----------------------------------------------------------------------------------------------------------------
def _uv(h2, w2):
    v, u = np.mgrid[0:h2, 0:w2]
    return u.astype(np.float64), v.astype(np.float64)


def _q(mx, my):
    return np.stack([np.rint(32 * mx), np.rint(32 * my)], -1).astype(np.int64)


def map_identity(h, w, h2, w2):
    u, v = _uv(h2, w2)
    return _q(u, v)


def map_half_pixel(h, w, h2, w2):                 # a = b = 16 everywhere
    return map_identity(h, w, h2, w2) + 16


def map_warp(h, w, h2, w2):                       # a smooth warp that covers the source, all 32 x 32 fractions
    u, v = _uv(h2, w2)
    mx = u * (w - 1) / max(w2 - 1, 1) + 1.3 * np.sin(v / 5.0 + 0.3) + 0.011 * v + 0.37 * np.sin(u / 3.0)
    my = v * (h - 1) / max(h2 - 1, 1) + 0.9 * np.cos(u / 7.0) - 0.007 * u + 0.23 * np.sin(v / 2.0)
    return _q(mx, my)


def map_leaving(h, w, h2, w2):                    # leaves the image on all four sides (1.5 x zoom out + a shear)
    u, v = _uv(h2, w2)
    du, dv = u - (w2 - 1) / 2, v - (h2 - 1) / 2
    mx = du * 1.5 * w / w2 + (w - 1) / 2 + 0.4 * dv
    my = dv * 1.5 * h / h2 + (h - 1) / 2 + 0.9 * du * h / w2
    return _q(mx, my)


def map_last_cells(h, w, h2, w2):                 # exactly w - 1 / h - 1 with fraction 0 (right half / bottom half)
    u, v = _uv(h2, w2)
    qx = np.where(u >= w2 // 2, 32 * (w - 1), 32 * np.minimum(u, w - 1) - 8 * (u % 3)).astype(np.int64)
    qy = np.where(v >= h2 // 2, 32 * (h - 1), 32 * np.minimum(v, h - 1) - 16 * (v % 2)).astype(np.int64)
    return np.stack([qx, qy], -1)


def map_outside(h, w, h2, w2):                    # fully outside: the host's clip values and the int32 extremes
    u, v = _uv(h2, w2)
    qx = np.choose((u.astype(int) + v.astype(int)) % 4, [-64, 32 * (w + 1), INT_MAX, INT_MIN]).astype(np.int64)
    qy = np.choose((u.astype(int) // 2) % 3, [32 * (h + 1), -64, INT_MIN]).astype(np.int64)
    return np.stack([qx, qy], -1)


MAPS = [map_identity, map_half_pixel, map_warp, map_leaving, map_last_cells, map_outside]


def test_the_map_kinds_are_what_they_claim():
    h, w = 33, 130
    tr = R.taps_read(map_leaving(h, w, h, w), h, w).any(-1)
    assert not tr[0].all() and not tr[-1].all() and not tr[:, 0].all() and not tr[:, -1].all() and tr[h // 2, w // 2]
    assert not R.taps_read(map_outside(h, w, h, w), h, w).any()
    last = map_last_cells(h, w, h, w)
    assert (last[-1, -1] == [32 * (w - 1), 32 * (h - 1)]).all()
    assert R.taps_read(last, h, w)[-1, -1].tolist() == [True, False, False, False]
    assert (map_half_pixel(h, w, h, w) % 32 == 16).all()
    assert len({tuple(c) for c in (map_warp(h, w, h, w) % 32).reshape(-1, 2)}) > 900


# ---- the launch ----------------------------------------------------------------------------------------------------------
def launch(lib, frames, maps, idx, h2, w2, bilinear, border, out_block=None, out_list=None, stream=None):
    f0 = frames[0]
    P, h, w = f0.shape
    src = (C.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
    ix = (C.c_int * len(frames))(*idx)
    dst = None if out_list is None else (C.c_void_p * len(out_list))(*[o.data_ptr() for o in out_list])
    blk = None if out_block is None else C.c_void_p(out_block.data_ptr())
    return lib.st_rectify_remap(src, len(frames), P, h, w, C.c_void_p(maps.data_ptr()), maps.shape[0], ix, dst, blk, h2, w2,
                                f0.element_size(), int(bilinear), border, stream)


def _frames(rng, F, P, h, w, dtype=np.uint8):
    if dtype == np.float32:
        return [rng.standard_normal((P, h, w)).astype(np.float32) for _ in range(F)]
    info = np.iinfo(dtype)
    return [rng.randint(info.min, int(info.max) + 1, (P, h, w)).astype(dtype) for _ in range(F)]


SIZES = [((1, 4), (1, 4)), ((5, 7), (5, 7)), ((33, 130), (33, 130)), ((96, 160), (96, 160)), ((33, 130), (17, 9))]


@pytest.mark.parametrize('F', [1, 3, 16])
@pytest.mark.parametrize('P', [1, 3])
@pytest.mark.parametrize('size,out_size', SIZES)
def test_bilinear_bit_exact_against_the_restatement(cuda, stlib, size, out_size, P, F):
    """Every map kind as map 0 and as map 1 of a two-map launch (pairs (k, k + 1)), map_index alternating (into one
    block) and all frames on map 1 (into separate destinations), border 0 and 200."""
    (h, w), (h2, w2) = size, out_size
    rng = np.random.RandomState(h * 1000 + w + 7 * P + F)
    host = _frames(rng, F, P, h, w)
    frames = [torch.from_numpy(f).to(cuda) for f in host]
    kinds = [m(h, w, h2, w2) for m in MAPS]
    ref = {}                                      # (kind, border) -> frames remapped once

    def want(k, f, border):
        key = (k, f, border)
        if key not in ref:
            ref[key] = R.remap(host[f], kinds[k], True, border)
        return ref[key]

    for k in range(len(MAPS)):
        pair = (k, (k + 1) % len(MAPS))
        maps = torch.from_numpy(np.stack([kinds[pair[0]], kinds[pair[1]]]).astype(np.int32)).to(cuda)
        for border in (0, 200):
            idx = [f % 2 for f in range(F)]
            block = torch.full((F, P, h2, w2), 0x5A, dtype=torch.uint8, device=cuda)
            assert launch(stlib, frames, maps, idx, h2, w2, 1, border, out_block=block) == 0, stlib.st_last_error()
            outs = [torch.full((P, h2, w2), 0xA5, dtype=torch.uint8, device=cuda) for _ in range(F)]
            assert launch(stlib, frames, maps, [1] * F, h2, w2, 1, border, out_list=outs) == 0, stlib.st_last_error()
            got = block.cpu().numpy()
            for f in range(F):
                assert np.array_equal(got[f], want(pair[idx[f]], f, border)), (MAPS[pair[idx[f]]].__name__, border, f)
                assert np.array_equal(outs[f].cpu().numpy(), want(pair[1], f, border)), (MAPS[pair[1]].__name__, border, f)
    if size == out_size:
        assert np.array_equal(want(0, 0, 0), host[0])                       # identity: the frame itself
    assert (want(5, 0, 200) == 200).all() and (want(5, 0, 0) == 0).all()    # fully outside: the border


@pytest.mark.parametrize('dtype', [np.uint8, np.int16, np.float32])
@pytest.mark.parametrize('size,out_size,P', [((5, 7), (5, 7), 1), ((33, 130), (17, 9), 3), ((33, 130), (33, 130), 3)])
def test_nearest_bit_exact_for_1_2_and_4_byte_elements(cuda, stlib, size, out_size, P, dtype):
    (h, w), (h2, w2) = size, out_size
    rng = np.random.RandomState(h + w + P)
    F = 5
    host = _frames(rng, F, P, h, w, dtype)
    frames = [torch.from_numpy(f).to(cuda) for f in host]
    for k in range(len(MAPS)):
        kinds = [MAPS[k](h, w, h2, w2), MAPS[(k + 1) % len(MAPS)](h, w, h2, w2)]
        maps = torch.from_numpy(np.stack(kinds).astype(np.int32)).to(cuda)
        idx = [f % 2 for f in range(F)]
        block = torch.from_numpy(np.full((F, P, h2, w2), 77, dtype)).to(cuda)
        assert launch(stlib, frames, maps, idx, h2, w2, 0, 200, out_block=block) == 0, stlib.st_last_error()
        got = block.cpu().numpy()
        for f in range(F):
            want = R.remap(host[f], kinds[idx[f]], False, 200)
            assert np.array_equal(got[f].view(np.uint8), want.view(np.uint8)), (MAPS[k].__name__, f)
    outside = R.remap(host[0], MAPS[5](h, w, h2, w2), False, 200)
    assert (outside == (200 if dtype == np.uint8 else 0)).all()


def test_refused_calls_return_a_status_and_a_message(cuda, stlib):
    h, w = 8, 12
    f32 = [torch.zeros(1, h, w, device=cuda)]
    u8 = [torch.zeros(1, h, w, dtype=torch.uint8, device=cuda) for _ in range(33)]
    maps = torch.zeros(1, h, w, 2, dtype=torch.int32, device=cuda)
    out = torch.zeros(33, 1, h, w, device=cuda)
    assert launch(stlib, f32, maps, [0], h, w, 1, 0, out_block=out) == -1          # fp32 bilinear: ST_ERR_INVALID
    assert b'bilinear' in stlib.st_last_error()
    assert launch(stlib, f32, maps, [0], h, w, 0, 0, out_block=out) == 0           # ... nearest is the fp32 mode
    assert launch(stlib, u8, maps, [0] * 33, h, w, 1, 0, out_block=out) == -1      # more than 32 frames
    assert launch(stlib, u8[:2], maps, [0, 1], h, w, 1, 0, out_block=out) == -1    # map index outside [0, M)
    assert launch(stlib, u8[:2], maps, [0, 0], h, w, 1, 0) == -1                   # no destination
    assert launch(stlib, u8[:2], maps, [0, 0], h, w, 1, 0, out_block=out, out_list=u8[2:4]) == -1      # both
    assert launch(stlib, u8[:2], maps, [0, 0], h, w, 1, 256, out_block=out) == -1  # border
    two = [torch.zeros(2, h, w, dtype=torch.uint8, device=cuda)]
    assert launch(stlib, two, maps, [0], h, w, 1, 0, out_block=out) == -1          # P = 2
    torch.cuda.synchronize()


# ---- the memory contract -------------------------------------------------------------------------------------------------
def test_memory_contract_guard_bands_stale_outputs_and_sources_that_end_their_allocation(cuda, stlib):
    (h, w), (h2, w2), P, F = (33, 130), (33, 130), 3, 3
    rng = np.random.RandomState(5)
    host = _frames(rng, F, P, h, w)
    kinds = [map_leaving(h, w, h2, w2), map_last_cells(h, w, h2, w2)]
    idx = [0, 1, 1]
    frames = [gm.arena(torch.from_numpy(f), device=cuda) for f in host]
    maps = gm.arena(torch.from_numpy(np.stack(kinds).astype(np.int32)), device=cuda)
    results = []
    for fill in (0xFF, 0x00):
        block = gm.arena(torch.full((F, P, h2, w2), fill, dtype=torch.uint8), device=cuda)
        outs = [gm.arena(torch.full((P, h2, w2), fill, dtype=torch.uint8), device=cuda) for _ in range(F)]
        assert launch(stlib, frames, maps, idx, h2, w2, 1, 9, out_block=block) == 0, stlib.st_last_error()
        assert launch(stlib, frames, maps, idx, h2, w2, 1, 9, out_list=outs) == 0, stlib.st_last_error()
        torch.cuda.synchronize()
        assert gm.bands_intact(block, maps, *frames, *outs), 'a guard band was written'
        results.append((block.cpu().numpy(), [o.cpu().numpy() for o in outs]))
    for f in range(F):
        want = R.remap(host[f], kinds[idx[f]], True, 9)
        for blk, outs in results:                 # over 0xFF and over 0x00: every output byte is written
            assert np.array_equal(blk[f], want) and np.array_equal(outs[f], want)
    for f, hf in zip(frames, host):
        assert np.array_equal(f.cpu().numpy(), hf), 'a source was written'
    assert np.array_equal(maps.cpu().numpy(), np.stack(kinds).astype(np.int32)), 'the maps were written'
    # sources that END their allocation, under the map of last columns / rows: a tap of weight 0 is not read, so the
    # cells behind the last element are never addressed.  (Nothing is provoked: the rule is that the read never happens.)
    nbytes = P * h * w
    size = (nbytes + 511) // 512 * 512            # the allocator's granule: the frame's last byte is the block's last
    tails = []
    for hf in host:
        buf = torch.empty(size, dtype=torch.uint8, device=cuda)
        t = buf[size - nbytes:].view(P, h, w)
        t.copy_(torch.from_numpy(hf))
        tails.append(t)
    last = torch.from_numpy(kinds[1][None].astype(np.int32)).to(cuda)
    block = torch.empty(F, P, h2, w2, dtype=torch.uint8, device=cuda)
    assert launch(stlib, tails, last, [0] * F, h2, w2, 1, 9, out_block=block) == 0, stlib.st_last_error()
    torch.cuda.synchronize()
    for f in range(F):
        assert np.array_equal(block[f].cpu().numpy(), R.remap(host[f], kinds[1], True, 9))


# ---- through the layers above --------------------------------------------------------------------------------------------
ORI = (96, 160)
_K = [[150.0, 0.0, 79.5], [0.0, 150.0, 47.5], [0.0, 0.0, 1.0]]
_P = [[150.0, 0.0, 79.5, 0.0], [0.0, 150.0, 47.5, 0.0], [0.0, 0.0, 1.0, 0.0]]
_EYE = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def _rot(v):
    v = np.asarray(v, np.float64)
    th = np.linalg.norm(v)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx).tolist()


def identity_cal():
    cam = dict(K=_K, D=[0.0] * 4, R=_EYE, P=_P)
    return dict(type='StereoRectify', left=cam, right=dict(cam), size=ORI)


def warping_cal():
    """Rotating and distorting cameras (different left and right), border 0."""
    return dict(type='StereoRectify', size=ORI,
                left=dict(K=[[152.0, 0, 78.0], [0, 151.0, 49.0], [0, 0, 1]], D=[-0.12, 0.03, 0.001, -0.002, 0.01],
                          R=_rot([0.02, -0.03, 0.015]), P=_P),
                right=dict(K=[[149.0, 0, 81.0], [0, 150.5, 46.0], [0, 0, 1]], D=[-0.1, 0.02, -0.001, 0.001],
                           R=_rot([-0.015, 0.02, -0.02]), P=[[150.0, 0.0, 79.5, -30.0], [0.0, 150.0, 47.5, 0.0], [0.0, 0.0, 1.0, 0.0]]))


def _model(cuda, rectify=None, dense_batch=8, inflight=2):
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.synthetic import synthetic_state_dict
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'stereo_yolox_s_mot_airdrone_sgbm.py'))
    for part in ('backbone', 'neck'):
        cfg.model.detector[part]['widen_factor'] = 0.375
    cfg.model.detector.bbox_head.head_module['widen_factor'] = 0.375
    cfg.model.tracker['init_track_thr'] = 0.03
    cfg.model.tracker['obj_score_thr'] = 0.02
    model = MODELS.build(dict(cfg.model, autotune=False, dense_batch=dense_batch, inflight=inflight, rectify=rectify))
    sd = synthetic_state_dict(list(model.detector._table), seed=5, prior_prob=0.2, logit_std=2.5)
    model.detector.load_state_dict(sd, strict=False)
    return model


_SEQ = {}


def _sequence(T):
    """The first T frames of ONE 11-frame synthetic stereo sequence (numpy, built once and left unchanged)."""
    if not _SEQ:
        from stereotracking_amd.sequence import synthetic_sequence
        fr = list(synthetic_sequence(11, 3, ORI[0], ORI[1], 48, seed=2))
        _SEQ.update(left=[f['left'] for f in fr], right=[f['right'] for f in fr])
    return _SEQ['left'][:T], _SEQ['right'][:T]


def _dev(frames, cuda):
    return [torch.from_numpy(f)[None].to(cuda) for f in frames]


def _samples(lo, hi, **extra):
    from stereotracking_amd.structures import TrackDataSample
    return [TrackDataSample(dict(frame_id=t, ori_shape=ORI, img_shape=ORI, scale_factor=(1.0, 1.0), **extra))
            for t in range(lo, hi)]


def _assert_same_results(a_list, b_list, need_tracks=True):
    assert len(a_list) == len(b_list)
    n = 0
    for a, b in zip(a_list, b_list):
        ta, tb = a.pred_track_instances, b.pred_track_instances
        assert ta.instances_id.tolist() == tb.instances_id.tolist()
        for key in ('bboxes', 'scores', 'depth', 'scales'):
            assert torch.equal(ta[key].nan_to_num(-7.0), tb[key].nan_to_num(-7.0)), key
        assert torch.equal(a.pred_det_instances.bboxes, b.pred_det_instances.bboxes)
        assert torch.equal(a.pred_det_instances.scores, b.pred_det_instances.scores)
        n += len(ta)
    assert n > 0 or not need_tracks, 'no tracks in the scenario'


def _step(model, left, right, cuda, lo=0):
    out = model.test_step(dict(inputs=dict(img=_dev(left, cuda), right=_dev(right, cuda)),
                               data_samples=_samples(lo, lo + len(left))))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('T', [2, 11])
def test_shell_identity_calibration_equals_the_shell_without_rectify(cuda, T):
    left, right = _sequence(T)
    _assert_same_results(_step(_model(cuda, identity_cal()), left, right, cuda), _step(_model(cuda), left, right, cuda),
                         need_tracks=T > 2)


@pytest.mark.parametrize('T', [2, 11])
def test_shell_rectify_equals_host_rectified_frames_and_the_per_chunk_split(cuda, T):
    """test_step(raw frames, rectify=cal) == test_step(frames remapped on the host by rectify_ref, rectify=None); at 11
    frames (chunks of 8 + 3) also == the calls of 8 and of 3 frames."""
    from stereotracking_amd.rectify import StereoRectify
    cal = warping_cal()
    left, right = _sequence(T)
    got = _step(_model(cuda, cal), left, right, cuda)
    maps = StereoRectify(**{k: v for k, v in cal.items() if k != 'type'}).maps
    hl = [R.remap(f, maps[0], True, 0) for f in left]
    hr = [R.remap(f, maps[1], True, 0) for f in right]
    assert not np.array_equal(hl[0], left[0]) and not np.array_equal(hr[0], right[0])
    _assert_same_results(got, _step(_model(cuda), hl, hr, cuda), need_tracks=T > 2)
    if T == 11:
        per = _model(cuda, cal)
        split = _step(per, left[:8], right[:8], cuda) + _step(per, left[8:], right[8:], cuda, lo=8)
        _assert_same_results(got, split)


def test_multistream_shares_the_calibration(cuda):
    """Two streams (the sequence and its frames in reverse order) through MultiStreamTracker over a rectifying model:
    each stream receives what the rectifying shell returns for its frames alone."""
    from stereotracking_amd.multistream import MultiStreamTracker
    cal, T = warping_cal(), 4
    left, right = _sequence(T)
    seqs = [(left, right), (left[::-1], right[::-1])]
    # (lowered score gates: a frame of the tiny model starts a few hundred tracks)
    mst = MultiStreamTracker(_model(cuda, cal, dense_batch=2), streams=2, max_tracks=512)
    got = [[], []]
    for t in range(T):
        data = dict(inputs=dict(img=_dev([s[0][t] for s in seqs], cuda), right=_dev([s[1][t] for s in seqs], cuda)),
                    data_samples=[_samples(t, t + 1, stream=s)[0] for s in range(2)])
        for s, out in enumerate(mst.step(data)):
            got[s].append(out)
    torch.cuda.synchronize()
    for s, (l, r) in enumerate(seqs):
        want = _step(_model(cuda, cal, dense_batch=2), l, r, cuda)
        assert len(want) == len(got[s]) == T
        for a, b in zip(got[s], want):
            ta, tb = a.pred_track_instances, b.pred_track_instances
            assert ta.instances_id.tolist() == tb.instances_id.tolist()
            for key in ('bboxes', 'scores', 'depth'):
                assert torch.equal(ta[key].nan_to_num(-7.0).cpu(), tb[key].nan_to_num(-7.0).cpu()), key
