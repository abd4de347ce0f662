"""GPU: every stage of the camera-motion kernels (csrc/cmc_flow.hip) against the numpy restatement (tests/cmc_ref.py)
across batch sizes, frame geometries and glme options - the scenarios of tests/cmc_cases.py, whose preconditions
tests/test_cpu_cmc.py asserts without a GPU.  The two later stages are entered through st_cmc_mesh_fit / st_cmc_fit
(cmc.mesh_fit / cmc.fit), which run the launches of st_cmc_estimate on a given flow field / point set."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmc_cases as K
import cmc_ref as R
from test_cpu_cmc import CORNER_TOL, _corner_error

pytestmark = pytest.mark.gpu
H, W = K.IMG_H, K.IMG_W


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


# ---- front -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geometry', K.GEOMETRIES, ids=K.geometry_id)
def test_front_bit_exact_per_geometry(geometry, cuda):
    """Crop, resize (down, up, identity, odd, portrait), grey and equalizeHist (constant, two-valued, all-but-one)
    equal the restatement bit for bit, from the uint8 list and from padded fp32 canvases with the crop strictly inside."""
    from stereotracking_amd import cmc
    fh, fw, h, w = geometry
    frames = [K.front_frame(kind, geometry) for kind in K.FRONT_KINDS]
    want = np.stack([R.front(f, h, w) for f in frames])
    got_u8 = cmc.front([_dev(f[None], cuda) for f in frames], h, w).cpu().numpy()
    canvases = np.stack([K.canvas_f32(f, h, w) for f in frames])
    assert canvases.shape[2] > h and canvases.shape[3] > w and canvases[0, 0, -1, -1] == K.PAD_VALUE
    got_f32 = cmc.front(_dev(canvases, cuda), h, w).cpu().numpy()
    for i, kind in enumerate(K.FRONT_KINDS):
        assert np.array_equal(got_u8[i], want[i]), f'uint8 list, {kind}: {(got_u8[i] != want[i]).sum()} pixels differ'
        assert np.array_equal(got_f32[i], want[i]), f'fp32 batch, {kind}: {(got_f32[i] != want[i]).sum()} pixels differ'
    # integral values outside 0..255 saturate as numpy's clip + astype(uint8)
    o = K.out_of_range_f32(geometry)
    got = cmc.front(_dev(o[None], cuda), h, w).cpu().numpy()[0]
    assert np.array_equal(got, R.front(np.clip(o, 0, 255).astype(np.uint8), h, w))


def test_front_u8_list_crosses_the_32_frame_chunk(cuda):
    from stereotracking_amd import cmc
    fh, fw, h, w = K.FRONT_BATCH_GEOMETRY
    frames = [K.front_frame('random', K.FRONT_BATCH_GEOMETRY, seed=i) for i in range(K.FRONT_BATCH)]
    out = torch.full((K.FRONT_BATCH + 1, 255, 255), 7, dtype=torch.uint8, device=cuda)
    cmc.front([_dev(f[None], cuda) for f in frames], h, w, out=out[:K.FRONT_BATCH])
    got = out.cpu().numpy()
    for i, f in enumerate(frames):
        assert np.array_equal(got[i], R.front(f, h, w)), f'plane {i} of {K.FRONT_BATCH}'
    assert np.all(got[K.FRONT_BATCH] == 7), 'wrote past the last plane'


# ---- flow ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene_planes(cuda):
    """Device planes of the three scenes, (3, 255, 255) prev and curr; they are the restatement's planes bit for bit."""
    from stereotracking_amd import cmc
    prev, curr = [], []
    for name in K.FLOW_SCENES:
        f0, f1 = K.scene_frames(name)
        p = cmc.front([_dev(K.grey_to_bgr(f)[None], cuda) for f in (f0, f1)], H, W)
        want = K.scene_planes(name)
        assert np.array_equal(p[0].cpu().numpy(), want[0]) and np.array_equal(p[1].cpu().numpy(), want[1])
        prev.append(p[0])
        curr.append(p[1])
    return torch.stack(prev), torch.stack(curr)


@pytest.mark.parametrize('winsize', K.FLOW_WINSIZES)
def test_flow_per_level_per_window_and_pair(winsize, scene_planes, cuda):
    """|gpu - ref64|max <= 2 |ref32 - ref64|max + 1e-5 per level, for every pair of an N = 3 batch of different motions
    at every window; and each pair of the batch equals its own N = 1 run bit for bit (per-pair workspace indexing)."""
    from stereotracking_amd import cmc
    prev, curr = scene_planes
    flow, lev = cmc.flow(prev, curr, winsize, per_level=True)
    assert len(lev) == 3 and torch.equal(_bits(flow), _bits(lev[0]))
    failures = []
    for n, name in enumerate(K.FLOW_SCENES):
        pp, pc = K.scene_planes(name)
        ref64 = R.farneback(pp, pc, winsize, np.float64, per_level=True)
        ref32 = R.farneback(pp, pc, winsize, np.float32, per_level=True)
        for k, (g, r64, r32) in enumerate(zip(lev, ref64, ref32)):
            d_gpu = np.abs(g[n].cpu().numpy().astype(np.float64) - r64).max()
            d_32 = np.abs(r32.astype(np.float64) - r64).max()
            print(f'flow winsize {winsize} pair {name} level {k}: gpu {d_gpu:.3g} fp32 restatement {d_32:.3g}')
            if not d_gpu <= 2 * d_32 + 1e-5:
                failures.append(f'{name} level {k}: gpu {d_gpu:.3g} vs fp32 restatement {d_32:.3g}')
        one, lev1 = cmc.flow(prev[n:n + 1], curr[n:n + 1], winsize, per_level=True)
        assert torch.equal(_bits(one[0]), _bits(flow[n])), f'pair {n} of the batch differs from its N = 1 run'
        for a, b in zip(lev1, lev):
            assert torch.equal(_bits(a[0]), _bits(b[n])), f'pair {n}: a level differs from its N = 1 run'
    assert not failures, failures


# ---- mesh ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def device_flow(scene_planes):
    from stereotracking_amd import cmc
    prev, curr = scene_planes
    return cmc.flow(prev, curr, 31)          # (3, 255, 255, 2)


@pytest.mark.parametrize('size', K.MESH_SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('step', K.MESH_STEPS)
def test_mesh_equals_restatement(step, size, device_flow, cuda):
    """Per-cell medians (odd and even counts, exact ties, -0.0) and the double scaling by the image size: array_equal
    with R.mesh for every field of one batch, through the flow injection point."""
    from stereotracking_amd import cmc
    fields = dict(K.flow_fields())
    for n, name in enumerate(K.FLOW_SCENES):
        fields['device flow: ' + name] = device_flow[n].cpu().numpy()
    batch = _dev(np.stack(list(fields.values())), cuda)
    _, mesh, _ = cmc.mesh_fit(batch, size[0], size[1], dict(step=step), with_mesh=True)
    mesh = mesh.cpu().numpy()
    assert mesh.shape == (len(fields), (255 // step) ** 2, 4)
    for n, (name, f) in enumerate(fields.items()):
        src, dst = R.mesh(f, size[0], size[1], step)
        assert np.array_equal(mesh[n, :, 0:2], src), f'{name}: cell centres differ'
        assert np.array_equal(mesh[n, :, 2:4], dst), f'{name}: {(mesh[n, :, 2:4] != dst).any(1).sum()} cells differ'


@pytest.mark.parametrize('step', [8, 11])
def test_mesh_through_estimate(step, scene_planes, device_flow):
    from stereotracking_amd import cmc
    prev, curr = scene_planes
    _, mesh, _ = cmc.estimate(prev, curr, H, W, dict(step=step), with_mesh=True)
    for n in range(len(K.FLOW_SCENES)):
        src, dst = R.mesh(device_flow[n].cpu().numpy(), H, W, step)
        m = mesh[n].cpu().numpy()
        assert np.array_equal(m[:, 0:2], src) and np.array_equal(m[:, 2:4], dst), f'pair {n}'


# ---- fit -------------------------------------------------------------------------------------------------------------------
def _check_fit_row(name, row, inl):
    c = K.fit_case(name)
    p = c['points']
    src, dst = p[:, :2], p[:, 2:]
    warp, ratio, rinl, winner = K.fit_reference(name, np.float32)
    inl = inl.astype(bool)
    assert np.array_equal(inl, rinl), f'{name}: {(inl != rinl).sum()} inlier flags differ from the restatement'
    if winner is None:
        assert not row.any() and not inl.any(), f'{name}: no usable hypothesis must give a zero row'
        return
    assert row[0] == (1.0 if warp is not None else 0.0), f'{name}: valid'
    assert row[1] == np.float32(ratio), f'{name}: ratio {row[1]} vs {ratio}'
    want = R.lsq_similarity(src[rinl], dst[rinl])
    np.testing.assert_allclose(row[2:].reshape(2, 3), want, rtol=1e-4, atol=1e-4 * np.abs(want).max(), err_msg=name)
    if 'motion' in c:
        A = c['motion']
        got = np.array([row[2], row[5], row[4], row[7]])
        np.testing.assert_allclose(got, [A[0, 0], A[1, 0], A[0, 2], A[1, 2]], rtol=1e-3, atol=0, err_msg=name)
        assert row[3] == -row[5] and row[6] == row[2]


@pytest.mark.parametrize('name', list(K.FIT_CASES))
def test_fit_point_sets(name, cuda):
    """Inlier flags, valid and ratio exactly the restatement's; the refit against lsq_similarity over that set."""
    from stereotracking_amd import cmc
    c = K.fit_case(name)
    warps, inl = cmc.fit(_dev(c['points'][None], cuda), c['thr'], c['min_ratio'])
    _check_fit_row(name, warps[0].cpu().numpy(), inl[0].cpu().numpy())


@pytest.mark.parametrize('batch', list(K.FIT_BATCHES))
def test_fit_batch_rows_equal_their_own_single_runs(batch, cuda):
    """N = 5 in one call over a workspace full of stale bits: each row is the restatement's and equals its N = 1 result
    bit for bit (per-pair keys, their memset, the per-pair point offset)."""
    from stereotracking_amd import _lib, cmc
    names = K.FIT_BATCHES[batch]
    pts = _dev(np.stack([K.fit_case(n)['points'] for n in names]), cuda)
    ws = torch.full((int(_lib.load().st_cmc_workspace_bytes(len(names))),), 0xFF, dtype=torch.uint8, device=cuda)
    warps, inl = cmc.fit(pts, 5.0, 0.3, ws=ws)
    again, _ = cmc.fit(pts, 5.0, 0.3, ws=ws)             # the keys of the first call are stale now
    assert torch.equal(_bits(warps), _bits(again))
    for n, name in enumerate(names):
        c = K.fit_case(name)
        assert (c['thr'], c['min_ratio']) == (5.0, 0.3)
        _check_fit_row(name, warps[n].cpu().numpy(), inl[n].cpu().numpy())
        w1, i1 = cmc.fit(pts[n:n + 1], 5.0, 0.3)
        assert torch.equal(_bits(w1[0]), _bits(warps[n])) and torch.equal(i1[0], inl[n]), f'row {n} ({name})'


# ---- options end to end ----------------------------------------------------------------------------------------------------
def _check_estimate_vs_restatement(row, mesh, inl, fl, h, w, p):
    """The rule of test_cmc_gpu.test_mesh_and_fit_vs_restatement at the options `p`, on the device's own flow `fl`."""
    src, dst = R.mesh(fl, h, w, p['step'])
    assert np.array_equal(mesh[:, 0:2], src) and np.array_equal(mesh[:, 2:4], dst)
    thr = p['ransac_thr']
    warp, ratio, rinl = R.consensus_fit(src, dst, thr, p['min_inlier_ratio'], np.float32)
    assert inl.any()
    own = R.lsq_similarity(src[inl], dst[inl])
    np.testing.assert_allclose(row[2:].reshape(2, 3), own, rtol=1e-4, atol=1e-4 * np.abs(own).max())
    assert row[1] == np.float32(inl.sum()) / np.float32(len(inl))
    assert row[0] == (1.0 if row[1] >= np.float32(p['min_inlier_ratio']) else 0.0)
    differ = inl != rinl
    if differ.any():     # only points whose residual sits on the threshold may differ
        res = R.residuals(src, dst, R.lsq_similarity(src[rinl], dst[rinl]))
        assert np.all(np.abs(res[differ] - thr) <= 1e-3 + 1e-3 * thr), f'{differ.sum()} inlier flags differ'
    else:
        assert row[0] == (1.0 if warp is not None else 0.0) and abs(row[1] - ratio) < 1e-6
        want = R.lsq_similarity(src[rinl], dst[rinl])
        np.testing.assert_allclose(row[2:].reshape(2, 3), want, rtol=1e-4, atol=1e-4 * np.abs(want).max())


def test_estimate_with_glme_overrides(scene_planes):
    """step 8 (961 points, 461 280 hypotheses), winsize 15, thr 3, ratio 0.5 reach the device: the estimate is the
    restatement's at the same options, and the known motion is recovered."""
    from stereotracking_amd import cmc
    n = list(K.FLOW_SCENES).index(K.OPTIONS_SCENE)
    prev, curr = scene_planes[0][n:n + 1], scene_planes[1][n:n + 1]
    fl = cmc.flow(prev, curr, K.OPTIONS['winsize'])[0].cpu().numpy()
    warps, mesh, inl = cmc.estimate(prev, curr, H, W, K.OPTIONS, with_mesh=True)
    row, mesh, inl = warps[0].cpu().numpy(), mesh[0].cpu().numpy(), inl[0].cpu().numpy().astype(bool)
    assert mesh.shape == (961, 4)
    _check_estimate_vs_restatement(row, mesh, inl, fl, H, W, K.OPTIONS)
    # the default options give another row: the overrides are not ignored
    assert not np.array_equal(cmc.estimate(prev, curr, H, W)[0].cpu().numpy(), row)
    warp = cmc.warp_or_none(row)
    assert warp is not None and row[1] >= 0.9
    assert _corner_error(warp, K.FLOW_SCENES[K.OPTIONS_SCENE][0]) <= CORNER_TOL


@pytest.mark.parametrize('backend', ['native', 'python'])
def test_tracker_hands_its_glme_overrides_to_the_device(backend, cuda, monkeypatch):
    """A tracker configured with glme overrides estimates with exactly those: the row its estimate call returns is the
    row cmc.estimate gives for the two frames at those options, and the warp it applies is that row's."""
    from stereotracking_amd import cmc
    from stereotracking_amd.motion import KalmanFilter
    from stereotracking_amd.structures import InstanceData, TrackDataSample
    from stereotracking_amd.trackers import OCSORTTracker_Disparity

    class _M:
        motion = KalmanFilter()
    trk = OCSORTTracker_Disparity(obj_score_thr=0.3, init_track_thr=0.7, weight_iou_with_det_scores=False,
                                  match_iou_thr=0.3, num_tentatives=3, vel_delta_t=3, num_frames_retain=30,
                                  backend=backend, cmc=dict(method='glme_affine', glme=dict(K.OPTIONS)))
    f0, f1 = K.scene_frames(K.OPTIONS_SCENE)
    imgs = []
    for f in (f0, f0, f1):      # frame 0: no tracks yet; frame 1: first CMC image; frame 2: the estimate
        c = np.full((1, 3, 736, 1280), K.PAD_VALUE, np.float32)
        c[0, :, :H, :W] = K.grey_to_bgr(f)
        imgs.append(_dev(c, cuda))
    calls = []
    real = cmc.estimate

    def spy(prev, curr, h, w, params=None, **kw):
        out = real(prev, curr, h, w, params, **kw)
        calls.append((dict(params), int(h), int(w), out.cpu().numpy().copy()))
        return out
    monkeypatch.setattr(cmc, 'estimate', spy)
    boxes = torch.tensor([[100., 100., 160., 180.], [600., 300., 680., 380.]])
    for t, img in enumerate(imgs):
        s = TrackDataSample(dict(frame_id=t, img_shape=(H, W)))
        s.pred_det_instances = InstanceData(bboxes=boxes.clone(), scores=torch.full((2,), 0.9),
                                            labels=torch.zeros(2, dtype=torch.long), depth=torch.full((2,), 10.0),
                                            scales=torch.ones(2))
        trk.track(_M(), img, None, s)
    assert len(calls) == 1, 'one estimate: the pair (frame 1, frame 2)'
    params, h, w, rows = calls[0]
    assert params == cmc.glme_params(K.OPTIONS) and (h, w) == (H, W)
    planes = cmc.front(torch.cat(imgs[1:]), H, W)
    want = real(planes[0:1], planes[1:2], H, W, K.OPTIONS)[0].cpu().numpy()
    assert np.array_equal(rows[0], want) and want[0] == 1
    assert not np.array_equal(want, real(planes[0:1], planes[1:2], H, W)[0].cpu().numpy())
    # and through estimate_camera_motion itself: the warp is that row's
    trk.reset_cmc()
    meta = dict(frame_id=1, img_shape=(H, W))
    assert trk.estimate_camera_motion(imgs[1], meta) is None
    got = trk.estimate_camera_motion(imgs[2], dict(meta, frame_id=2))
    assert np.array_equal(got, cmc.warp_or_none(want))


# ---- refusals --------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A


class _Refusal:
    """Buffers full of a sentinel; `refused` asserts a non-zero return and, after a sync, that no byte of them changed."""

    def __init__(self, cuda, N=1, P=225):
        from stereotracking_amd import _lib
        self.lib, self.L, self.N, self.P = _lib.load(), _lib, N, P
        self.bytes = int(self.lib.st_cmc_workspace_bytes(N))
        mk = lambda n: torch.full((n,), SENTINEL, dtype=torch.uint8, device=cuda)  # noqa: E731
        self.ws, self.planes = mk(self.bytes), mk(2 * N * 255 * 255)
        self.flow, self.warps, self.mesh, self.inl = mk(N * 255 * 255 * 8), mk(N * 32), mk(N * 1024 * 16), mk(N * 1024)
        self.stream = _lib.current_stream()

    def prm(self, **kw):
        p = dict(step=16, winsize=31, ransac_thr=5.0, min_inlier_ratio=0.3)
        p.update(kw)
        size = p.pop('struct_size', C.sizeof(self.L.StCmcParams))
        return self.L.StCmcParams(size, p['step'], p['winsize'], p['ransac_thr'], p['min_inlier_ratio'])

    def refused(self, rc, what):
        assert rc != 0, f'{what}: accepted'
        assert self.lib.st_last_error(), f'{what}: no error message'
        torch.cuda.synchronize()
        for name in ('ws', 'planes', 'flow', 'warps', 'mesh', 'inl'):
            assert bool((getattr(self, name) == SENTINEL).all()), f'{what}: wrote to {name}'

    def estimate(self, prm, ws_bytes=None, prev=True, warps=True, N=None, hw=(720, 1280)):
        p = self.L.ptr
        return self.lib.st_cmc_estimate(p(self.planes) if prev else None, p(self.planes[255 * 255:]),
                                        self.N if N is None else N, hw[0], hw[1], C.byref(prm) if prm else None,
                                        p(self.ws), self.bytes if ws_bytes is None else ws_bytes,
                                        p(self.warps) if warps else None, p(self.mesh), p(self.inl), self.stream)

    def flow_(self, winsize, ws_bytes=None, prev=True, ws=True, N=None):
        p = self.L.ptr
        return self.lib.st_cmc_flow(p(self.planes) if prev else None, p(self.planes[255 * 255:]),
                                    self.N if N is None else N, winsize, p(self.ws) if ws else None,
                                    self.bytes if ws_bytes is None else ws_bytes, p(self.flow), None, self.stream)

    def mesh_fit(self, prm, ws_bytes=None, flow=True, warps=True, ws=True, N=None, hw=(720, 1280)):
        p = self.L.ptr
        return self.lib.st_cmc_mesh_fit(p(self.flow) if flow else None, self.N if N is None else N, hw[0], hw[1],
                                        C.byref(prm) if prm else None, p(self.ws) if ws else None,
                                        self.bytes if ws_bytes is None else ws_bytes, p(self.warps) if warps else None,
                                        p(self.mesh), p(self.inl), self.stream)

    def fit(self, P=225, ws_bytes=None, points=True, warps=True, ws=True, N=None):
        p = self.L.ptr
        return self.lib.st_cmc_fit(p(self.mesh) if points else None, self.N if N is None else N, P, 5.0, 0.3,
                                   p(self.ws) if ws else None, self.bytes if ws_bytes is None else ws_bytes,
                                   p(self.warps) if warps else None, p(self.inl), self.stream)


@pytest.mark.parametrize('winsize', [0, 30, 65, -1])
def test_refuses_bad_winsize(winsize, cuda):
    r = _Refusal(cuda)
    r.refused(r.flow_(winsize), f'st_cmc_flow winsize {winsize}')
    r.refused(r.estimate(r.prm(winsize=winsize)), f'st_cmc_estimate winsize {winsize}')


@pytest.mark.parametrize('step', [7, 17, 0, 256])
def test_refuses_bad_step(step, cuda):
    r = _Refusal(cuda)
    r.refused(r.estimate(r.prm(step=step)), f'st_cmc_estimate step {step}')
    r.refused(r.mesh_fit(r.prm(step=step)), f'st_cmc_mesh_fit step {step}')


def test_refuses_short_workspace_and_wrong_struct_size(cuda):
    r = _Refusal(cuda, N=2)
    short = r.bytes - 1
    assert int(r.lib.st_cmc_workspace_bytes(0)) == 0 and r.bytes > int(r.lib.st_cmc_workspace_bytes(1))
    r.refused(r.flow_(31, ws_bytes=short), 'st_cmc_flow short workspace')
    r.refused(r.estimate(r.prm(), ws_bytes=short), 'st_cmc_estimate short workspace')
    r.refused(r.mesh_fit(r.prm(), ws_bytes=short), 'st_cmc_mesh_fit short workspace')
    r.refused(r.fit(ws_bytes=short), 'st_cmc_fit short workspace')
    # the workspace of N - 1 pairs does not serve N
    r.refused(r.fit(ws_bytes=int(r.lib.st_cmc_workspace_bytes(1))), 'st_cmc_fit workspace of one pair for two')
    size = C.sizeof(r.L.StCmcParams)
    for wrong in (size - 4, size + 4, 0):
        r.refused(r.estimate(r.prm(struct_size=wrong)), f'st_cmc_estimate struct_size {wrong}')
        r.refused(r.mesh_fit(r.prm(struct_size=wrong)), f'st_cmc_mesh_fit struct_size {wrong}')
    r.refused(r.estimate(None), 'st_cmc_estimate null params')
    r.refused(r.mesh_fit(None), 'st_cmc_mesh_fit null params')


def test_refuses_null_and_out_of_range_arguments(cuda):
    r = _Refusal(cuda)
    r.refused(r.flow_(31, prev=False), 'st_cmc_flow null planes')
    r.refused(r.flow_(31, ws=False), 'st_cmc_flow null workspace')
    r.refused(r.flow_(31, N=0), 'st_cmc_flow N = 0')
    r.refused(r.estimate(r.prm(), prev=False), 'st_cmc_estimate null planes')
    r.refused(r.estimate(r.prm(), warps=False), 'st_cmc_estimate null warps')
    r.refused(r.estimate(r.prm(), hw=(0, 1280)), 'st_cmc_estimate img_h = 0')
    r.refused(r.mesh_fit(r.prm(), flow=False), 'st_cmc_mesh_fit null flow')
    r.refused(r.mesh_fit(r.prm(), warps=False), 'st_cmc_mesh_fit null warps')
    r.refused(r.mesh_fit(r.prm(), ws=False), 'st_cmc_mesh_fit null workspace')
    r.refused(r.mesh_fit(r.prm(), N=0), 'st_cmc_mesh_fit N = 0')
    r.refused(r.mesh_fit(r.prm(), hw=(720, 0)), 'st_cmc_mesh_fit img_w = 0')
    r.refused(r.fit(points=False), 'st_cmc_fit null points')
    r.refused(r.fit(warps=False), 'st_cmc_fit null warps')
    r.refused(r.fit(ws=False), 'st_cmc_fit null workspace')
    r.refused(r.fit(N=0), 'st_cmc_fit N = 0')
    for P in (1, 0, -5, 1025):
        r.refused(r.fit(P=P), f'st_cmc_fit P = {P}')


def test_front_refusals(cuda):
    r = _Refusal(cuda)
    p = r.L.ptr
    fh, fw, N = 8, 12, 36
    frames = [torch.full((3, fh, fw), 100 + i, dtype=torch.uint8, device=cuda) for i in range(N)]
    out = torch.full((N, 255, 255), SENTINEL, dtype=torch.uint8, device=cuda)

    def call(ptrs, n=N, h=fh, w=fw, planes=out, lst=True):
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        return r.lib.st_cmc_front_u8(arr if lst else None, n, fh, fw, h, w, p(planes) if planes is not None else None,
                                     r.stream)

    def refused(rc, what):
        r.refused(rc, what)
        assert bool((out == SENTINEL).all()), f'{what}: wrote planes'
    good = [f.data_ptr() for f in frames]
    refused(call(good, h=fh + 1), 'st_cmc_front_u8 h > fh')
    refused(call(good, w=fw + 1), 'st_cmc_front_u8 w > fw')
    refused(call(good, h=0), 'st_cmc_front_u8 h = 0')
    refused(call(good, n=0), 'st_cmc_front_u8 N = 0')
    refused(call(good, planes=None), 'st_cmc_front_u8 null planes')
    refused(call(good, lst=False), 'st_cmc_front_u8 null list')
    refused(call([None] + good[1:]), 'st_cmc_front_u8 null first frame')
    # a null frame behind the first 32-frame chunk: that chunk must not have been launched either
    refused(call(good[:34] + [None] + good[35:]), 'st_cmc_front_u8 null frame 34')
    batch = torch.full((1, 3, fh, fw), 9.0, device=cuda)
    f32 = lambda b, h, w, planes=out, n=1: r.lib.st_cmc_front_f32(  # noqa: E731
        p(b), n, fh, fw, h, w, p(planes) if planes is not None else None, r.stream)
    refused(f32(batch, fh + 1, fw), 'st_cmc_front_f32 h > H')
    refused(f32(batch, fh, fw + 1), 'st_cmc_front_f32 w > W')
    refused(f32(None, fh, fw), 'st_cmc_front_f32 null batch')
    refused(f32(batch, fh, fw, planes=None), 'st_cmc_front_f32 null planes')
    refused(f32(batch, fh, fw, n=0), 'st_cmc_front_f32 N = 0')
    # and the accepted call writes
    assert call(good) == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())
