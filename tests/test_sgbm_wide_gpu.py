"""GPU: StereoSGBM (csrc/sgbm.hip) at 128, 192 and 256 disparity levels - 2, 3 and 4 levels per lane of the wave - bit for
bit against the numpy restatement (tests/sgbm_ref.py) on the scenarios of tests/sgbm_wide_cases.py, whose preconditions
tests/test_cpu_sgbm_wide.py asserts without a GPU; then both entry points, a one-level-per-lane module next to a wide one,
a dirty workspace, the dense pipeline and the MOT shell."""
import os

import numpy as np
import pytest
import torch

import sgbm_ref as R
import sgbm_wide_cases as W
from sgbm_check import assert_stages_bit_exact, batch, up

pytestmark = pytest.mark.gpu


def _stages(cuda, pairs, kw, **more):
    L, Rt = [p[0] for p in pairs], [p[1] for p in pairs]
    return assert_stages_bit_exact(cuda, L, Rt, kw, refs=[W.reference(a, b, kw) for a, b in pairs], **more)


# ---- every scenario, stage by stage ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b', W.BANDS, ids=W.bands_id)
def test_bands_bit_exact(cuda, b):
    """N = 3: true disparities in every 64-level slot."""
    _stages(cuda, W.bands_pairs(b), W.bands_kw(b))


def test_staircase_bit_exact(cuda):
    """Levels on both sides of every lane and slot edge: the d +- 1 neighbours of the paths and of the subpixel fit."""
    _stages(cuda, W.staircase_pairs(), W.STAIRCASE_KW)


@pytest.mark.parametrize('uniq', W.TIES_UNIQ)
@pytest.mark.parametrize('D', sorted(W.TIES_SHAPES))
@pytest.mark.parametrize('name', W.TIES_NAMES)
def test_ties_bit_exact(cuda, name, D, uniq):
    """Minima of S whole periods (up to 64 levels) apart: the lowest level wins, the uniqueness test is per level."""
    _stages(cuda, [W.ties_pair(name, D), W.ties_pair(W.ties_partner(name), D)], W.ties_kw(D, uniq))


@pytest.mark.parametrize('g', W.GEOMETRY, ids=W.geometry_id)
def test_geometry_bit_exact(cuda, g):
    _stages(cuda, W.geometry_pairs(g), W.geometry_kw(g))


@pytest.mark.parametrize('kw', W.OPTIONS, ids=W.options_id)
def test_options_bit_exact(cuda, kw):
    _stages(cuda, W.options_pairs(), W.options_kw(kw))


def test_bound_bit_exact(cuda):
    """P2 at the int16 bound, D = 256: S above 2^14 through the packed int16 volumes."""
    _stages(cuda, W.bound_pairs(), W.BOUND_KW)


# ---- the entry points ----------------------------------------------------------------------------------------------------------
def test_u8_frames_equal_f32_batch_with_random_padding(cuda):
    from stereotracking_amd.engine import RawChunk
    from stereotracking_amd.sgbm import StereoSGBM
    b = W.BANDS[0]
    pairs, kw = W.bands_pairs(b), W.bands_kw(b)
    assert kw['num_disparities'] == 128
    h, w = pairs[0][0].shape[1:]
    H, W_ = up(h), up(w)
    assert W_ > w
    noise = np.random.RandomState(3).randint(0, 256, (len(pairs), 3, H, W_)).astype(np.float32)
    m = StereoSGBM(**kw)
    a = torch.full((len(pairs), 3, H, W_), -1.0, device=cuda)
    c = torch.full((len(pairs), 3, H, W_), -1.0, device=cuda)
    m.compute(batch([p[0] for p in pairs], H, W_, cuda, noise), batch([p[1] for p in pairs], H, W_, cuda, noise), (h, w), a)
    st_f32 = int(m.last_status.item())
    lc = RawChunk([torch.from_numpy(p[0]).to(cuda) for p in pairs], 114.0)
    rc = RawChunk([torch.from_numpy(p[1]).to(cuda) for p in pairs], 114.0)
    m.compute(lc, rc, (h, w), c)
    torch.cuda.synchronize()
    assert torch.equal(a, c)
    assert st_f32 == 0 and int(m.last_status.item()) == 0
    for i, p in enumerate(pairs):
        assert np.array_equal(a[i].cpu().numpy(), R.disp_postp(W.reference(p[0], p[1], kw)['final'], H, W_)), f'pair {i}'


def test_wide_and_narrow_modules_alternate_on_one_device(cuda):
    """A D = 128 module (2 levels per lane) and a D = 48 module (1 level per lane, idle lanes) on the same pairs, turn by
    turn: each keeps its own workspace and its own answer."""
    from stereotracking_amd.sgbm import StereoSGBM
    pairs = W.options_pairs()
    h, w = W.OPTIONS_HW
    H, W_ = up(h), up(w)
    lb, rb = batch([p[0] for p in pairs], H, W_, cuda), batch([p[1] for p in pairs], H, W_, cuda)
    kws = [dict(num_disparities=128, speckle_window_size=50), dict(num_disparities=48, speckle_window_size=50)]
    mods = [StereoSGBM(**kw) for kw in kws]
    want = [np.stack([R.disp_postp(W.reference(p[0], p[1], kw)['final'], H, W_) for p in pairs]) for kw in kws]
    assert not np.array_equal(want[0], want[1]) and want[0].any() and want[1].any()
    for turn in range(4):
        k = turn % 2
        out = torch.full((len(pairs), 3, H, W_), -1.0, device=cuda)
        mods[k].compute(lb, rb, (h, w), out)
        assert np.array_equal(out.cpu().numpy(), want[k]), f'turn {turn}: D = {kws[k]["num_disparities"]}'
        assert int(mods[k].last_status.item()) == 0


@pytest.mark.parametrize('order', [(0, 1), (1, 0)], ids=['constant-then-stripes', 'stripes-then-constant'])
def test_second_compute_on_a_dirty_workspace(cuda, order):
    """D = 256, ratio 0: the constant pair (every pixel level 0) and a striped pair (levels 8 / 9) through one module and
    one workspace, in both orders."""
    from stereotracking_amd.sgbm import StereoSGBM
    D = 256
    h, w = W.TIES_SHAPES[D]
    H, W_ = up(h), up(w)
    kw = W.ties_kw(D, 0)
    names = ('const63', 'period10-roll9')
    refs = [W.reference(*W.ties_pair(n, D), kw)['final'] for n in names]
    assert (refs[0][:, D:] == 0).all() and (refs[1][:, D:] >= 16 * 8).all()
    m = StereoSGBM(**kw)
    for k in order:
        left, right = W.ties_pair(names[k], D)
        out = torch.full((1, 3, H, W_), -1.0, device=cuda)
        m.compute(batch([left], H, W_, cuda), batch([right], H, W_, cuda), (h, w), out)
        assert len(m._ws) == 1, 'both scenarios share one workspace'
        assert np.array_equal(out[0].cpu().numpy(), R.disp_postp(refs[k], H, W_)), names[k]
        assert int(m.last_status.item()) == 0


# ---- through the layers above -------------------------------------------------------------------------------------------------
PIPE_HW, PIPE_D = (96, 160), 128       # the frame of the D = 48 pipeline tests: the smallest multiple of 32 above 128


def _pairs(N, h, w, D, seed):
    from stereotracking_amd.synthetic import synthetic_stereo_pair
    ps = [synthetic_stereo_pair(seed + i, h, w, max_disp=D) for i in range(N)]
    return [p['left'] for p in ps], [p['right'] for p in ps]


def _clone(out, ctx):
    return {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor)}


@pytest.mark.parametrize('contexts', [1, 3])
def test_pipeline_sgbm_equals_mono_fed_its_own_disparity(cuda, contexts):
    """StereoDensePipeline(sgbm=dict(num_disparities=128)): detections, depths and scaled boxes are those of the mono
    pipeline given the module's own disp_postp, bit for bit, through 1 and 3 in-flight contexts."""
    from stereotracking_amd.pipeline import InflightPipelines
    from stereotracking_amd.synthetic import synthetic_state_dict
    N, (h, w) = 2, PIPE_HW
    cfg = dict(type='StereoSGBM', num_disparities=PIPE_D)
    sg = InflightPipelines(contexts, N, (h, w), 0.375, 0.33, 1, stereo=False, sgbm=cfg, max_det=256)
    mono = InflightPipelines(contexts, N, (h, w), 0.375, 0.33, 1, stereo=False, max_det=256)
    assert sg.takes_right and not mono.takes_right
    sd = synthetic_state_dict(sg.param_table(), seed=0, prior_prob=0.2, logit_std=2.5)
    sg.load_state_dict(sd, autotune=False)
    mono.load_state_dict(sd, autotune=False)
    got = []
    for k in range(4):
        L, Rt = _pairs(N, h, w, PIPE_D, seed=40 + 3 * k)
        img, right = batch(L, h, w, cuda), batch(Rt, h, w, cuda)
        got.append((img, right, sg.submit(img, right=right, post=_clone)[0]))
    sg.synchronize()
    kept = 0
    for img, right, a in got:
        b = mono.submit(img, disp_postp=a['disp_postp'], post=_clone)[0]
        mono.synchronize()
        for key in ('counts', 'boxes', 'scores', 'labels', 'prior_idx', 'depth', 'scales', 'scaled_boxes'):
            assert torch.equal(a[key].nan_to_num(-7.0), b[key].nan_to_num(-7.0)), key   # NaN depth: equal positions
        kept += int(a['counts'].sum())
    assert kept > 0, 'scenario kept no boxes'
    L, Rt = _pairs(N, h, w, PIPE_D, seed=40)
    want = np.stack([R.disp_postp(R.sgbm(x, y, num_disparities=PIPE_D), h, w) for x, y in zip(L, Rt)])
    assert want.any()
    assert np.array_equal(got[0][2]['disp_postp'].cpu().numpy(), want)


def _sgbm_model(cuda, dense_batch=4, inflight=2):
    from stereotracking_amd import mot  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import MODELS
    from stereotracking_amd.synthetic import synthetic_state_dict
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(root, 'configs', 'stereo_tracking', 'ocsort', 'stereo_yolox_s_mot_airdrone_sgbm.py'))
    for part in ('backbone', 'neck'):
        cfg.model.detector[part]['widen_factor'] = 0.375
    cfg.model.detector.bbox_head.head_module['widen_factor'] = 0.375
    cfg.model.tracker['init_track_thr'] = 0.03
    cfg.model.tracker['obj_score_thr'] = 0.02
    cfg.model.stereo['num_disparities'] = PIPE_D
    model = MODELS.build(dict(cfg.model, autotune=False, dense_batch=dense_batch, inflight=inflight))
    assert model.stereo.num_disparities == PIPE_D
    sd = synthetic_state_dict(list(model.detector._table), seed=5, prior_prob=0.2, logit_std=2.5)
    model.detector.load_state_dict(sd, strict=False)
    return model


def test_shell_sgbm_config_test_step_equals_per_chunk_calls(cuda):
    from stereotracking_amd.sequence import synthetic_sequence
    from stereotracking_amd.structures import TrackDataSample
    ori, T = PIPE_HW, 12            # whole chunks of 4: every call runs the same batch-4 launch plan
    fr = list(synthetic_sequence(T, 3, ori[0], ori[1], PIPE_D, seed=2))
    left = [torch.from_numpy(f['left'])[None].to(cuda) for f in fr]
    right = [torch.from_numpy(f['right'])[None].to(cuda) for f in fr]

    def samples(lo, hi):
        return [TrackDataSample(dict(frame_id=t, ori_shape=ori, img_shape=ori, scale_factor=(1.0, 1.0)))
                for t in range(lo, hi)]
    one = _sgbm_model(cuda)
    whole = one.test_step(dict(inputs=dict(img=left, right=right), data_samples=samples(0, T)))
    per = _sgbm_model(cuda)
    chunks = []
    for lo in range(0, T, 4):
        chunks += per.test_step(dict(inputs=dict(img=left[lo:lo + 4], right=right[lo:lo + 4]),
                                     data_samples=samples(lo, lo + 4)))
    torch.cuda.synchronize()
    assert len(whole) == len(chunks) == T
    n = 0
    for a, b in zip(whole, chunks):
        ta, tb = a.pred_track_instances, b.pred_track_instances
        assert ta.instances_id.tolist() == tb.instances_id.tolist()
        for key in ('bboxes', 'scores', 'depth', 'scales'):
            assert torch.equal(ta[key].nan_to_num(-7.0), tb[key].nan_to_num(-7.0)), key
        assert torch.equal(a.pred_det_instances.bboxes, b.pred_det_instances.bboxes)
        n += len(ta)
    assert n > 0, 'no tracks in the scenario'
