"""Host-side checks of the plan-forcing helper (tests/plan_utils.py): no GPU needed - st_detector_create,
st_detector_op_desc and st_detector_get / set_tuning are host code."""
import pytest
import torch

from oracle.torch_model import OracleDetector
from plan_utils import (TAPS, direct_shape, forced_tuning, oracle_taps, plan_ops, resident_shape, streaming_shape,
                        summarise, tile_valid, wino_shape)
from stereotracking_amd.engine import HipDetector
from stereotracking_amd.synthetic import synthetic_batch, synthetic_state_dict

# (N, H, W, widen, deepen, kwargs) -> ops of the plan
MATRIX = [
    ((1, 96, 160, 0.5, 0.33, {}), 71),
    ((3, 224, 352, 0.5, 0.67, {}), 97),
    ((1, 128, 192, 0.5, 1.0, {}), 123),
    ((1, 736, 1280, 0.5, 0.33, {}), 71),
    ((3, 224, 352, 0.375, 0.33, {}), 71),
    ((1, 96, 160, 0.375, 0.33, {}), 71),
    ((2, 96, 160, 0.75, 0.67, {}), 102),
    ((1, 128, 192, 1.0, 1.0, {}), 123),
    ((2, 96, 160, 0.5, 0.33, dict(stereo=True)), 72),
    ((2, 96, 160, 0.5, 0.33, dict(rgb_only=True)), 65),
]


def make(cfg):
    N, H, W, widen, deepen, kw = cfg
    return HipDetector(N, H, W, widen, deepen, 1, **kw)


@pytest.mark.parametrize('cfg,nops', MATRIX)
def test_every_policy_vector_is_accepted(cfg, nops):
    det = make(cfg)
    ops = plan_ops(det)
    assert len(ops) == nops
    assert det.get_tuning() == [-1] * nops
    for policy in 'SHT':
        t = forced_tuning(det, policy)
        assert len(t) == nops
        det.set_tuning(t)                      # st_detector_set_tuning validates every tile against the op's Cout
        assert det.get_tuning() == t
        for o, v in zip(ops, t):               # and the special instances sit on shapes their kernels take
            assert v == -1 or o.kind == 'conv'
            if v == 41: assert streaming_shape(o) and not resident_shape(o)
            if v == 42: assert direct_shape(o)
            if v in (43, 44): assert wino_shape(o) and (v == 43 or o.cout % 64 == 0)
            if v == 46: assert resident_shape(o)
            if 0 <= v < 40: assert tile_valid(v, o.cout)
    assert forced_tuning(det, 'H') == [-1] * nops
    assert det.launch_report() == [(40 if o.kind == 'stem' else 47 if o.kind == 'pred' else -1, -1) for o in ops], \
        'no forward has run: every owner is -1'


def test_policy_s_marks_the_head_towers_and_the_chains_at_widen_half():
    det = make((1, 96, 160, 0.5, 0.33, {}))
    ops, t = plan_ops(det), forced_tuning(det, 'S')
    first = [i for i, o in enumerate(ops) if '_convs.' in o.name and o.name.endswith('.0.conv')]
    second = [i for i, o in enumerate(ops) if '_convs.' in o.name and o.name.endswith('.1.conv')]
    assert len(first) == 3 and len(second) == 6 and first == list(range(first[0], first[0] + 3)) and \
        second == list(range(first[0] + 3, first[0] + 9)), 'tower convs are emitted depth-major, level by level'
    assert all(t[i] == 43 for i in first + second)
    assert [(ops[i].cin, ops[i].cout) for i in first] == [(128, 256)] * 3      # cls | reg conv0 fused along Cout
    assert [(ops[i].H, ops[i].W) for i in first] == [(12, 20), (6, 10), (3, 5)]
    # the two CSP layers whose main|short conv is resident-shaped with mid = 64: both ops of the pair get 46
    for name in ('backbone.stage2.1', 'neck.top_down_layers.1'):
        i = next(k for k, o in enumerate(ops) if o.name == name + '.main_conv.conv')
        assert ops[i].split and ops[i].cout == 128 and ops[i + 1].name == name + '.blocks.0.conv1.conv'
        assert t[i] == 46 and t[i + 1] == 46
    # stage-1 shapes: 3x3/s2 front conv has no special instance, its bottleneck conv2 is a Winograd layer
    i = next(k for k, o in enumerate(ops) if o.name == 'backbone.stage1.0.conv')
    assert t[i] == -1 and (ops[i].k, ops[i].stride, ops[i].cin, ops[i].cout) == (3, 2, 32, 64)
    assert t[i + 3] == 43 and ops[i + 3].res


def test_policy_t_uses_every_alternate_somewhere():
    seen = set()
    for cfg, _ in MATRIX[:5]:
        seen |= set(forced_tuning(make(cfg), 'T'))
    assert {42, 43, 44, 12, 13, 15, 18, 0, 3, 7, 19} <= seen
    assert not seen & {41, 46}


def test_summarise_counts_launches_and_riders():
    rep = [(40, 0), (45, 1), (45, 1), (45, 1), (56, 4), (56, 4), (46, 6), (46, 6), (46, 8), (3, 9), (-1, 10),
           (48, 11), (49, 11), (49, 11), (47, 14)]
    assert summarise(rep) == {'40': 1, '45+2': 1, '56+1': 1, '46+1': 1, '46': 1, 'tile': 1, 'other': 1, '48+2': 1, '47': 1}
    with pytest.raises(AssertionError):
        summarise([(46, 0), (46, -1)])          # an op that never ran
    with pytest.raises(AssertionError):
        summarise([(48, 0), (48, 0)])           # a grouped rider must report 49


def test_oracle_taps_names_shapes_and_fusion_point():
    N, H, W = 2, 64, 96
    det = HipDetector(N, H, W, 0.375, 0.33, 1)
    sd = synthetic_state_dict(det.param_table(), seed=0)
    ora = OracleDetector(0.33, 0.375, 1).eval()
    ora.load_state_dict(sd, strict=False)
    batch = synthetic_batch(range(N), H - 16, W, 64)
    taps = oracle_taps(ora, batch)
    assert set(taps) == set(TAPS) | {'head0', 'head1', 'head2'}
    assert taps['stage1_rgb'].shape == (N, 48, H // 4, W // 4) == taps['stage1_fused'].shape
    with torch.no_grad():
        disp_side = ora.backbone.disp_stage1(ora.backbone.disp_stem(batch['disp_postp']))
        feats = ora.backbone(batch)
    assert torch.equal(taps['stage1_fused'], (taps['stage1_rgb'] + disp_side) / 2.)
    for name, ref in zip(('stage2', 'stage3', 'stage4'), feats):
        assert torch.equal(taps[name], ref)
    assert taps['p3_inner'].shape == (N, 96, H // 8, W // 8) and taps['p3'].shape == (N, 96, H // 8, W // 8)
    assert taps['p5'].shape == (N, 96, H // 32, W // 32)
    assert [tuple(taps[f'head{l}'].shape) for l in range(3)] == [(N, (H >> s) * (W >> s), 6) for s in (3, 4, 5)]
    both = oracle_taps(ora, batch, right=batch['right'])
    assert both['stage1_rgb'].shape[0] == 2 * N and torch.equal(both['stage1_rgb'][:N], taps['stage1_rgb'])
    assert not ora.backbone.stage1._forward_hooks and not ora.neck.out_layers[0]._forward_hooks   # hooks removed
