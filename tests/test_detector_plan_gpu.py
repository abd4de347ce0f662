"""Per-tap parity of FORCED launch plans of the detector against the fp64 oracle.

The fast paths of the plan (csrc/detector.cpp: run_ops) are fusions and special instances that exist only when the ops
are tuned to them; the other deterministic detector tests pin the heuristic plan, where `Op::tuned == -1` and the
chained resident 1x1 pair (46 + rider) and the grouped Winograd launches of the head towers (48 / 49) never run.  Here
every configuration runs three plans chosen from the op shapes (plan_utils.forced_tuning: H heuristic, S the plan
with chains and groups, T the alternates) and for each:

  1. the launch report (HipDetector.launch_report) must equal EXPECTED below - a table written from reading
     StDetector::build / run_ops, so a fusion that silently falls back to separate launches fails here;
  2. every tap and head level is compared with the fp64 oracle: rel_err <= FACTOR x the error of the fp32 CPU oracle
     against the same fp64 tensors (the larger of its mkldnn and native evaluations).  FACTOR = 4: two correct fp32
     evaluations differ by up to 1.76 x in their maximum error (the two CPU runs over all taps), Winograd F(2x2,3x3)
     is 1.55 x direct fp32 (profiles/r06_wino_f4_numerics.json); 1.76 x 1.55 = 2.7, rounded up.  And never above the
     1e-3 every other parity test allows;
  3. S and T against H, tap by tap, within the sum of the two bars (localises a difference to the first tap that moves).

Measured ratios err_gpu / yardstick are written by parity_utils.write_record as detector_plan_parity.json (copy: profiles/).
"""
import copy

import pytest
import torch

from oracle.torch_model import OracleDetector
from parity_utils import rel_err, write_record
from plan_utils import TAPS, forced_tuning, oracle_taps, summarise
from stereotracking_amd.engine import HipDetector
from stereotracking_amd.synthetic import synthetic_batch, synthetic_state_dict

pytestmark = pytest.mark.gpu

FACTOR = 4.0
NAMES = TAPS + ('head0', 'head1', 'head2')

# id -> (N, H, W, widen, deepen, HipDetector kwargs)
CONFIGS = {
    'w050_d033_1x96x160': (1, 96, 160, 0.5, 0.33, {}),       # 3x5 map: under one Winograd tile block, 15 < 32 pixels for 47
    'w050_d067_3x224x352': (3, 224, 352, 0.5, 0.67, {}),     # odd maps, N = 3, two stage-1 bottlenecks, six behind a 46 chain
    'w050_d100_1x128x192': (1, 128, 192, 0.5, 1.0, {}),      # three stage-1 bottlenecks
    'w050_d033_1x736x1280': (1, 736, 1280, 0.5, 0.33, {}),   # the shipped geometry at a batch the committed plan was not made for
    'w0375_d033_3x224x352': (3, 224, 352, 0.375, 0.33, {}),  # feat 96, Cin tails, first tower group only
    'w075_d067_2x96x160': (2, 96, 160, 0.75, 0.67, {}),      # feat 192: un-fused Cout = 1 / 5 prediction convs, mid = 48
    'w100_d100_1x128x192': (1, 128, 192, 1.0, 1.0, {}),      # feat 256, 64-wide stem, the 46 chain in stage 1
    'w050_d033_2x96x160_stereo': (2, 96, 160, 0.5, 0.33, dict(stereo=True)),
    'w050_d033_2x96x160_rgb': (2, 96, 160, 0.5, 0.33, dict(rgb_only=True)),
}

# Launches per plan (plan_utils.summarise: '<instance>' = a launch of its own, '<instance>+<r>' = with r riders; 'tile' =
# the implicit-GEMM tiles 0..21, 'other' = SPP pooling).  Derived by hand from StDetector::build and run_ops:
#  * 40: one fused stem per input (image, disparity; left + right + disparity in a stereo context; image alone rgb-only)
#  * 45+2 / 56+1: the stage-1 front and tail fusions exist at c1 = 32, c2 = 64 only (widen 0.5), once per branch, in
#    every plan (they do not look at Op::tuned); with n1 > 1 bottlenecks the tail takes the LAST conv2 only
#  * 46+1: a CSP layer with mid = 64 whose main|short conv is 128 -> 128 or 256 -> 128: backbone.stage2.1 and
#    neck.top_down_layers.1 at widen 0.5, stage1.1 / disp_stage1.1 at widen 1.0 (mid = 64 there, so no 45 / 56)
#  * 48+2 / 48+5: the three cls|reg conv0 and the six second tower convs, when Cout % 64 == 0 and Cin % 32 == 0: both
#    at feat 128 / 192 / 256, the first only at feat 96 (96 -> 96 stays six launches of 43); T tunes them to 44, which
#    groups just the same (run_ops accepts 43 or 44)
#  * 47: feat in {96, 128, 256}; at feat 192 the six prediction convs are ordinary tiles
#  * 41 under S: the conv1 (32 -> 32) of the second and third stage-1 bottlenecks; the first is a rider of 45
#  * 43 / 44 / 42: one per bottleneck conv2 outside the fusions (S: all 43; T: 42 at Cin = Cout in {32, 48, 64}, else 44
#    at Cout % 64 == 0, else 43)
_W050_D033 = dict(
    H={'40': 2, '45+2': 2, '56+1': 2, '47': 1, 'other': 1, 'tile': 57},
    S={'40': 2, '45+2': 2, '56+1': 2, '46+1': 2, '46': 11, '43': 11, '48+2': 1, '48+5': 1, '47': 1, 'other': 1, 'tile': 22},
    T={'40': 2, '45+2': 2, '56+1': 2, '42': 4, '44': 7, '48+2': 1, '48+5': 1, '47': 1, 'other': 1, 'tile': 37})
EXPECTED = {
    'w050_d033_1x96x160': _W050_D033,
    'w050_d033_1x736x1280': _W050_D033,
    'w050_d067_3x224x352': dict(
        H={'40': 2, '45+2': 2, '56+1': 2, '47': 1, 'other': 1, 'tile': 83},
        S={'40': 2, '45+2': 2, '56+1': 2, '46+1': 2, '46': 20, '41': 2, '43': 24, '48+2': 1, '48+5': 1, '47': 1,
           'other': 1, 'tile': 24},
        T={'40': 2, '45+2': 2, '56+1': 2, '42': 10, '44': 14, '48+2': 1, '48+5': 1, '47': 1, 'other': 1, 'tile': 50}),
    'w050_d100_1x128x192': dict(
        H={'40': 2, '45+2': 2, '56+1': 2, '47': 1, 'other': 1, 'tile': 109},
        S={'40': 2, '45+2': 2, '56+1': 2, '46+1': 2, '46': 29, '41': 4, '43': 37, '48+2': 1, '48+5': 1, '47': 1,
           'other': 1, 'tile': 26},
        T={'40': 2, '45+2': 2, '56+1': 2, '42': 16, '44': 21, '48+2': 1, '48+5': 1, '47': 1, 'other': 1, 'tile': 63}),
    'w0375_d033_3x224x352': dict(
        H={'40': 2, '47': 1, 'other': 1, 'tile': 67},
        S={'40': 2, '43': 17, '48+2': 1, '47': 1, 'other': 1, 'tile': 47},
        T={'40': 2, '42': 4, '43': 11, '44': 2, '48+2': 1, '47': 1, 'other': 1, 'tile': 47}),
    'w075_d067_2x96x160': dict(
        H={'40': 2, 'other': 1, 'tile': 99},
        S={'40': 2, '43': 26, '48+2': 1, '48+5': 1, 'other': 1, 'tile': 64},
        T={'40': 2, '42': 4, '43': 8, '44': 14, '48+2': 1, '48+5': 1, 'other': 1, 'tile': 64}),
    'w100_d100_1x128x192': dict(
        H={'40': 2, '47': 1, 'other': 1, 'tile': 119},
        S={'40': 2, '46+1': 2, '46': 18, '43': 39, '48+2': 1, '48+5': 1, '47': 1, 'other': 1, 'tile': 49},
        T={'40': 2, '42': 6, '44': 33, '48+2': 1, '48+5': 1, '47': 1, 'other': 1, 'tile': 71}),
    'w050_d033_2x96x160_stereo': {p: dict(v, **{'40': 3}) for p, v in _W050_D033.items()},
    'w050_d033_2x96x160_rgb': {p: dict(v, **{'40': 1, '45+2': 1, '56+1': 1}) for p, v in _W050_D033.items()},
}

RECORD = {}


def _setup(cid):
    """-> det, device-side run(), fp64 taps, per-name bar, per-name yardstick."""
    N, H, W, widen, deepen, kw = CONFIGS[cid]
    det = HipDetector(N, H, W, widen, deepen, 1, **kw)
    sd = synthetic_state_dict(det.param_table(), seed=0)
    det.load_state_dict(sd)
    ora = OracleDetector(deepen, widen, 1, rgb_only=bool(kw.get('rgb_only'))).eval()
    missing, unexpected = ora.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith('num_batches_tracked') for k in missing)
    batch = synthetic_batch(range(N), H - 16, W, 64)          # 16 padded rows: a padded band exists
    assert batch['img'].shape[-2:] == (H, W)
    # a stereo context reads plane 0 of the disparity with plane-summed weights: a 3-channel repeat on both sides
    assert torch.equal(batch['disp_postp'][:, 0], batch['disp_postp'][:, 1])
    right = synthetic_batch(range(100, 100 + N), H - 16, W, 64)['img'] if kw.get('stereo') else None
    inp = {k: batch[k] for k in ('img', 'disp_postp')}
    ref64 = oracle_taps(copy.deepcopy(ora).double(), {k: v.double() for k, v in inp.items()},
                        None if right is None else right.double())
    cpu_a = oracle_taps(ora, inp, right)
    with torch.backends.mkldnn.flags(enabled=False):
        cpu_b = oracle_taps(ora, inp, right)
    yard = {n: max(rel_err(cpu_a[n], ref64[n]), rel_err(cpu_b[n], ref64[n])) for n in NAMES}
    return det, batch, right, ref64, yard


def _forward(det, batch, right, dev, order=None):
    """One forward -> {name: CPU tensor in the oracle's layout}.  order: a permutation of the batch."""
    pick = (lambda t: t) if order is None else (lambda t: t[order].contiguous())
    img, disp = pick(batch['img']).to(dev), pick(batch['disp_postp']).to(dev)
    if det.stereo:
        det.forward_phase(0, img=img, right=pick(right).to(dev))
        head = det.forward_phase(1, disp=disp)
    else:
        head = det.forward(img, None if det.rgb_only else disp)
    torch.cuda.synchronize()
    out = {n: det.tap(n).cpu().permute(0, 3, 1, 2).contiguous() for n in TAPS}
    for l, rows in enumerate(det.head_levels(head)):
        out[f'head{l}'] = rows[..., :6].cpu().contiguous()
    return out


@pytest.mark.parametrize('cid', list(CONFIGS))
def test_forced_plans_run_their_paths_and_match_fp64(cid, cuda):
    det, batch, right, ref64, yard = _setup(cid)
    problems, got, rec = [], {}, {'yardstick': yard, 'ratio': {}, 'launches': {}}
    for policy in 'HST':
        det.set_tuning(forced_tuning(det, policy))
        got[policy] = _forward(det, batch, right, cuda)
        launches = dict(summarise(det.launch_report()))
        rec['launches'][policy] = launches
        print(f'{cid} {policy}: {sorted(launches.items())}')
        if launches != EXPECTED[cid][policy]:
            problems.append(f'{policy}: launches {sorted(launches.items())} != expected {sorted(EXPECTED[cid][policy].items())}')
        rec['ratio'][policy] = {}
        for n in NAMES:
            assert got[policy][n].shape == ref64[n].shape, (n, got[policy][n].shape, ref64[n].shape)
            err = rel_err(got[policy][n], ref64[n])
            rec['ratio'][policy][n] = err / yard[n]
            print(f'  {n:13s} gpu-vs-fp64 {err:.2e}  cpu32-vs-fp64 {yard[n]:.2e}  ratio {err / yard[n]:.2f}')
            if not (err <= FACTOR * yard[n] and err <= 1e-3):
                problems.append(f'{policy} {n}: {err:.3e} > {FACTOR} x {yard[n]:.3e}')
    for policy in 'ST':
        for n in NAMES:
            d = rel_err(got[policy][n], got['H'][n])
            if not d <= 2 * FACTOR * yard[n]:
                problems.append(f'{policy} vs H, {n}: {d:.3e} > 2 x {FACTOR} x {yard[n]:.3e}')
    rec['max_ratio'] = {p: max(rec['ratio'][p].values()) for p in 'HST'}
    RECORD[cid] = rec
    write_record('detector_plan_parity.json', RECORD)
    assert not problems, '\n'.join(problems)


def test_expected_table_covers_every_path_away_from_the_benched_shape():
    """Every fast path of the plan runs under S or T in some configuration other than the benched one (N = 8, 736x1280),
    each case above asserting that its report EQUALS the table."""
    seen = {}
    for cid, per in EXPECTED.items():
        for policy in 'ST':
            for key in per[policy]:
                seen.setdefault(key, []).append((cid, policy))
    for key in ('40', '45+2', '56+1', '46+1', '48+2', '48+5', '47', '43', '44', '41', '42'):
        assert key in seen, key
    feat = {cid: int(256 * CONFIGS[cid][3]) for cid in CONFIGS}
    for f in (96, 128, 256):                                   # head_pred<3>, <4>, <8> and the first tower group
        assert any(feat[c] == f for c, _ in seen['47']) and any(feat[c] == f for c, _ in seen['48+2'])
    for f in (128, 256):                                       # the second tower group
        assert any(feat[c] == f for c, _ in seen['48+5'])
    assert not any(feat[c] == 96 for c, _ in seen['48+5'])


def test_invariants_of_the_chained_grouped_plan(cuda):
    """Under S at N = 3: reversing the batch reverses every tap and the head bit for bit; a second forward is
    bit-identical; a forward under H in between leaves no trace (S again reproduces the first S result)."""
    cid = 'w050_d067_3x224x352'
    N, H, W, widen, deepen, kw = CONFIGS[cid]
    det = HipDetector(N, H, W, widen, deepen, 1, **kw)
    det.load_state_dict(synthetic_state_dict(det.param_table(), seed=0))
    batch = synthetic_batch(range(N), H - 16, W, 64)
    s_plan = forced_tuning(det, 'S')
    det.set_tuning(s_plan)
    first = _forward(det, batch, None, cuda)
    assert dict(summarise(det.launch_report())) == EXPECTED[cid]['S']
    again = _forward(det, batch, None, cuda)
    rev = _forward(det, batch, None, cuda, order=list(range(N - 1, -1, -1)))
    det.set_tuning(forced_tuning(det, 'H'))
    other = _forward(det, batch, None, cuda)
    assert dict(summarise(det.launch_report())) == EXPECTED[cid]['H']
    det.set_tuning(s_plan)
    back = _forward(det, batch, None, cuda)
    assert dict(summarise(det.launch_report())) == EXPECTED[cid]['S']
    for n in NAMES:
        assert torch.equal(again[n], first[n]), f'{n}: two forwards differ'
        assert torch.equal(rev[n].flip(0), first[n]), f'{n}: not batch-order invariant'
        assert torch.equal(back[n], first[n]), f'{n}: state leaked between plans'
    assert any(not torch.equal(other[n], first[n]) for n in NAMES), 'H and S plans computed identical bits: S did not run'
