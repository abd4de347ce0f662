"""GPU: what the device entries built on stereotracking_amd/_packed.py promise about `timing` and LAUNCHES.

For every entry, on a small case of its own test file: timing=True returns bit for bit what timing=False returns; the
timing dict has the keys the tools/*_bench.py scripts read - stages_ms with exactly the entry's stage names, every value
finite and >= 0, and the host clock's four parts; the module's LAUNCHES counter moves by one per stage (two for
st_mot_file_round: ground truth and predictions)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_schedule as ss  # noqa: E402
from stereotracking_amd import aflink, mot_eval, tracklets  # noqa: E402

pytestmark = pytest.mark.gpu
CLOCK = ('host_prepare_s', 'device_and_copies_s', 'host_finish_s', 'total_s')
SCORING = ('st_mot_similarity', 'st_mot_walk', 'st_mot_hota_match', 'st_mot_hota_accumulate')
CHALLENGE = {'st_mot_file_round': 2, 'st_mot_challenge_preprocess': 1}


def _evaluate_packed(cuda):
    import mot_eval_cases as cases
    packed = mot_eval.pack_sequences(*cases.scenario('random_b3'))
    return lambda timing: mot_eval.evaluate_packed(packed, 0.5, device=cuda, timing=timing, return_arrays=True)


def _kitti(cuda):
    import kitti_eval_cases as cases
    s = cases.rule_sequence()
    return lambda timing: mot_eval.kitti_keep_masks([s], cases.BOTH, device=cuda, timing=timing)


def _challenge(entry):
    def build(cuda):
        import motchallenge_ref as ref
        gts, preds = zip(*ref.videos().values())
        return lambda timing: entry(list(gts), list(preds), 'MOT17', device=cuda, videos=list(ref.videos()), timing=timing)
    return build


def _tracklets(cuda):
    from test_tracklets_gpu import _mixed_tracks
    sets, _ = _mixed_tracks()
    it = tracklets.InterpolateTracklets(use_gsi=True, backend='device')
    return lambda timing: it.forward_many(sets, device=cuda, timing=timing)


def _aflink(cuda):
    import aflink_cases as cases
    c = cases.case(n_tracks=30)
    link = aflink.AppearanceFreeLink(c['state_dict'], confidence_threshold=c['threshold'], backend='device')
    return lambda timing: link.forward_many([c['rows'], np.zeros((0, 7))], device=cuda, timing=timing)


# entry -> (its run(timing) builder, the module that counts, {stage: launches} in stages_ms order, the nested dict's stages)
ENTRIES = {
    'evaluate_packed': (_evaluate_packed, mot_eval, dict.fromkeys(SCORING, 1), None),
    'kitti_keep_masks': (_kitti, mot_eval, {'st_mot_kitti_preprocess': 1}, None),
    'motchallenge_keep_masks': (_challenge(mot_eval.motchallenge_keep_masks), mot_eval, CHALLENGE, None),
    'evaluate_motchallenge': (_challenge(mot_eval.evaluate_motchallenge), mot_eval, dict.fromkeys(SCORING, 1), CHALLENGE),
    'InterpolateTracklets': (_tracklets, tracklets, {'st_tracklet_interpolate': 1, 'st_tracklet_gsi': 1}, None),
    'AppearanceFreeLink': (_aflink, aflink, {'st_aflink_run': 1}, None),
}


def _check_stages(stages_ms, names, where):
    assert list(stages_ms) == list(names), where
    for k, v in stages_ms.items():
        assert isinstance(v, float) and math.isfinite(v) and v >= 0.0, (where, k, v)


@pytest.mark.parametrize('entry', list(ENTRIES))
def test_timing_changes_no_result_and_has_the_keys_the_benches_read(cuda, entry):
    build, module, stages, nested = ENTRIES[entry]
    run = build(cuda)
    expected = dict(stages, **(nested or {}))
    before = dict(module.LAUNCHES)
    plain = run(False)
    moved = {k: module.LAUNCHES[k] - before.get(k, 0) for k in set(module.LAUNCHES) | set(expected)}
    assert {k: v for k, v in moved.items() if v} == expected, entry
    before = dict(module.LAUNCHES)
    timed, tm = run(True)
    assert {k: module.LAUNCHES[k] - before.get(k, 0) for k in expected} == expected, entry
    assert len(plain) > 0 and not ss.differences(plain, timed), (entry, ss.differences(plain, timed)[:8])

    assert set(CLOCK) | {'stages_ms'} <= set(tm), entry
    _check_stages(tm['stages_ms'], stages, entry)
    for k in CLOCK:
        assert isinstance(tm[k], float) and math.isfinite(tm[k]) and tm[k] >= 0.0, (entry, k, tm[k])
    assert abs(tm['host_prepare_s'] + tm['device_and_copies_s'] + tm['host_finish_s'] - tm['total_s']) <= 1e-9 * 3, entry
    if nested:
        assert set(tm['challenge']) == {'stages_ms', 'host_prepare_s', 'device_and_copies_s'}
        _check_stages(tm['challenge']['stages_ms'], nested, entry + '.challenge')
        assert all(tm['challenge'][k] >= 0.0 for k in CLOCK[:2])
    else:
        assert 'challenge' not in tm
