"""GPU: AppearanceFreeLink's device backend (csrc/aflink.hip) stage by stage and end to end.  Gate and transform are
bit-equal to the host's; the confidences are held to the fp64 restatement of tests/aflink_ref.py in units of the fp32
restatement's own error (tests/aflink_cases.py: ref_err, logit_err); the linked rows equal the host backend's, whose
decisions the generator's preconditions (tests/test_cpu_aflink.py) make independent of the summation order."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aflink_cases as cases  # noqa: E402
import aflink_ref as ref  # noqa: E402
from stereotracking_amd import _lib, aflink  # noqa: E402
from stereotracking_amd.aflink import AppearanceFreeLink  # noqa: E402

pytestmark = pytest.mark.gpu
_CACHE = {}


def linker(**kw):
    """One device linker (one packed copy of the generator's weights) for the whole module."""
    key = tuple(sorted(kw.items()))
    if key not in _CACHE:
        c = cases.case()
        _CACHE[key] = AppearanceFreeLink(c['state_dict'], confidence_threshold=c['threshold'], backend='device', **kw)
    return _CACHE[key]


def group_pairs():
    return int(_lib.load().st_aflink_group_pairs())


def singles():
    """(conf, logits) of the first 3 P + 5 candidates of the generator, every one scored in a call of its own."""
    if 'singles' not in _CACHE:
        x = cases.case()['x'][:3 * group_pairs() + 5]
        got = [linker().device_stages(None, x=x[k:k + 1]) for k in range(len(x))]
        _CACHE['singles'] = (np.concatenate([g['conf'] for g in got]), np.concatenate([g['logits'] for g in got]))
    return _CACHE['singles']


def host_candidates(row_arrays, temporal=(0, 30), spatial=75):
    """(K, 3) (set, i, j) in row-major order and the (K, 2, 30, 3) inputs, by the host backend's functions."""
    cand, x = [], []
    for s, rows in enumerate(row_arrays):
        info = aflink.build_tracks(rows)['info']
        for i, j in np.argwhere(aflink.gate(info, temporal, spatial)):
            cand.append((s, i, j))
            x.append(np.stack(aflink.transform(info[i], info[j])))
    return np.array(cand, np.int32).reshape(-1, 3), np.array(x, np.float32).reshape(-1, 2, 30, 3)


def track(tid, frames, x, y):
    f = np.asarray(frames, np.float64)
    x, y = np.broadcast_to(np.asarray(x, np.float64), f.shape), np.broadcast_to(np.asarray(y, np.float64), f.shape)
    return np.column_stack([f, np.full(len(f), float(tid)), x, y, x + 10, y + 20, np.full(len(f), 0.9)])


# ---------------------------------------------------------------------- gate
@pytest.mark.parametrize('n_tracks', [0, 1, 2, 70])
def test_gate_equals_the_host(n_tracks):
    rows = cases.video(11, n_tracks, frames=40) if n_tracks != 70 else cases.case()['rows']
    got = linker().device_stages([rows], want=('gate',))['cand']
    want, _ = host_candidates([rows])
    assert got.dtype == np.int32 and np.array_equal(got, want)
    if n_tracks == 70:
        assert np.array_equal(got[:, 1:], cases.case()['pairs']) and len(got) > 300
        flags = np.zeros((70, 70), bool)
        flags[got[:, 1], got[:, 2]] = True
        assert np.array_equal(flags, ref.gate_flags(cases.case()['infos']))


def test_gate_of_several_sets_in_one_call():
    sets = [cases.video(24, 15, frames=30), np.zeros((0, 7)), cases.video(22, 33, frames=60), cases.video(23, 1)]
    got = linker().device_stages(sets, want=('gate',))['cand']
    want, _ = host_candidates(sets)
    assert len(want) > 40 and set(want[:, 0]) == {0, 2} and np.array_equal(got, want)
    other = AppearanceFreeLink(None, temporal_threshold=(-5, 12), spatial_threshold=40.5, backend='device')
    want, _ = host_candidates(sets, (-5, 12), 40.5)
    assert len(want) > 10 and np.array_equal(other.device_stages(sets, want=('gate',))['cand'], want)


def test_gate_boundaries():
    up = np.nextafter(75.0, np.inf)
    sets = [np.concatenate([track(1, [3, 10], 0, 0), track(2, [10 + dt, 50], 45, 60)]) for dt in (-1, 0, 30, 31)]
    sets.append(np.concatenate([track(1, [0, 1], 0, 0), track(2, [2, 3], 45, 60), track(3, [2, 3], 0, up),
                                track(4, [2, 3], -45, -60)]))
    got = linker().device_stages(sets, want=('gate',))['cand']
    assert got.tolist() == [[1, 0, 1], [2, 0, 1], [4, 0, 1], [4, 0, 3]]
    assert np.array_equal(got, host_candidates(sets)[0])


# ---------------------------------------------------------------------- transform
def test_transform_is_bit_equal_to_the_host():
    sets = []
    for ni, nj in [(1, 1), (29, 31), (30, 30), (31, 29), (1, 40), (45, 2)]:
        rng = np.random.default_rng(ni * 100 + nj)
        a = track(1, 99000 + np.arange(ni), 50 + rng.uniform(0, 20, ni), 60 + rng.uniform(0, 20, ni))
        b = track(2, 99000 + ni + 2 + np.arange(nj), 50 + rng.uniform(0, 20, nj), 60 + rng.uniform(0, 20, nj))
        sets.append(np.concatenate([a, b]))
    const = np.concatenate([track(1, np.arange(30), 12.5, np.arange(30) * 2.0), track(2, 30 + np.arange(30), 12.5, 30.0)])
    sets.append(const)
    got = linker().device_stages(sets, want=('gate', 'transform'))
    cand, x = host_candidates(sets)
    assert len(cand) == len(sets) and np.array_equal(got['cand'], cand)
    assert got['x'].dtype == np.float32 and np.array_equal(got['x'].view(np.uint32), x.view(np.uint32))
    assert np.all(got['x'][-1][:, :, 1] == 0)                                # the constant column
    c = cases.case()
    got = linker().device_stages([c['rows']], want=('gate', 'transform'))
    assert np.array_equal(got['x'], c['x']) and np.array_equal(got['x'], host_candidates([c['rows']])[1])


# ---------------------------------------------------------------------- score
def score_counts():
    p = group_pairs()
    return [1, p - 1, p, p + 1, 3 * p + 5]


@pytest.mark.parametrize('which', range(5))
def test_score_counts_around_the_group_size(which):
    c, n = cases.case(), score_counts()[which]
    got = linker().device_stages(None, x=c['x'][:n])
    one_conf, one_logits = singles()
    assert got['conf'].shape == (n,) and got['conf'].dtype == np.float32
    # a candidate's bytes do not depend on its neighbours or its place in a group
    assert np.array_equal(got['conf'].view(np.uint32), one_conf[:n].view(np.uint32))
    assert np.array_equal(got['logits'].view(np.uint32), one_logits[:n].view(np.uint32))
    err = np.abs(got['conf'].astype(np.float64) - c['conf64'][:n]).max()
    lerr = np.abs(got['logits'].astype(np.float64) - c['logits64'][:n]).max()
    print(f'n {n}: conf err {err:.3e} = {err / c["ref_err"]:.2f} ref_err, logit err {lerr:.3e} = {lerr / c["logit_err"]:.2f} '
          f'logit_err')
    assert err <= 4 * c['ref_err'] + 2.0 ** -23
    assert lerr <= 4 * c['logit_err']


def test_score_of_all_candidates_against_fp64():
    c = cases.case()
    got = linker().device_stages(None, x=c['x'])
    err = np.abs(got['conf'].astype(np.float64) - c['conf64']).max()
    lerr = np.abs(got['logits'].astype(np.float64) - c['logits64']).max()
    print(f'{len(c["x"])} candidates: conf err {err:.3e} = {err / c["ref_err"]:.2f} ref_err (ref_err {c["ref_err"]:.3e}), '
          f'logit err {lerr:.3e} = {lerr / c["logit_err"]:.2f} logit_err (logit_err {c["logit_err"]:.3e})')
    assert err <= 4 * c['ref_err'] + 2.0 ** -23 and lerr <= 4 * c['logit_err']
    assert np.array_equal(got['conf'][:len(singles()[0])].view(np.uint32), singles()[0].view(np.uint32))
    assert np.array_equal(got['conf'] >= c['threshold'], c['conf64'] >= c['threshold'])
    again = linker().device_stages(None, x=c['x'])
    assert np.array_equal(again['conf'].view(np.uint32), got['conf'].view(np.uint32))


# ---------------------------------------------------------------------- end to end
def host_rows():
    if 'host' not in _CACHE:
        c = cases.case()
        host = AppearanceFreeLink(c['state_dict'], confidence_threshold=c['threshold'])
        sub = c['rows'][c['rows'][:, 1] < 35]                  # its candidates are a subset of the generator's
        _CACHE['host'] = ([c['rows'], np.zeros((0, 7)), sub], [host.forward(c['rows']), np.zeros((0, 7)), host.forward(sub)])
    return _CACHE['host']


def test_forward_many_equals_the_host_and_repeats_byte_for_byte():
    sets, want = host_rows()
    before = aflink.LAUNCHES['st_aflink_run']
    got = linker().forward_many(sets)
    assert aflink.LAUNCHES['st_aflink_run'] == before + 1                     # one call for all sets
    assert len(got) == 3
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == np.float64 and np.array_equal(g, w)
    assert len(np.unique(got[0][:, 1])) < 70
    again = linker().forward_many(sets)
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got))
    one = linker().forward(sets[0])
    assert aflink.LAUNCHES['st_aflink_run'] == before + 3 and one.tobytes() == got[0].tobytes()


def test_rounds_by_workspace_budget_do_not_change_the_result():
    sets, want = host_rows()
    small, timing = linker().forward_many(sets, workspace_budget=720 * 7, timing=True)
    assert timing['rounds'] == -(-timing['capacity'] // 7) and timing['rounds'] > 50
    assert timing['candidates'] <= timing['capacity']
    assert all(np.array_equal(s, w) for s, w in zip(small, want))
    with pytest.raises(ValueError, match='workspace'):
        linker().forward_many(sets, workspace_budget=719)


def test_sets_without_candidates():
    far = np.concatenate([track(1, [0, 1], 0, 0), track(2, [40, 41], 0, 0)])
    out = linker().forward_many([far, np.zeros((0, 7))])
    assert np.array_equal(out[0], far) and out[1].shape == (0, 7)
    near = np.concatenate([track(1, [0, 1], 0, 0), track(2, [4, 5], 500, 0)])      # passes the temporal rule only
    assert np.array_equal(linker().forward(near), near)


# ---------------------------------------------------------------------- refusals, stale memory
def test_refusing_entry_points_write_nothing():
    lib = _lib.load()
    link = linker()
    dev = torch.device('cuda', torch.cuda.current_device())
    weights = link.device_weights(dev)
    c = cases.case()
    p = link.plan([c['rows']])
    cap = p['capacity']
    tabs = {k: torch.from_numpy(np.ascontiguousarray(p[k])).to(dev) for k in ('feat', 'trk_off', 'trk_set', 'set_off')}
    out = torch.full((2 + 3 * cap + cap + p['T'] + 1 + 180 * cap,), 0x5A5A5A5A, dtype=torch.int32, device=dev)

    def args(**kw):
        a = link._args(p, cap, cap)
        for k, v in tabs.items():
            setattr(a, k, C.c_void_p(v.data_ptr()))
        base = out.data_ptr()
        a.header, a.cand, a.conf = (C.c_void_p(base + 4 * o) for o in (0, 2, 2 + 3 * cap))
        a.ws_off, a.ws_x = C.c_void_p(base + 4 * (2 + 4 * cap)), C.c_void_p(base + 4 * (2 + 4 * cap + p['T'] + 1))
        a.count = cap
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    stream = _lib.current_stream()
    too_many = int(lib.st_aflink_max_candidates()) + 1
    for bad in (dict(struct_size=8), dict(capacity=too_many), dict(capacity=-1), dict(header=None), dict(num_tracks=-1),
                dict(num_rows=2 ** 31 // 3 + 1), dict(feat=None), dict(cand=None), dict(ws_off=None), dict(chunk=0),
                dict(ws_x=None), dict(conf=None)):
        assert lib.st_aflink_run(C.byref(args(**bad)), weights.handle, stream) != 0, bad
    assert lib.st_aflink_run(C.byref(args()), None, stream) != 0
    assert lib.st_aflink_gate(C.byref(args(trk_set=None)), stream) != 0
    for bad in (dict(first=-1), dict(first=1, count=cap), dict(count=-1), dict(ws_x=None)):
        assert lib.st_aflink_transform(C.byref(args(**bad)), stream) != 0, bad
        assert lib.st_aflink_score(C.byref(args(**bad)), weights.handle, stream) != 0, bad
    assert lib.st_aflink_score(C.byref(args()), None, stream) != 0
    assert b'st_aflink_score' in lib.st_last_error()
    handle = C.c_void_p()
    packed = aflink.pack_weights(c['state_dict'])
    assert lib.st_aflink_weights_create(packed.ctypes.data_as(C.c_void_p), packed.size - 1, C.byref(handle)) != 0
    assert not handle.value
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A5A5A).all())
    # the same buffers, nothing refused: the call works
    assert lib.st_aflink_run(C.byref(args()), weights.handle, stream) == 0
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert host[0] == len(c['pairs']) and host[1] == 0
    assert np.array_equal(host[2:2 + 3 * host[0]].reshape(-1, 3)[:, 1:], c['pairs'])
    with pytest.raises(ValueError, match='32-bit'):
        many = np.concatenate([track(k, [0], 0, 0) for k in range(3)])
        fake = AppearanceFreeLink(None, backend='device')
        fake.plan = lambda rows: dict(AppearanceFreeLink.plan(fake, rows), capacity=too_many)
        fake.forward(many)


def test_stale_bits_in_the_buffers_change_nothing():
    c = cases.case()
    sets = [c['rows'][c['rows'][:, 1] < 30], np.zeros((0, 7)), cases.video(22, 12, frames=40)]
    clean = linker().device_stages(sets, poison=0x00)
    for poison in (0xFF, 0x7F):
        dirty = linker().device_stages(sets, poison=poison)
        assert len(dirty['cand']) == len(clean['cand']) > 50
        for k in ('cand', 'x', 'conf', 'logits'):
            assert dirty[k].tobytes() == clean[k].tobytes(), (k, poison)
