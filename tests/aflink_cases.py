"""Shared generator of the AppearanceFreeLink tests: weights whose confidences spread over (0, 1), fragmented tracks whose
pairs pass the gate, and a confidence threshold that lies in a gap of the fp64 confidences.  Everything is computed
once per process and handed out unchanged."""
import functools

import numpy as np
import torch

import aflink_ref as ref


def fragments(seed, n_tracks, frames=120, max_len=45, extent=160.0, first_id=0, id_step=1):
    """(N, 7) rows of n_tracks fragments: random start frames, 1 .. max_len rows with a few frames missing, corners on a
    slow random walk inside an extent x extent window (so a good share of the pairs passes the 75-pixel gate)."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n_tracks):
        n = int(rng.integers(1, max_len + 1))
        start = int(rng.integers(0, frames))
        steps = rng.integers(1, 3, n)
        f = start + np.cumsum(steps) - steps[0]
        xy = rng.uniform(0, extent, 2) + np.cumsum(rng.normal(0, 2.0, (n, 2)), 0)
        wh = rng.uniform(10, 40, 2)
        for t in range(n):
            rows.append([f[t], first_id + k * id_step, xy[t, 0], xy[t, 1], xy[t, 0] + wh[0], xy[t, 1] + wh[1],
                         rng.uniform(0.3, 1.0)])
    return np.array(rows, np.float64).reshape(-1, 7)


def _sorted_back(rows):
    """The rows of the ids interleaved at random, every id's own rows still in frame order (the input rule)."""
    order = np.lexsort((rows[:, 0], rows[:, 1]))
    rng = np.random.default_rng(len(rows))
    ids = rows[order, 1]
    # a stable sort by a random key per row that is monotone inside every id
    key = np.zeros(len(rows))
    for i in np.unique(ids):
        m = ids == i
        key[m] = np.sort(rng.uniform(0, 1, int(m.sum())))
    return rows[order][np.argsort(key, kind='stable')]


def video(seed, n_tracks, **kw):
    return _sorted_back(fragments(seed, n_tracks, **kw)) if n_tracks else np.zeros((0, 7))


def candidates(rows):
    """-> (infos, pairs (K, 2), x (K, 2, 30, 3) fp32) by the restatement."""
    _, _, infos = ref.tracks(rows)
    pairs = np.argwhere(ref.gate_flags(infos))
    return infos, pairs, ref.inputs(infos, pairs)


AFLINK_SHAPES = tuple(
    [(f'TemporalModule_{m}.{l}.conv.weight', (co, ci, 7, 1)) for m in (1, 2)
     for l, (ci, co) in enumerate(((1, 32), (32, 64), (64, 128), (128, 256)))] +
    [(f'FusionBlock_{m}.conv.weight', (256, 256, 1, 3)) for m in (1, 2)] +
    [('classifier.fc1.weight', (128, 512)), ('classifier.fc1.bias', (128,)),
     ('classifier.fc2.weight', (2, 128)), ('classifier.fc2.bias', (2,))])
AFLINK_NORMS = tuple([(f'TemporalModule_{m}.{l}.{bn}', c) for m in (1, 2) for l, c in enumerate((32, 64, 128, 256))
                      for bn in ('bnf', 'bnx', 'bny')] + [(f'FusionBlock_{m}.bn', 256) for m in (1, 2)])


def recipe_state_dict(seed):
    """The link network's state dict (reference naming) from numpy's legacy RandomState, whose stream is frozen: the same
    bytes on every machine and under every torch.  tests/golden/reference/aflink.npz is recorded with these weights (a
    stored state dict would be 4.2 MB) and keeps their sha256 (state_dict_sha256 below)."""
    rng = np.random.RandomState(seed)
    sd = {}
    for name, shape in AFLINK_SHAPES:
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        scale = np.float32(np.sqrt(2.0 / fan_in)) if len(shape) > 1 else np.float32(0.05)
        sd[name] = torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * scale)
    for prefix, c in AFLINK_NORMS:
        sd[prefix + '.weight'] = torch.from_numpy(rng.uniform(0.5, 1.5, c).astype(np.float32))
        sd[prefix + '.bias'] = torch.from_numpy((rng.standard_normal(c) * 0.1).astype(np.float32))
        sd[prefix + '.running_mean'] = torch.from_numpy((rng.standard_normal(c) * 0.1).astype(np.float32))
        sd[prefix + '.running_var'] = torch.from_numpy(rng.uniform(0.5, 1.5, c).astype(np.float32))
        sd[prefix + '.num_batches_tracked'] = torch.zeros((), dtype=torch.long)
    return sd


def state_dict_sha256(sd):
    import hashlib
    h = hashlib.sha256()
    for k in sorted(sd):
        if not k.endswith('num_batches_tracked'):
            h.update(k.encode() + np.ascontiguousarray(sd[k].numpy()).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def case(seed=0, n_tracks=70):
    """dict(state_dict, rows, infos, pairs, x, conf64, conf32, logits64, logits32, ref_err, logit_err, threshold).
    The weights: the module's initialisation, BatchNorm statistics randomised, fc2 rescaled and re-biased so that the
    fp64 confidences of this video's candidates spread over (0, 1)."""
    from stereotracking_amd.aflink import AFLinkModel
    torch.manual_seed(seed)
    sd = {k: v.clone() for k, v in AFLinkModel().state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    for k in sd:
        if k.endswith('running_mean'):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.1
        elif k.endswith('running_var'):
            sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
        elif '.bn' in k and k.endswith('.weight'):
            sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
        elif '.bn' in k and k.endswith('.bias'):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.1
    rows = video(seed + 2, n_tracks)
    infos, pairs, x = candidates(rows)
    assert len(pairs) >= 40, f'the generator made {len(pairs)} candidates only'
    _, lg = ref.scores(sd, x, torch.float64)
    d = lg[:, 1] - lg[:, 0]
    scale = 2.5 / max(float(d.std()), 1e-12)                    # logit difference: median 0, spread 2.5
    w, b = sd['classifier.fc2.weight'].double(), sd['classifier.fc2.bias'].double()
    shift = float(np.median(d)) * scale
    sd['classifier.fc2.weight'] = (w * scale).float()
    sd['classifier.fc2.bias'] = (b * scale - torch.tensor([-shift / 2, shift / 2], dtype=torch.float64)).float()
    conf64, logits64 = ref.scores(sd, x, torch.float64)
    conf32, logits32 = ref.scores(sd, x, torch.float32)
    ref_err = float(np.abs(conf32.astype(np.float64) - conf64).max())
    logit_err = float(np.abs(logits32.astype(np.float64) - logits64).max())
    # the threshold: the middle of the widest gap of the sorted fp64 confidences between the quartiles
    s = np.sort(conf64)
    q0, q1 = len(s) // 4, 3 * len(s) // 4
    k = q0 + int(np.argmax(np.diff(s[q0:q1 + 1])))
    threshold = float((s[k] + s[k + 1]) / 2)
    return dict(state_dict=sd, rows=rows, infos=infos, pairs=pairs, x=x, conf64=conf64, conf32=conf32, logits64=logits64,
                logits32=logits32, ref_err=ref_err, logit_err=logit_err, threshold=threshold)
