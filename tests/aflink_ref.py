"""The yardstick of the AppearanceFreeLink tests: an independent restatement of the rules of DESIGN.md section 18, written
from the rules and sharing no code with stereotracking_amd/aflink.py.  The network is evaluated with torch's functional
operators straight from a state dict, in fp32 AND in fp64: |fp32 - fp64| is the reference's own error, the unit of the
device tolerances."""
import numpy as np
import torch
import torch.nn.functional as F

INF = 1e5


def tracks(rows):
    """-> (rows in a stable sort by frame, ids by (first frame, id), per id its (n, 3) rows (frame, c0, c1))."""
    rows = np.asarray(rows, np.float64).reshape(-1, 7)
    rows = rows[np.argsort(rows[:, 0], kind='stable')]
    per_id = {}
    for r in rows:
        per_id.setdefault(int(r[1]), []).append([r[0], r[2], r[3]])
    ids = sorted(per_id, key=lambda k: (per_id[k][0][0], k))
    return rows, ids, [np.array(per_id[k]) for k in ids]


def gate_flags(infos, temporal=(0, 30), spatial=75):
    n = len(infos)
    keep = np.zeros((n, n), bool)
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            dt = infos[j][0][0] - infos[i][-1][0]
            if dt < temporal[0] or dt > temporal[1]:
                continue
            dx = infos[i][-1][1] - infos[j][0][1]
            dy = infos[i][-1][2] - infos[j][0][2]
            if np.sqrt(dx * dx + dy * dy) > spatial:
                continue
            keep[i, j] = True
    return keep


def transform64(info_i, info_j, length=30):
    """The two (30, 3) inputs in fp64 (cast to fp32 for the network)."""
    a = np.zeros((length, 3))
    b = np.zeros((length, 3))
    tail = info_i[-length:]
    head = info_j[:length]
    a[length - len(tail):] = tail
    b[:len(head)] = head
    both = np.vstack([a, b])
    lo, hi = both.min(0), both.max(0)
    sub = (hi + lo) / 2
    div = (hi - lo) / 2 + 1e-5
    return (a - sub) / div, (b - sub) / div


def _bn(x, sd, prefix, dtype):
    shape = [1, -1] + [1] * (x.dim() - 2)
    mean, var = sd[prefix + '.running_mean'].to(dtype).view(shape), sd[prefix + '.running_var'].to(dtype).view(shape)
    return (x - mean) / torch.sqrt(var + 1e-5) * sd[prefix + '.weight'].to(dtype).view(shape) + \
        sd[prefix + '.bias'].to(dtype).view(shape)


def net_logits(sd, x1, x2, dtype):
    """x1, x2: (B, 30, 3) fp32 arrays -> (B, 2) logits evaluated in `dtype`."""
    feats = []
    for m, x in ((1, x1), (2, x2)):
        x = torch.as_tensor(np.asarray(x, np.float32)).to(dtype)[:, None]           # (B, 1, 30, 3)
        for layer in range(4):
            p = f'TemporalModule_{m}.{layer}'
            x = F.conv2d(x, sd[p + '.conv.weight'].to(dtype))
            x = torch.stack([_bn(x[..., c], sd, f'{p}.{name}', dtype) for c, name in enumerate(('bnf', 'bnx', 'bny'))], -1)
            x = torch.relu(x)
        x = F.conv2d(x, sd[f'FusionBlock_{m}.conv.weight'].to(dtype))
        x = torch.relu(_bn(x, sd, f'FusionBlock_{m}.bn', dtype))
        feats.append(x.mean(dim=(2, 3)))
    h = torch.relu(F.linear(torch.cat(feats, 1), sd['classifier.fc1.weight'].to(dtype), sd['classifier.fc1.bias'].to(dtype)))
    return F.linear(h, sd['classifier.fc2.weight'].to(dtype), sd['classifier.fc2.bias'].to(dtype))


def confidence(logits):
    return torch.softmax(logits, dim=1)[:, 1]


def inputs(infos, pairs):
    """(K, 2, 30, 3) fp32 network inputs of the pairs."""
    x = np.zeros((len(pairs), 2, 30, 3), np.float32)
    for k, (i, j) in enumerate(pairs):
        a, b = transform64(infos[i], infos[j])
        x[k, 0], x[k, 1] = a.astype(np.float32), b.astype(np.float32)
    return x


def scores(sd, x, dtype, batch=64):
    """-> (conf (K,), logits (K, 2)) as numpy arrays of `dtype`."""
    lg = []
    with torch.no_grad():
        for k in range(0, len(x), batch):
            lg.append(net_logits(sd, x[k:k + batch, 0], x[k:k + batch, 1], dtype))
    if not lg:
        return np.zeros(0), np.zeros((0, 2))
    lg = torch.cat(lg)
    return confidence(lg).numpy(), lg.numpy()


def link(rows, pairs, conf32, threshold):
    """Cost, assignment, chain resolution, relabelling, duplicates, output order."""
    from scipy.optimize import linear_sum_assignment
    rows, ids, _ = tracks(rows)
    n = len(ids)
    if n == 0:
        return np.zeros((0, 7))
    cost = np.full((n, n), INF)
    for (i, j), c in zip(pairs, np.asarray(conf32, np.float32)):
        if float(c) >= threshold:
            cost[i, j] = float(np.float32(1) - np.float32(c))
    ri, ci = linear_sum_assignment(cost)
    first = {}
    for i, j in zip(ri, ci):
        if cost[i, j] < INF:
            first[ids[i]] = ids[j]
    final = {}
    for k, v in first.items():
        if k in final:
            final[v] = final[k]
        else:
            final[v] = k
    rows = rows.copy()
    for k, v in final.items():
        rows[rows[:, 1] == k, 1] = v
    seen, keep = set(), []
    for r in range(len(rows)):
        key = (rows[r, 0], rows[r, 1])
        if key not in seen:
            seen.add(key)
            keep.append(r)
    rows = rows[keep]
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))]


def forward(rows, sd, temporal=(0, 30), spatial=75, threshold=0.95):
    _, _, infos = tracks(rows)
    pairs = np.argwhere(gate_flags(infos, temporal, spatial))
    conf, _ = scores(sd, inputs(infos, pairs), torch.float32)
    return link(rows, pairs, conf, threshold)
