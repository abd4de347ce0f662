"""Tracklet linking after the tracker has run: AppearanceFreeLink (AFLink; StrongSORT, arXiv 2202.13514).  A small
convolutional network scores every plausible (earlier track, later track) pair from their motion alone, a linear
assignment picks the links, the later track takes the earlier one's id.

Behavioural spec: reference mmtrack/models/task_modules/track/aflink.py, restated.  Rows are
(frame, id, c0, c1, c2, c3, score) in fp64; only frame, id, c0, c1 take part, the other columns are carried through.
  1. tracks: per id the rows (frame, c0, c1) in frame order;
  2. gate, every ordered pair i != j: dt = first_frame(j) - last_frame(i) with temporal_threshold[0] <= dt <=
     temporal_threshold[1], and sqrt(dx**2 + dy**2) <= spatial_threshold between the corners of i's last and j's first
     row (fp64, unfused, in this order);
  3. transform: i's last 30 rows (zero rows in front when shorter), j's first 30 (zero rows behind); per column
     (v - (max + min) / 2) / ((max - min) / 2 + 1e-5) with min and max over all 60 rows, the pads included; fp64, then
     one cast to fp32;
  4. network (AFLinkModel, eval mode): two temporal modules of four blocks (conv (7, 1) without bias, one BatchNorm per
     column, ReLU; channels 1-32-64-128-256, time 30-24-18-12-6), a fusion block each (conv (1, 3), BatchNorm2d, ReLU),
     the mean over the 6 positions, fc1 512 -> 128, ReLU, fc2 128 -> 2, softmax; the confidence is class 1;
  5. cost: float64(float32(1) - conf32) where float(conf32) >= confidence_threshold (compared in fp64), else 1e5;
  6. scipy's linear_sum_assignment on the dense matrix, matches below 1e5 accepted, the reference's chain resolution
     and relabelling in insertion order, duplicate (frame, id) rows removed.

Decided where the reference is wrong or undefined ("parity unpinned"):
  * links are made between ids: the reference stores matrix indices and compares them with the id column, which is
    right only when the ids are 0 .. N - 1 in order of first appearance;
  * track order (it decides ties of the assignment only): first frame, then id, ascending;
  * output order: ascending frame, then ascending id (as InterpolateTracklets);
  * two linked tracks may share a frame when dt = 0: the row that comes first in a stable sort of the input by frame
    is kept;
  * frames and ids must be integral and the frames of one id strictly increasing in input order (the checks of
    tracklets._sorted_tracks), c0 and c1 finite, else ValueError; empty input returns (0, 7); a track of one row is a
    track - nothing is dropped.

backend='host' (numpy, the torch CPU module pair by pair) is the executable specification.  backend='device' runs
csrc/aflink.hip (st_aflink_run; include/stereotrack.h section 18): gate and transform are bit-equal to the host's, the
confidences are another correct fp32 evaluation of the network; the assignment and the relabelling are the same host
code on both backends.  There is no fallback from 'device' to 'host'.
"""
import collections
import collections.abc
import ctypes as C
import time

import numpy as np
import torch
from torch import nn

from . import _lib
from ._packed import PackedCall
from .metrics import _check_backend
from .registry import TASK_UTILS
from .tracklets import _as_rows, _finish, _sorted_tracks

INFINITY = 1e5
LENGTH = 30                          # rows of a transformed track
WORKSPACE_BUDGET_BYTES = 256 << 20   # the transformed inputs of one round of st_aflink_run (720 bytes per candidate)
LAUNCHES = collections.Counter()     # calls of every st_aflink_* stage entry (tests read it)
TEMPORAL_CHANNELS = (1, 32, 64, 128, 256)


# ---------------------------------------------------------------------- the link network
class TemporalBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, (7, 1), bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.bnf = nn.BatchNorm1d(cout)
        self.bnx = nn.BatchNorm1d(cout)
        self.bny = nn.BatchNorm1d(cout)

    def forward(self, x):
        x = self.conv(x)                                                  # (B, C, T, 3)
        x = torch.stack([bn(x[..., c]) for c, bn in enumerate((self.bnf, self.bnx, self.bny))], dim=-1)
        return self.relu(x)


class FusionBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, (1, 3), bias=False)
        self.bn = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.relu(self.bn(self.conv(x)))


class Classifier(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.fc1 = nn.Linear(cin * 2, cin // 2)
        self.relu = nn.ReLU(inplace=True)
        self.fc2 = nn.Linear(cin // 2, cout)

    def forward(self, x1, x2):
        return self.fc2(self.relu(self.fc1(torch.cat((x1, x2), dim=1))))


class AFLinkModel(nn.Module):
    """The link network under the reference's module names, so that a published AFLink checkpoint loads with
    load_state_dict.  Evaluation only.  forward(x1, x2): (B, 1, 30, >= 3) each -> (B,) probability of class 1."""

    def __init__(self):
        super().__init__()
        ch = TEMPORAL_CHANNELS
        self.TemporalModule_1 = nn.Sequential(*[TemporalBlock(ch[i], ch[i + 1]) for i in range(4)])
        self.TemporalModule_2 = nn.Sequential(*[TemporalBlock(ch[i], ch[i + 1]) for i in range(4)])
        self.FusionBlock_1 = FusionBlock(256, 256)
        self.FusionBlock_2 = FusionBlock(256, 256)
        self.pooling = nn.AdaptiveAvgPool2d((1, 1))
        self.classifier = Classifier(256, 2)

    def logits(self, x1, x2):
        if self.training:
            raise RuntimeError('AFLinkModel: only evaluation is supported, call eval()')
        x1 = self.FusionBlock_1(self.TemporalModule_1(x1[..., :3]))
        x2 = self.FusionBlock_2(self.TemporalModule_2(x2[..., :3]))
        return self.classifier(self.pooling(x1).flatten(1), self.pooling(x2).flatten(1))

    def forward(self, x1, x2):
        return torch.softmax(self.logits(x1, x2), dim=1)[:, 1]


def _fold_bn(sd, prefix):
    """BatchNorm with running statistics as scale and shift, folded in fp64, rounded once to fp32."""
    g, b = sd[prefix + '.weight'].double(), sd[prefix + '.bias'].double()
    scale = g / torch.sqrt(sd[prefix + '.running_var'].double() + 1e-5)
    return scale.float().numpy(), (b - sd[prefix + '.running_mean'].double() * scale).float().numpy()


def pack_weights(state_dict):
    """The network as the one fp32 array st_aflink_weights_create takes.  Per temporal module, layer 1 .. 4: the conv
    weights as [tap][cin][cout], then scale and shift as [column][cout]; the fusion conv as [tap = column][cin][cout]
    with its scale and shift; then fc1 transposed ([512][128]), its bias, fc2 ([2][128]), its bias."""
    sd = {k: v.detach().cpu() for k, v in state_dict.items()}
    parts = []
    for m in (1, 2):
        for layer in range(4):
            p = f'TemporalModule_{m}.{layer}'
            parts.append(sd[p + '.conv.weight'].float()[:, :, :, 0].permute(2, 1, 0).contiguous().numpy())
            folded = [_fold_bn(sd, f'{p}.{bn}') for bn in ('bnf', 'bnx', 'bny')]
            parts.append(np.stack([f[0] for f in folded]))
            parts.append(np.stack([f[1] for f in folded]))
        p = f'FusionBlock_{m}'
        parts.append(sd[p + '.conv.weight'].float()[:, :, 0, :].permute(2, 1, 0).contiguous().numpy())
        parts.extend(_fold_bn(sd, p + '.bn'))
    parts.append(sd['classifier.fc1.weight'].float().t().contiguous().numpy())
    parts.append(sd['classifier.fc1.bias'].float().numpy())
    parts.append(sd['classifier.fc2.weight'].float().numpy())
    parts.append(sd['classifier.fc2.bias'].float().numpy())
    return np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in parts]))


class DeviceWeights:
    """The packed network on the device (owned by the library until this object goes)."""

    def __init__(self, state_dict, device):
        lib = _lib.load()
        packed = pack_weights(state_dict)
        if packed.size != int(lib.st_aflink_packed_floats()):
            raise _lib.StError(f'AppearanceFreeLink: {packed.size} packed floats, the library expects '
                               f'{int(lib.st_aflink_packed_floats())}')
        self.handle, self._destroy = C.c_void_p(), lib.st_aflink_weights_destroy      # kept: __del__ may run at exit
        with torch.cuda.device(device):
            _lib.check(lib.st_aflink_weights_create(packed.ctypes.data_as(C.c_void_p), packed.size, C.byref(self.handle)),
                       'st_aflink_weights_create')

    def __del__(self):
        if getattr(self, 'handle', None):
            self._destroy(self.handle)
            self.handle = None


# ---------------------------------------------------------------------- steps 1-3 and 5-6 on the host
def build_tracks(rows):
    """rows -> dict(rows: the (N, 7) input in a stable sort by frame, ids: the track ids by (first frame, id), info: per
    track its (n, 3) fp64 rows (frame, c0, c1) in frame order) after the input checks."""
    try:
        rows = _as_rows(rows)
        by_id, starts, key = _sorted_tracks(rows)
    except ValueError as e:
        raise ValueError(str(e).replace('InterpolateTracklets', 'AppearanceFreeLink')) from None
    if not np.all(np.isfinite(rows[:, 2:4])):
        bad = int(np.argmax(~np.isfinite(rows[:, 2:4]).all(1)))
        raise ValueError(f'AppearanceFreeLink: id {rows[bad, 1]:g} has a non-finite corner at frame {rows[bad, 0]:g}')
    ends = list(starts[1:]) + [len(by_id)]
    tracks = [(by_id[a, 0], int(key[a]), by_id[a:b][:, [0, 2, 3]]) for a, b in zip(starts, ends)]
    tracks.sort(key=lambda t: (t[0], t[1]))
    return dict(rows=rows[np.argsort(rows[:, 0], kind='stable')] if len(rows) else rows,
                ids=np.array([t[1] for t in tracks], np.int64), info=[np.ascontiguousarray(t[2]) for t in tracks])


def gate(info, temporal_threshold=(0, 30), spatial_threshold=75):
    """(N, N) bool: the ordered pairs (i, j) that go to the network."""
    n = len(info)
    keep = np.zeros((n, n), bool)
    for i in range(n):
        last = info[i][-1]
        for j in range(n):
            if i == j:
                continue
            first = info[j][0]
            if not temporal_threshold[0] <= first[0] - last[0] <= temporal_threshold[1]:
                continue
            dx, dy = last[1] - first[1], last[2] - first[2]
            keep[i, j] = np.sqrt(dx ** 2 + dy ** 2) <= spatial_threshold
    return keep


def transform(info_i, info_j):
    """The two (30, 3) fp32 network inputs of the pair (earlier track i, later track j)."""
    a, b = info_i[-LENGTH:], info_j[:LENGTH]
    a = np.concatenate([np.zeros((LENGTH - len(a), 3)), a])
    b = np.concatenate([b, np.zeros((LENGTH - len(b), 3))])
    both = np.concatenate([a, b])
    lo, hi = both.min(axis=0), both.max(axis=0)
    sub, div = (hi + lo) / 2, (hi - lo) / 2 + 1e-5
    return ((a - sub) / div).astype(np.float32), ((b - sub) / div).astype(np.float32)


def link_from_scores(rows, pairs, conf, confidence_threshold=0.95):
    """Steps 5-6: rows (N, 7), pairs (K, 2) track indices (i, j) in the order of build_tracks, conf (K,) fp32 ->
    the linked rows (M, 7)."""
    from scipy.optimize import linear_sum_assignment
    t = rows if isinstance(rows, dict) else build_tracks(rows)
    out, ids = t['rows'].copy(), t['ids']
    n = len(ids)
    if n == 0:
        return np.zeros((0, 7))
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    conf = np.asarray(conf, np.float32).reshape(-1)
    cost = np.full((n, n), INFINITY)
    for (i, j), c in zip(pairs, conf):
        if float(c) >= confidence_threshold:                  # compared in fp64
            cost[i, j] = np.float64(np.float32(1) - c)
    first, final = {}, {}
    for i, j in zip(*linear_sum_assignment(cost)):
        if cost[i, j] < INFINITY:
            first[int(ids[i])] = int(ids[j])
    for k, v in first.items():                                # chain resolution, in insertion order
        final[v] = final[k] if k in final else k
    for k, v in final.items():                                # relabelling, in insertion order
        out[out[:, 1] == k, 1] = v
    _, keep = np.unique(out[:, :2], return_index=True, axis=0)     # the first of every (frame, id) in frame order
    return _finish(out[keep])


@TASK_UTILS.register_module(name=['AppearanceFreeLink', 'mmtrack.AppearanceFreeLink'])
class AppearanceFreeLink:
    """See the module docstring.  checkpoint: a local path, a state-dict mapping, or falsy for the initialised weights.
    forward(rows) -> (M, 7); forward_many(list of row arrays) -> list of (M, 7)."""

    def __init__(self, checkpoint, temporal_threshold=(0, 30), spatial_threshold=75, confidence_threshold=0.95,
                 backend='host'):
        _check_backend(backend)
        self.temporal_threshold = (temporal_threshold[0], temporal_threshold[1])
        self.spatial_threshold, self.confidence_threshold = spatial_threshold, confidence_threshold
        self.backend = backend
        self.model = AFLinkModel()
        if checkpoint:
            if isinstance(checkpoint, collections.abc.Mapping):
                self.model.load_state_dict(checkpoint)
            else:
                from .checkpoint import load_checkpoint
                report = load_checkpoint(self.model, checkpoint)['_load_report']
                if report['missing'] or report['mismatched']:
                    raise RuntimeError(f'AppearanceFreeLink: {checkpoint} does not hold the link network: missing '
                                       f'{report["missing"][:3]}, mismatched {report["mismatched"][:3]}')
        self.model.eval()
        self._device_weights = {}

    # ------------------------------------------------------------------ host: the executable specification
    def score_host(self, info, pairs):
        """conf (K,) fp32 of the pairs, one batch-1 forward each."""
        conf = np.zeros(len(pairs), np.float32)
        with torch.no_grad():
            for k, (i, j) in enumerate(pairs):
                a, b = transform(info[i], info[j])
                conf[k] = self.model(torch.from_numpy(a)[None, None], torch.from_numpy(b)[None, None])[0].numpy()
        return conf

    def _forward_host(self, rows):
        t = build_tracks(rows)
        pairs = np.argwhere(gate(t['info'], self.temporal_threshold, self.spatial_threshold))
        return link_from_scores(t, pairs, self.score_host(t['info'], pairs), self.confidence_threshold)

    def link_from_scores(self, rows, pairs, conf):
        return link_from_scores(rows, pairs, conf, self.confidence_threshold)

    def forward(self, pred_tracks):
        """(N, >= 7) fp64 rows (frame, id, c0, c1, c2, c3, score) -> (M, 7)."""
        if self.backend == 'device':
            return self.forward_many([pred_tracks])[0]
        return self._forward_host(pred_tracks)

    # ------------------------------------------------------------------ many videos / sweep members
    def forward_many(self, row_arrays, device=None, workspace_budget=None, timing=False):
        """forward() of every array of the list.  backend='device': ONE upload, the launches of one st_aflink_run, ONE
        wait and ONE copy back of (set, i, j, conf) for the whole list; the assignment and the relabelling then run on
        the host per set.  workspace_budget: bytes of transformed inputs one round of the network may hold (default
        WORKSPACE_BUDGET_BYTES); the result does not depend on it.  timing: returns (list, dict)."""
        row_arrays = list(row_arrays)
        if self.backend == 'host':
            t0 = time.perf_counter()
            out = [self._forward_host(r) for r in row_arrays]
            return (out, dict(total_s=time.perf_counter() - t0)) if timing else out
        return self._forward_many_device(row_arrays, device, workspace_budget, timing)

    def plan(self, row_arrays):
        """The host preparation of the device path: the tracks of all sets and the tables of include/stereotrack.h
        section 18.  capacity: the pairs that pass the temporal rule, an upper bound of the candidates that follows
        from the frame numbers alone."""
        tracks = [build_tracks(r) for r in row_arrays]
        info = [i for t in tracks for i in t['info']]
        n_trk = np.array([len(t['ids']) for t in tracks], np.int64)
        n_rows = np.array([len(i) for i in info], np.int64)
        lo, hi = self.temporal_threshold
        capacity = 0
        for t in tracks:
            if not t['info']:
                continue
            firsts = np.array([i[0, 0] for i in t['info']])              # ascending: the track order
            lasts = np.array([i[-1, 0] for i in t['info']])
            inside = np.searchsorted(firsts, lasts + hi, 'right') - np.searchsorted(firsts, lasts + lo, 'left')
            own = (lo <= firsts - lasts) & (firsts - lasts <= hi)
            capacity += int(np.maximum(inside, 0).sum() - own.sum())
        return dict(tracks=tracks, capacity=capacity, T=int(n_trk.sum()), R=int(n_rows.sum()),
                    feat=np.ascontiguousarray(np.concatenate(info)) if info else np.zeros((0, 3)),
                    trk_off=np.concatenate([[0], np.cumsum(n_rows)]).astype(np.int32),
                    trk_set=np.repeat(np.arange(len(tracks)), n_trk).astype(np.int32),
                    set_off=np.concatenate([[0], np.cumsum(n_trk)]).astype(np.int32))

    def device_weights(self, dev):
        key = (dev.type, dev.index)
        if key not in self._device_weights:
            self._device_weights[key] = DeviceWeights(self.model.state_dict(), dev)
        return self._device_weights[key]

    def _forward_many_device(self, row_arrays, device, budget, timing):
        call = PackedCall('AppearanceFreeLink', 'csrc/aflink.hip', device, timing, LAUNCHES)
        lib, dev = call.lib, call.dev
        budget = WORKSPACE_BUDGET_BYTES if budget is None else int(budget)
        p = self.plan(row_arrays)
        B, T, cap = len(row_arrays), p['T'], p['capacity']
        if cap > int(lib.st_aflink_max_candidates()) or 3 * p['R'] >= 2 ** 31:
            raise ValueError(f'AppearanceFreeLink: {cap} candidate pairs of {p["R"]} rows: the offset tables are 32-bit '
                             f'(at most {int(lib.st_aflink_max_candidates())} pairs per call)')
        chunk = min(max(cap, 1), budget // (2 * LENGTH * 3 * 4))
        if chunk < 1:
            raise ValueError(f'AppearanceFreeLink: one candidate needs {2 * LENGTH * 3 * 4} bytes of workspace, the '
                             f'budget is {budget}')
        if T == 0 or cap == 0:
            out = [link_from_scores(t, np.zeros((0, 2)), np.zeros(0), self.confidence_threshold) for t in p['tracks']]
            return (out, dict(stages_ms={}, candidates=0, host_prepare_s=time.perf_counter() - call.t_start)) if timing else out
        weights = self.device_weights(dev)

        call.upload({k: p[k] for k in ('feat', 'trk_off', 'trk_set', 'set_off')})
        call.outputs((('header', (2,), np.int32), ('cand', (cap, 3), np.int32), ('conf', (cap,), np.float32)))
        ws_off = torch.empty(T + 1, dtype=torch.int32, device=dev)
        ws_x = torch.empty(chunk * 2 * LENGTH * 3, dtype=torch.float32, device=dev)
        args = self._args(p, cap, chunk)
        call.bind(args)
        args.ws_off, args.ws_x = C.c_void_p(ws_off.data_ptr()), C.c_void_p(ws_x.data_ptr())
        with call.stages():
            call.launch('st_aflink_run', C.byref(args), weights.handle)
        host = call.fetch()
        header = host['header']
        if header[1] or header[0] > cap:
            raise _lib.StError(f'AppearanceFreeLink: the device reports status {int(header[1])} with {int(header[0])} '
                               f'candidates in {cap} slots: the host tables and the buffers disagree')
        n = int(header[0])
        cand, conf = host['cand'][:n], host['conf'][:n]
        set_off = np.searchsorted(cand[:, 0], np.arange(B + 1))
        out = [link_from_scores(p['tracks'][s], cand[set_off[s]:set_off[s + 1], 1:], conf[set_off[s]:set_off[s + 1]],
                                self.confidence_threshold) for s in range(B)]
        if timing:
            return out, call.timing_dict(candidates=n, capacity=cap, rounds=-(-cap // chunk), tracks=T, rows_in=p['R'])
        return out

    def _args(self, p, capacity, chunk):
        args = _lib.StAflinkArgs()
        args.struct_size = C.sizeof(_lib.StAflinkArgs)
        args.num_sets, args.num_tracks, args.num_rows = len(p['tracks']), p['T'], p['R']
        args.capacity, args.first, args.count, args.chunk = capacity, 0, 0, chunk
        args.t_lo, args.t_hi = float(self.temporal_threshold[0]), float(self.temporal_threshold[1])
        args.spatial_thr = float(self.spatial_threshold)
        return args

    # ------------------------------------------------------------------ the device stages one by one (tests, tools)
    def device_stages(self, row_arrays, x=None, device=None, poison=None, want=('gate', 'transform', 'score')):
        """Runs the stage entries one by one, with a wait after each, and returns what each wrote: dict(cand (K, 3),
        x (K, 2, 30, 3) fp32, conf (K,), logits (K, 2), stage_ms).  x: score these inputs instead (row_arrays is then
        ignored).  poison: a byte every output and workspace buffer is filled with before the first launch."""
        lib = _lib.load()
        dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        weights = self.device_weights(dev)
        res, ms = {}, {}

        def buf(n, dtype):
            t = torch.empty(max(int(n), 1), dtype=dtype, device=dev)
            if poison is not None:
                t.view(torch.uint8).fill_(poison)
            return t

        def timed(name, call):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            LAUNCHES[name] += 1
            _lib.check(call(), name)
            ev[1].record()
            torch.cuda.synchronize(dev)
            ms[name] = ev[0].elapsed_time(ev[1])

        with torch.cuda.device(dev):
            stream = _lib.current_stream()
            if x is None:
                p = self.plan(row_arrays)
                cap = p['capacity']
                args = self._args(p, cap, max(cap, 1))
                keep = {k: torch.from_numpy(np.ascontiguousarray(p[k])).to(dev) for k in ('feat', 'trk_off', 'trk_set', 'set_off')}
                for k, v in keep.items():
                    setattr(args, k, C.c_void_p(v.data_ptr()))
                header, cand, ws_off = buf(2, torch.int32), buf(cap * 3, torch.int32), buf(p['T'] + 1, torch.int32)
                args.header, args.cand, args.ws_off = (C.c_void_p(t.data_ptr()) for t in (header, cand, ws_off))
                timed('st_aflink_gate', lambda: lib.st_aflink_gate(C.byref(args), stream))
                h = header.cpu().numpy()
                if h[1] or h[0] > cap:
                    raise _lib.StError(f'AppearanceFreeLink: gate status {int(h[1])}, {int(h[0])} candidates in {cap} slots')
                n = int(h[0])
                res['cand'] = cand.cpu().numpy()[:n * 3].reshape(n, 3)
                if 'transform' not in want:
                    return dict(res, stage_ms=ms)
                xbuf = buf(cap * 2 * LENGTH * 3, torch.float32)
                args.ws_x, args.first, args.count = C.c_void_p(xbuf.data_ptr()), 0, cap
                timed('st_aflink_transform', lambda: lib.st_aflink_transform(C.byref(args), stream))
                res['x'] = xbuf.cpu().numpy()[:n * 2 * LENGTH * 3].reshape(n, 2, LENGTH, 3)
                if 'score' not in want:
                    return dict(res, stage_ms=ms)
            else:
                x = np.ascontiguousarray(x, np.float32).reshape(-1, 2, LENGTH, 3)
                n = cap = len(x)
                args = self._args(dict(tracks=[], T=0, R=0), cap, max(cap, 1))
                header = torch.tensor([n, 0], dtype=torch.int32, device=dev)
                xbuf = torch.from_numpy(x).to(dev) if n else buf(1, torch.float32)
                args.header, args.ws_x, args.count = C.c_void_p(header.data_ptr()), C.c_void_p(xbuf.data_ptr()), cap
            conf, logits = buf(cap, torch.float32), buf(cap * 2, torch.float32)
            args.conf, args.logits = C.c_void_p(conf.data_ptr()), C.c_void_p(logits.data_ptr())
            timed('st_aflink_score', lambda: lib.st_aflink_score(C.byref(args), weights.handle, stream))
            res['conf'] = conf.cpu().numpy()[:n]
            res['logits'] = logits.cpu().numpy()[:n * 2].reshape(n, 2)
        return dict(res, stage_ms=ms)
