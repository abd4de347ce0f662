"""CPU: the restatement of the default per-box depth estimator (tests/depth_methods_ref.py, DEFAULT = 'reference') and
the inputs of tests/box_depth_cases.py, before any GPU run:
  * the restatement agrees with oracle/depth.py, the line-by-line restatement of the reference, on every builder's inputs
    (this links two references; it does not test the kernel);
  * the inputs reach every branch (coverage facts, asserted from the restatement's trace);
  * the inputs can see each plausible error: every mutant of the restatement changes at least one box by more than 1 ulp
    or flips a -1 / NaN decision."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import box_depth_cases as B
import depth_methods_ref as R
from oracle import depth as odepth

F = np.float32


def all_cases():
    return [c for b in B.BUILDERS for c in B.cases(b)]


def all_rows():
    """(case, image, box index, value, scale, trace) of every evaluated box."""
    for case in all_cases():
        for n, (vals, scales, traces) in enumerate(B.reference(case)):
            for k, t in enumerate(traces):
                yield case, n, k, vals[k], scales[k], t


# ---- known answers ----------------------------------------------------------------------------------------------------
def test_known_answers():
    d = np.zeros((8, 12), F)
    d[2, 2:12] = np.arange(1, 11)                               # one row, n = 10, corner rows 1 and 3 are 0
    v, ok, t = R.value(d, [2, 2, 12, 3], R.DEFAULT, trace=True)
    # mid = s[5] = 6; corner means (1 + 2) / 4 and (9 + 10) / 4: cnt = 0 -> s[4:10] = 5..10
    assert ok and (t.cnt, t.n, t.a, t.b, t.fallback) == (0, 10, 4, 10, False) and v == F(7.5)
    d[1, 2:4] = 1000.0                                          # top-left mean > mid: cnt = 1, same fraction
    d[3, 10:12] = 1000.0
    d[1, 10:12] = 1000.0                                        # cnt = 3 -> fraction 0.25: s[2:8] = 3..8
    v, ok, t = R.value(d, [2, 2, 12, 3], R.DEFAULT, trace=True)
    assert (t.cnt, t.a, t.b) == (3, 2, 8) and v == F(5.5)
    d[3, 2:4] = 1000.0                                          # cnt = 4 -> fraction 0: s[0:6] = 1..6
    v, ok, t = R.value(d, [2, 2, 12, 3], R.DEFAULT, trace=True)
    assert (t.cnt, t.a, t.b) == (4, 0, 6) and v == F(3.5)
    one = np.zeros((6, 6), F)
    one[2, 2] = 30.0
    one[1, 2], one[3, 2] = 1000.0, 1000.0                       # n = 1, every corner mean > 30: s[0:0], s[:-1] empty
    v, ok, t = R.value(one, [2, 2, 3, 3], R.DEFAULT, trace=True)
    assert ok and np.isnan(v) and t.fallback and t.cnt == 4 and np.isnan(R.scale_of_default(v))
    vals, scales = R.extract_depth(one, [[2, 2, 3, 3], [4, 4, 6, 6]], R.DEFAULT)     # the second window is all 0
    assert np.isnan(vals[0]) and np.isnan(scales[0]) and (vals[1], scales[1]) == (F(-1.0), F(1.0))


def test_scale_of_default():
    assert R.scale_of_default(0.5) == F(1.0) and R.scale_of_default(1.0) == F(1.0)
    assert R.scale_of_default(F(1.5)) == F(2.25)
    d = F(1.7320508)
    assert R.scale_of_default(d) == min(F(d * d), F(3.0))
    assert R.scale_of_default(2.0) == F(3.0) and R.scale_of_default(1e30) == F(3.0)
    assert np.isnan(R.scale_of_default(np.nan))
    assert R.scale_of_default(-1.5) == F(2.25)                  # the scale of a value, whatever its sign


def test_corner_mean_is_numpy_mean_of_the_view():
    rng = np.random.RandomState(0)
    d = rng.uniform(0.0, 200.0, (40, 40)).astype(F)
    differ = 0
    for _ in range(2000):
        y, x = rng.randint(0, 39, 2)
        blk = d[y:y + 2, x:x + 2]
        assert R.corner_mean(blk) == np.mean(blk)
        a, b, c, e = blk.ravel()
        differ += F(F(F(a + b) + F(c + e)) / F(4)) != R.corner_mean(blk)
    assert differ > 0, 'the pairwise order never differs: the rule would not matter'
    assert np.isnan(R.corner_mean(d[3:3, 0:2])) and R.corner_mean(d[39:41, 0:2]) == F(F(d[39, 0] + d[39, 1]) / F(2))


def test_segment_bounds_do_not_depend_on_contraction():
    """int(w_start + 0.6 * n) with the product and the sum rounded separately equals the fused multiply-add's integer
    (one rounding of the exact w_start + 0.6 * n): every n < 30 000 and every 13th n from there to 200 000 (every n
    below 200 000 was checked once, when the rule was written down)."""
    c = Fraction(0.6)
    for frac in (0.4, 0.25, 0.0):
        for n in list(range(1, 30000)) + list(range(30000, 200000, 13)):
            w_start = frac * n
            fused = float(Fraction(w_start) + c * n)            # float(Fraction) rounds to nearest even, once
            assert int(w_start + 0.6 * n) == int(fused), (frac, n)


# ---- the two references agree ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('builder', B.BUILDERS)
def test_restatement_agrees_with_the_line_by_line_oracle(builder):
    checked = 0
    for case in B.cases(builder):
        for dmap, boxes, (vals, scales, traces) in zip(B.depth_maps(case), case.boxes, B.reference(case)):
            k = len(vals)
            ov, os_ = odepth.extract_depth(torch.from_numpy(dmap.copy()), torch.from_numpy(boxes[:k].copy()))
            ov, os_ = np.asarray([float(v) for v in ov], F), np.asarray([float(s) for s in os_], F)
            assert np.array_equal(ov == -1, vals == -1), f'{case.name}: -1 decisions'
            assert np.array_equal(np.isnan(ov), np.isnan(vals)), f'{case.name}: NaN decisions'
            for i, t in enumerate(traces):
                if t.cnt is None or np.isnan(vals[i]):
                    assert os_[i] == scales[i] or (np.isnan(os_[i]) and np.isnan(scales[i]))
                    continue
                # np.mean sums float32 pairwise: within (b - a) * 2**-24 * |ref| of the exact sum, whatever the order
                bound = (t.b - t.a) * 2.0 ** -24 * abs(float(ov[i])) + float(np.spacing(abs(ov[i])))
                assert abs(float(vals[i]) - float(ov[i])) <= bound, (case.name, i, vals[i], ov[i], t[:5])
                if vals[i] == ov[i]:
                    assert scales[i] == os_[i], (case.name, i)
                checked += 1
    assert checked > 0


# ---- the inputs reach every branch ----------------------------------------------------------------------------------
def test_coverage_facts():
    rows = list(all_rows())
    est = [(v, s, t) for _, _, _, v, s, t in rows if t.cnt is not None]
    assert {t.cnt for _, _, t in est} == {0, 1, 2, 3, 4}
    assert any(t.fallback for _, _, t in est), 'the s[:-1] fallback'
    assert any(np.isnan(v) and np.isnan(s) for v, s, _ in est), 'the NaN result'
    gone = [t for _, _, _, v, _, t in rows if t.cnt is None]
    assert all(v == -1 and s == 1 for _, _, _, v, s, t in rows if t.cnt is None)
    assert any(t.window == 0 for t in gone), '-1 by an empty window'
    assert any(t.window > 0 and t.n == 0 and t.width <= R.MAX_WIDTH for t in gone), '-1 by an all-invalid window'
    assert any(t.n > 0 and t.width > R.MAX_WIDTH for t in gone), '-1 by w > 800 alone'
    assert any(t.n > 0 and t.width == R.MAX_WIDTH for _, _, t in est), 'w == 800 is kept'
    # ties: a run of equal sorted depths that the slice [a, b) cuts
    cut_a = [t for _, _, t in est if 0 < t.a < t.b and t.s[t.a - 1] == t.s[t.a]]
    cut_b = [t for _, _, t in est if t.a < t.b < t.n and t.s[t.b - 1] == t.s[t.b]]
    assert cut_a and cut_b, 'ties across a, ties across b - 1'
    assert any(0 < t.a < t.b < t.n and t.s[t.a - 1] == t.s[t.b] for _, _, t in est), 'one run across both bounds'
    assert any(t.a < t.b and t.s[t.a] != t.s[t.b - 1] for t in cut_a) and \
        any(t.a < t.b and t.s[t.a] != t.s[t.b - 1] for t in cut_b), 'cut runs with two different bound values'
    assert any(t.n > 1 and t.s[0] == t.s[-1] for _, _, t in est), 'a constant window: all 7 ranks select one value'
    scales = np.asarray([s for _, s, _ in est], F)
    assert ((scales > 1) & (scales < 3)).any() and (scales == 1).any() and (scales == 3).any()
    windows = [t.window for _, _, t in est]
    assert any(0 < w < B.BD_CACHE for w in windows) and any(w == B.BD_CACHE - 1 for w in windows)
    assert any(w == B.BD_CACHE for w in windows) and any(w == B.BD_CACHE + 1 for w in windows)
    assert any(w > 2 * B.BD_CACHE for w in windows)


def test_branch_grid_forces_cnt_and_sweeps_n():
    case, = B.branch_grid()
    (vals, _, traces), = B.reference(case)
    assert [(t.n, t.cnt) for t in traces] == [(n, k) for n in B.GRID_N for k in range(5)]
    assert all(len(np.unique(t.s)) == t.n and t.s[0] > 1 and t.s[-1] < 140 for t in traces)
    assert [i for i, v in enumerate(vals) if np.isnan(v)] == [3, 4]         # n = 1 with cnt 3 and 4
    for frac, k in ((0.4, 0), (0.25, 3), (0.0, 4)):
        assert all((t.a, t.b) == (int(frac * t.n), int(frac * t.n + 0.6 * t.n)) for t in traces
                   if t.cnt == k and not t.fallback)


def test_geometry_counts_clamp_and_streamed_column_counts():
    for case in B.geometry():
        M = case.boxes.shape[1]
        assert case.counts[0] < M < case.counts[1]
        assert [len(r[0]) for r in B.reference(case)] == [case.counts[0], M]
    wide = B.geometry()[0]
    streamed = {}
    for box, t in zip(wide.boxes[1], B.reference(wide)[1][2]):
        if t.window > B.BD_CACHE and t.cnt is not None:
            cols = int(box[2]) - int(box[0])
            streamed.setdefault(cols, set()).add((t.window // cols) % 4)
    for cols in (63, 64, 65, 255, 256, 257, 513, 800):
        assert {1, 2, 3} <= streamed[cols], cols                  # the last group of 4 rows holds 1, 2 and 3 rows
    tall = B.geometry()[1]
    assert {2561, 2562, 2563} <= {t.window for box, t in zip(tall.boxes[1], B.reference(tall)[1][2])
                                  if int(box[2]) - int(box[0]) == 1}
    assert {c.maps.shape[1] for c in B.geometry()} == {1, 3}


# ---- the inputs can see each error ----------------------------------------------------------------------------------
MUTANTS = ('segment_shifted', 'segment_end_short', 'median_lower', 'corner_ge', 'cnt3_as_2', 'cnt4_as_3',
           'all_ties_taken', 'valid_le_150', 'valid_ge_0', 'corner_valid_only', 'corner_pairwise', 'no_wrap')


def _default(depth, box, mutant=None):
    """The default estimator once more, with one rule broken on request -> float32 value (-1: not estimated)."""
    x1, y1, x2, y2 = (int(c) for c in np.asarray(box, F))
    sl = slice
    if mutant == 'no_wrap':                                     # negative bounds clamp to 0 instead of wrapping
        def sl(lo, hi):
            return slice(max(lo, 0), max(hi, 0))
    win = depth[sl(y1, y2), sl(x1, x2)]
    with np.errstate(invalid='ignore'):
        ok = ((win <= 150) if mutant == 'valid_le_150' else (win < 150)) & \
             ((win >= 0) if mutant == 'valid_ge_0' else (win > 0))
    s = np.sort(win[ok])
    n = len(s)
    if n < 1 or (x2 - x1) > 800:
        return F(-1.0)
    mid = s[(n - 1) // 2] if mutant == 'median_lower' else s[n // 2]

    def cmean(rows, cols):
        blk = depth[rows, cols]
        if mutant == 'corner_valid_only':
            blk = blk[(blk < 150) & (blk > 0)]
        if mutant == 'corner_pairwise' and blk.size == 4:
            a, b, c, d = blk.ravel()
            with np.errstate(over='ignore', invalid='ignore'):
                return F(F(F(a + b) + F(c + d)) / F(4))
        return R.corner_mean(blk)
    corners = [cmean(sl(y1, y1 + 2), sl(x1, x1 + 2)), cmean(sl(y1, y1 + 2), sl(x2 - 2, x2)),
               cmean(sl(y2 - 2, y2), sl(x1, x1 + 2)), cmean(sl(y2 - 2, y2), sl(x2 - 2, x2))]
    cnt = sum(bool(c >= mid) if mutant == 'corner_ge' else bool(c > mid) for c in corners)
    if (mutant, cnt) in (('cnt3_as_2', 3), ('cnt4_as_3', 4)):
        cnt -= 1
    w_start = min(1 - cnt / 4, 0.4) * n
    w_end = w_start + 0.6 * n
    a, b = int(w_start), int(w_end)
    if mutant == 'segment_shifted':
        a, b = a + 1, b + 1
    if mutant == 'segment_end_short':
        b -= 1
    seg = s[a:b]
    if mutant == 'all_ties_taken' and len(seg):
        seg = s[(s >= seg[0]) & (s <= seg[-1])]
    if len(seg) == 0:
        seg = s[:-1]
    if len(seg) == 0:
        return F(np.nan)
    return F(np.sum(seg, dtype=np.float64) / len(seg))


def _differs(got, ref):
    """A flipped -1 / NaN decision, or more than 1 ulp."""
    if np.isnan(got) or np.isnan(ref):
        return bool(np.isnan(got) != np.isnan(ref))
    if got == -1 or ref == -1:
        return bool(got != ref)
    return bool(abs(float(got) - float(ref)) > float(np.spacing(abs(ref))))


def test_the_helper_without_a_mutant_is_the_restatement():
    for case in all_cases():
        for dmap, boxes, (vals, _, _) in zip(B.depth_maps(case), case.boxes, B.reference(case)):
            got = np.asarray([_default(dmap, box) for box in boxes[:len(vals)]], F)
            assert got.tobytes() == vals.tobytes() or np.array_equal(got, vals, equal_nan=True), case.name


@pytest.mark.parametrize('mutant', MUTANTS)
def test_inputs_see_the_mutant(mutant):
    seen = []
    for case in all_cases():
        for n, (dmap, boxes, (vals, _, traces)) in enumerate(zip(B.depth_maps(case), case.boxes, B.reference(case))):
            for k, ref in enumerate(vals):
                if _differs(_default(dmap, boxes[k], mutant), ref):
                    seen.append((case.name, n, k))
    print(f'{mutant}: {len(seen)} boxes differ, first {seen[:3]}')
    assert seen, f'no box of any builder notices {mutant}'


# ---- the GPU file's comparison itself -------------------------------------------------------------------------------
def test_the_gpu_comparison_accepts_the_restatement_and_rejects_small_errors():
    """assert_case of tests/test_box_depth_default_gpu.py on made-up kernel outputs: the restatement's own rows pass
    with distance 0; 1 ulp passes; 2 ulps, a wrong scale, a stale row past the count and a flipped decision do not."""
    from test_box_depth_default_gpu import assert_case
    case = B.geometry()[2]
    N, M = case.boxes.shape[:2]

    def outputs():
        d, s, b = np.zeros((N, M), F), np.zeros((N, M), F), np.zeros((N, M, 4), F)
        for n, (vals, scales, _) in enumerate(B.reference(case)):
            k = len(vals)
            d[n, :k], s[n, :k], b[n, :k] = vals, scales, R.scale_bbox(case.boxes[n, :k], scales)
        return d, s, b
    assert assert_case(case, outputs()) == 0.0
    vals = B.reference(case)[0][0]
    i = int(np.flatnonzero(np.isfinite(vals) & (vals > 2))[0])     # scale 3 on both sides: only the depth moves
    d, s, b = outputs()
    d[0, i] = np.nextafter(vals[i], F(np.inf))
    assert assert_case(case, (d, s, b)) == 1.0
    d[0, i] = np.nextafter(d[0, i], F(np.inf))
    with pytest.raises(AssertionError, match='beyond 1 ulp'):
        assert_case(case, (d, s, b))
    d, s, b = outputs()
    s[0, i] = np.nextafter(s[0, i], F(0))
    with pytest.raises(AssertionError, match='scale'):
        assert_case(case, (d, s, b))
    d, s, b = outputs()
    assert case.counts[0] < M
    b[0, M - 1, 2] = 7.0
    with pytest.raises(AssertionError, match='rows past'):
        assert_case(case, (d, s, b))
    d, s, b = outputs()
    j = int(np.flatnonzero(vals == -1)[0])
    d[0, j] = np.nan
    with pytest.raises(AssertionError, match='decisions'):
        assert_case(case, (d, s, b))
