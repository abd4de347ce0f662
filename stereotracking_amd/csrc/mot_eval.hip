// MOT evaluation (CLEAR, Identity, HOTA of stereotracking_amd/metrics.py, the executable specification) on the device,
// behind st_mot_similarity / st_mot_walk / st_mot_hota_match / st_mot_hota_accumulate (include/stereotrack.h section 15,
// DESIGN.md section 15).
//
// Everything that decides a result is fp64 or an integer count.  There is no floating-point atomic: every fp64 sum is
// taken in a fixed order, so two runs give the same bits.  The launch count is fixed and nothing waits for the device.
//
//   similarity       k_similarity   one wave per (sequence, frame): input checks, the frame's G x P IoU matrix with the
//                                   operation order of box_iou_xywh, its row sums (numpy's pairwise order) and column sums
//   walk             k_potential    one workgroup per sequence, frames in order, the threads cover a frame's pairs: id counts,
//                                   HOTA's potential (fp64, += per frame) and Identity's potential (int)
//                    k_walk         one wave per sequence, frames in order: CLEAR's matching with the previous-frame state
//   hota_match       k_hota_match   one wave per (sequence, frame): align * IoU, one assignment, the matched column of every row
//   hota_accumulate  k_hota_acc     one workgroup per (sequence, alpha): TP / FN / FP, the IoU sum, the integer matches
//                                   matrix (integer atomics) and the AssA / AssRe / AssPr sums
//
//   kitti_preprocess k_kitti        one wave per (frame, class): KITTI's 2-D box preprocessing behind st_mot_kitti_preprocess
//                                   (section 16): class split by ballots, thresholded IoU, one assignment, the keep bytes
//
//   file_round       k_file_round   elementwise: what a reader of the MOTChallenge text files gets ('%d' / '%.3f' per column),
//                                   behind st_mot_file_round (section 21)
//   challenge_prep.  k_challenge    one wave per frame: TrackEval's MOTChallenge preprocessing behind
//                                   st_mot_challenge_preprocess (section 21): IoU thresholded at 0.5, one assignment, keep bytes
//
// One solver serves k_walk, k_hota_match, k_kitti and k_challenge: solve_assignment, the shortest-augmenting-path (Jonker-Volgenant /
// Hungarian) method for one wave, exact on a rectangular matrix of non-negative fp64 weights.
#include <climits>
#include <cmath>

#include "st_common.h"

namespace {

constexpr int kMaxObj = ST_MOT_MAX_OBJECTS;   // rows of either kind in one frame
constexpr int kMaxAlphas = ST_MOT_MAX_ALPHAS;
constexpr int kAccThreads = 256;
constexpr int kPotThreads = 256;
constexpr int kLdsCells = 4096;                  // a weight matrix of up to 64 x 64 cells is solved out of LDS, larger ones out of the workspace
constexpr double kEps = 2.220446049250313e-16;   // np.finfo(float).eps = 2^-52

enum : int {
  kNonFinite = 1,    // a box coordinate that is NaN / Inf
  kDupId = 2,        // an id twice in one frame
  kUnsorted = 4,     // a row outside its frame, or frame numbers that do not ascend
  kFrameLimit = 8,   // more than kMaxObj rows of one kind in a frame
  kBadId = 16,       // a dense id outside [0, ng) / [0, nt)
};

typedef long long i64;

struct Workspace {
  double *sim, *base, *weight, *rowsum, *colsum, *match_sim;
  int *prev_tracker, *prev_step, *cur_step, *match_tid, *matches;
  size_t sim_offset, total;
};

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

void carve(const StMotArgs* a, void* base, Workspace* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? (char*)base + off : nullptr; off += align256(bytes); return (void*)p; };
  const size_t NP = (size_t)a->num_pairs, NG = (size_t)a->num_gt, NR = (size_t)a->num_pred, IDS = (size_t)a->num_gids;
  w->sim_offset = off;
  w->sim = (double*)take((NP + 1) * sizeof(double));
  w->base = (double*)take((NP + 1) * sizeof(double));     // CLEAR's score without the bonus: written once, only read after
  w->weight = (double*)take((NP + 1) * sizeof(double));   // the solver's matrix of a frame too large for LDS
  w->rowsum = (double*)take((NG + 1) * sizeof(double));
  w->colsum = (double*)take((NR + 1) * sizeof(double));
  w->match_sim = (double*)take((NG + 1) * sizeof(double));
  w->match_tid = (int*)take((NG + 1) * sizeof(int));
  w->prev_tracker = (int*)take((IDS + 1) * sizeof(int));
  w->prev_step = (int*)take((IDS + 1) * sizeof(int));
  w->cur_step = (int*)take((IDS + 1) * sizeof(int));
  w->matches = (int*)take(((size_t)a->num_cells * (size_t)a->num_alphas + 1) * sizeof(int));
  w->total = off;
}

__device__ inline void report(int* status, int bit, int kind, int value) {
  atomicOr(&status[0], bit);
  atomicMax(&status[1 + kind], value);
}

// ---- numpy's summation orders -------------------------------------------------------------------------------------
// np.add.reduce over a contiguous axis: pairwise summation, blocks of at most 128 elements on 8 accumulators.
__device__ inline double np_block_sum(const double* __restrict__ a, int n) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
  int i = 8;
  const int lim = n - (n % 8);
  for (; i < lim; i += 8) {
    r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
    r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) res += a[i];
  return res;
}

template <int DEPTH>
__device__ inline double np_pairwise_sum(const double* __restrict__ a, int n) {
  if (n <= 128) return np_block_sum(a, n);
  int n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise_sum<DEPTH - 1>(a, n2) + np_pairwise_sum<DEPTH - 1>(a + n2, n - n2);
}
template <>
__device__ inline double np_pairwise_sum<0>(const double* __restrict__ a, int n) { return np_block_sum(a, n); }
static_assert(kMaxObj <= 512, "np_pairwise_sum<2> splits at most twice: 512 elements");

// ---- checks, IoU, row and column sums ----------------------------------------------------------------------------
__device__ inline bool check_rows(const double* __restrict__ rows, int s, int e, double frame, int nid, int lane,
                                  int* status, int report_value) {
  bool bad = false;
  for (int r = s + lane; r < e; r += 64) {
    const double* row = rows + 6 * (size_t)r;
    bool fin = true;
    for (int c = 2; c < 6; ++c) fin = fin && isfinite(row[c]);
    if (!fin) { report(status, kNonFinite, 0, report_value); bad = true; }
    if (!(row[0] == frame)) { report(status, kUnsorted, 2, report_value); bad = true; }
    const double idv = row[1];
    if (!(idv >= 0.0 && idv < (double)nid && idv == floor(idv))) {
      report(status, kBadId, 4, report_value);
      bad = true;
      continue;
    }
    for (int q = s; q < r; ++q)
      if (rows[6 * (size_t)q + 1] == idv) { report(status, kDupId, 1, report_value); bad = true; break; }
  }
  return bad;
}

__global__ __launch_bounds__(64) void k_similarity(StMotArgs a, Workspace w) {
  const int f = blockIdx.x, lane = threadIdx.x;
  const int gs = a.frame_gt_off[f], G = a.frame_gt_off[f + 1] - gs;
  const int ps = a.frame_pred_off[f], P = a.frame_pred_off[f + 1] - ps;
  const int seq = a.frame_seq[f];
  const int rep = a.num_frames - f;
  if (lane == 0 && f > a.seq_frame_off[seq] && a.frame_no[f - 1] >= a.frame_no[f]) report(a.status, kUnsorted, 2, rep);
  if (G > kMaxObj || P > kMaxObj || G < 0 || P < 0) {
    if (lane == 0) report(a.status, kFrameLimit, 3, rep);
    return;
  }
  const double frame = (double)a.frame_no[f];
  bool bad = check_rows(a.gt_rows, gs, gs + G, frame, a.seq_ng[seq], lane, a.status, rep);
  bad = check_rows(a.pred_rows, ps, ps + P, frame, a.seq_nt[seq], lane, a.status, rep) || bad;
  if (__any(bad)) return;
  double* __restrict__ sim = w.sim + a.frame_pair_off[f];
  double* __restrict__ base = w.base + a.frame_pair_off[f];   // CLEAR's score without the continuity bonus
  const double thr = a.iou_thr - kEps;
  const int cells = G * P;
  for (int c = lane; c < cells; c += 64) {
    const int i = c / P, j = c - i * P;
    const double* g = a.gt_rows + 6 * (size_t)(gs + i) + 2;
    const double* p = a.pred_rows + 6 * (size_t)(ps + j) + 2;
    const double ax2 = g[0] + g[2], ay2 = g[1] + g[3], bx2 = p[0] + p[2], by2 = p[1] + p[3];
    double iw = fmin(ax2, bx2) - fmax(g[0], p[0]);
    double ih = fmin(ay2, by2) - fmax(g[1], p[1]);
    iw = iw < 0.0 ? 0.0 : iw;
    ih = ih < 0.0 ? 0.0 : ih;
    const double inter = iw * ih;
    const double uni = (g[2] * g[3] + p[2] * p[3]) - inter;
    const double sv = uni > 0.0 ? inter / fmax(uni, 1e-12) : 0.0;
    sim[c] = sv;
    base[c] = sv < thr ? 0.0 : sv;
  }
  __syncthreads();
  // sim.sum(1): pairwise along the contiguous axis.  sim.sum(0): row after row, except that a G x 1 matrix is
  // contiguous along the reduced axis and numpy sums it pairwise as well.
  for (int i = lane; i < G; i += 64) w.rowsum[gs + i] = np_pairwise_sum<2>(sim + (size_t)i * P, P);
  for (int j = lane; j < P; j += 64) {
    double r;
    if (P == 1) {
      r = np_pairwise_sum<2>(sim, G);
    } else {
      r = 0.0;
      for (int i = 0; i < G; ++i) r += sim[(size_t)i * P + j];
    }
    w.colsum[ps + j] = r;
  }
}

// ---- the assignment solver -----------------------------------------------------------------------------------------
struct SolverLds {
  double u[kMaxObj + 1], v[kMaxObj + 1], minv[kMaxObj + 1];   // duals of the rows / columns, shortest distances
  int p[kMaxObj + 1], way[kMaxObj + 1], used[kMaxObj + 1];   // row of a column (-1 free), predecessor column, visited
  int mcol[kMaxObj];                                          // result: prediction of every ground-truth row, or -1
  int gid[kMaxObj], tid[kMaxObj];                             // dense ids of the frame's rows (the callers' use)
};

// Before the search, the bound that settles most frames of a tracker's output: an assignment cannot exceed the sum of
// the row maxima (nor that of the column maxima); where the positive row maxima (or column maxima) sit in pairwise
// distinct columns (rows), taking them attains the bound and is the optimum.  Rows without a positive weight stay
// unmatched: a pair of weight zero is dropped by every rule that reads the result.
__device__ bool maxima_are_an_assignment(const double* W, int G, int P, SolverLds& s, int lane) {
  for (int j = lane; j < P; j += 64) s.p[j] = -1;       // row that took column j
  for (int i = lane; i < G; i += 64) { s.way[i] = -1; s.mcol[i] = -1; }   // column that took row i
  __syncthreads();
  bool ok = true;
  for (int i = lane; i < G; i += 64) {
    double best = 0.0;
    int bj = -1;
    for (int k = 0; k < P; ++k) {
      int j = k + i;                 // rotated start: the lanes of a wave read different LDS banks
      j = j >= P ? j % P : j;
      const double wv = W[(size_t)i * P + j];
      if (wv > best || (wv == best && bj >= 0 && j < bj)) { best = wv; bj = j; }
    }
    s.mcol[i] = bj;
    if (bj >= 0 && atomicCAS(&s.p[bj], -1, i) != -1) ok = false;
  }
  if (__all(ok)) { __syncthreads(); return true; }
  __syncthreads();
  ok = true;
  for (int j = lane; j < P; j += 64) {
    double best = 0.0;
    int bi = -1;
    for (int i = 0; i < G; ++i) {
      const double wv = W[(size_t)i * P + j];
      if (wv > best) { best = wv; bi = i; }
    }
    s.p[j] = bi;
    if (bi >= 0 && atomicCAS(&s.way[bi], -1, j) != -1) ok = false;
  }
  __syncthreads();
  if (!__all(ok)) return false;
  for (int i = lane; i < G; i += 64) s.mcol[i] = s.way[i];
  __syncthreads();
  return true;
}

// Exact maximum-sum assignment of the G x P matrix W (row-major, weights >= 0) by ONE wave of a 64-thread workgroup:
// min(G, P) pairs, as scipy.optimize.linear_sum_assignment(-W) returns them; s.mcol[i] = the column of row i or -1.
// Shortest augmenting paths with dual variables on costs -W: the columns go across the lanes, one row is added per
// outer step, every inner step takes one more column into the tree, so the work is bounded by n * (m + 1) steps.
// The shorter side plays the rows (n <= m), by strides; column m is the virtual root of the path.
__device__ void solve_assignment(const double* W, int G, int P, SolverLds& s, int lane) {
  if (maxima_are_an_assignment(W, G, P, s, lane)) return;
  const bool tr = G > P;
  const int n = tr ? P : G, m = tr ? G : P;
  const size_t rs = tr ? 1 : (size_t)P, cs = tr ? (size_t)P : 1;
  for (int j = lane; j <= m; j += 64) { s.v[j] = 0.0; s.p[j] = -1; }
  for (int i = lane; i < n; i += 64) s.u[i] = 0.0;
  for (int g = lane; g < G; g += 64) s.mcol[g] = -1;
  __syncthreads();
  for (int i = 0; i < n; ++i) {
    for (int j = lane; j <= m; j += 64) { s.minv[j] = INFINITY; s.used[j] = 0; }
    if (lane == 0) s.p[m] = i;
    __syncthreads();
    int j0 = m;
    bool found = false;
    for (int it = 0; it <= m; ++it) {
      const int i0 = s.p[j0];
      const double ui = s.u[i0];
      if (lane == 0) s.used[j0] = 1;
      __syncthreads();
      double best = INFINITY;
      int bj = INT_MAX;
      for (int j = lane; j < m; j += 64) {
        if (s.used[j]) continue;
        const double cur = (-W[i0 * rs + j * cs] - ui) - s.v[j];
        double mv = s.minv[j];
        if (cur < mv) { mv = cur; s.minv[j] = cur; s.way[j] = j0; }
        if (mv < best) { best = mv; bj = j; }
      }
      for (int o = 32; o > 0; o >>= 1) {   // the smallest distance; the lowest column on equal distances
        const double ob = __shfl_xor(best, o);
        const int oj = __shfl_xor(bj, o);
        if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
      }
      if (bj == INT_MAX) break;   // only non-finite weights get here, and those inputs are refused by the status word
      for (int j = lane; j <= m; j += 64) {
        if (s.used[j]) { s.u[s.p[j]] += best; s.v[j] -= best; } else { s.minv[j] -= best; }
      }
      __syncthreads();
      j0 = bj;
      if (s.p[j0] < 0) { found = true; break; }
    }
    if (!found) break;
    if (lane == 0) {
      int j = j0;
      while (j != m) { const int j1 = s.way[j]; s.p[j] = s.p[j1]; j = j1; }
    }
    __syncthreads();
  }
  for (int j = lane; j < m; j += 64) {
    const int r = s.p[j];
    if (r >= 0) { if (tr) s.mcol[j] = r; else s.mcol[r] = j; }
  }
  __syncthreads();
}

// All LDS of the two solver kernels is dynamic (a 16-byte aligned base): the solver's vectors, then room for the weight
// matrix of the largest frame of the call, when that is at most kLdsCells cells (lds_cells; 0: the workspace is used).
extern __shared__ __attribute__((aligned(16))) char mot_smem[];
constexpr size_t kSolverBytes = (sizeof(SolverLds) + 15) / 16 * 16;

inline int lds_cells_of(const StMotArgs* a) {
  const long long m = a->max_frame_objects;
  return m <= 0 ? 0 : (int)(m * m < kLdsCells ? m * m : kLdsCells);   // smaller frames of the call still fit
}

__device__ inline void load_ids(const StMotArgs& a, int gs, int G, int ps, int P, SolverLds& s, int lane) {
  for (int i = lane; i < G; i += 64) s.gid[i] = (int)a.gt_rows[6 * (size_t)(gs + i) + 1];
  for (int j = lane; j < P; j += 64) s.tid[j] = (int)a.pred_rows[6 * (size_t)(ps + j) + 1];
}

// ---- the sequence walk ------------------------------------------------------------------------------------------------
// Counts and both potentials.  A cell (g, t) is touched by one thread per frame (ids are unique inside a frame) and the
// frames follow each other behind a barrier, so every cell is summed in frame order without an atomic.
__global__ __launch_bounds__(kPotThreads) void k_potential(StMotArgs a, Workspace w) {
  if (a.status[0]) return;
  const int seq = blockIdx.x, tid = threadIdx.x;
  const bool do_clear = (a.flags & ST_MOT_CLEAR) != 0, do_hota = (a.flags & ST_MOT_HOTA) != 0;
  const int nt = a.seq_nt[seq];
  int* __restrict__ gt_count = a.gt_count + a.seq_gid_off[seq];
  int* __restrict__ tr_count = a.tr_count + a.seq_tid_off[seq];
  int* __restrict__ idp = a.id_potential + a.seq_mat_off[seq];
  double* __restrict__ hp = a.hota_potential + a.seq_mat_off[seq];
  const double thr = a.iou_thr - kEps;
  for (int f = a.seq_frame_off[seq]; f < a.seq_frame_off[seq + 1]; ++f) {
    __syncthreads();
    const int gs = a.frame_gt_off[f], G = a.frame_gt_off[f + 1] - gs;
    const int ps = a.frame_pred_off[f], P = a.frame_pred_off[f + 1] - ps;
    for (int i = tid; i < G; i += kPotThreads) gt_count[(int)a.gt_rows[6 * (size_t)(gs + i) + 1]] += 1;
    for (int j = tid; j < P; j += kPotThreads) tr_count[(int)a.pred_rows[6 * (size_t)(ps + j) + 1]] += 1;
    const int cells = G * P;
    const double* __restrict__ sim = w.sim + a.frame_pair_off[f];
    for (int c = tid; c < cells; c += kPotThreads) {
      const double sv = sim[c];
      const bool hit = do_clear && sv >= thr;
      const bool pot = do_hota && sv != 0.0;      // siou of a zero IoU is zero: adding it changes no bit
      if (!hit && !pot) continue;
      const int i = c / P, j = c - i * P;
      const int g = (int)a.gt_rows[6 * (size_t)(gs + i) + 1], t = (int)a.pred_rows[6 * (size_t)(ps + j) + 1];
      const size_t cell = (size_t)g * nt + t;
      if (pot) {
        const double den = (w.colsum[ps + j] + w.rowsum[gs + i]) - sv;
        if (den > kEps) hp[cell] += sv / den;
      }
      if (hit) idp[cell] += 1;
    }
  }
}

// CLEAR.  The frame's score matrix is k_similarity's thresholded IoU plus 1000 where the prediction is the ground truth's
// match of the previous matched frame: at most one cell per row, patched here, since that state exists only in frame order.
__global__ __launch_bounds__(64) void k_walk(StMotArgs a, Workspace w, int lds_cells) {
  SolverLds& S = *reinterpret_cast<SolverLds*>(mot_smem);
  double* Wl = reinterpret_cast<double*>(mot_smem + kSolverBytes);
  if (a.status[0]) return;
  const int seq = blockIdx.x, lane = threadIdx.x;
  const int ng = a.seq_ng[seq];
  const i64 go = a.seq_gid_off[seq];
  int* prev_tracker = w.prev_tracker + go;   // last tracker id ever matched to a gt, -1 none
  int* prev_step = w.prev_step + go;         // tracker id matched in the previous matched frame, -1 none
  int* cur_step = w.cur_step + go;           // -1 between frames
  int tp = 0, fn = 0, fp = 0, idsw = 0;
  double motp = 0.0;
  for (int f = a.seq_frame_off[seq]; f < a.seq_frame_off[seq + 1]; ++f) {
    __syncthreads();
    const int gs = a.frame_gt_off[f], G = a.frame_gt_off[f + 1] - gs;
    const int ps = a.frame_pred_off[f], P = a.frame_pred_off[f + 1] - ps;
    if (G == 0) { fp += P; continue; }
    load_ids(a, gs, G, ps, P, S, lane);
    __syncthreads();
    if (P == 0) {
      fn += G;
      for (int i = lane; i < G; i += 64) a.gt_frames[go + S.gid[i]] += 1;
      continue;
    }
    const double* __restrict__ sim = w.sim + a.frame_pair_off[f];
    const int cells = G * P;
    const double* __restrict__ base = w.base + a.frame_pair_off[f];
    double* W = cells <= lds_cells ? Wl : w.weight + a.frame_pair_off[f];   // a copy: the stage may be repeated
    for (int c = lane; c < cells; c += 64) W[c] = base[c];
    __syncthreads();
    for (int i = lane; i < G; i += 64) {
      const int want = prev_step[S.gid[i]];
      if (want < 0) continue;
      for (int j = 0; j < P; ++j)
        if (S.tid[j] == want) {
          const size_t c = (size_t)i * P + j;
          if (!(sim[c] < a.iou_thr - kEps)) W[c] = 1000.0 + sim[c];
          break;
        }
    }
    __syncthreads();
    solve_assignment(W, G, P, S, lane);
    int nm = 0;
    double ms = 0.0;
    for (int i = lane; i < G; i += 64) {
      const int j = S.mcol[i];
      if (j < 0 || !(W[(size_t)i * P + j] > kEps)) continue;
      const int g = S.gid[i], t = S.tid[j];
      const int prev = prev_tracker[g];
      if (prev >= 0 && prev != t) ++idsw;
      prev_tracker[g] = t;
      cur_step[g] = t;
      ++nm;
      ms += sim[(size_t)i * P + j];
    }
    for (int o = 32; o > 0; o >>= 1) { nm += __shfl_xor(nm, o); ms += __shfl_xor(ms, o); }
    __syncthreads();
    for (int g = lane; g < ng; g += 64) {
      const bool before = prev_step[g] >= 0;
      const int c = cur_step[g];
      if (c >= 0) {
        a.gt_matched[go + g] += 1;
        if (!before) a.gt_frag[go + g] += 1;   // a new tracked segment of this gt starts
      }
      prev_step[g] = c;
      cur_step[g] = -1;
    }
    for (int i = lane; i < G; i += 64) a.gt_frames[go + S.gid[i]] += 1;
    tp += nm;
    fn += G - nm;
    fp += P - nm;
    motp += ms;
  }
  for (int o = 32; o > 0; o >>= 1) idsw += __shfl_xor(idsw, o);
  if (lane == 0) {
    a.clear_counts[4 * seq] = tp;
    a.clear_counts[4 * seq + 1] = fn;
    a.clear_counts[4 * seq + 2] = fp;
    a.clear_counts[4 * seq + 3] = idsw;
    a.motp_sum[seq] = motp;
  }
}

// ---- HOTA pass 2 -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_hota_match(StMotArgs a, Workspace w, int lds_cells) {
  SolverLds& S = *reinterpret_cast<SolverLds*>(mot_smem);
  double* Wl = reinterpret_cast<double*>(mot_smem + kSolverBytes);
  if (a.status[0]) return;
  const int f = blockIdx.x, lane = threadIdx.x;
  const int gs = a.frame_gt_off[f], G = a.frame_gt_off[f + 1] - gs;
  const int ps = a.frame_pred_off[f], P = a.frame_pred_off[f + 1] - ps;
  if (G == 0) return;
  if (P == 0) {
    for (int i = lane; i < G; i += 64) { w.match_tid[gs + i] = -1; w.match_sim[gs + i] = 0.0; }
    return;
  }
  const int seq = a.frame_seq[f];
  const int nt = a.seq_nt[seq];
  const int* __restrict__ gt_count = a.gt_count + a.seq_gid_off[seq];
  const int* __restrict__ tr_count = a.tr_count + a.seq_tid_off[seq];
  const double* __restrict__ hp = a.hota_potential + a.seq_mat_off[seq];
  const double* __restrict__ sim = w.sim + a.frame_pair_off[f];
  load_ids(a, gs, G, ps, P, S, lane);
  __syncthreads();
  const int cells = G * P;
  double* W = cells <= lds_cells ? Wl : w.weight + a.frame_pair_off[f];
  for (int c = lane; c < cells; c += 64) {
    const int i = c / P, j = c - i * P;
    const int g = S.gid[i], t = S.tid[j];
    const double pot = hp[(size_t)g * nt + t];
    const double align = pot / (((double)gt_count[g] + (double)tr_count[t]) - pot);
    W[c] = align * sim[c];
  }
  __syncthreads();
  solve_assignment(W, G, P, S, lane);
  for (int i = lane; i < G; i += 64) {
    const int j = S.mcol[i];
    w.match_tid[gs + i] = j >= 0 ? S.tid[j] : -1;
    w.match_sim[gs + i] = j >= 0 ? sim[(size_t)i * P + j] : 0.0;
  }
}

// sum over the workgroup in a fixed tree order; every thread returns the total
__device__ inline double block_sum(double v, double* red, int tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = kAccThreads / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kAccThreads) void k_hota_acc(StMotArgs a, Workspace w) {
  __shared__ double red[kAccThreads];
  __shared__ int tp_total;
  if (a.status[0]) return;
  const int A = a.num_alphas;
  const int seq = blockIdx.x / A, al = blockIdx.x % A, tid = threadIdx.x;
  const int f0 = a.seq_frame_off[seq], f1 = a.seq_frame_off[seq + 1];
  const int r0 = a.frame_gt_off[f0], r1 = a.frame_gt_off[f1];
  const int npred = a.frame_pred_off[f1] - a.frame_pred_off[f0];
  const int ng = a.seq_ng[seq], nt = a.seq_nt[seq];
  const double thr = a.alphas[al] - kEps;
  int* mc = w.matches + (size_t)al * (size_t)a.num_cells + a.seq_mat_off[seq];
  if (tid == 0) tp_total = 0;
  __syncthreads();
  int tp = 0;
  double loc = 0.0;
  for (int r = r0 + tid; r < r1; r += kAccThreads) {
    const int t = w.match_tid[r];
    if (t < 0) continue;
    const double sv = w.match_sim[r];
    if (!(sv >= thr)) continue;
    ++tp;
    loc += sv;
    const int g = (int)a.gt_rows[6 * (size_t)r + 1];
    atomicAdd(&mc[(size_t)g * nt + t], 1);
  }
  if (tp) atomicAdd(&tp_total, tp);
  loc = block_sum(loc, red, tid);
  __threadfence();
  __syncthreads();
  const int TP = tp_total;
  const int* __restrict__ gt_count = a.gt_count + a.seq_gid_off[seq];
  const int* __restrict__ tr_count = a.tr_count + a.seq_tid_off[seq];
  double assa = 0.0, assre = 0.0, asspr = 0.0;
  const i64 cells = (i64)ng * nt;
  for (i64 c = tid; c < cells; c += kAccThreads) {
    const int m = __hip_atomic_load(&mc[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (m == 0) continue;
    const int g = (int)(c / nt), t = (int)(c - (i64)g * nt);
    const double md = (double)m, gc = (double)gt_count[g], tc = (double)tr_count[t];
    assa += md * (md / fmax(1.0, (gc + tc) - md));
    assre += md * (md / fmax(1.0, gc));
    asspr += md * (md / fmax(1.0, tc));
  }
  assa = block_sum(assa, red, tid);
  assre = block_sum(assre, red, tid);
  asspr = block_sum(asspr, red, tid);
  if (tid == 0) {
    int* hc = a.hota_counts + 3 * (size_t)blockIdx.x;
    double* hs = a.hota_sums + 4 * (size_t)blockIdx.x;
    hc[0] = TP;
    hc[1] = (r1 - r0) - TP;
    hc[2] = npred - TP;
    hs[0] = loc;
    hs[1] = assa;
    hs[2] = assre;
    hs[3] = asspr;
  }
}

// ---- KITTI 2-D box preprocessing (include/stereotrack.h section 16, metrics.py kitti_preprocess) ---------------------
constexpr int kGtCols = 9, kPredCols = 8, kIgnCols = 5;        // row widths; the boxes start at columns 5, 3 and 1
constexpr int kMaxDistractors = ST_MOT_KITTI_MAX_DISTRACTORS;
constexpr int kWsSlot = 32;                                     // status bit: a frame's workspace slot is too small

struct KittiBox { double x1, y1, x2, y2; };

__device__ inline KittiBox load_box(const double* __restrict__ p) { return KittiBox{p[0], p[1], p[2], p[3]}; }

__device__ inline bool finite_box(const double* __restrict__ p) {
  return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(p[3]);
}

// intersection and the two areas, in the operation order of TrackEval's _calculate_box_ious on x0y0x1y1 boxes
__device__ inline double kitti_inter(const KittiBox& a, const KittiBox& b, double* a1, double* a2) {
  double iw = fmin(a.x2, b.x2) - fmax(a.x1, b.x1);
  double ih = fmin(a.y2, b.y2) - fmax(a.y1, b.y1);
  iw = iw < 0.0 ? 0.0 : iw;
  ih = ih < 0.0 ? 0.0 : ih;
  *a1 = (a.x2 - a.x1) * (a.y2 - a.y1);
  *a2 = (b.x2 - b.x1) * (b.y2 - b.y1);
  return iw * ih;
}

// the rows of [s, e) that `pick` selects, in row order, as indices in list[0 .. kMaxObj); returns how many there are
template <typename Pick>
__device__ inline int compact_rows(int s, int e, int lane, int* list, Pick pick) {
  int count = 0;
  for (int base = s; base < e; base += 64) {
    const int r = base + lane;
    const bool in = r < e && pick(r);
    const unsigned long long mask = __ballot(in);
    const int pos = count + __popcll(mask & ((1ull << lane) - 1ull));
    if (in && pos < kMaxObj) list[pos] = r;
    count += __popcll(mask);
  }
  return count;
}

__global__ __launch_bounds__(64) void k_kitti(StMotKittiArgs a, double* ws, int lds_cells) {
  SolverLds& S = *reinterpret_cast<SolverLds*>(mot_smem);
  double* Wl = reinterpret_cast<double*>(mot_smem + kSolverBytes);
  const int f = blockIdx.x / a.num_classes, ci = blockIdx.x - f * a.num_classes, lane = threadIdx.x;
  const int rep = a.num_frames - f;
  const int gs = a.frame_gt_off[f], ge = a.frame_gt_off[f + 1];
  const int ps = a.frame_pred_off[f], pe = a.frame_pred_off[f + 1];
  const int is = a.frame_ignore_off[f], ie = a.frame_ignore_off[f + 1];
  if (gs < 0 || ge < gs || ge > a.num_gt || ps < 0 || pe < ps || pe > a.num_pred || is < 0 || ie < is || ie > a.num_ignore) {
    if (lane == 0) report(a.status, kFrameLimit, 3, rep);      // an offset table that does not fit the row arrays
    return;
  }
  bool bad = false;
  for (int r = gs + lane; r < ge; r += 64) bad = bad || !finite_box(a.gt_rows + (size_t)kGtCols * r + 5);
  for (int r = ps + lane; r < pe; r += 64) bad = bad || !finite_box(a.pred_rows + (size_t)kPredCols * r + 3);
  for (int r = is + lane; r < ie; r += 64) bad = bad || !finite_box(a.ignore_rows + (size_t)kIgnCols * r + 1);
  if (bad) report(a.status, kNonFinite, 0, rep);
  if (__any(bad)) return;

  const int* __restrict__ ct = a.class_table + (1 + kMaxDistractors) * ci;
  const double cls = (double)ct[0];
  double dis[kMaxDistractors];
  for (int k = 0; k < kMaxDistractors; ++k) dis[k] = (double)ct[1 + k];
  auto is_distractor = [&](double c) {
    bool d = false;
    for (int k = 0; k < kMaxDistractors; ++k) d = d || (ct[1 + k] >= 0 && c == dis[k]);
    return d;
  };
  // step 1: G = the ground truth of the class or a distractor (S.gid), P = the predictions of the class (S.tid)
  const int G = compact_rows(gs, ge, lane, S.gid, [&](int r) {
    const double c = a.gt_rows[(size_t)kGtCols * r + 2];
    return c == cls || is_distractor(c);
  });
  const int P = compact_rows(ps, pe, lane, S.tid, [&](int r) { return a.pred_rows[(size_t)kPredCols * r + 2] == cls; });
  if (G > kMaxObj || P > kMaxObj) {
    if (lane == 0) report(a.status, kFrameLimit, 3, rep);
    return;
  }
  __syncthreads();
  // step 5: the ground truth kept for scoring needs no matching
  unsigned char* __restrict__ gt_keep = a.gt_keep + (size_t)ci * (size_t)a.num_gt;
  unsigned char* __restrict__ pred_keep = a.pred_keep + (size_t)ci * (size_t)a.num_pred;
  for (int i = lane; i < G; i += 64) {
    const double* row = a.gt_rows + (size_t)kGtCols * S.gid[i];
    if (row[2] == cls && row[4] <= a.max_occlusion && row[3] <= a.max_truncation) gt_keep[S.gid[i]] = 1;
  }
  // steps 2 and 3: the thresholded IoU matrix, one assignment; S.used[j]: 0 unmatched, 1 matched and kept, 2 removed
  const int cells = G * P;
  if (cells > 0) {
    double* W = Wl;
    if (cells > lds_cells) {
      const long long w0 = a.frame_ws_off[f], w1 = a.frame_ws_off[f + 1];
      if (w0 < 0 || w1 > a.num_ws_cells || w1 - w0 < (long long)cells) {
        if (lane == 0) report(a.status, kWsSlot, 5, rep);
        return;
      }
      W = ws + (size_t)ci * (size_t)a.num_ws_cells + (size_t)w0;
    }
    const double thr = a.match_thr - kEps;
    for (int c = lane; c < cells; c += 64) {
      const int i = c / P, j = c - i * P;
      const KittiBox g = load_box(a.gt_rows + (size_t)kGtCols * S.gid[i] + 5);
      const KittiBox p = load_box(a.pred_rows + (size_t)kPredCols * S.tid[j] + 3);
      double a1, a2;
      double inter = kitti_inter(g, p, &a1, &a2);
      double uni = (a1 + a2) - inter;
      if (a1 <= kEps || a2 <= kEps || uni <= kEps) inter = 0.0;
      if (uni <= kEps) uni = 1.0;
      const double sv = inter / uni;
      W[c] = sv < thr ? 0.0 : sv;
    }
    __syncthreads();
    solve_assignment(W, G, P, S, lane);
    for (int j = lane; j < P; j += 64) S.used[j] = 0;
    __syncthreads();
    for (int i = lane; i < G; i += 64) {
      const int j = S.mcol[i];
      if (j < 0 || !(W[(size_t)i * P + j] > kEps)) continue;
      const double* row = a.gt_rows + (size_t)kGtCols * S.gid[i];
      const bool remove = is_distractor(row[2]) || row[4] > a.max_occlusion + kEps || row[3] > a.max_truncation + kEps;
      S.used[j] = remove ? 2 : 1;      // the columns of an assignment are distinct
    }
    __syncthreads();
  }
  // step 4: the unmatched predictions
  for (int j = lane; j < P; j += 64) {
    const int r = S.tid[j];
    const int state = cells > 0 ? S.used[j] : 0;
    bool keep = state == 1;
    if (state == 0) {
      const KittiBox p = load_box(a.pred_rows + (size_t)kPredCols * r + 3);
      bool removed = (p.y2 - p.y1) <= a.min_height + kEps;
      for (int k = is; k < ie && !removed; ++k) {
        const KittiBox g = load_box(a.ignore_rows + (size_t)kIgnCols * k + 1);
        double a1, a2;
        double inter = kitti_inter(p, g, &a1, &a2);
        if (a1 <= kEps) { inter = 0.0; a1 = 1.0; }
        removed = inter / a1 > a.ignore_thr + kEps;
      }
      keep = !removed;
    }
    if (keep) pred_keep[r] = 1;
  }
}

// ---- MOTChallenge protocol (include/stereotrack.h section 21, metrics.py motchallenge_file_rows / _preprocess) ----------
constexpr int kModeCopy = ST_MOT_FILE_COPY, kModeTrunc = ST_MOT_FILE_TRUNCATE, kModeRound3 = ST_MOT_FILE_ROUND3;
constexpr int kFileCols = ST_MOT_FILE_MAX_COLS;
constexpr int kTooLarge = 2;                                    // st_mot_file_round's status bit: |x| >= 2^43 in a round3 column
constexpr double kRound3Limit = 8796093022208.0;                // 2^43: x * 1000 stays below 2^53
constexpr int kChGtCols = 8, kChPredCols = 7;                   // (frame, id, x, y, w, h, conf, class) / (..., score)
constexpr int kChMaxDistractors = ST_MOT_CHALLENGE_MAX_DISTRACTORS;

struct FileModes { int m[kFileCols]; };

// float('%.3f' % x): the EXACT value of x to 3 decimals, ties to even, then the nearest double to that decimal.
// p = x * 1000 is rounded; e = the exact residual x * 1000 - p (one fused multiply-add); n = rint(p) is the candidate
// and the exact distance of x * 1000 from n is d + e with d = p - n exact (|d| <= 0.5).  The candidate is off by one
// where d + e lies beyond +-0.5, and on an exact tie the even neighbour is taken.
__device__ inline double round3(double x) {
  const double p = x * 1000.0;
  const double e = __builtin_fma(x, 1000.0, -p);
  double n = rint(p);
  const double d = p - n;
  const double hi = (d - 0.5) + e, lo = (d + 0.5) + e;
  const bool odd = (((long long)n) & 1ll) != 0;
  if (hi > 0.0 || (hi == 0.0 && odd)) n += 1.0;
  else if (lo < 0.0 || (lo == 0.0 && odd)) n -= 1.0;
  return n / 1000.0;
}

__global__ __launch_bounds__(256) void k_file_round(const double* __restrict__ rows, double* __restrict__ out, i64 num_rows,
                                                    int cols, FileModes modes, int* status) {
  const i64 total = num_rows * cols;
  for (i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += (i64)gridDim.x * blockDim.x) {
    const i64 r = c / cols;
    const int mode = modes.m[(int)(c - r * cols)];
    const double x = rows[c];
    const int rep = (int)(num_rows - r);
    double y = x;
    if (mode != kModeCopy) {
      if (!isfinite(x)) {
        report(status, kNonFinite, 0, rep);
      } else if (mode == kModeTrunc) {
        y = trunc(x) + 0.0;                                    // + 0.0: int(-0.5) is 0, not -0
      } else if (fabs(x) >= kRound3Limit) {
        report(status, kTooLarge, 1, rep);
      } else {
        y = round3(x);
      }
    }
    out[c] = y;
  }
}

// One wave per frame: TrackEval's MotChallenge2DBox preprocessing as metrics.motchallenge_preprocess states it.
// S.used[j]: 1 = prediction j of the frame is matched to ground truth of a distractor class and removed.
__global__ __launch_bounds__(64) void k_challenge(StMotChallengeArgs a, double* ws, int lds_cells) {
  SolverLds& S = *reinterpret_cast<SolverLds*>(mot_smem);
  double* Wl = reinterpret_cast<double*>(mot_smem + kSolverBytes);
  const int f = blockIdx.x, lane = threadIdx.x;
  const int rep = a.num_frames - f;
  const int gs = a.frame_gt_off[f], ge = a.frame_gt_off[f + 1];
  const int ps = a.frame_pred_off[f], pe = a.frame_pred_off[f + 1];
  if (gs < 0 || ge < gs || ge > a.num_gt || ps < 0 || pe < ps || pe > a.num_pred) {
    if (lane == 0) report(a.status, kFrameLimit, 3, rep);      // an offset table that does not fit the row arrays
    return;
  }
  const int G = ge - gs, P = pe - ps;
  if (G > kMaxObj || P > kMaxObj) {
    if (lane == 0) report(a.status, kFrameLimit, 3, rep);
    return;
  }
  bool bad = false;
  for (int r = gs + lane; r < ge; r += 64) bad = bad || !finite_box(a.gt_rows + (size_t)kChGtCols * r + 2);
  for (int r = ps + lane; r < pe; r += 64) bad = bad || !finite_box(a.pred_rows + (size_t)kChPredCols * r + 2);
  if (bad) report(a.status, kNonFinite, 0, rep);
  if (__any(bad)) return;

  for (int i = lane; i < G; i += 64) {
    const double* row = a.gt_rows + (size_t)kChGtCols * (gs + i);
    if (row[6] != 0.0 && (!a.do_preproc || row[7] == 1.0)) a.gt_keep[gs + i] = 1;
  }
  const int cells = G * P;
  const bool match = a.do_preproc && cells > 0;
  if (match) {
    double* W = Wl;
    if (cells > lds_cells) {
      const long long w0 = a.frame_ws_off[f], w1 = a.frame_ws_off[f + 1];
      if (w0 < 0 || w1 > a.num_ws_cells || w1 - w0 < (long long)cells) {
        if (lane == 0) report(a.status, kWsSlot, 5, rep);
        return;
      }
      W = ws + (size_t)w0;
    }
    const double thr = 0.5 - kEps;                             // TrackEval's constant, not the scorers' iou_thr
    for (int c = lane; c < cells; c += 64) {                   // box_iou_xywh, operation for operation
      const int i = c / P, j = c - i * P;
      const double* g = a.gt_rows + (size_t)kChGtCols * (gs + i) + 2;
      const double* p = a.pred_rows + (size_t)kChPredCols * (ps + j) + 2;
      const double ax2 = g[0] + g[2], ay2 = g[1] + g[3], bx2 = p[0] + p[2], by2 = p[1] + p[3];
      double iw = fmin(ax2, bx2) - fmax(g[0], p[0]);
      double ih = fmin(ay2, by2) - fmax(g[1], p[1]);
      iw = iw < 0.0 ? 0.0 : iw;
      ih = ih < 0.0 ? 0.0 : ih;
      const double inter = iw * ih;
      const double uni = (g[2] * g[3] + p[2] * p[3]) - inter;
      const double sv = uni > 0.0 ? inter / fmax(uni, 1e-12) : 0.0;
      W[c] = sv < thr ? 0.0 : sv;
    }
    __syncthreads();
    solve_assignment(W, G, P, S, lane);
    for (int j = lane; j < P; j += 64) S.used[j] = 0;
    __syncthreads();
    for (int i = lane; i < G; i += 64) {
      const int j = S.mcol[i];
      if (j < 0 || !(W[(size_t)i * P + j] > kEps)) continue;
      const double cls = a.gt_rows[(size_t)kChGtCols * (gs + i) + 7];
      bool distractor = false;
      for (int k = 0; k < kChMaxDistractors; ++k) distractor = distractor || (k < a.num_distractors && cls == (double)a.distractors[k]);
      if (distractor) S.used[j] = 1;                           // the columns of an assignment are distinct
    }
    __syncthreads();
  }
  for (int j = lane; j < P; j += 64)
    if (!(match && S.used[j])) a.pred_keep[ps + j] = 1;
}

int validate_challenge(const StMotChallengeArgs* a) {
  ST_REQUIRE(a != nullptr, "st_mot_challenge: args is NULL");
  ST_REQUIRE(a->struct_size == (int)sizeof(StMotChallengeArgs), "st_mot_challenge: struct_size %d != %d", a->struct_size,
             (int)sizeof(StMotChallengeArgs));
  ST_REQUIRE(a->num_frames >= 0 && a->num_gt >= 0 && a->num_pred >= 0,
             "st_mot_challenge: num_frames %d / num_gt %d / num_pred %d must be >= 0", a->num_frames, a->num_gt, a->num_pred);
  ST_REQUIRE(a->num_distractors >= 0 && a->num_distractors <= kChMaxDistractors,
             "st_mot_challenge: num_distractors %d outside 0..%d", a->num_distractors, kChMaxDistractors);
  ST_REQUIRE(a->num_ws_cells >= 0, "st_mot_challenge: num_ws_cells must be >= 0");
  ST_REQUIRE(a->ws != nullptr && a->ws_bytes >= st_mot_challenge_workspace_bytes(a),
             "st_mot_challenge: workspace %zu < %zu bytes", a->ws_bytes, st_mot_challenge_workspace_bytes(a));
  ST_REQUIRE(a->status != nullptr && (a->num_gt == 0 || a->gt_keep != nullptr) && (a->num_pred == 0 || a->pred_keep != nullptr),
             "st_mot_challenge: status / gt_keep / pred_keep is NULL");
  ST_REQUIRE((a->num_gt == 0 || a->gt_rows != nullptr) && (a->num_pred == 0 || a->pred_rows != nullptr),
             "st_mot_challenge: gt_rows / pred_rows is NULL");
  ST_REQUIRE(a->num_frames == 0 || (a->frame_gt_off && a->frame_pred_off && a->frame_ws_off),
             "st_mot_challenge: an offset table is NULL");
  return ST_OK;
}

int validate_kitti(const StMotKittiArgs* a) {
  ST_REQUIRE(a != nullptr, "st_mot_kitti: args is NULL");
  ST_REQUIRE(a->struct_size == (int)sizeof(StMotKittiArgs), "st_mot_kitti: struct_size %d != %d", a->struct_size,
             (int)sizeof(StMotKittiArgs));
  ST_REQUIRE(a->num_frames >= 0 && a->num_classes >= 1 && a->num_gt >= 0 && a->num_pred >= 0 && a->num_ignore >= 0,
             "st_mot_kitti: num_frames %d / num_gt %d / num_pred %d / num_ignore %d must be >= 0, num_classes %d >= 1",
             a->num_frames, a->num_gt, a->num_pred, a->num_ignore, a->num_classes);
  ST_REQUIRE((long long)a->num_frames * a->num_classes < (1ll << 31) - 1, "st_mot_kitti: num_frames x num_classes too large");
  ST_REQUIRE(a->num_ws_cells >= 0, "st_mot_kitti: num_ws_cells must be >= 0");
  ST_REQUIRE(a->ws != nullptr && a->ws_bytes >= st_mot_kitti_workspace_bytes(a), "st_mot_kitti: workspace %zu < %zu bytes",
             a->ws_bytes, st_mot_kitti_workspace_bytes(a));
  ST_REQUIRE(a->status != nullptr && a->gt_keep != nullptr && a->pred_keep != nullptr,
             "st_mot_kitti: status / gt_keep / pred_keep is NULL");
  ST_REQUIRE(a->num_frames == 0 || (a->frame_gt_off && a->frame_pred_off && a->frame_ignore_off && a->frame_ws_off &&
                                    a->class_table), "st_mot_kitti: an offset table or the class table is NULL");
  return ST_OK;
}

int validate(const StMotArgs* a) {
  ST_REQUIRE(a != nullptr, "st_mot: args is NULL");
  ST_REQUIRE(a->struct_size == (int)sizeof(StMotArgs), "st_mot: struct_size %d != %d", a->struct_size,
             (int)sizeof(StMotArgs));
  ST_REQUIRE(a->num_seqs >= 1 && a->num_frames >= 0 && a->num_gt >= 0 && a->num_pred >= 0,
             "st_mot: num_seqs %d must be >= 1, num_frames %d / num_gt %d / num_pred %d >= 0", a->num_seqs,
             a->num_frames, a->num_gt, a->num_pred);
  ST_REQUIRE(a->num_alphas >= 0 && a->num_alphas <= kMaxAlphas, "st_mot: num_alphas %d outside 0..%d", a->num_alphas,
             kMaxAlphas);
  ST_REQUIRE((long long)a->num_seqs * (a->num_alphas > 0 ? a->num_alphas : 1) < (1ll << 30),
             "st_mot: num_seqs x num_alphas too large");
  ST_REQUIRE(a->num_pairs >= 0 && a->num_cells >= 0 && a->num_gids >= 0 && a->num_tids >= 0,
             "st_mot: num_pairs / num_cells / num_gids / num_tids must be >= 0");
  ST_REQUIRE(a->ws != nullptr, "st_mot: workspace is NULL");
  ST_REQUIRE(a->status != nullptr, "st_mot: status is NULL");
  Workspace w;
  carve(a, a->ws, &w);
  ST_REQUIRE(a->ws_bytes >= w.total, "st_mot: workspace %zu < %zu bytes", a->ws_bytes, w.total);
  return ST_OK;
}

int zero(void* p, int value, size_t bytes, hipStream_t stream) {
  if (p && bytes) ST_CHECK_HIP(hipMemsetAsync(p, value, bytes, stream));
  return ST_OK;
}

}  // namespace

extern "C" {

int st_mot_max_objects(void) { return kMaxObj; }
int st_mot_max_alphas(void) { return kMaxAlphas; }

size_t st_mot_workspace_bytes(const StMotArgs* args) {
  if (!args || args->struct_size != (int)sizeof(StMotArgs) || args->num_pairs < 0 || args->num_cells < 0 ||
      args->num_gids < 0 || args->num_gt < 0 || args->num_pred < 0 || args->num_alphas < 0)
    return 0;
  Workspace w;
  carve(args, nullptr, &w);
  return w.total;
}

size_t st_mot_workspace_sim_offset(const StMotArgs* args) {
  if (!args || args->struct_size != (int)sizeof(StMotArgs)) return 0;
  Workspace w;
  carve(args, nullptr, &w);
  return w.sim_offset;
}

int st_mot_similarity(const StMotArgs* a, st_stream_t stream_) {
  ST_CHECK(validate(a));
  hipStream_t stream = (hipStream_t)stream_;
  Workspace w;
  carve(a, a->ws, &w);
  ST_CHECK(zero(a->status, 0, 8 * sizeof(int), stream));
  if (a->num_frames > 0) hipLaunchKernelGGL(k_similarity, dim3(a->num_frames), dim3(64), 0, stream, *a, w);
  ST_CHECK_HIP(hipGetLastError());
  ST_REQUIRE(a->max_frame_objects <= kMaxObj, "st_mot: a frame holds %d rows of one kind, a launch supports %d "
             "(st_mot_max_objects); the status word names the frame", a->max_frame_objects, kMaxObj);
  return ST_OK;
}

int st_mot_walk(const StMotArgs* a, st_stream_t stream_) {
  ST_CHECK(validate(a));
  ST_REQUIRE((a->flags & (ST_MOT_CLEAR | ST_MOT_HOTA)) != 0 && (a->flags & ~(ST_MOT_CLEAR | ST_MOT_HOTA)) == 0,
             "st_mot_walk: flags %d must be ST_MOT_CLEAR and / or ST_MOT_HOTA", a->flags);
  hipStream_t stream = (hipStream_t)stream_;
  Workspace w;
  carve(a, a->ws, &w);
  const size_t IDS = (size_t)a->num_gids, TIDS = (size_t)a->num_tids, CELLS = (size_t)a->num_cells;
  ST_CHECK(zero(a->gt_count, 0, IDS * sizeof(int), stream));
  ST_CHECK(zero(a->tr_count, 0, TIDS * sizeof(int), stream));
  ST_CHECK(zero(a->id_potential, 0, CELLS * sizeof(int), stream));
  ST_CHECK(zero(a->hota_potential, 0, CELLS * sizeof(double), stream));
  ST_CHECK(zero(a->gt_frames, 0, IDS * sizeof(int), stream));
  ST_CHECK(zero(a->gt_matched, 0, IDS * sizeof(int), stream));
  ST_CHECK(zero(a->gt_frag, 0, IDS * sizeof(int), stream));
  ST_CHECK(zero(w.prev_tracker, 0xff, IDS * sizeof(int), stream));
  ST_CHECK(zero(w.prev_step, 0xff, IDS * sizeof(int), stream));
  ST_CHECK(zero(w.cur_step, 0xff, IDS * sizeof(int), stream));
  hipLaunchKernelGGL(k_potential, dim3(a->num_seqs), dim3(kPotThreads), 0, stream, *a, w);
  const int lds_cells = lds_cells_of(a);
  if (a->flags & ST_MOT_CLEAR)
    hipLaunchKernelGGL(k_walk, dim3(a->num_seqs), dim3(64), kSolverBytes + lds_cells * sizeof(double), stream, *a, w, lds_cells);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

int st_mot_hota_match(const StMotArgs* a, st_stream_t stream_) {
  ST_CHECK(validate(a));
  hipStream_t stream = (hipStream_t)stream_;
  Workspace w;
  carve(a, a->ws, &w);
  const int lds_cells = lds_cells_of(a);
  if (a->num_frames > 0)
    hipLaunchKernelGGL(k_hota_match, dim3(a->num_frames), dim3(64), kSolverBytes + lds_cells * sizeof(double), stream, *a, w,
                       lds_cells);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

int st_mot_hota_accumulate(const StMotArgs* a, st_stream_t stream_) {
  ST_CHECK(validate(a));
  ST_REQUIRE(a->num_alphas >= 1 && a->alphas != nullptr, "st_mot_hota_accumulate: no alpha table");
  hipStream_t stream = (hipStream_t)stream_;
  Workspace w;
  carve(a, a->ws, &w);
  ST_CHECK(zero(w.matches, 0, (size_t)a->num_cells * (size_t)a->num_alphas * sizeof(int), stream));
  hipLaunchKernelGGL(k_hota_acc, dim3(a->num_seqs * a->num_alphas), dim3(kAccThreads), 0, stream, *a, w);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

size_t st_mot_kitti_workspace_bytes(const StMotKittiArgs* args) {
  if (!args || args->struct_size != (int)sizeof(StMotKittiArgs) || args->num_classes < 1 || args->num_ws_cells < 0) return 0;
  return align256(((size_t)args->num_classes * (size_t)args->num_ws_cells + 1) * sizeof(double));
}

int st_mot_kitti_preprocess(const StMotKittiArgs* a, st_stream_t stream_) {
  ST_CHECK(validate_kitti(a));
  hipStream_t stream = (hipStream_t)stream_;
  ST_CHECK(zero(a->status, 0, 8 * sizeof(int), stream));
  ST_CHECK(zero(a->gt_keep, 0, (size_t)a->num_classes * (size_t)a->num_gt, stream));
  ST_CHECK(zero(a->pred_keep, 0, (size_t)a->num_classes * (size_t)a->num_pred, stream));
  const long long m = a->max_frame_objects;
  const int lds_cells = m <= 0 ? 0 : (int)(m * m < kLdsCells ? m * m : kLdsCells);
  if (a->num_frames > 0)
    hipLaunchKernelGGL(k_kitti, dim3(a->num_frames * a->num_classes), dim3(64), kSolverBytes + lds_cells * sizeof(double),
                       stream, *a, (double*)a->ws, lds_cells);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

int st_mot_file_round(const double* rows_dev, double* out_dev, long long num_rows, int num_cols, const int* col_modes,
                      int* status_dev, st_stream_t stream_) {
  ST_REQUIRE(num_rows >= 0 && num_cols >= 1 && num_cols <= kFileCols, "st_mot_file_round: num_rows %lld must be >= 0, "
             "num_cols %d in 1..%d", num_rows, num_cols, kFileCols);
  ST_REQUIRE(num_rows < (1ll << 31) - 1, "st_mot_file_round: num_rows %lld: the status word holds 32-bit row numbers", num_rows);
  ST_REQUIRE(col_modes != nullptr && status_dev != nullptr, "st_mot_file_round: col_modes / status is NULL");
  ST_REQUIRE(num_rows == 0 || (rows_dev != nullptr && out_dev != nullptr), "st_mot_file_round: rows / out is NULL");
  FileModes modes = {};
  for (int c = 0; c < num_cols; ++c) {
    ST_REQUIRE(col_modes[c] == kModeCopy || col_modes[c] == kModeTrunc || col_modes[c] == kModeRound3,
               "st_mot_file_round: col_modes[%d] = %d is not a mode", c, col_modes[c]);
    modes.m[c] = col_modes[c];
  }
  hipStream_t stream = (hipStream_t)stream_;
  ST_CHECK(zero(status_dev, 0, 8 * sizeof(int), stream));
  const long long total = num_rows * num_cols;
  if (total > 0) {
    const long long want = (total + 255) / 256;
    hipLaunchKernelGGL(k_file_round, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, stream, rows_dev, out_dev,
                       (i64)num_rows, num_cols, modes, status_dev);
  }
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

size_t st_mot_challenge_workspace_bytes(const StMotChallengeArgs* args) {
  if (!args || args->struct_size != (int)sizeof(StMotChallengeArgs) || args->num_ws_cells < 0) return 0;
  return align256(((size_t)args->num_ws_cells + 1) * sizeof(double));
}

int st_mot_challenge_preprocess(const StMotChallengeArgs* a, st_stream_t stream_) {
  ST_CHECK(validate_challenge(a));
  hipStream_t stream = (hipStream_t)stream_;
  ST_CHECK(zero(a->status, 0, 8 * sizeof(int), stream));
  ST_CHECK(zero(a->gt_keep, 0, (size_t)a->num_gt, stream));
  ST_CHECK(zero(a->pred_keep, 0, (size_t)a->num_pred, stream));
  const long long m = a->max_frame_objects;
  const int lds_cells = m <= 0 ? 0 : (int)(m * m < kLdsCells ? m * m : kLdsCells);
  if (a->num_frames > 0)
    hipLaunchKernelGGL(k_challenge, dim3(a->num_frames), dim3(64), kSolverBytes + lds_cells * sizeof(double), stream, *a,
                       (double*)a->ws, lds_cells);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

}  // extern "C"
