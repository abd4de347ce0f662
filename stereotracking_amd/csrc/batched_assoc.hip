// Batched GPU association: the depth-guided OC-SORT step of MANY independent sequences advanced in
// lockstep on the device - one workgroup (one wave) per sequence and frame.
//
// Behavioural spec = the host routine csrc/ocsort_tracker.cpp (st_tracker_track), i.e. reference (the Kalman filter, the
// box helpers, the observation history and the feeding of a track are the host routine's own: csrc/ocsort_core.h)
//   OCSORTTracker_Disparity.track            mmtrack/models/trackers/ocsort_tracker_disparity.py:345-618
//     ocm_assign_ids / ocr_assign_ids / online_smooth          :187-265, :273-317, :319-343
//   KalmanFilter initiate / predict / update                   mmtrack/models/motion/kalman_filter.py:60-189
//   lap.lapjv(extend_cost=True, cost_limit)                    -> the same dense Jonker-Volgenant as csrc/lapjv.cpp
// The ids and every row this kernel returns are EQUAL to the host routine's on the same detections
// (tests/test_batched_assoc_gpu.py): the association arithmetic is the same single IEEE operations in the same order
// (float32 boxes / IoU / direction term, float64 Kalman filter and assignment; the file is built with
// -ffp-contract=off), the assignment walks the same comparisons in the same order.  One documented last-bit
// difference: acosf (ocml here, glibc on the host: <= 1 ulp on the direction term).  The per-track state (Kalman mean /
// covariance, the saved filter, observation window, velocity direction: st_batched_tracker_get_states) is held EQUAL
// to the host routine's on the bits after every step by tests/test_tracker_state_gpu.py.
//
// Why a wave per sequence.  One sequence is a SEQUENTIAL algorithm (the north_star keeps it on the CPU, and for one
// video the CPU wins: 0.05 ms per frame).  The GPU form pays when there are hundreds of short sequences per step
// (multi-camera serving): the embarrassingly parallel parts of a sequence (Kalman prediction per track, the
// tracks x detections cost matrix, the Kalman updates per matched track) run across the 64 lanes, the branchy
// bookkeeping and the Jonker-Volgenant path search run on lane 0 with their working set in LDS / L2, and the chip runs
// thousands of such waves at once.  State lives in device memory between steps (no per-frame host round trip).
//
// Tracker-option sweeps (include/stereotrack.h section 20): the step of one sequence and frame is the device routine
// assoc_frame; assoc_step_kernel calls it once, assoc_run_kernel walks a whole recorded detection stream with it - one
// launch per run, the sequence's own option set read from device memory, the detections of a video shared by every
// sequence that tracks it.  Same routine, same state, same order of operations: a run equals its steps on the bits.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "ocsort_core.h"
#include "st_common.h"

namespace st {
namespace ba {

using namespace oc;   // KState, DTrack, WINCAP, the Kalman filter, the box helpers and the routines that feed a track

constexpr double kBig = 1000000.0;

// `poisoned`: sticky status of the sequence.  A capacity overflow is detected after the association has already
// mutated the tracks (Kalman predictions, observation windows, ids handed out), so the sequence is INVALID from then
// on: every later step reports the same status with an output count of 0 until frame_id 0 resets it.
struct SeqHeader { int n_tracks; int poisoned; long long num_tracks; };

struct Cfg {
  float obj_score_thr, init_track_thr, match_iou_thr, vel_consist_weight;
  int weight_iou_with_det_scores, num_tentatives, vel_delta_t, num_frames_retain;
  int max_tracks, max_dets;
};

// ---- dense Jonker-Volgenant on lap's (R + C)^2 extension, never materialised: at(i, j) is computed ----------------
struct Lap {
  const double* cost;   // R x C row major
  int R, C, n;
  double half;          // cost_limit / 2
  double* v;
  double* d;
  int *row_to_col, *col_to_row, *free_rows, *pred, *cols;
  char* once;
  int n_free;
  __device__ double at(int i, int j) const {
    if (i < R) {
      if (j < C) {
        const double c = cost[(size_t)i * C + j];
        return c != c ? 1e6 : c;
      }
      return half;
    }
    return j < C ? half : 0.0;
  }
  // ---- wave-cooperative form: every lane of the sequence's wave calls these; the O(n^2) scans run across the 64
  // lanes with EXACTLY the comparisons' outcomes of the serial solver (csrc/lapjv.cpp) - per-column work is
  // independent, value-only minima are order-free, and the (best, second) pair of a row scan is "lowest index of
  // the minimum, lowest index of the second smallest value among the rest", which is what the serial update rule
  // leaves behind (rows containing an unmatchable 1e6 sentinel fall back to the serial scan on lane 0).
  __device__ void reduce_columns(int lane, int* ctl) {
    for (int i = lane; i < n; i += 64) { row_to_col[i] = -1; col_to_row[i] = 0; v[i] = kBig; once[i] = 1; }
    __syncthreads();
    for (int j = lane; j < n; j += 64) {       // a lane owns its columns: rows in ascending order, strict <
      double vj = kBig;
      int cj = 0;
      for (int i = 0; i < n; ++i) {
        const double a = at(i, j);
        if (a < vj) { vj = a; cj = i; }
      }
      v[j] = vj;
      col_to_row[j] = cj;
    }
    __syncthreads();
    if (lane == 0) {
      for (int j = n - 1; j >= 0; --j) {
        const int i = col_to_row[j];
        if (row_to_col[i] < 0) {
          row_to_col[i] = j;
        } else {
          once[i] = 0;
          col_to_row[j] = -1;
        }
      }
      int nf = 0;
      for (int i = 0; i < n; ++i)
        if (row_to_col[i] < 0) free_rows[nf++] = i;
      n_free = nf;
      ctl[0] = nf;
    }
    __syncthreads();
    n_free = ctl[0];
    // reduction transfer, rows in ascending order (a row's slack uses the prices the earlier rows left)
    for (int i = 0; i < n; ++i) {
      const int j = row_to_col[i];
      if (j < 0 || !once[i]) continue;          // uniform: all lanes read the same values
      double slack = kBig;
      for (int k = lane; k < n; k += 64) {
        if (k == j) continue;
        const double r = at(i, k) - v[k];
        if (r < slack) slack = r;
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(slack, off);
        if (o < slack) slack = o;
      }
      __syncthreads();
      if (lane == 0) v[j] -= slack;
      __syncthreads();
    }
  }
  // serial row scan (the solver's own loop): used by lane 0 for rows that contain a sentinel
  __device__ void scan_row_serial(int i, int& best, int& second, double& u1, double& u2) const {
    best = 0; second = -1;
    u1 = at(i, 0) - v[0]; u2 = kBig;
    for (int j = 1; j < n; ++j) {
      const double r = at(i, j) - v[j];
      if (r < u2) {
        if (r >= u1) { u2 = r; second = j; }
        else { u2 = u1; u1 = r; second = best; best = j; }
      }
    }
  }
  __device__ void reduce_rows(int lane, int* ctl, double* ctld) {
    // ctl: 1 = cur, 2 = kept, 3 = todo, 4 = row i of this iteration (-1: done), 5.. scan results
    if (lane == 0) { ctl[1] = 0; ctl[2] = 0; ctl[3] = n_free; }
    long long sweeps = 0;
    __syncthreads();
    while (true) {
      if (lane == 0) ctl[4] = ctl[1] < ctl[3] ? free_rows[ctl[1]] : -1;
      __syncthreads();
      const int i = ctl[4];
      if (i < 0) break;
      ++sweeps;
      // parallel scan: lexicographic minimum of (r, j), then of the rest
      double b1 = kBig * 4; int j1 = 0x7fffffff; bool sentinel = false;
      for (int j = lane; j < n; j += 64) {
        const double r = at(i, j) - v[j];
        if (!(r < kBig)) sentinel = true;
        if (r < b1 || (r == b1 && j < j1)) { b1 = r; j1 = j; }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(b1, off);
        const int oj = __shfl_xor(j1, off);
        if (ob < b1 || (ob == b1 && oj < j1)) { b1 = ob; j1 = oj; }
      }
      const bool any_sentinel = __ballot(sentinel) != 0ull;
      double b2 = kBig * 4; int j2 = 0x7fffffff;
      for (int j = lane; j < n; j += 64) {
        if (j == j1) continue;
        const double r = at(i, j) - v[j];
        if (r < b2 || (r == b2 && j < j2)) { b2 = r; j2 = j; }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(b2, off);
        const int oj = __shfl_xor(j2, off);
        if (ob < b2 || (ob == b2 && oj < j2)) { b2 = ob; j2 = oj; }
      }
      __syncthreads();
      if (lane == 0) {
        int best, second;
        double u1, u2;
        if (any_sentinel || n < 2) scan_row_serial(i, best, second, u1, u2);
        else { best = j1; u1 = b1; second = j2; u2 = b2; }
        int cur = ctl[1] + 1, kept = ctl[2];
        int owner = col_to_row[best];
        const double lowered = v[best] - (u2 - u1);
        const bool lowers = lowered < v[best];
        if (sweeps < (long long)cur * n) {
          if (lowers) {
            v[best] = lowered;
          } else if (owner >= 0 && second >= 0) {
            best = second;
            owner = col_to_row[second];
          }
          if (owner >= 0) {
            if (lowers) free_rows[--cur] = owner;
            else free_rows[kept++] = owner;
          }
        } else if (owner >= 0) {
          free_rows[kept++] = owner;
        }
        row_to_col[i] = best;
        col_to_row[best] = i;
        ctl[1] = cur; ctl[2] = kept;
      }
      __syncthreads();
    }
    n_free = ctl[2];
    (void)ctld;
  }
  __device__ int shortest_path(int start) {   // lane 0 (the SCAN / TODO partition is order-dependent)
    int lo = 0, hi = 0, ready = 0, sink = -1;
    while (sink < 0) {
      if (lo == hi) {
        ready = lo;
        hi = lo + 1;
        double dmin = d[cols[lo]];
        for (int k = hi; k < n; ++k) {
          const int j = cols[k];
          if (d[j] <= dmin) {
            if (d[j] < dmin) { hi = lo; dmin = d[j]; }
            cols[k] = cols[hi];
            cols[hi++] = j;
          }
        }
        for (int k = lo; k < hi; ++k)
          if (col_to_row[cols[k]] < 0) sink = cols[k];
      }
      if (sink < 0) {
        int l = lo, h = hi;
        bool found = false;
        while (l != h && !found) {
          int j = cols[l++];
          const int i = col_to_row[j];
          const double dmin = d[j];
          const double base = at(i, j) - v[j] - dmin;
          for (int k = h; k < n; ++k) {
            j = cols[k];
            const double r = at(i, j) - v[j] - base;
            if (r < d[j]) {
              d[j] = r;
              pred[j] = i;
              if (r == dmin) {
                if (col_to_row[j] < 0) { sink = j; found = true; break; }
                cols[k] = cols[h];
                cols[h++] = j;
              }
            }
          }
        }
        if (!found) { lo = l; hi = h; }
      }
    }
    const double dmin = d[cols[lo]];
    for (int k = 0; k < ready; ++k) {
      const int j = cols[k];
      v[j] += d[j] - dmin;
    }
    return sink;
  }
  __device__ void solve(int lane, int* ctl, double* ctld) {
    reduce_columns(lane, ctl);
    for (int pass = 0; pass < 2; ++pass) {
      if (n_free <= 0) break;                    // uniform (n_free is set from ctl on every lane)
      reduce_rows(lane, ctl, ctld);
    }
    for (int f = 0; f < n_free; ++f) {
      const int start = free_rows[f];
      for (int j = lane; j < n; j += 64) {       // the path search's initial distances, across the lanes
        cols[j] = j;
        pred[j] = start;
        d[j] = at(start, j) - v[j];
      }
      __syncthreads();
      if (lane == 0) {
        int j = shortest_path(start);
        int i = -1;
        while (i != start) {
          i = pred[j];
          col_to_row[j] = i;
          const int prev = row_to_col[i];
          row_to_col[i] = j;
          j = prev;
        }
      }
      __syncthreads();
    }
  }
};

// per-sequence scratch (global memory, L2-resident): sizes in elements for n = max_tracks + max_dets
struct Scratch {
  double* cost;      // max_tracks x max_dets
  double *v, *d;     // n
  int *row_to_col, *col_to_row, *free_rows, *pred, *cols;   // n each
  char* once;        // n
  int *cand, *rest, *tidx, *confirmed, *tentative, *lost, *matched_det, *matched_trk, *d2r, *order;   // max_dets / max_tracks
  long long* ids;    // max_dets
  char* is_matched;  // max_tracks
};

__host__ __device__ inline size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

__host__ __device__ inline size_t scratch_bytes(int T, int M) {
  const size_t n = (size_t)T + M;
  size_t o = 0;
  o += align8(sizeof(double) * (size_t)T * M);
  o += 2 * align8(sizeof(double) * n);
  o += 5 * align8(sizeof(int) * n);
  o += align8(n);
  o += 10 * align8(sizeof(int) * n);
  o += align8(sizeof(long long) * (size_t)M);
  o += align8((size_t)T);
  return o;
}

__device__ inline Scratch carve(char* base, int T, int M) {
  const size_t n = (size_t)T + M;
  Scratch s;
  size_t o = 0;
  auto take = [&](size_t bytes) { char* p = base + o; o += align8(bytes); return p; };
  s.cost = (double*)take(sizeof(double) * (size_t)T * M);
  s.v = (double*)take(sizeof(double) * n);
  s.d = (double*)take(sizeof(double) * n);
  s.row_to_col = (int*)take(sizeof(int) * n);
  s.col_to_row = (int*)take(sizeof(int) * n);
  s.free_rows = (int*)take(sizeof(int) * n);
  s.pred = (int*)take(sizeof(int) * n);
  s.cols = (int*)take(sizeof(int) * n);
  s.once = take(n);
  s.cand = (int*)take(sizeof(int) * n);
  s.rest = (int*)take(sizeof(int) * n);
  s.tidx = (int*)take(sizeof(int) * n);
  s.confirmed = (int*)take(sizeof(int) * n);
  s.tentative = (int*)take(sizeof(int) * n);
  s.lost = (int*)take(sizeof(int) * n);
  s.matched_det = (int*)take(sizeof(int) * n);
  s.matched_trk = (int*)take(sizeof(int) * n);
  s.d2r = (int*)take(sizeof(int) * n);
  s.order = (int*)take(sizeof(int) * n);
  s.ids = (long long*)take(sizeof(long long) * (size_t)M);
  s.is_matched = take((size_t)T);
  return s;
}

// one association stage: rows = tracks tidx[0..R), cols = detections pool[0..Cn) -> d2r[c] = row matched to column c
// or -1.  The cost matrix is filled by all 64 lanes, the assignment runs on lane 0.  An entry is cost_entry
// (ocsort_core.h), as in StTracker::assign (ocsort_tracker.cpp); what a track brings to its row (tb, ko, valid) is
// written out in both loops: as a shared routine it changes this kernel's code.
__device__ void assign_stage(const Cfg& cfg, DTrack* tracks, const int* tidx, int R, const int* pool, int Cn,
                             const float* dets, bool with_motion, Scratch& s, int lane) {
  for (int c = lane; c < Cn; c += 64) s.d2r[c] = -1;
  if (R == 0 || Cn == 0) {
    __syncthreads();
    return;
  }
  for (int e = lane; e < R * Cn; e += 64) {
    const int r = e / Cn, c = e - r * Cn;
    const DTrack& t = tracks[tidx[r]];
    float tb[4];
    if (with_motion) {
      const float m[4] = {(float)t.kf.mean[0], (float)t.kf.mean[1], (float)t.kf.mean[2], (float)t.kf.mean[3]};
      cxcyah_to_xyxy(m, tb);
    } else {
      for (int k = 0; k < 4; ++k) tb[k] = t.last_valid[k];
    }
    const float* ko = with_motion ? k_step_observation(t, cfg.vel_delta_t) : nullptr;
    const bool valid = with_motion && !t.vel_placeholder && (((ko[0] + ko[1]) + ko[2]) + ko[3]) != -4.0f;
    const float* dd = dets + (size_t)pool[c] * 8;
    const float dist = cost_entry(tb, dd, with_motion, ko, t.vel, valid, cfg.weight_iou_with_det_scores,
                                  cfg.vel_consist_weight);
    s.cost[(size_t)r * Cn + c] = (double)dist;
  }
  __syncthreads();
  __shared__ int lap_ctl[8];
  __shared__ double lap_ctld[2];
  Lap lap;
  lap.cost = s.cost; lap.R = R; lap.C = Cn; lap.n = R + Cn;
  lap.half = (1.0 - (double)cfg.match_iou_thr) / 2.0;
  lap.v = s.v; lap.d = s.d; lap.row_to_col = s.row_to_col; lap.col_to_row = s.col_to_row;
  lap.free_rows = s.free_rows; lap.pred = s.pred; lap.cols = s.cols; lap.once = s.once; lap.n_free = 0;
  lap.solve(lane, lap_ctl, lap_ctld);
  for (int c = lane; c < Cn; c += 64) s.d2r[c] = lap.col_to_row[c] < R ? lap.col_to_row[c] : -1;
  __syncthreads();
}

// status codes written per sequence
constexpr int kOk = 0, kTrackOverflow = 1, kDetOverflow = 2, kBadVideo = 3;

// The assignment's working arrays (37 B per row / column of the extended matrix) in the block's dynamic LDS instead of
// the sequence's slice of the global scratch.  In place, called by the kernels under `if (lap_in_lds)`: as a routine that
// RETURNS the scratch, the step kernel's dense-sequence time rose by 3 %.
__device__ __forceinline__ void assignment_arrays_in_lds(Scratch& s, int T, int M) {
  extern __shared__ double ba_dyn[];
  const size_t n = (size_t)T + M;
  char* base = reinterpret_cast<char*>(ba_dyn);
  size_t o = 0;
  auto take = [&](size_t bytes) { char* q = base + o; o += align8(bytes); return q; };
  s.v = (double*)take(sizeof(double) * n);
  s.d = (double*)take(sizeof(double) * n);
  s.row_to_col = (int*)take(sizeof(int) * n);
  s.col_to_row = (int*)take(sizeof(int) * n);
  s.free_rows = (int*)take(sizeof(int) * n);
  s.pred = (int*)take(sizeof(int) * n);
  s.cols = (int*)take(sizeof(int) * n);
  s.once = take(n);
}

// ONE frame of ONE sequence, by the sequence's wave: frame `frame_id` with the n detection rows `dets` -> the output
// rows / ids / count and the sequence's status.  Called once by assoc_step_kernel and once per frame by
// assoc_run_kernel.  Every exit is uniform across the wave (so is every __syncthreads()); a caller that goes on to
// another frame puts a barrier behind the call: it orders sh[], lap_ctl, the assignment's arrays and the state in
// global memory that lanes wrote here for the lanes that read them in the next frame.  cfg and s come by value: by
// reference the compiler keeps the scratch pointers in private memory (184 B of it against the 12 B the step kernel had).
// The step kernel's code is sensitive to this signature (scalar-register spills move): DESIGN.md 20 has the timings.
__device__ __forceinline__ void assoc_frame(const Cfg cfg, Scratch s, SeqHeader* hdr, DTrack* tracks, int frame_id,
                                            int n, const float* __restrict__ dets, float* __restrict__ orow,
                                            long long* __restrict__ oid, int* __restrict__ out_n,
                                            int* __restrict__ status, int lane) {
  const int T = cfg.max_tracks, M = cfg.max_dets;
  __shared__ int sh[12];   // n_tracks, n_order, n_cand, n_conf, n_tent, n_lost, n_matched, first_stage flag, status
  if (n < 0) {             // padding slot: this sequence has no frame in this step
    if (lane == 0) *out_n = -1;
    return;
  }
  if (frame_id != 0 && hdr->poisoned != kOk) {   // an earlier step overflowed: the state is not a tracker state any more
    if (lane == 0) { *out_n = 0; *status = hdr->poisoned; }
    return;
  }
  if (n > M) {
    if (lane == 0) { *out_n = 0; *status = kDetOverflow; hdr->poisoned = kDetOverflow; }
    return;
  }
  if (lane == 0) {
    if (frame_id == 0) { hdr->n_tracks = 0; hdr->num_tracks = 0; hdr->poisoned = kOk; }
    sh[0] = hdr->n_tracks;
    sh[8] = kOk;
    int n_order = 0;
    const bool first = hdr->n_tracks == 0 || n == 0;
    sh[7] = first;
    if (first) {
      for (int i = 0; i < n; ++i)
        if (dets[(size_t)i * 8 + 4] > cfg.init_track_thr) { s.order[n_order] = i; s.ids[n_order] = hdr->num_tracks++; ++n_order; }
      sh[1] = n_order;
    } else {
      int nc = 0;
      for (int i = 0; i < n; ++i) {
        if (enters_association(dets + (size_t)i * 8, cfg.obj_score_thr)) s.cand[nc++] = i;
      }
      int ncf = 0, nt = 0;
      for (int k = 0; k < hdr->n_tracks; ++k) {
        if (tracks[k].tentative) s.tentative[nt++] = k; else s.confirmed[ncf++] = k;
      }
      sh[2] = nc; sh[3] = ncf; sh[4] = nt; sh[6] = 0;
    }
  }
  __syncthreads();
  const bool first = sh[7];
  if (!first) {
    // 1. KF predict of the confirmed tracks (lanes over tracks)
    for (int q = lane; q < sh[3]; q += 64) {
      DTrack& t = tracks[s.confirmed[q]];
      if (t.last_frame != frame_id - 1) t.kf.mean[7] = 0;
      if (t.tracked) t.saved = t.kf;
      kf_predict(t.kf);
    }
    __syncthreads();
    // 2. confirmed, 3. tentative (OCM), 4. OCR on the still unmatched tracks
    for (int stage = 0; stage < 3; ++stage) {
      if (stage == 2) {
        if (lane == 0) {
          const int ntr = sh[0];
          for (int k = 0; k < ntr; ++k) s.is_matched[k] = 0;
          for (int i = 0; i < sh[6]; ++i) s.is_matched[s.matched_trk[i]] = 1;
          int nl = 0;
          for (int k = 0; k < ntr; ++k)
            if (!s.is_matched[k]) s.lost[nl++] = k;
          sh[5] = nl;
        }
        __syncthreads();
        if (sh[5] == 0) break;   // uniform
      }
      const int* tidx = stage == 0 ? s.confirmed : (stage == 1 ? s.tentative : s.lost);
      const int R = stage == 0 ? sh[3] : (stage == 1 ? sh[4] : sh[5]);
      assign_stage(cfg, tracks, tidx, R, s.cand, sh[2], dets, stage < 2, s, lane);
      if (lane == 0) {   // apply: matched pairs in column order, the rest stays in the pool
        int nm = sh[6], nr = 0;
        const int Cn = sh[2];
        for (int c = 0; c < Cn; ++c) {
          if (s.d2r[c] > -1) { s.matched_det[nm] = s.cand[c]; s.matched_trk[nm] = tidx[s.d2r[c]]; ++nm; }
          else s.rest[nr++] = s.cand[c];
        }
        for (int c = 0; c < nr; ++c) s.cand[c] = s.rest[c];
        sh[6] = nm; sh[2] = nr;
      }
      __syncthreads();
    }
    // 5. re-found tracks: smooth the KF over the gap (lanes over matches); unmatched tracks: mark lost
    if (lane == 0) {
      const int ntr = sh[0];
      for (int k = 0; k < ntr; ++k) s.is_matched[k] = 0;
      for (int i = 0; i < sh[6]; ++i) s.is_matched[s.matched_trk[i]] = 1;
    }
    __syncthreads();
    for (int i = lane; i < sh[6]; i += 64) {
      DTrack& t = tracks[s.matched_trk[i]];
      if (!t.tracked) online_smooth(t, dets + (size_t)s.matched_det[i] * 8);
    }
    for (int k = lane; k < sh[0]; k += 64)
      if (!s.is_matched[k]) { tracks[k].tracked = 0; push_obs(tracks[k], nullptr, cfg.vel_delta_t); }
    __syncthreads();
    if (lane == 0) {
      int n_order = 0;
      for (int i = 0; i < sh[6]; ++i) { s.order[n_order] = s.matched_det[i]; s.ids[n_order] = tracks[s.matched_trk[i]].id; ++n_order; }
      for (int c = 0; c < sh[2]; ++c) { s.order[n_order] = s.cand[c]; s.ids[n_order] = hdr->num_tracks++; ++n_order; }
      sh[1] = n_order;
    }
    __syncthreads();
  }
  // BaseTracker.update: feed every output row to its track.  Rows [0, n_matched) are the matched detections (their
  // track slot is known: no search by id), the rest start new tracks in fresh slots, in order.
  if (lane == 0) {
    int ntr = sh[0];
    const int n_order = sh[1];
    const int n_matched = first ? 0 : sh[6];
    for (int i = 0; i < n_order; ++i) {
      int k;
      if (i < n_matched) {
        k = s.matched_trk[i];
      } else if (ntr >= T) {
        sh[8] = kTrackOverflow;
        k = 0;
      } else {
        k = ntr++;
        tracks[k].id = -1;   // marks a slot to initialise below
      }
      s.tidx[i] = k;
    }
    if (sh[8] == kOk) hdr->n_tracks = ntr;
    sh[0] = ntr;
  }
  __syncthreads();
  if (sh[8] != kOk) {
    if (lane == 0) { *status = sh[8]; *out_n = 0; hdr->poisoned = sh[8]; }
    return;
  }
  for (int i = lane; i < sh[1]; i += 64) {
    const float* row = dets + (size_t)s.order[i] * 8;
    DTrack& t = tracks[s.tidx[i]];
    if (t.id < 0) init_track(t, s.ids[i], row, frame_id, cfg.vel_delta_t);
    else update_track(t, row, frame_id, cfg.num_tentatives, cfg.vel_delta_t);
    for (int e = 0; e < 8; ++e) orow[(size_t)i * 8 + e] = row[e];
    oid[i] = s.ids[i];
  }
  __syncthreads();
  // pop the invalid tracks: order-preserving compaction; lane 0 decides the destinations, the wave moves the records
  if (lane == 0) {
    int w = 0;
    const int ntr = sh[0];
    for (int k = 0; k < ntr; ++k) {
      const bool drop = is_dropped(&tracks[k], frame_id, cfg.num_frames_retain);
      s.rest[k] = drop ? -1 : w;
      if (!drop) ++w;
    }
    hdr->n_tracks = w;
    *out_n = sh[1];
  }
  __syncthreads();
  {
    constexpr int WORDS = (int)(sizeof(DTrack) / 8);
    static_assert(sizeof(DTrack) % 8 == 0, "DTrack is moved as 8-byte words");
    const int ntr = sh[0];
    for (int k = 0; k < ntr; ++k) {          // ascending: a destination is never a slot that is still to be read
      const int w = s.rest[k];
      if (w < 0 || w == k) continue;         // uniform
      const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&tracks[k]);
      unsigned long long* dst = reinterpret_cast<unsigned long long*>(&tracks[w]);
      for (int e = lane; e < WORDS; e += 64) dst[e] = src[e];
      __syncthreads();
    }
  }
}


__global__ __launch_bounds__(64) void assoc_step_kernel(Cfg cfg, const int* __restrict__ frame_ids,
                                                        const float* __restrict__ dets_all,
                                                        const int* __restrict__ counts, char* state_all,
                                                        size_t state_stride, char* scratch_all, size_t scratch_stride,
                                                        float* __restrict__ out_rows, long long* __restrict__ out_ids,
                                                        int* __restrict__ out_n, int* __restrict__ status,
                                                        int lap_in_lds) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int T = cfg.max_tracks, M = cfg.max_dets;
  SeqHeader* hdr = reinterpret_cast<SeqHeader*>(state_all + (size_t)b * state_stride);
  DTrack* tracks = reinterpret_cast<DTrack*>(reinterpret_cast<char*>(hdr) + sizeof(SeqHeader));
  Scratch s = carve(scratch_all + (size_t)b * scratch_stride, T, M);
  if (lap_in_lds) assignment_arrays_in_lds(s, T, M);
  assoc_frame(cfg, s, hdr, tracks, frame_ids[b], counts[b], dets_all + (size_t)b * M * 8, out_rows + (size_t)b * M * 8,
              out_ids + (size_t)b * M, out_n + b, status + b, lane);
}

// A whole recorded detection stream in ONE launch: the wave of sequence b walks frames [f_begin, f_end) of video
// video_of[b] (null: video b) and writes every frame's rows / ids / count.  Equal on the bits to f_end - f_begin launches
// of assoc_step_kernel on inputs gathered through video_of: the same routine on the same state, which lives in global
// memory between frames as it does between steps.  cfgs (null: `cfg` for every sequence) = the sequences' own option
// sets, read once per wave; the capacities are the tracker's.  Sequences that share a video read the same rows.
__global__ __launch_bounds__(64) void assoc_run_kernel(Cfg cfg, const Cfg* __restrict__ cfgs,
                                                       const int* __restrict__ frame_ids,
                                                       const float* __restrict__ dets_all,
                                                       const int* __restrict__ counts,
                                                       const int* __restrict__ video_of, int V, int F, int f_begin,
                                                       int f_end, char* state_all, size_t state_stride,
                                                       char* scratch_all, size_t scratch_stride,
                                                       float* __restrict__ out_rows, long long* __restrict__ out_ids,
                                                       int* __restrict__ out_n, int* __restrict__ status,
                                                       int lap_in_lds) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int T = cfg.max_tracks, M = cfg.max_dets;
  if (cfgs) {
    cfg = cfgs[b];
    cfg.max_tracks = T; cfg.max_dets = M;
  }
  const int v = video_of ? video_of[b] : b;
  if (v < 0 || v >= V) {   // nothing of this sequence is read or advanced
    if (lane == 0) {
      status[b] = kBadVideo;
      for (int f = f_begin; f < f_end; ++f) out_n[(size_t)b * F + f] = 0;
    }
    return;
  }
  SeqHeader* hdr = reinterpret_cast<SeqHeader*>(state_all + (size_t)b * state_stride);
  DTrack* tracks = reinterpret_cast<DTrack*>(reinterpret_cast<char*>(hdr) + sizeof(SeqHeader));
  Scratch s = carve(scratch_all + (size_t)b * scratch_stride, T, M);
  if (lap_in_lds) assignment_arrays_in_lds(s, T, M);
  for (int f = f_begin; f < f_end; ++f) {
    const size_t in = (size_t)v * F + f, on = (size_t)b * F + f;
    assoc_frame(cfg, s, hdr, tracks, frame_ids[in], counts[in], dets_all + in * M * 8, out_rows + on * M * 8,
                out_ids + on * M, out_n + on, status + b, lane);
    __syncthreads();   // the frame's writes (LDS, scratch, state) before the next frame's reads
  }
}

}  // namespace ba
}  // namespace st

// ---- C ABI ------------------------------------------------------------------------------------------------------------
struct StBatchedTracker {
  st::ba::Cfg cfg;
  int batch;
  size_t state_stride, scratch_stride;
  size_t lap_lds_bytes;   // dynamic LDS for the assignment's working arrays; 0 = they stay in the L2-resident scratch
  int lds_set, lds_set_run;
  // per-sequence option sets (st_batched_tracker_create_multi; empty otherwise) and their device copy, which the
  // first launch makes: creating a tracker touches no device
  std::vector<st::ba::Cfg> cfgs_host;
  st::ba::Cfg* cfgs_dev;
};

namespace {

// the tracker object of either create function; `cfg` has passed the checks
std::unique_ptr<StBatchedTracker> new_batched_tracker(const StTrackerConfig* cfg, int batch, int max_tracks, int max_dets) {
  using namespace st;
  auto t = std::make_unique<StBatchedTracker>();
  t->cfg = ba::Cfg{cfg->obj_score_thr, cfg->init_track_thr, cfg->match_iou_thr, cfg->vel_consist_weight,
                   cfg->weight_iou_with_det_scores, cfg->num_tentatives, cfg->vel_delta_t, cfg->num_frames_retain,
                   max_tracks, max_dets};
  t->batch = batch;
  t->state_stride = ba::align8(sizeof(ba::SeqHeader) + sizeof(ba::DTrack) * (size_t)max_tracks);
  t->scratch_stride = ba::scratch_bytes(max_tracks, max_dets);
  const size_t n = (size_t)max_tracks + max_dets;
  const size_t need = 2 * ba::align8(sizeof(double) * n) + 5 * ba::align8(sizeof(int) * n) + ba::align8(n);
  t->lap_lds_bytes = need <= 64 * 1024 ? need : 0;
  t->lds_set = t->lds_set_run = 0;
  t->cfgs_dev = nullptr;
  return t;
}

bool options_in_range(const StTrackerConfig* cfg) {
  return cfg->vel_delta_t >= 0 && cfg->vel_delta_t + 1 <= st::ba::WINCAP && cfg->num_tentatives >= 1 &&
         cfg->num_frames_retain >= 1;
}

int launch_run(StBatchedTracker* t, const int32_t* frame_ids_dev, const float* dets_dev, const int32_t* counts_dev,
               const int32_t* video_of_dev, int V, int F, int f_begin, int f_end, void* state_dev, void* scratch_dev,
               float* out_rows_dev, int64_t* out_ids_dev, int32_t* out_counts_dev, int32_t* status_dev,
               st_stream_t stream) {
  using namespace st;
  if (!t->cfgs_host.empty() && !t->cfgs_dev) {
    const size_t bytes = sizeof(ba::Cfg) * t->cfgs_host.size();
    ba::Cfg* p = nullptr;
    ST_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&p), bytes));
    const hipError_t e = hipMemcpy(p, t->cfgs_host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(p);
      ST_CHECK_HIP(e);
    }
    t->cfgs_dev = p;
  }
  ST_ENSURE_DYNAMIC_LDS(ba::assoc_run_kernel, t->lap_lds_bytes, t->lds_set_run);
  hipLaunchKernelGGL(ba::assoc_run_kernel, dim3(t->batch), dim3(64), t->lap_lds_bytes,
                     static_cast<hipStream_t>(stream), t->cfg, t->cfgs_dev, frame_ids_dev, dets_dev, counts_dev,
                     video_of_dev, V, F, f_begin, f_end, static_cast<char*>(state_dev), t->state_stride,
                     static_cast<char*>(scratch_dev), t->scratch_stride, out_rows_dev,
                     reinterpret_cast<long long*>(out_ids_dev), out_counts_dev, status_dev, t->lap_lds_bytes ? 1 : 0);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

}  // namespace

extern "C" int st_batched_tracker_create(const StTrackerConfig* cfg, int batch, int max_tracks, int max_dets,
                                         StBatchedTracker** out) {
  using namespace st;
  if (!cfg || !out) return set_error(ST_ERR_INVALID, "st_batched_tracker_create: null argument");
  ST_REQUIRE(cfg->struct_size == (int)sizeof(StTrackerConfig), "st_batched_tracker_create: struct_size mismatch");
  ST_REQUIRE(batch > 0 && max_tracks > 0 && max_dets > 0 && max_tracks + max_dets < (1 << 15),
             "st_batched_tracker_create: bad batch / capacities");
  ST_REQUIRE(options_in_range(cfg), "st_batched_tracker_create: vel_delta_t must be in [0, %d]", ba::WINCAP - 1);
  *out = new_batched_tracker(cfg, batch, max_tracks, max_dets).release();
  return ST_OK;
}

extern "C" int st_batched_tracker_create_multi(const StTrackerConfig* cfgs, int batch, int max_tracks, int max_dets,
                                               StBatchedTracker** out) {
  using namespace st;
  if (!cfgs || !out) return set_error(ST_ERR_INVALID, "st_batched_tracker_create_multi: null argument");
  ST_REQUIRE(batch > 0 && max_tracks > 0 && max_dets > 0 && max_tracks + max_dets < (1 << 15),
             "st_batched_tracker_create_multi: bad batch / capacities");
  for (int b = 0; b < batch; ++b) {   // every member, before any device call
    ST_REQUIRE(cfgs[b].struct_size == (int)sizeof(StTrackerConfig),
               "st_batched_tracker_create_multi: member %d: struct_size mismatch", b);
    ST_REQUIRE(options_in_range(&cfgs[b]), "st_batched_tracker_create_multi: member %d: vel_delta_t must be in [0, %d]",
               b, ba::WINCAP - 1);
  }
  auto t = new_batched_tracker(&cfgs[0], batch, max_tracks, max_dets);
  t->cfgs_host.resize((size_t)batch);
  for (int b = 0; b < batch; ++b)
    t->cfgs_host[b] = ba::Cfg{cfgs[b].obj_score_thr, cfgs[b].init_track_thr, cfgs[b].match_iou_thr, cfgs[b].vel_consist_weight,
                      cfgs[b].weight_iou_with_det_scores, cfgs[b].num_tentatives, cfgs[b].vel_delta_t,
                      cfgs[b].num_frames_retain, max_tracks, max_dets};
  *out = t.release();
  return ST_OK;
}

extern "C" int st_batched_tracker_destroy(StBatchedTracker* t) {
  if (t && t->cfgs_dev) (void)hipFree(t->cfgs_dev);
  delete t;
  return ST_OK;
}

extern "C" size_t st_batched_tracker_state_bytes(const StBatchedTracker* t) {
  return t ? t->state_stride * (size_t)t->batch : 0;
}
extern "C" size_t st_batched_tracker_scratch_bytes(const StBatchedTracker* t) {
  return t ? t->scratch_stride * (size_t)t->batch : 0;
}

extern "C" int st_batched_tracker_get_states(const StBatchedTracker* t, const void* state_dev, int b,
                                             StTrackState* out_host, int cap, int struct_size, int* n_tracks,
                                             long long* next_id, int* status, st_stream_t stream) {
  using namespace st;
  static_assert(ST_TRACK_WINDOW == ba::WINCAP, "StTrackState holds the device window");
  if (!t || !state_dev || !n_tracks) return set_error(ST_ERR_INVALID, "st_batched_tracker_get_states: null argument");
  ST_REQUIRE(struct_size == (int)sizeof(StTrackState), "st_batched_tracker_get_states: struct_size mismatch");
  ST_REQUIRE(b >= 0 && b < t->batch, "st_batched_tracker_get_states: sequence %d of a batch of %d", b, t->batch);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const char* seq = static_cast<const char*>(state_dev) + (size_t)b * t->state_stride;
  ba::SeqHeader hdr;
  ST_CHECK_HIP(hipMemcpyAsync(&hdr, seq, sizeof(hdr), hipMemcpyDeviceToHost, s));
  ST_CHECK_HIP(hipStreamSynchronize(s));
  if (status) *status = hdr.poisoned;
  if (next_id) *next_id = hdr.num_tracks;
  *n_tracks = 0;
  if (hdr.poisoned != ba::kOk) return ST_OK;   // the slots of an overflowed sequence are not a tracker state
  const int n = hdr.n_tracks;
  ST_REQUIRE(n >= 0 && n <= t->cfg.max_tracks, "st_batched_tracker_get_states: header holds %d tracks (max_tracks %d): "
             "not a state buffer of this tracker", n, t->cfg.max_tracks);
  ST_REQUIRE(cap >= n && (n == 0 || out_host), "st_batched_tracker_get_states: capacity %d < %d live tracks", cap, n);
  if (n == 0) return ST_OK;
  std::unique_ptr<ba::DTrack[]> tracks(new ba::DTrack[n]);
  ST_CHECK_HIP(hipMemcpyAsync(tracks.get(), seq + sizeof(ba::SeqHeader), sizeof(ba::DTrack) * (size_t)n,
                              hipMemcpyDeviceToHost, s));
  ST_CHECK_HIP(hipStreamSynchronize(s));
  for (int k = 0; k < n; ++k) {
    const ba::DTrack& d = tracks[k];
    StTrackState& o = out_host[k];
    std::memset(&o, 0, sizeof(o));
    o.struct_size = (int)sizeof(StTrackState);
    o.id = d.id;
    o.tentative = d.tentative != 0; o.tracked = d.tracked != 0; o.last_frame = d.last_frame; o.n_fed = d.n_fed;
    o.n_obs = d.n_obs; o.trailing_none = d.trailing_none; o.vel_placeholder = d.vel_placeholder != 0;
    o.win_len = d.win_len;                       // reported as stored; only the copy below is clamped
    std::memcpy(o.mean, d.kf.mean, sizeof(o.mean));
    std::memcpy(o.cov, d.kf.cov, sizeof(o.cov));
    std::memcpy(o.saved_mean, d.saved.mean, sizeof(o.saved_mean));
    std::memcpy(o.saved_cov, d.saved.cov, sizeof(o.saved_cov));
    for (int w = 0; w < std::min(std::max(d.win_len, 0), ba::WINCAP); ++w) {   // slots >= win_len: an earlier track's leftovers
      std::memcpy(o.win[w], d.win[w], sizeof(o.win[w]));
      o.win_valid[w] = d.win_valid[w] != 0;
    }
    std::memcpy(o.last_valid, d.last_valid, sizeof(o.last_valid));
    o.vel[0] = d.vel[0]; o.vel[1] = d.vel[1];
  }
  *n_tracks = n;
  return ST_OK;
}

extern "C" int st_batched_tracker_step(StBatchedTracker* t, const int32_t* frame_ids_dev, const float* dets_dev,
                                       const int32_t* counts_dev, void* state_dev, void* scratch_dev,
                                       float* out_rows_dev, int64_t* out_ids_dev, int32_t* out_counts_dev,
                                       int32_t* status_dev, st_stream_t stream) {
  using namespace st;
  if (!t) return set_error(ST_ERR_INVALID, "st_batched_tracker_step: null tracker");
  ST_REQUIRE(frame_ids_dev && dets_dev && counts_dev && state_dev && scratch_dev && out_rows_dev && out_ids_dev &&
                 out_counts_dev && status_dev,
             "st_batched_tracker_step: null pointer");
  if (!t->cfgs_host.empty())   // per-sequence options: the run kernel over one frame, video b = sequence b
    return launch_run(t, frame_ids_dev, dets_dev, counts_dev, nullptr, t->batch, 1, 0, 1, state_dev, scratch_dev,
                      out_rows_dev, out_ids_dev, out_counts_dev, status_dev, stream);
  ST_ENSURE_DYNAMIC_LDS(ba::assoc_step_kernel, t->lap_lds_bytes, t->lds_set);
  hipLaunchKernelGGL(ba::assoc_step_kernel, dim3(t->batch), dim3(64), t->lap_lds_bytes,
                     static_cast<hipStream_t>(stream), t->cfg, frame_ids_dev, dets_dev, counts_dev,
                     static_cast<char*>(state_dev), t->state_stride, static_cast<char*>(scratch_dev),
                     t->scratch_stride, out_rows_dev, reinterpret_cast<long long*>(out_ids_dev), out_counts_dev,
                     status_dev, t->lap_lds_bytes ? 1 : 0);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

extern "C" int st_batched_tracker_run(StBatchedTracker* t, const int32_t* frame_ids_dev, const float* dets_dev,
                                      const int32_t* counts_dev, const int32_t* video_of_dev, int V, int F, int f_begin,
                                      int f_end, void* state_dev, void* scratch_dev, float* out_rows_dev,
                                      int64_t* out_ids_dev, int32_t* out_counts_dev, int32_t* status_dev,
                                      st_stream_t stream) {
  using namespace st;
  if (!t) return set_error(ST_ERR_INVALID, "st_batched_tracker_run: null tracker");
  ST_REQUIRE(frame_ids_dev && dets_dev && counts_dev && video_of_dev && state_dev && scratch_dev && out_rows_dev &&
                 out_ids_dev && out_counts_dev && status_dev,
             "st_batched_tracker_run: null pointer");
  ST_REQUIRE(V > 0 && F > 0, "st_batched_tracker_run: %d videos x %d frames", V, F);
  ST_REQUIRE(f_begin >= 0 && f_begin < f_end && f_end <= F, "st_batched_tracker_run: bad frame range [%d, %d) of %d frames",
             f_begin, f_end, F);
  return launch_run(t, frame_ids_dev, dets_dev, counts_dev, video_of_dev, V, F, f_begin, f_end, state_dev, scratch_dev,
                    out_rows_dev, out_ids_dev, out_counts_dev, status_dev, stream);
}
