// COCO bbox evaluation (pycocotools COCOeval.evaluateImg / accumulate, restated: tests/coco_eval_ref.py and DESIGN.md
// "COCO bbox evaluation") on the device, behind st_coco_prepare / st_coco_match / st_coco_accumulate.
//
// Everything that decides a result is fp64 or an integer count, and every output is one IEEE division of two counts
// (or a copy), so the result does not depend on the launch geometry: no floating-point atomics, no reassociated sums.
// The launch count is fixed (it does not grow with the number of images) and nothing here waits for the device.
//
//   prepare     k_seg_offsets      rows are grouped by image (non-decreasing image index): first row of every image
//               k_prepare          one wave per (image, category): rank of every detection inside its group by counting
//                                  (score descending, arrival order on ties = a stable sort), the group's slots of the
//                                  score-ordered list `order`, and the 64-bit key of the global sort
//               k_npig             non-ignored ground truth per (category, area range): integer atomics
//   match       k_match            one wave per (image, category); lane p = (threshold, area range) pair p
//   accumulate  rocprim radix sort of (category, score descending) keys, stable, over slots that are already in
//               (image, category, rank) order = pycocotools' mergesort over its per-image concatenation
//               k_seg_offsets      first sorted position of every category
//               k_gather_sorted    rank, tables and score of every sorted position, contiguous
//               k_accumulate       one workgroup per (threshold, category, area range, max_dets entry)
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include <climits>
#include <cmath>
#include <vector>

#include "st_common.h"

namespace {

constexpr int kMaxGt = ST_COCO_MAX_GT;   // ground-truth boxes per (image, category) group held in LDS
constexpr int kMaxPairs = 64;            // T * A: one lane of a wave each
constexpr int kMaxRec = 128;             // recall points
constexpr int kAccThreads = 1024;

enum : int {
  kBadDetImg = 1,    // det_img decreasing or outside [0, num_images)
  kBadGtImg = 2,     // gt_img likewise
  kNonFinite = 4,    // a detection box or score that is NaN / Inf
  kBadLabel = 8,     // a detection label outside [0, num_cats)
  kGtOverflow = 16,  // a group with more than kMaxGt ground-truth boxes
  kBadGtCat = 32,    // a ground-truth category outside [0, num_cats)
};

typedef unsigned long long u64;

// off[j] = first row i with idx[i] >= j, for j = 0 .. nseg (off[nseg] = n).  idx: int rows, or the high word of the
// sorted 64-bit keys (keys != nullptr).  One thread per row boundary i = 0 .. n.
__global__ void k_seg_offsets(const int* __restrict__ idx, const u64* __restrict__ keys, int n, int nseg,
                              int* __restrict__ off, int* __restrict__ status, int bad_bit) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  auto at = [&](int r) -> int { return keys ? (int)(keys[r] >> 32) : idx[r]; };
  int prev = i == 0 ? -1 : at(i - 1);
  int cur = i == n ? nseg : at(i);
  if (i < n && (cur < 0 || cur >= nseg)) atomicOr(&status[0], bad_bit);
  if (i > 0 && (prev < 0 || prev >= nseg)) prev = nseg;   // flagged by its own thread; write nothing here
  if (cur < prev) {
    atomicOr(&status[0], bad_bit);
    return;
  }
  if (cur > nseg) cur = nseg;
  for (int j = prev + 1; j <= cur; ++j) off[j] = i;
}

__device__ inline unsigned score_key_desc(float s) {
  if (s == 0.0f) s = 0.0f;                         // -0 and +0 compare equal: one key
  unsigned u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending in the float order
  return ~u;                                       // descending
}

__global__ __launch_bounds__(64) void k_prepare(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ labels,
    const int* __restrict__ det_off, int K, int max_det_last, int D, int* __restrict__ det_rank,
    u64* __restrict__ det_matched, u64* __restrict__ det_ignored, int* __restrict__ order, u64* __restrict__ keys,
    int* __restrict__ status) {
  if (status[0] & (kBadDetImg | kBadGtImg)) return;
  const int img = blockIdx.x / K, k = blockIdx.x % K, lane = threadIdx.x;
  const int s = det_off[img], e = det_off[img + 1];
  if (k == 0) {   // validation, once per row
    for (int i = s + lane; i < e; i += 64) {
      bool ok = isfinite(scores[i]);
      for (int c = 0; c < 4; ++c) ok = ok && isfinite(boxes[4 * (size_t)i + c]);
      const int l = labels[i];
      if (!ok) { atomicOr(&status[0], kNonFinite); atomicMax(&status[1], D - i); }
      if (l < 0 || l >= K) {
        atomicOr(&status[0], kBadLabel);
        atomicMax(&status[2], D - i);
        det_rank[i] = -1; det_matched[i] = 0; det_ignored[i] = 0;
      }
    }
  }
  int below = 0;   // rows of this image whose slots come before this group's: smaller label, or no valid label
  for (int i = s + lane; i < e; i += 64) {
    const int l = labels[i];
    below += (l >= 0 && l < k) ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) below += __shfl_xor(below, o);
  for (int i = s + lane; i < e; i += 64) {
    if (labels[i] != k) continue;
    const float sc = scores[i];
    int rank = 0;
    for (int j = s; j < e; ++j) {
      const float sj = scores[j];
      rank += (labels[j] == k && (sj > sc || (sj == sc && j < i))) ? 1 : 0;
    }
    const bool kept = rank < max_det_last;
    const int slot = s + below + rank;
    det_rank[i] = kept ? rank : -1;
    if (!kept) { det_matched[i] = 0; det_ignored[i] = 0; }
    order[slot] = i;
    keys[slot] = kept ? (((u64)k << 32) | score_key_desc(sc)) : (((u64)K << 32) | 0xffffffffu);
  }
  // rows without a valid label take the image's last slots (the launch fails anyway; the sort stays in bounds)
  if (k == 0) {
    int nvalid = 0;
    for (int i = s + lane; i < e; i += 64) nvalid += (labels[i] >= 0 && labels[i] < K) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) nvalid += __shfl_xor(nvalid, o);
    if (nvalid < e - s && lane == 0) {
      int slot = s + nvalid;
      for (int i = s; i < e; ++i)
        if (labels[i] < 0 || labels[i] >= K) { order[slot] = i; keys[slot] = ((u64)K << 32) | 0xffffffffu; ++slot; }
    }
  }
}

__global__ void k_npig(const double* __restrict__ gt_area, const int* __restrict__ gt_crowd,
                       const int* __restrict__ gt_cat, int G, int K, int A, const double* __restrict__ area_rng,
                       int* __restrict__ npig, int* __restrict__ status) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int k = gt_cat[g];
  if (k < 0 || k >= K) { atomicOr(&status[0], kBadGtCat); return; }
  if (gt_crowd[g]) return;
  const double ar = gt_area[g];
  for (int a = 0; a < A; ++a)
    if (!(ar < area_rng[2 * a] || ar > area_rng[2 * a + 1])) atomicAdd(&npig[k * A + a], 1);
}

// One wave per (image, category).  The group's ground truth sits in LDS; a detection's IoU row is recomputed per
// detection (kMaxGt doubles), never a D x G table.  Lane p walks the ground truth for pair p = t * A + a.
__global__ __launch_bounds__(64) void k_match(
    const float* __restrict__ boxes, const int* __restrict__ labels, const int* __restrict__ det_off,
    const int* __restrict__ order, const double* __restrict__ gt_boxes, const double* __restrict__ gt_area,
    const int* __restrict__ gt_crowd, const int* __restrict__ gt_cat, const int* __restrict__ gt_off, int K, int T,
    int A, int max_det_last, const double* __restrict__ iou_thrs, const double* __restrict__ area_rng,
    u64* __restrict__ det_matched, u64* __restrict__ det_ignored, int* __restrict__ status) {
  __shared__ double gx[kMaxGt], gy[kMaxGt], gw[kMaxGt], gh[kMaxGt], giou[kMaxGt];
  __shared__ u64 gtm[kMaxGt];          // bit p: matched for pair p
  __shared__ unsigned gflag[kMaxGt];   // bit 0 crowd, bit 1 + a: ignored for area range a
  if (status[0]) return;
  const int img = blockIdx.x / K, k = blockIdx.x % K, lane = threadIdx.x;
  const int s = det_off[img], e = det_off[img + 1];
  int below = 0, n = 0;
  for (int i = s + lane; i < e; i += 64) {
    const int l = labels[i];
    below += l < k ? 1 : 0;
    n += l == k ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) { below += __shfl_xor(below, o); n += __shfl_xor(n, o); }
  if (n == 0) return;      // ground truth alone leaves nothing to write per detection
  const int nd = n < max_det_last ? n : max_det_last;

  // the group's ground truth, in arrival order
  const int gs = gt_off[img], ge = gt_off[img + 1];
  int ng = 0;
  for (int b = gs; b < ge; b += 64) {
    const int g = b + lane;
    const bool mine = g < ge && gt_cat[g] == k;
    const u64 m = __ballot(mine);
    const int pos = ng + __popcll(m & ((1ull << lane) - 1ull));
    if (mine && pos < kMaxGt) {
      gx[pos] = gt_boxes[4 * (size_t)g]; gy[pos] = gt_boxes[4 * (size_t)g + 1];
      gw[pos] = gt_boxes[4 * (size_t)g + 2]; gh[pos] = gt_boxes[4 * (size_t)g + 3];
      const double ar = gt_area[g];
      const unsigned crowd = gt_crowd[g] ? 1u : 0u;
      unsigned f = crowd;
      for (int a = 0; a < A; ++a)
        if (crowd || ar < area_rng[2 * a] || ar > area_rng[2 * a + 1]) f |= 2u << a;
      gflag[pos] = f;
      gtm[pos] = 0;
    }
    ng += __popcll(m);
  }
  if (ng > kMaxGt) {
    if (lane == 0) atomicOr(&status[0], kGtOverflow);
    return;
  }
  const int T_A = T * A;
  const bool active = lane < T_A;
  const int t = active ? lane / A : 0, a = active ? lane % A : 0;
  const double thr = fmin(iou_thrs[t], 1 - 1e-10);
  const double alo = area_rng[2 * a], ahi = area_rng[2 * a + 1];
  const unsigned ign_bit = 2u << a;
  const u64 my_bit = 1ull << lane;
  __syncthreads();

  for (int r = 0; r < nd; ++r) {
    const int row = order[s + below + r];
    const double dx = (double)boxes[4 * (size_t)row], dy = (double)boxes[4 * (size_t)row + 1];
    const double dw = (double)boxes[4 * (size_t)row + 2] - dx, dh = (double)boxes[4 * (size_t)row + 3] - dy;
    const double da = dw * dh;
    for (int g = lane; g < ng; g += 64) {
      double o = 0.0;
      const double iw = fmin(dx + dw, gx[g] + gw[g]) - fmax(dx, gx[g]);
      if (iw > 0) {
        const double ih = fmin(dy + dh, gy[g] + gh[g]) - fmax(dy, gy[g]);
        if (ih > 0) {
          const double inter = iw * ih;
          const double uni = (gflag[g] & 1u) ? da : da + gw[g] * gh[g] - inter;
          o = inter / uni;
        }
      }
      giou[g] = o;
    }
    __syncthreads();
    double best = thr;
    int m = -1;
    for (int pass = 0; pass < 2; ++pass) {       // the non-ignored boxes, then (nothing taken yet) the ignored ones
      const bool walk = active && m < 0;
      if (!__any(walk)) break;
      if (walk) {
        const unsigned want = pass ? ign_bit : 0u;
        for (int g = 0; g < ng; ++g) {
          const unsigned f = gflag[g];
          if ((f & ign_bit) != want) continue;
          if ((gtm[g] & my_bit) && !(f & 1u)) continue;
          const double o = giou[g];
          if (o < best) continue;
          best = o;
          m = g;
        }
      }
    }
    const bool matched = active && m >= 0;
    bool ign = false;
    if (matched) {
      ign = (gflag[m] & ign_bit) != 0;
      atomicOr(&gtm[m], my_bit);
    } else if (active) {
      ign = da < alo || da > ahi;
    }
    const u64 mm = __ballot(matched), im = __ballot(ign);
    if (lane == 0) { det_matched[row] = mm; det_ignored[row] = im; }
    __syncthreads();
  }
}

// The tables in sorted order, once: k_accumulate then streams them instead of chasing slot -> row -> table per position.
__global__ void k_gather_sorted(const int* __restrict__ sorted_rows, int D, const int* __restrict__ det_rank,
                                const u64* __restrict__ det_matched, const u64* __restrict__ det_ignored,
                                const float* __restrict__ det_scores, int* __restrict__ s_rank,
                                u64* __restrict__ s_matched, u64* __restrict__ s_ignored, float* __restrict__ s_score,
                                const int* __restrict__ status) {
  if (status[0]) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D) return;
  const int row = sorted_rows[i];
  s_rank[i] = det_rank[row];
  s_matched[i] = det_matched[row];
  s_ignored[i] = det_ignored[row];
  s_score[i] = det_scores[row];
}

// number of recall thresholds <= x (rec ascending)
__device__ inline int rec_upper(const double* rec, int R, double x) {
  int lo = 0, hi = R;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rec[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One workgroup per (t, k, a, m).  Pass 1 counts tp / fp of the category's sorted list; pass 2 walks it from the end
// in chunks of kAccThreads: counts at a position = totals - what lies behind it, precision = one division, running
// maximum from the end; the first position that reaches a recall point takes the maximum and the score there.
__global__ __launch_bounds__(kAccThreads) void k_accumulate(
    const int* __restrict__ cat_start, const int* __restrict__ s_rank, const u64* __restrict__ s_matched,
    const u64* __restrict__ s_ignored, const float* __restrict__ s_score, const int* __restrict__ npig_all, int T, int K, int A, int M, int R, const int* __restrict__ max_dets,
    const double* __restrict__ rec_thrs, double* __restrict__ precision, double* __restrict__ recall,
    double* __restrict__ scores_out, const int* __restrict__ status) {
  __shared__ double rec[kMaxRec], q[kMaxRec], qs[kMaxRec];
  __shared__ int first[kMaxRec];
  __shared__ double prbuf[kAccThreads];
  __shared__ int wtp[kAccThreads / 64], wfp[kAccThreads / 64];
  __shared__ double wmax[kAccThreads / 64];
  __shared__ int tot[2];
  if (status[0]) return;
  int b = blockIdx.x;
  const int m = b % M; b /= M;
  const int a = b % A; b /= A;
  const int k = b % K; b /= K;
  const int t = b;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int np = npig_all[k * A + a];
  const size_t rec_idx = (((size_t)t * K + k) * A + a) * M + m;
  auto out_idx = [&](int r) -> size_t { return ((((size_t)t * R + r) * K + k) * A + a) * M + m; };
  if (np == 0) {
    if (tid < R) { precision[out_idx(tid)] = -1.0; scores_out[out_idx(tid)] = -1.0; }
    if (tid == 0) recall[rec_idx] = -1.0;
    return;
  }
  const int s = cat_start[k], e = cat_start[k + 1];
  if (e <= s) {
    if (tid < R) { precision[out_idx(tid)] = 0.0; scores_out[out_idx(tid)] = 0.0; }
    if (tid == 0) recall[rec_idx] = 0.0;
    return;
  }
  const int lim = max_dets[m];
  const u64 bit = 1ull << (t * A + a);
  if (tid < R) { rec[tid] = rec_thrs[tid]; q[tid] = 0.0; qs[tid] = 0.0; first[tid] = -1; }
  if (tid < 2) tot[tid] = 0;
  __syncthreads();
  {
    int ntp = 0, nfp = 0;
    for (int i = s + tid; i < e; i += kAccThreads) {
      if (s_rank[i] < lim && !(s_ignored[i] & bit)) {
        if (s_matched[i] & bit) ++ntp; else ++nfp;
      }
    }
    for (int o = 32; o > 0; o >>= 1) { ntp += __shfl_xor(ntp, o); nfp += __shfl_xor(nfp, o); }
    if (lane == 0) { atomicAdd(&tot[0], ntp); atomicAdd(&tot[1], nfp); }
  }
  __syncthreads();
  const int TP = tot[0], FP = tot[1];
  const double dnp = (double)np;
  if (tid == 0) recall[rec_idx] = (double)TP / dnp;
  const double eps = 2.220446049250313e-16;   // np.spacing(1) = 2^-52
  const int nchunks = (e - s + kAccThreads - 1) / kAccThreads;
  int behind_tp = 0, behind_fp = 0;   // counts at positions after the current chunk
  double behind_max = 0.0;
  for (int ch = nchunks - 1; ch >= 0; --ch) {
    const int cb = s + ch * kAccThreads;
    const int i = cb + tid;
    bool tp = false, fp = false;
    if (i < e && s_rank[i] < lim && !(s_ignored[i] & bit)) {
      tp = (s_matched[i] & bit) != 0;
      fp = !tp;
    }
    const u64 mt = __ballot(tp), mf = __ballot(fp);
    if (lane == 0) { wtp[wave] = __popcll(mt); wfp[wave] = __popcll(mf); }
    __syncthreads();
    const u64 higher = lane == 63 ? 0ull : (~0ull << (lane + 1));
    int after_tp = behind_tp + __popcll(mt & higher), after_fp = behind_fp + __popcll(mf & higher);
    int chunk_tp = 0, chunk_fp = 0;
    for (int w = 0; w < kAccThreads / 64; ++w) {
      chunk_tp += wtp[w]; chunk_fp += wfp[w];
      if (w > wave) { after_tp += wtp[w]; after_fp += wfp[w]; }
    }
    const int ctp = TP - after_tp, cfp = FP - after_fp;    // inclusive running counts at position i
    double pr = 0.0;
    if (i < e) pr = (double)ctp / ((double)cfp + (double)ctp + eps);
    prbuf[tid] = pr;
    if (tp) {   // the first position whose count is ctp: it is where rc first reaches ctp / npig
      const int lo = rec_upper(rec, R, (double)(ctp - 1) / dnp), hi = rec_upper(rec, R, (double)ctp / dnp);
      for (int r = lo; r < hi; ++r) first[r] = i;
    }
    if (i == s) {   // recall points that a count of zero already reaches (r = 0): the first position
      const int hi = rec_upper(rec, R, 0.0 / dnp);
      for (int r = 0; r < hi; ++r) first[r] = s;
    }
    double mx = pr;
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if (lane == 0) wmax[wave] = mx;
    __syncthreads();
    if (tid < R) {
      const int f = first[tid];
      if (f >= cb && f < cb + kAccThreads) {
        double v = behind_max;
        const int end = (e - cb) < kAccThreads ? (e - cb) : kAccThreads;
        for (int j = f - cb; j < end; ++j) v = fmax(v, prbuf[j]);
        q[tid] = v;
        qs[tid] = (double)s_score[f];
      }
    }
    for (int w = 0; w < kAccThreads / 64; ++w) behind_max = fmax(behind_max, wmax[w]);
    behind_tp += chunk_tp;
    behind_fp += chunk_fp;
    __syncthreads();
  }
  if (tid < R) { precision[out_idx(tid)] = q[tid]; scores_out[out_idx(tid)] = qs[tid]; }
}

struct Workspace {
  int *det_off, *gt_off, *order, *sorted_rows, *cat_start, *max_dets, *s_rank;
  u64 *keys, *keys_sorted, *s_matched, *s_ignored;
  float* s_score;
  void* sort_tmp;
  size_t sort_tmp_bytes, total;
};

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

int key_bits(int K) {
  int bits = 1;
  while ((1 << bits) <= K) ++bits;   // categories 0 .. K (K = dropped rows)
  return 32 + bits;
}

int carve(const StCocoArgs* a, void* base, Workspace* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? (char*)base + off : nullptr; off += align256(bytes); return (void*)p; };
  const size_t D = (size_t)a->num_dets, I = (size_t)a->num_images;
  w->det_off = (int*)take((I + 1) * sizeof(int));
  w->gt_off = (int*)take((I + 1) * sizeof(int));
  w->order = (int*)take((D + 1) * sizeof(int));
  w->sorted_rows = (int*)take((D + 1) * sizeof(int));
  w->cat_start = (int*)take(((size_t)a->num_cats + 2) * sizeof(int));
  w->max_dets = (int*)take((size_t)a->M * sizeof(int));
  w->keys = (u64*)take((D + 1) * sizeof(u64));
  w->keys_sorted = (u64*)take((D + 1) * sizeof(u64));
  w->s_rank = (int*)take((D + 1) * sizeof(int));
  w->s_score = (float*)take((D + 1) * sizeof(float));
  w->s_matched = (u64*)take((D + 1) * sizeof(u64));
  w->s_ignored = (u64*)take((D + 1) * sizeof(u64));
  w->sort_tmp_bytes = 0;
  if (D > 0) {
    hipError_t e = rocprim::radix_sort_pairs(nullptr, w->sort_tmp_bytes, (u64*)nullptr, (u64*)nullptr, (int*)nullptr,
                                             (int*)nullptr, D, 0, key_bits(a->num_cats), (hipStream_t) nullptr);
    if (e != hipSuccess) return st::set_error(ST_ERR_HIP, "rocprim::radix_sort_pairs (size query): %s", hipGetErrorString(e));
  }
  w->sort_tmp = take(w->sort_tmp_bytes + 256);
  w->total = off;
  return ST_OK;
}

int validate(const StCocoArgs* a) {
  ST_REQUIRE(a != nullptr, "st_coco: args is NULL");
  ST_REQUIRE(a->struct_size == (int)sizeof(StCocoArgs), "st_coco: struct_size %d != %d", a->struct_size,
             (int)sizeof(StCocoArgs));
  ST_REQUIRE(a->num_images >= 1 && a->num_cats >= 1 && a->num_dets >= 0 && a->num_gts >= 0,
             "st_coco: num_images %d / num_cats %d must be >= 1, num_dets %d / num_gts %d >= 0", a->num_images,
             a->num_cats, a->num_dets, a->num_gts);
  ST_REQUIRE((long long)a->num_images * a->num_cats < (1ll << 30), "st_coco: num_images x num_cats too large");
  ST_REQUIRE(a->T >= 1 && a->A >= 1 && a->T * a->A <= kMaxPairs && a->A <= 16,
             "st_coco: T x A = %d x %d pairs, one lane each: at most %d (A <= 16)", a->T, a->A, kMaxPairs);
  ST_REQUIRE(a->M >= 1 && a->M <= 16 && a->R >= 1 && a->R <= kMaxRec, "st_coco: M %d must be 1..16, R %d 1..%d", a->M,
             a->R, kMaxRec);
  ST_REQUIRE(a->max_dets != nullptr && a->max_dets[0] >= 1, "st_coco: max_dets must be >= 1");
  for (int m = 1; m < a->M; ++m)
    ST_REQUIRE(a->max_dets[m] >= a->max_dets[m - 1], "st_coco: max_dets must not decrease (the match is made at the last)");
  ST_REQUIRE(a->ws != nullptr, "st_coco: workspace is NULL");
  return ST_OK;
}

}  // namespace

extern "C" {

int st_coco_max_gt(void) { return kMaxGt; }

size_t st_coco_workspace_bytes(const StCocoArgs* args) {
  if (!args || args->struct_size != (int)sizeof(StCocoArgs) || args->num_dets < 0 || args->num_images < 1 ||
      args->num_cats < 1 || args->M < 1)
    return 0;
  Workspace w;
  if (carve(args, nullptr, &w) != ST_OK) return 0;
  return w.total;
}

int st_coco_prepare(const StCocoArgs* a, st_stream_t stream_) {
  ST_CHECK(validate(a));
  hipStream_t stream = (hipStream_t)stream_;
  Workspace w;
  ST_CHECK(carve(a, a->ws, &w));
  ST_REQUIRE(a->ws_bytes >= w.total, "st_coco: workspace %zu < %zu bytes", a->ws_bytes, w.total);
  // the ground truth is the host's: refuse what the match kernel cannot hold before anything is launched
  ST_REQUIRE(a->num_gts == 0 || (a->gt_img_host && a->gt_cat_host), "st_coco: host copies of gt_img / gt_cat are NULL");
  {
    int run = 0, prev_img = -1;
    std::vector<int> counts((size_t)a->num_cats, 0);
    int* per_cat = counts.data();
    for (int g = 0; g < a->num_gts; ++g) {
      const int im = a->gt_img_host[g], c = a->gt_cat_host[g];
      ST_REQUIRE(im >= prev_img && im < a->num_images, "st_coco: gt_img must be non-decreasing in [0, %d) (row %d: %d)",
                 a->num_images, g, im);
      ST_REQUIRE(c >= 0 && c < a->num_cats, "st_coco: gt_cat[%d] = %d outside [0, %d)", g, c, a->num_cats);
      if (im != prev_img) { for (int k = 0; k < a->num_cats; ++k) per_cat[k] = 0; prev_img = im; }
      run = ++per_cat[c];
      ST_REQUIRE(run <= kMaxGt, "st_coco: image %d has more than %d ground-truth boxes of category %d: "
                 "a launch holds a group's ground truth in LDS (st_coco_max_gt)", im, kMaxGt, c);
    }
  }
  const int D = a->num_dets, G = a->num_gts, I = a->num_images, K = a->num_cats;
  ST_CHECK_HIP(hipMemsetAsync(a->status, 0, 4 * sizeof(int), stream));
  ST_CHECK_HIP(hipMemsetAsync(a->npig, 0, (size_t)K * a->A * sizeof(int), stream));
  ST_CHECK_HIP(hipMemcpyAsync(w.max_dets, a->max_dets, (size_t)a->M * sizeof(int), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(k_seg_offsets, dim3(st::ceil_div(D + 1, 256)), dim3(256), 0, stream, a->det_img, (const u64*)nullptr,
                     D, I, w.det_off, a->status, (int)kBadDetImg);
  hipLaunchKernelGGL(k_seg_offsets, dim3(st::ceil_div(G + 1, 256)), dim3(256), 0, stream, a->gt_img, (const u64*)nullptr,
                     G, I, w.gt_off, a->status, (int)kBadGtImg);
  hipLaunchKernelGGL(k_prepare, dim3(I * K), dim3(64), 0, stream, a->det_boxes, a->det_scores, a->det_labels, w.det_off,
                     K, a->max_dets[a->M - 1], D, a->det_rank, a->det_matched, a->det_ignored, w.order, w.keys, a->status);
  if (G > 0)
    hipLaunchKernelGGL(k_npig, dim3(st::ceil_div(G, 256)), dim3(256), 0, stream, a->gt_area, a->gt_crowd, a->gt_cat, G,
                       K, a->A, a->area_rng, a->npig, a->status);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

int st_coco_match(const StCocoArgs* a, st_stream_t stream_) {
  ST_CHECK(validate(a));
  hipStream_t stream = (hipStream_t)stream_;
  Workspace w;
  ST_CHECK(carve(a, a->ws, &w));
  ST_REQUIRE(a->ws_bytes >= w.total, "st_coco: workspace %zu < %zu bytes", a->ws_bytes, w.total);
  hipLaunchKernelGGL(k_match, dim3(a->num_images * a->num_cats), dim3(64), 0, stream, a->det_boxes, a->det_labels,
                     w.det_off, w.order, a->gt_boxes, a->gt_area, a->gt_crowd, a->gt_cat, w.gt_off, a->num_cats, a->T,
                     a->A, a->max_dets[a->M - 1], a->iou_thrs, a->area_rng, a->det_matched, a->det_ignored, a->status);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

int st_coco_accumulate(const StCocoArgs* a, st_stream_t stream_) {
  ST_CHECK(validate(a));
  hipStream_t stream = (hipStream_t)stream_;
  Workspace w;
  ST_CHECK(carve(a, a->ws, &w));
  ST_REQUIRE(a->ws_bytes >= w.total, "st_coco: workspace %zu < %zu bytes", a->ws_bytes, w.total);
  const int D = a->num_dets, K = a->num_cats;
  if (D > 0) {
    size_t tmp = w.sort_tmp_bytes;
    ST_CHECK_HIP(rocprim::radix_sort_pairs(w.sort_tmp, tmp, w.keys, w.keys_sorted, w.order, w.sorted_rows, (size_t)D, 0,
                                           key_bits(K), stream));
  }
  hipLaunchKernelGGL(k_seg_offsets, dim3(st::ceil_div(D + 1, 256)), dim3(256), 0, stream, (const int*)nullptr,
                     (const u64*)w.keys_sorted, D, K + 1, w.cat_start, a->status, (int)kBadLabel);
  if (D > 0)
    hipLaunchKernelGGL(k_gather_sorted, dim3(st::ceil_div(D, 256)), dim3(256), 0, stream, w.sorted_rows, D, a->det_rank,
                       a->det_matched, a->det_ignored, a->det_scores, w.s_rank, w.s_matched, w.s_ignored, w.s_score,
                       a->status);
  hipLaunchKernelGGL(k_accumulate, dim3(a->T * K * a->A * a->M), dim3(kAccThreads), 0, stream, w.cat_start, w.s_rank,
                     w.s_matched, w.s_ignored, w.s_score, a->npig, a->T, K, a->A, a->M, a->R,
                     w.max_dets, a->rec_thrs, a->precision, a->recall, a->scores, a->status);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

}  // extern "C"
