// Dense stereo evaluation (stereo_eval.stereo_error_stats / StereoMetric): the error of a disparity map
// against a ground-truth depth or disparity map, accumulated per (frame, region, depth bin) CELL.  No reference function
// exists; the per-pixel definitions are listed in include/stereotrack.h section 22 and restated, operation by operation,
// in tests/stereo_eval_ref.py (numpy float32 / float64), to which this file is held: counts and histogram equal, the
// fp64 sums up to the order of summation.
//
// One pass over the two maps.  The pixels of frame n inside its extent (h_n, w_n) are cut into UNITS of 4 consecutive
// columns of one row (the last unit of a row is short when w_n % 4 != 0); workgroup g of the frame owns the units
// [g * SE_UNITS, (g + 1) * SE_UNITS) and nothing else, thread t takes unit g * SE_UNITS + it * 256 + t in turn `it`.  A
// whole unit is fetched with one 16-byte load per map when the rows are 16-byte aligned (VEC), a short one and every
// unit of an unaligned map with scalar loads.  Nothing outside plane 0 / the extent / the counted box rows is read.
//
//   integers   per turn and per cell present in the wave: every lane packs its (at most 4) pixels' counter bits into
//              10-bit fields, a butterfly over the wave adds them, lane 0 adds the wave's totals to the wave's own LDS
//              row.  The histogram goes through LDS atomics (512 bins per cell) and then, per non-empty bin, one 64-bit
//              integer atomic on the output, which the entry point zeroed.  Integer sums do not depend on the order.
//   fp64 sums  no floating-point atomics anywhere.  A lane adds its own pixels of the cell in column order, the same
//              butterfly adds the 64 lanes (a fixed tree), lane 0 adds the result to the wave's LDS row in turn order,
//              the four rows are added in wave order and ONE partial per cell goes to the workspace; a second small
//              launch adds the partials of a frame in workgroup order.  The order depends on the inputs and the launch
//              geometry alone: two calls on the same inputs return the same bytes.
//
// Workgroups past the end of a frame's extent write zero partials, so the second launch reads only defined memory and
// defines every cell of `counts` and `sums`; `hist` is zeroed on the stream before the first launch.
#include <algorithm>
#include <cstdint>

#include "st_common.h"

namespace st {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SE_THREADS = 256;
constexpr int SE_WAVES = SE_THREADS / 64;
constexpr int SE_TURNS = 4;
constexpr int SE_UNITS = SE_THREADS * SE_TURNS;                  // units (of 4 pixels) per workgroup
constexpr int SE_MAX_CELLS = 2 * ST_STEREO_EVAL_MAX_BINS;         // region x depth bin
constexpr int SE_MAX_COUNTS = ST_STEREO_EVAL_MAX_THRESHOLDS + 6;  // n_gt, n_both, bad[T], d1, delta[3]
constexpr int SE_SUMS = ST_STEREO_EVAL_NUM_SUMS;
constexpr int SE_HIST = ST_STEREO_EVAL_HIST_BINS;
constexpr int SE_WORDS = (SE_MAX_COUNTS + 2) / 3;                 // three 10-bit counters per 32-bit word
constexpr int SE_AHEAD = 16;                                      // partials the second launch keeps in flight per thread

static_assert(SE_MAX_CELLS * SE_MAX_COUNTS <= SE_THREADS, "one thread per (cell, counter) in the epilogue");

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// What one pixel contributes.  cell < 0: no valid ground truth (nothing is counted).  bits: bit j = counter j of the
// cell (0 n_gt, 1 n_both, 2 .. T+1 bad, T+2 d1, T+3 .. T+5 delta).  term[] and bin are defined when bit 1 is set.
struct SePixel {
  int cell;
  unsigned bits;
  int bin;
  double term[SE_SUMS];
};

__device__ __forceinline__ void se_pixel(const StStereoEvalArgs& a, float p, float g, int x, int y, const float* sbox,
                                         int nb, SePixel& o) {
  o.cell = -1;
  o.bits = 0;
  o.bin = 0;
#pragma unroll
  for (int s = 0; s < SE_SUMS; ++s) o.term[s] = 0.0;
  if (!(__builtin_isfinite(g) && g > 0.0f)) return;
  const int K = a.num_bins, T = a.num_thresholds;
  float gz, gd;
  if (a.gt_kind == ST_STEREO_GT_DEPTH) {
    gz = g;
    gd = a.bf / gz;
  } else {
    gd = g;
    gz = a.bf / gd;
  }
  if (!(a.depth_edges[0] < gz && gz <= a.depth_edges[K])) return;
  int b = 0;
  for (int k = 1; k < K; ++k) b += gz > a.depth_edges[k] ? 1 : 0;
  int region = 0;
  const float fx = (float)x, fy = (float)y;
  for (int r = 0; r < nb; ++r) {
    const float x1 = sbox[4 * r], y1 = sbox[4 * r + 1], x2 = sbox[4 * r + 2], y2 = sbox[4 * r + 3];
    if (x1 <= fx && fx < x2 && y1 <= fy && fy < y2) region = 1;
  }
  o.cell = region * K + b;
  o.bits = 1u;
  if (!(__builtin_isfinite(p) && p > 0.0f)) return;
  const float pz = a.bf / p;
  const float e = fabsf(p - gd);
  unsigned bits = 3u;
  for (int t = 0; t < T; ++t) bits |= (e > a.bad_thresholds[t] ? 1u : 0u) << (2 + t);
  const float rel = 0.05f * gd;
  bits |= ((e > 3.0f && e > rel) ? 1u : 0u) << (T + 2);
  const float q1 = pz / gz, q2 = gz / pz;
  const float r = q1 > q2 ? q1 : q2;
  bits |= (r < 1.25f ? 1u : 0u) << (T + 3);
  bits |= (r < 1.5625f ? 1u : 0u) << (T + 4);
  bits |= (r < 1.953125f ? 1u : 0u) << (T + 5);
  o.bits = bits;
  const float e16 = e * 16.0f;
  o.bin = e16 >= (float)(SE_HIST - 1) ? SE_HIST - 1 : (int)e16;      // also for e = +Inf
  const double ed = (double)e, gzd = (double)gz;
  const double dz = (double)pz - gzd;
  const double dz2 = dz * dz;
  o.term[0] = ed;
  o.term[1] = ed * ed;
  o.term[2] = fabs(dz) / gzd;
  o.term[3] = dz2 / gzd;
  o.term[4] = dz2;
}

template <bool VEC>
__global__ __launch_bounds__(SE_THREADS) void stereo_eval_kernel(StStereoEvalArgs a, const float* __restrict__ pred,
                                                                 const float* __restrict__ gt,
                                                                 const int* __restrict__ extent,
                                                                 const float* __restrict__ boxes,
                                                                 const int* __restrict__ box_counts,
                                                                 unsigned long long* __restrict__ hist,
                                                                 double* __restrict__ ws_sums, int* __restrict__ ws_counts) {
  extern __shared__ unsigned lds_hist[];                         // [ncell][SE_HIST]
  __shared__ float sbox[ST_STEREO_EVAL_MAX_BOXES * 4];
  __shared__ unsigned wcnt[SE_WAVES][SE_MAX_CELLS][SE_MAX_COUNTS];
  __shared__ double wsum[SE_WAVES][SE_MAX_CELLS][SE_SUMS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = blockIdx.y, g = blockIdx.x, G = gridDim.x;
  const int K = a.num_bins, NC = a.num_thresholds + 6, ncell = 2 * K;
  const int hn = min(max(extent[2 * n], 0), a.H), wn = min(max(extent[2 * n + 1], 0), a.W);
  const int nb = boxes ? min(max(box_counts[n], 0), a.max_boxes) : 0;

  for (int i = tid; i < ncell * SE_HIST; i += SE_THREADS) lds_hist[i] = 0u;
  for (int i = tid; i < nb * 4; i += SE_THREADS) sbox[i] = boxes[(size_t)n * a.max_boxes * 4 + i];
  for (int i = tid; i < SE_WAVES * SE_MAX_CELLS * SE_MAX_COUNTS; i += SE_THREADS) (&wcnt[0][0][0])[i] = 0u;
  for (int i = tid; i < SE_WAVES * SE_MAX_CELLS * SE_SUMS; i += SE_THREADS) (&wsum[0][0][0])[i] = 0.0;
  __syncthreads();

  const int WQ = (wn + 3) >> 2;
  const int units = hn * WQ;                                     // <= H * W < 2^31 (checked by the entry point)
  const float* pn = pred + (size_t)n * a.pred_img_pitch;
  const float* gn = gt + (size_t)n * a.gt_img_pitch;
  const float nanf_ = __builtin_nanf("");
  for (int turn = 0; turn < SE_TURNS; ++turn) {
    const long long first = (long long)g * SE_UNITS + (long long)turn * SE_THREADS;
    if (first >= units) break;                                   // uniform over the workgroup
    const int u = (int)first + tid;
    float pv[4] = {nanf_, nanf_, nanf_, nanf_}, gv[4] = {nanf_, nanf_, nanf_, nanf_};
    int y = 0, x0 = 0;
    if (u < units) {
      y = u / WQ;
      x0 = 4 * (u - y * WQ);
      const size_t at = (size_t)y * a.W + x0;
      if (VEC && x0 + 4 <= wn) {
        const f32x4 p4 = *reinterpret_cast<const f32x4*>(pn + at);
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(gn + at);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          pv[k] = p4[k];
          gv[k] = g4[k];
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (x0 + k < wn) {
            pv[k] = pn[at + k];
            gv[k] = gn[at + k];
          }
        }
      }
    }
    SePixel px[4];
    unsigned present = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      se_pixel(a, pv[k], gv[k], x0 + k, y, sbox, nb, px[k]);      // a pixel that was not loaded holds NaN: no cell
      if (px[k].cell >= 0) present |= 1u << px[k].cell;
      if (px[k].bits & 2u) atomicAdd(&lds_hist[px[k].cell * SE_HIST + px[k].bin], 1u);
    }
    for (int c = 0; c < ncell; ++c) {
      if (__ballot((present >> c) & 1u) == 0ull) continue;       // uniform over the wave
      unsigned word[SE_WORDS];
      double s[SE_SUMS];
#pragma unroll
      for (int w = 0; w < SE_WORDS; ++w) word[w] = 0u;
#pragma unroll
      for (int j = 0; j < SE_SUMS; ++j) s[j] = 0.0;
      bool both = false;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (px[k].cell != c) continue;
        const unsigned f = px[k].bits;
#pragma unroll
        for (int w = 0; w < SE_WORDS; ++w)
          word[w] += ((f >> (3 * w)) & 1u) | (((f >> (3 * w + 1)) & 1u) << 10) | (((f >> (3 * w + 2)) & 1u) << 20);
        if (f & 2u) {
          both = true;
#pragma unroll
          for (int j = 0; j < SE_SUMS; ++j) s[j] += px[k].term[j];
        }
      }
#pragma unroll
      for (int w = 0; w < SE_WORDS; ++w) word[w] = wave_sum(word[w]);
      const bool any_both = __ballot(both) != 0ull;
      if (any_both) {
#pragma unroll
        for (int j = 0; j < SE_SUMS; ++j) s[j] = wave_sum(s[j]);
      }
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < SE_MAX_COUNTS; ++j) wcnt[wave][c][j] += (word[j / 3] >> (10 * (j % 3))) & 1023u;
        if (any_both) {
#pragma unroll
          for (int j = 0; j < SE_SUMS; ++j) wsum[wave][c][j] += s[j];
        }
      }
    }
  }
  __syncthreads();

  const size_t slot = ((size_t)n * G + g) * ncell;               // this workgroup's partials: [ncell][NC] / [ncell][5]
  if (tid < ncell * NC) {
    const int c = tid / NC, j = tid - c * NC;
    unsigned t = 0u;
#pragma unroll
    for (int w = 0; w < SE_WAVES; ++w) t += wcnt[w][c][j];
    ws_counts[slot * NC + tid] = (int)t;
  }
  if (tid < ncell * SE_SUMS) {
    const int c = tid / SE_SUMS, j = tid - c * SE_SUMS;
    double t = wsum[0][c][j];
#pragma unroll
    for (int w = 1; w < SE_WAVES; ++w) t += wsum[w][c][j];
    ws_sums[slot * SE_SUMS + tid] = t;
  }
  unsigned long long* hn_ = hist + (size_t)n * ncell * SE_HIST;
  for (int i = tid; i < ncell * SE_HIST; i += SE_THREADS) {
    const unsigned v = lds_hist[i];
    if (v) atomicAdd(hn_ + i, (unsigned long long)v);
  }
}

// counts[n][cell][j] / sums[n][cell][j] = the frame's partials added in workgroup order, one thread per output.
__global__ __launch_bounds__(256) void stereo_eval_reduce_kernel(int N, int G, int ncell, int NC,
                                                                 const double* __restrict__ ws_sums,
                                                                 const int* __restrict__ ws_counts,
                                                                 long long* __restrict__ counts, double* __restrict__ sums) {
  const int per = ncell * (NC + SE_SUMS);
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * per) return;
  const int n = idx / per, r = idx - n * per;
  if (r < ncell * NC) {
    long long t = 0;
    for (int g0 = 0; g0 < G; g0 += SE_AHEAD) {                     // SE_AHEAD loads in flight, added in index order
      int v[SE_AHEAD];
#pragma unroll
      for (int k = 0; k < SE_AHEAD; ++k) v[k] = g0 + k < G ? ws_counts[((size_t)n * G + g0 + k) * ncell * NC + r] : 0;
#pragma unroll
      for (int k = 0; k < SE_AHEAD; ++k) t += v[k];
    }
    counts[(size_t)n * ncell * NC + r] = t;
  } else {
    const int q = r - ncell * NC;
    double t = 0.0;
    for (int g0 = 0; g0 < G; g0 += SE_AHEAD) {                     // a slot past G adds +0.0: exact, the sums are >= 0
      double v[SE_AHEAD];
#pragma unroll
      for (int k = 0; k < SE_AHEAD; ++k) v[k] = g0 + k < G ? ws_sums[((size_t)n * G + g0 + k) * ncell * SE_SUMS + q] : 0.0;
#pragma unroll
      for (int k = 0; k < SE_AHEAD; ++k) t += v[k];
    }
    sums[(size_t)n * ncell * SE_SUMS + q] = t;
  }
}

static int se_check(const StStereoEvalArgs* a, const char* who) {
  ST_REQUIRE(a && a->struct_size == (int)sizeof(StStereoEvalArgs), "%s: struct_size mismatch", who);
  ST_REQUIRE(a->N >= 1 && a->N <= 65535 && a->H >= 1 && a->W >= 1 && (long long)a->H * a->W < (1ll << 31),
             "%s: bad shape N=%d H=%d W=%d", who, a->N, a->H, a->W);
  ST_REQUIRE(a->gt_kind == ST_STEREO_GT_DEPTH || a->gt_kind == ST_STEREO_GT_DISP, "%s: gt_kind %d", who, a->gt_kind);
  ST_REQUIRE(a->num_bins >= 1 && a->num_bins <= ST_STEREO_EVAL_MAX_BINS, "%s: num_bins %d outside 1..%d", who,
             a->num_bins, ST_STEREO_EVAL_MAX_BINS);
  ST_REQUIRE(a->num_thresholds >= 1 && a->num_thresholds <= ST_STEREO_EVAL_MAX_THRESHOLDS,
             "%s: num_thresholds %d outside 1..%d", who, a->num_thresholds, ST_STEREO_EVAL_MAX_THRESHOLDS);
  ST_REQUIRE(a->max_boxes >= 0 && a->max_boxes <= ST_STEREO_EVAL_MAX_BOXES, "%s: max_boxes %d outside 0..%d", who,
             a->max_boxes, ST_STEREO_EVAL_MAX_BOXES);
  ST_REQUIRE(a->pred_img_pitch >= (size_t)a->H * a->W && a->gt_img_pitch >= (size_t)a->H * a->W,
             "%s: an image pitch is smaller than one plane", who);
  ST_REQUIRE(a->bf > 0.0f && a->bf < __builtin_inff(), "%s: bf must be positive and finite", who);
  for (int k = 0; k <= a->num_bins; ++k)
    ST_REQUIRE(a->depth_edges[k] == a->depth_edges[k] && (k == 0 || a->depth_edges[k - 1] < a->depth_edges[k]),
               "%s: depth_edges must ascend strictly", who);
  for (int t = 0; t < a->num_thresholds; ++t)
    ST_REQUIRE(a->bad_thresholds[t] == a->bad_thresholds[t], "%s: a bad threshold is not a number", who);
  return ST_OK;
}

static int se_groups(const StStereoEvalArgs* a) {
  const long long units = (long long)a->H * ((a->W + 3) / 4);
  return (int)((units + SE_UNITS - 1) / SE_UNITS);
}

}  // namespace st

extern "C" size_t st_stereo_eval_workspace_bytes(const StStereoEvalArgs* args) {
  using namespace st;
  if (se_check(args, "st_stereo_eval_workspace_bytes") != ST_OK) return 0;
  const size_t slots = (size_t)args->N * se_groups(args) * 2 * args->num_bins;
  return slots * SE_SUMS * sizeof(double) + slots * (args->num_thresholds + 6) * sizeof(int);
}

extern "C" int st_stereo_eval(const StStereoEvalArgs* args, const float* pred_dev, const float* gt_dev,
                              const int32_t* extent_dev, const float* boxes_dev, const int32_t* box_counts_dev,
                              int64_t* counts_dev, double* sums_dev, int64_t* hist_dev, void* workspace_dev,
                              st_stream_t stream_) {
  using namespace st;
  ST_CHECK(se_check(args, "st_stereo_eval"));
  ST_REQUIRE(pred_dev && gt_dev && extent_dev && counts_dev && sums_dev && hist_dev && workspace_dev,
             "st_stereo_eval: null pointer");
  ST_REQUIRE(args->max_boxes == 0 || (boxes_dev && box_counts_dev), "st_stereo_eval: max_boxes > 0 without boxes");
  const size_t need = st_stereo_eval_workspace_bytes(args);
  ST_REQUIRE((reinterpret_cast<uintptr_t>(workspace_dev) & 7) == 0, "st_stereo_eval: workspace must be 8-byte aligned");
  if (args->workspace_bytes < need)
    return set_error(ST_ERR_WORKSPACE, "st_stereo_eval: workspace of %zu bytes, %zu needed", args->workspace_bytes, need);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int G = se_groups(args), ncell = 2 * args->num_bins, NC = args->num_thresholds + 6;
  const size_t slots = (size_t)args->N * G * ncell;
  double* ws_sums = static_cast<double*>(workspace_dev);
  int* ws_counts = reinterpret_cast<int*>(ws_sums + slots * SE_SUMS);
  const float* boxes = args->max_boxes > 0 ? boxes_dev : nullptr;
  ST_CHECK_HIP(hipMemsetAsync(hist_dev, 0, (size_t)args->N * ncell * SE_HIST * sizeof(int64_t), stream));
  const size_t lds = (size_t)ncell * SE_HIST * sizeof(unsigned);
  const bool vec = args->W % 4 == 0 && args->pred_img_pitch % 4 == 0 && args->gt_img_pitch % 4 == 0 &&
                   ((reinterpret_cast<uintptr_t>(pred_dev) | reinterpret_cast<uintptr_t>(gt_dev)) & 15) == 0;
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(hist_dev);
  if (vec)
    hipLaunchKernelGGL(stereo_eval_kernel<true>, dim3(G, args->N), dim3(SE_THREADS), lds, stream, *args, pred_dev, gt_dev,
                       extent_dev, boxes, box_counts_dev, hist, ws_sums, ws_counts);
  else
    hipLaunchKernelGGL(stereo_eval_kernel<false>, dim3(G, args->N), dim3(SE_THREADS), lds, stream, *args, pred_dev,
                       gt_dev, extent_dev, boxes, box_counts_dev, hist, ws_sums, ws_counts);
  ST_CHECK_HIP(hipGetLastError());
  const int outs = args->N * ncell * (NC + SE_SUMS);
  hipLaunchKernelGGL(stereo_eval_reduce_kernel, dim3((outs + 255) / 256), dim3(256), 0, stream, args->N, G, ncell, NC,
                     ws_sums, ws_counts, reinterpret_cast<long long*>(counts_dev), sums_dev);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}
