// Tracklet post-processing on the device (include/stereotrack.h section 17): linear gap filling
// and Gaussian-smoothed interpolation of tracker rows.  The rules are the statements of stereotracking_amd/tracklets.py
// (backend='host'); the filling is bit-equal to it, the smoothing is another correct fp64 evaluation of the same
// ill-conditioned system (tests/golden/gsi_truth.npz is the yardstick).
//
// k_gsi: one track per workgroup of 256 threads, persistent over the launch's range of the sorted track list.
//   A (n x n, row stride ld odd): the strict upper triangle keeps K for the final product, the lower triangle and the
//   diagonal hold K + 1e-10 I and become L.  n <= kLdsRows: A in LDS; else A in the workgroup's slot of ws and the
//   current 16-column panel of L in LDS for the trailing update.
//   Every sum is one fma chain of one thread in ascending index order: no reduction across threads, no atomics, so a
//   track's bytes depend on the track alone.
#include "st_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kNB = 16;                 // columns of a panel
constexpr int kMaxRows = 512;           // st_tracklet_max_rows
constexpr int kLdsRows = 128;           // the matrix stays in LDS up to here
constexpr int kLdsLd = kLdsRows + 1;
constexpr int kPanelLd = kNB + 1;
constexpr int kMatDoubles = kLdsRows * kLdsLd > kMaxRows * kPanelLd ? kLdsRows * kLdsLd : kMaxRows * kPanelLd;
constexpr double kAlpha = 1e-10;        // scikit-learn's default GaussianProcessRegressor(alpha)
// LDS: t and the four right-hand sides (5 x 512), the diagonal block (16 x 17), the matrix or the panel:
// (2560 + 272 + 16512) x 8 + the failure flag = 154760 bytes of the 160 KB: one workgroup per CU.

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }
inline size_t slot_doubles(int max_rows) {
  return max_rows <= kLdsRows ? 0 : align256((size_t)(max_rows | 1) * (size_t)max_rows * sizeof(double)) / sizeof(double);
}

struct GsiLds {
  double t[kMaxRows];
  double y[4][kMaxRows];
  double d[kNB][kPanelLd];
  double m[kMatDoubles];
  int fail;
};

// the diagonal block A[k .. k + 16)[k .. k + 16) into s.d (zero outside the matrix)
template <bool LDS>
__device__ __forceinline__ void stage_diag(GsiLds& s, const double* A, int ld, int n, int k, int tid) {
  const int r = tid / kNB, c = tid % kNB;
  s.d[r][c] = (k + r < n && k + c < n) ? A[(size_t)(k + r) * ld + k + c] : 0.0;
}

template <bool LDS>
__device__ void gsi_track(GsiLds& s, double* wsA, const StTrackletArgs& a, int trk, int off, int n) {
  const int tid = threadIdx.x;
  double* A = LDS ? s.m : wsA;
  double* P = s.m;                                   // !LDS: the panel rows below the diagonal block
  const int ld = LDS ? kLdsLd : (n | 1);
  const double ls = a.trk_len_scale[trk];
  // phase clocks (optional, thread 0): K, the factorisation, the solves, the product
  long long* ticks = a.phase_ticks ? a.phase_ticks + (size_t)blockIdx.x * 4 : nullptr;
  long long clk = ticks ? wall_clock64() : 0;
  auto lap = [&](int phase) {
    if (ticks && tid == 0) {
      const long long now = wall_clock64();
      ticks[phase] += now - clk;
      clk = now;
    }
  };

  for (int i = tid; i < n; i += kThreads) {
    const double* r = a.out_rows + (size_t)(off + i) * 7;
    s.t[i] = r[0];
#pragma unroll
    for (int c = 0; c < 4; ++c) s.y[c][i] = r[2 + c];
  }
  if (tid == 0) s.fail = 0;
  __syncthreads();

  // K: both triangles; the diagonal gets the jitter (the product below takes K_ii = exp(0) = 1)
  for (int e = tid; e < n * n; e += kThreads) {
    const int i = e / n, j = e - i * n;
    if (j < i) {
      const double d = (s.t[i] - s.t[j]) / ls;
      const double v = exp(-0.5 * (d * d));
      A[(size_t)i * ld + j] = v;
      A[(size_t)j * ld + i] = v;
    } else if (j == i) {
      A[(size_t)i * ld + i] = 1.0 + kAlpha;
    }
  }
  __syncthreads();
  lap(0);

  // ---- blocked right-looking Cholesky of the lower triangle
  bool failed = false;
  for (int k = 0; k < n; k += kNB) {
    const int nb = n - k < kNB ? n - k : kNB;
    // the diagonal block: thread r < nb owns row r, one column per step
    double r[kNB];
#pragma unroll
    for (int c = 0; c < kNB; ++c) r[c] = (tid < nb && c <= tid) ? A[(size_t)(k + tid) * ld + k + c] : 0.0;
#pragma unroll
    for (int j = 0; j < kNB; ++j) {
      if (tid == j && j < nb) {
        double v = r[j];
#pragma unroll
        for (int c = 0; c < j; ++c) v = __builtin_fma(-r[c], r[c], v);
        if (!(v > 0.0)) s.fail = 1;
        r[j] = sqrt(v);
#pragma unroll
        for (int c = 0; c <= j; ++c) s.d[j][c] = r[c];
      }
      __syncthreads();
      if (tid > j && tid < nb) {
        double v = r[j];
#pragma unroll
        for (int c = 0; c < j; ++c) v = __builtin_fma(-r[c], s.d[j][c], v);
        r[j] = v / s.d[j][j];
      }
    }
    if (tid < nb) {
#pragma unroll
      for (int c = 0; c < kNB; ++c)
        if (c <= tid) A[(size_t)(k + tid) * ld + k + c] = r[c];
    }
    __syncthreads();
    if (s.fail) {
      failed = true;
      break;
    }
    const int b0 = k + kNB;
    if (b0 >= n) break;
    // the panel below: one row per thread, L21 = A21 L11^-T
    for (int i = b0 + tid; i < n; i += kThreads) {
      double v[kNB];
#pragma unroll
      for (int c = 0; c < kNB; ++c) v[c] = A[(size_t)i * ld + k + c];
#pragma unroll
      for (int j = 0; j < kNB; ++j) {
        double x = v[j];
#pragma unroll
        for (int c = 0; c < j; ++c) x = __builtin_fma(-v[c], s.d[j][c], x);
        v[j] = x / s.d[j][j];
      }
#pragma unroll
      for (int c = 0; c < kNB; ++c) {
        A[(size_t)i * ld + k + c] = v[c];
        if (!LDS) P[(i - b0) * kPanelLd + c] = v[c];
      }
    }
    __syncthreads();
    // the trailing update A22 -= L21 L21^T, lower triangle, 4 x 4 outputs per thread
    const int m = n - b0, mt = (m + 3) / 4;
    const int ty = tid / 16, tx = tid % 16;
    for (int ti = ty; ti < mt; ti += 16) {
      for (int tj = tx; tj <= ti; tj += 16) {
        const int i0 = b0 + 4 * ti, j0 = b0 + 4 * tj;
        int ri[4], rj[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          ri[q] = i0 + q < n ? i0 + q : n - 1;       // rows past the matrix repeat the last one; never stored
          rj[q] = j0 + q < n ? j0 + q : n - 1;
        }
        double acc[4][4];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[p][q] = rj[q] <= ri[p] ? A[(size_t)ri[p] * ld + rj[q]] : 0.0;
#pragma unroll
        for (int c = 0; c < kNB; ++c) {
          double pr[4], pc[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            pr[q] = LDS ? A[(size_t)ri[q] * ld + k + c] : P[(ri[q] - b0) * kPanelLd + c];
            pc[q] = LDS ? A[(size_t)rj[q] * ld + k + c] : P[(rj[q] - b0) * kPanelLd + c];
          }
#pragma unroll
          for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[p][q] = __builtin_fma(-pr[p], pc[q], acc[p][q]);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (i0 + p < n && j0 + q <= i0 + p) A[(size_t)(i0 + p) * ld + j0 + q] = acc[p][q];
      }
    }
    __syncthreads();
  }
  lap(1);
  if (failed) {
    if (tid == 0) a.status[trk] |= 1;
    return;
  }

  // ---- L z = y, blocks of 16 rows
  for (int k = 0; k < n; k += kNB) {
    const int nb = n - k < kNB ? n - k : kNB;
    stage_diag<LDS>(s, A, ld, n, k, tid);
    __syncthreads();
    if (tid < 4) {
      for (int j = 0; j < nb; ++j) {
        double v = s.y[tid][k + j];
        for (int c = 0; c < j; ++c) v = __builtin_fma(-s.d[j][c], s.y[tid][k + c], v);
        s.y[tid][k + j] = v / s.d[j][j];
      }
    }
    __syncthreads();
    for (int i = k + kNB + tid; i < n; i += kThreads) {
      double v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = s.y[c][i];
      for (int j = 0; j < kNB; ++j) {
        const double l = A[(size_t)i * ld + k + j];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = __builtin_fma(-l, s.y[c][k + j], v[c]);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) s.y[c][i] = v[c];
    }
    __syncthreads();
  }
  // ---- L^T alpha = z, from the last block up
  for (int k = (n - 1) / kNB * kNB; k >= 0; k -= kNB) {
    const int nb = n - k < kNB ? n - k : kNB;
    stage_diag<LDS>(s, A, ld, n, k, tid);
    __syncthreads();
    if (tid < 4) {
      for (int j = nb - 1; j >= 0; --j) {
        double v = s.y[tid][k + j];
        for (int c = j + 1; c < nb; ++c) v = __builtin_fma(-s.d[c][j], s.y[tid][k + c], v);
        s.y[tid][k + j] = v / s.d[j][j];
      }
    }
    __syncthreads();
    for (int i = tid; i < k; i += kThreads) {
      double v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = s.y[c][i];
      for (int j = 0; j < nb; ++j) {
        const double l = A[(size_t)(k + j) * ld + i];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = __builtin_fma(-l, s.y[c][k + j], v[c]);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) s.y[c][i] = v[c];
    }
    __syncthreads();
  }
  lap(2);
  // ---- the mean K alpha, K from the upper triangle, K_ii = 1
  for (int i = tid; i < n; i += kThreads) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < n; ++j) {
      const double kij = j < i ? A[(size_t)j * ld + i] : (j == i ? 1.0 : A[(size_t)i * ld + j]);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = __builtin_fma(kij, s.y[c][j], v[c]);
    }
    double* r = a.out_rows + (size_t)(off + i) * 7;
#pragma unroll
    for (int c = 0; c < 4; ++c) r[2 + c] = v[c];
  }
  lap(3);
}

__global__ __launch_bounds__(kThreads) void k_gsi(StTrackletArgs a, size_t slot) {
  __shared__ GsiLds s;
  double* wsA = (double*)a.ws + (size_t)blockIdx.x * slot;
  for (int q = blockIdx.x; q < a.count; q += gridDim.x) {
    const int trk = a.trk_order[a.first + q];
    __syncthreads();                       // the previous track's reads of LDS are done
    if (trk < 0 || trk >= a.num_tracks) continue;
    const int off = a.trk_out_off[trk], n = a.trk_out_off[trk + 1] - off;
    if (n < 1 || n > a.max_rows || n > kMaxRows || off < 0 || (long long)off + n > a.num_out_rows) {
      if (threadIdx.x == 0) a.status[trk] |= 2;
      continue;
    }
    if (n <= kLdsRows)
      gsi_track<true>(s, wsA, a, trk, off, n);
    else
      gsi_track<false>(s, wsA, a, trk, off, n);
  }
}

__global__ __launch_bounds__(256) void k_interpolate(StTrackletArgs a) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < a.num_rows; r += gridDim.x * blockDim.x) {
    const int o = a.row_out_off[r], g = a.row_gap[r];
    const int fill = g > 1 ? g - 1 : 0;
    if (o < 0 || (long long)o + fill >= a.num_out_rows || (fill && r + 1 >= a.num_rows)) {
      a.status[0] = 2;      // every writer stores the same value into the zeroed word
      continue;
    }
    const double* left = a.rows + (size_t)r * 7;
    double* out = a.out_rows + (size_t)o * 7;
#pragma unroll
    for (int c = 0; c < 7; ++c) out[c] = left[c];
    if (!fill) continue;
    const double* right = left + 7;
    for (int j = 1; j < g; ++j) {
      double* w = out + (size_t)j * 7;
      const double f = (double)j / (double)g;
      w[0] = (double)j + left[0];
      w[1] = left[1];
#pragma unroll
      for (int c = 2; c < 6; ++c) w[c] = f * (right[c] - left[c]) + left[c];   // -ffp-contract=off: not fused
      w[6] = 1.0;
    }
  }
}

int validate(const StTrackletArgs* a) {
  ST_REQUIRE(a != nullptr && a->struct_size == (int)sizeof(StTrackletArgs), "st_tracklet: args missing or of another size");
  ST_REQUIRE(a->num_rows >= 0 && a->num_out_rows >= a->num_rows && a->num_tracks >= 0, "st_tracklet: bad sizes (%d rows, %d "
             "output rows, %d tracks)", a->num_rows, a->num_out_rows, a->num_tracks);
  ST_REQUIRE(a->num_rows == 0 || (a->rows && a->row_out_off && a->row_gap && a->out_rows),
             "st_tracklet: a row buffer is missing");
  ST_REQUIRE(a->num_tracks == 0 || (a->trk_out_off && a->trk_order && a->trk_len_scale && a->status),
             "st_tracklet: a track table is missing");
  return ST_OK;
}

}  // namespace

extern "C" {

int st_tracklet_max_rows(void) { return kMaxRows; }

size_t st_tracklet_gsi_workspace_bytes(const StTrackletArgs* args) {
  if (!args || args->struct_size != (int)sizeof(StTrackletArgs) || args->num_groups < 1 || args->max_rows < 1 ||
      args->max_rows > kMaxRows)
    return 0;
  return 256 + (size_t)args->num_groups * slot_doubles(args->max_rows) * sizeof(double);
}

int st_tracklet_interpolate(const StTrackletArgs* a, st_stream_t stream_) {
  ST_CHECK(validate(a));
  hipStream_t stream = (hipStream_t)stream_;
  if (a->num_tracks > 0) ST_CHECK_HIP(hipMemsetAsync(a->status, 0, (size_t)a->num_tracks * sizeof(int), stream));
  if (a->num_rows > 0 && a->num_tracks > 0) {
    const int blocks = st::ceil_div(a->num_rows, 256);
    hipLaunchKernelGGL(k_interpolate, dim3(blocks < 4096 ? blocks : 4096), dim3(256), 0, stream, *a);
  }
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

int st_tracklet_gsi(const StTrackletArgs* a, st_stream_t stream_) {
  ST_CHECK(validate(a));
  ST_REQUIRE(a->first >= 0 && a->count >= 0 && (long long)a->first + a->count <= a->num_tracks,
             "st_tracklet_gsi: range [%d, %d + %d) of %d tracks", a->first, a->first, a->count, a->num_tracks);
  if (a->count == 0) return ST_OK;
  ST_REQUIRE(a->num_groups >= 1 && a->num_groups <= 65535, "st_tracklet_gsi: %d workgroups", a->num_groups);
  ST_REQUIRE(a->max_rows >= 1 && a->max_rows <= kMaxRows, "st_tracklet_gsi: a track of %d rows, a launch supports %d "
             "(st_tracklet_max_rows)", a->max_rows, kMaxRows);
  const size_t need = st_tracklet_gsi_workspace_bytes(a);
  if (a->ws == nullptr || a->ws_bytes < need)
    return st::set_error(ST_ERR_WORKSPACE, "st_tracklet_gsi: workspace of %zu bytes, %zu needed", a->ws_bytes, need);
  hipLaunchKernelGGL(k_gsi, dim3(a->num_groups), dim3(kThreads), 0, (hipStream_t)stream_, *a, slot_doubles(a->max_rows));
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

}  // extern "C"
