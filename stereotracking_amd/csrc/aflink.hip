// AppearanceFreeLink on the device (include/stereotrack.h section 18): the gate over all ordered
// track pairs of all prediction sets, the 30-row min-max transform of every candidate pair and the link network.  The
// rules are the statements of stereotracking_amd/aflink.py (backend='host').
//
// k_gate_count / k_gate_scan / k_gate_fill: one thread per earlier track i walks the later tracks j of its set; the
//   candidate list is written at the offsets of an exclusive prefix sum over i, so it is exact-sized and row-major
//   without any atomic that decides an order.
// k_transform: one thread per (candidate, column): min / max over the 60 rows (zero pads included), the affine step in
//   fp64, one rounding to fp32: bit-equal to the host's.
// k_score: one workgroup of 256 threads per group of kP = 4 candidates.  Per temporal module the activations of the
//   group go from layer to layer in two LDS buffers ([pair][row = (time, column)][channel], row stride channels + 1 so
//   that the 32 rows of an MFMA operand fall into different banks).  Layers 2-4 and the fusion conv are GEMMs on
//   v_mfma_f32_32x32x2_f32: A rows = (pair, output time, column), K = (tap, input channel) read straight from the LDS
//   activations, B = the packed weights [K][Cout] read from global memory (L2 resident), one B fragment feeding every
//   M tile a wave owns.  BatchNorm is a per-(column, channel) scale and shift in the epilogue.  Layer 1 (K = 7), the
//   pooling and the classifier run on the VALU.  An MFMA result element is one k-ordered fmaf chain, so a candidate's
//   bytes do not depend on its place in a group or a launch.
#include "st_common.h"

namespace {

constexpr int kP = 4;                    // candidates per workgroup (st_aflink_group_pairs)
constexpr int kThreads = 256;
constexpr int kLen = 30;                 // rows of a transformed track
constexpr int kXFloats = 2 * kLen * 3;   // one candidate's network input
constexpr int kMaxCapacity = 1 << 28;    // candidate slots: (capacity, 3) int offsets and capacity * 180 stay countable

// ---- packed weights (floats).  Per temporal module: layer l = 1..4 W[l] ([tap][cin][cout]), scale and shift
// ([column][cout]); the fusion conv WF ([tap = column][cin][cout]) with its scale and shift ([cout]).  Then the
// classifier: fc1 transposed ([512][128]), its bias, fc2 ([2][128]), its bias.
constexpr int kC0 = 1, kC1 = 32, kC2 = 64, kC3 = 128, kC4 = 256;
constexpr int kW1 = 0, kS1 = kW1 + 7 * kC0 * kC1, kB1 = kS1 + 3 * kC1;
constexpr int kW2 = kB1 + 3 * kC1, kS2 = kW2 + 7 * kC1 * kC2, kB2 = kS2 + 3 * kC2;
constexpr int kW3 = kB2 + 3 * kC2, kS3 = kW3 + 7 * kC2 * kC3, kB3 = kS3 + 3 * kC3;
constexpr int kW4 = kB3 + 3 * kC3, kS4 = kW4 + 7 * kC3 * kC4, kB4 = kS4 + 3 * kC4;
constexpr int kWF = kB4 + 3 * kC4, kSF = kWF + 3 * kC4 * kC4, kBF = kSF + kC4;
constexpr int kModFloats = kBF + kC4;
constexpr int kFc1 = 2 * kModFloats, kFc1B = kFc1 + 512 * 128, kFc2 = kFc1B + 128, kFc2B = kFc2 + 2 * 128;
constexpr int kPackedFloats = kFc2B + 2;

// LDS activations per pair: buffer A holds the outputs of layers 2 and 4, buffer B those of layers 1, 3 and the fusion
constexpr int kBufA = 18 * (kC4 + 1) > 54 * (kC2 + 1) ? 18 * (kC4 + 1) : 54 * (kC2 + 1);
constexpr int kBufB = 36 * (kC3 + 1);
static_assert(kBufB >= 72 * (kC1 + 1) && kBufB >= 6 * (kC4 + 1), "buffer B holds layer 1 and the fusion output too");

struct ScoreLds {
  float a[kP * kBufA];
  float b[kP * kBufB];
  float feat[kP][2 * kC4];
  float x[kP][kXFloats];
  float logit[kP][2];
};
static_assert(sizeof(ScoreLds) <= 160 * 1024, "one workgroup's activations fit the CU's LDS");

struct AflinkWeights {
  float* dev;
};

typedef float f32x16 __attribute__((ext_vector_type(16)));

// out[pair][q][n] = relu(scale * sum_k in[pair][q * QMUL + tap * TS][ci] * W[tap * CIN + ci][n] + shift)
// in: [pair][QIN rows][CIN + 1], out: [pair][QOUT rows][COUT + 1].  PERCOL: scale and shift of column q % 3.
// The NT = COUT / 32 column tiles times MSPLIT row ranges are dealt to the four waves; a wave keeps MT row tiles of
// accumulators and feeds them all from one B fragment.
template <int CIN, int COUT, int QIN, int QOUT, int QMUL, int TS, int TAPS, bool PERCOL, int MSPLIT>
__device__ __forceinline__ void gemm_layer(const float* __restrict__ in, float* __restrict__ out,
                                           const float* __restrict__ W, const float* __restrict__ S,
                                           const float* __restrict__ Bv) {
  constexpr int M = kP * QOUT, LDI = CIN + 1, LDO = COUT + 1;
  constexpr int MT_TOTAL = (M + 31) / 32, NT = COUT / 32, MT = (MT_TOTAL + MSPLIT - 1) / MSPLIT;
  constexpr int KB = 16, NBLK = TAPS * CIN / 2 / KB;      // k steps (of 2) per block of prefetched B fragments
  static_assert(CIN % (2 * KB) == 0, "a block of k steps stays inside one tap");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hi = lane >> 5;
  for (int item = wave; item < NT * MSPLIT; item += kThreads / 64) {
    const int nt = item % NT, mt0 = (item / NT) * MT;
    int abase[MT];
    f32x16 acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      int r = (mt0 + i) * 32 + l31;
      r = r < M ? r : M - 1;                         // rows past the end read the last row and are not stored
      abase[i] = ((r / QOUT) * QIN + (r % QOUT) * QMUL) * LDI + hi;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    }
    const float* wp = W + nt * 32 + l31 + (size_t)hi * COUT;
    // K = (tap, ci) is contiguous in W; the B fragments of the next KB steps are loaded while this block's MFMAs run
    float bq[KB];
#pragma unroll
    for (int u = 0; u < KB; ++u) bq[u] = wp[(size_t)(2 * u) * COUT];
    for (int blk = 0; blk < NBLK; ++blk) {
      float bn[KB];
      if (blk + 1 < NBLK) {
#pragma unroll
        for (int u = 0; u < KB; ++u) bn[u] = wp[(size_t)(2 * ((blk + 1) * KB + u)) * COUT];
      }
      const int k0 = blk * KB * 2, aoff = (k0 / CIN) * TS * LDI + k0 % CIN;      // a block stays inside one tap
#pragma unroll
      for (int u = 0; u < KB; ++u) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
          if ((mt0 + i) * 32 < M)
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(in[abase[i] + aoff + 2 * u], bq[u], acc[i], 0, 0, 0);
      }
      if (blk + 1 < NBLK) {
#pragma unroll
        for (int u = 0; u < KB; ++u) bq[u] = bn[u];
      }
    }
    const int n = nt * 32 + l31;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = (mt0 + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * hi;
        if (r < M) {
          const int q = r % QOUT, col = PERCOL ? q % 3 : 0;
          const float v = acc[i][e] * S[col * COUT + n] + Bv[col * COUT + n];
          out[(size_t)r * LDO + n] = v > 0.f ? v : 0.f;       // r = pair * QOUT + q
        }
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_score(StAflinkArgs a, const float* __restrict__ w) {
  __shared__ ScoreLds s;
  const int tid = threadIdx.x;
  int total = a.header[0];
  total = total < a.capacity ? total : a.capacity;
  const long long left = (long long)total - a.first;
  const int n = left < a.count ? (int)(left > 0 ? left : 0) : a.count;      // candidates of this launch
  const int c0 = blockIdx.x * kP;
  if (c0 >= n) return;
  const int np = n - c0 < kP ? n - c0 : kP;

  for (int e = tid; e < kP * kXFloats; e += kThreads) {
    const int p = e / kXFloats;
    s.x[p][e % kXFloats] = p < np ? a.ws_x[(size_t)(c0 + p) * kXFloats + e % kXFloats] : 0.f;
  }
  __syncthreads();

  for (int m = 0; m < 2; ++m) {
    const float* wm = w + (size_t)m * kModFloats;
    // layer 1 on the VALU: [pair][(t, column)][32]
    for (int e = tid; e < kP * 72 * kC1; e += kThreads) {
      const int c = e % kC1, row = (e / kC1) % 72, p = e / (kC1 * 72), col = row % 3;
      const float* xs = &s.x[p][m * kLen * 3 + row];          // (t + tap) * 3 + column = row + 3 tap
      float v = 0.f;
#pragma unroll
      for (int tap = 0; tap < 7; ++tap) v = __builtin_fmaf(xs[tap * 3], wm[kW1 + tap * kC1 + c], v);
      v = v * wm[kS1 + col * kC1 + c] + wm[kB1 + col * kC1 + c];
      s.b[(p * 72 + row) * (kC1 + 1) + c] = v > 0.f ? v : 0.f;
    }
    __syncthreads();
    gemm_layer<kC1, kC2, 72, 54, 1, 3, 7, true, 2>(s.b, s.a, wm + kW2, wm + kS2, wm + kB2);
    __syncthreads();
    gemm_layer<kC2, kC3, 54, 36, 1, 3, 7, true, 1>(s.a, s.b, wm + kW3, wm + kS3, wm + kB3);
    __syncthreads();
    gemm_layer<kC3, kC4, 36, 18, 1, 3, 7, true, 1>(s.b, s.a, wm + kW4, wm + kS4, wm + kB4);
    __syncthreads();
    gemm_layer<kC4, kC4, 18, 6, 3, 1, 3, false, 1>(s.a, s.b, wm + kWF, wm + kSF, wm + kBF);
    __syncthreads();
    for (int e = tid; e < kP * kC4; e += kThreads) {
      const int c = e % kC4, p = e / kC4;
      float v = 0.f;
#pragma unroll
      for (int t = 0; t < 6; ++t) v += s.b[(p * 6 + t) * (kC4 + 1) + c];
      s.feat[p][m * kC4 + c] = v / 6.f;
    }
    __syncthreads();
  }

  // classifier: fc1 (512 -> 128) + ReLU into buffer A, fc2 (128 -> 2), softmax
  static_assert(kP == 4 && kThreads == 256, "two pairs per thread in fc1");
  {
    const int j = tid & 127, p0 = (tid >> 7) * 2;
    float v0 = w[kFc1B + j], v1 = v0;
#pragma unroll 32
    for (int k = 0; k < 2 * kC4; ++k) {                  // unrolled: the weight loads run ahead of the chain
      const float wk = w[kFc1 + k * 128 + j];
      v0 = __builtin_fmaf(wk, s.feat[p0][k], v0);
      v1 = __builtin_fmaf(wk, s.feat[p0 + 1][k], v1);
    }
    s.a[p0 * 128 + j] = v0 > 0.f ? v0 : 0.f;
    s.a[(p0 + 1) * 128 + j] = v1 > 0.f ? v1 : 0.f;
  }
  __syncthreads();
  if (tid < kP * 2) {
    const int p = tid >> 1, c = tid & 1;
    float v = w[kFc2B + c];
#pragma unroll 32
    for (int k = 0; k < 128; ++k) v = __builtin_fmaf(w[kFc2 + c * 128 + k], s.a[p * 128 + k], v);
    s.logit[p][c] = v;
  }
  __syncthreads();
  if (tid < np) {
    const size_t c = (size_t)a.first + c0 + tid;
    // the probability of class 1 of the two fp32 logits, evaluated in fp64 and rounded once
    a.conf[c] = (float)(1.0 / (1.0 + exp((double)s.logit[tid][0] - (double)s.logit[tid][1])));
    if (a.logits) {
      a.logits[c * 2] = s.logit[tid][0];
      a.logits[c * 2 + 1] = s.logit[tid][1];
    }
  }
}

// ---- gate
__device__ __forceinline__ bool gate_pass(const StAflinkArgs& a, int i, int j) {
  if (i == j) return false;
  const double* li = a.feat + (size_t)(a.trk_off[i + 1] - 1) * 3;      // the last row of i
  const double* fj = a.feat + (size_t)a.trk_off[j] * 3;                // the first row of j
  const double dt = fj[0] - li[0];
  if (!(a.t_lo <= dt && dt <= a.t_hi)) return false;
  const double dx = li[1] - fj[1], dy = li[2] - fj[2];
  return sqrt(dx * dx + dy * dy) <= a.spatial_thr;                      // -ffp-contract=off: not fused
}

__device__ __forceinline__ bool track_ok(const StAflinkArgs& a, int i, int* s0, int* s1) {
  const int set = a.trk_set[i];
  if (set < 0 || set >= a.num_sets) return false;
  *s0 = a.set_off[set];
  *s1 = a.set_off[set + 1];
  if (*s0 < 0 || *s1 > a.num_tracks || i < *s0 || i >= *s1) return false;
  return true;
}

__device__ __forceinline__ bool rows_ok(const StAflinkArgs& a, int i) {
  return a.trk_off[i] >= 0 && a.trk_off[i + 1] > a.trk_off[i] && a.trk_off[i + 1] <= a.num_rows;
}

__global__ __launch_bounds__(256) void k_gate_count(StAflinkArgs a) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.num_tracks; i += gridDim.x * blockDim.x) {
    int s0, s1, cnt = 0;
    if (!track_ok(a, i, &s0, &s1) || !rows_ok(a, i)) {
      atomicOr(&a.header[1], 2);
    } else {
      for (int j = s0; j < s1; ++j)
        if (rows_ok(a, j) && gate_pass(a, i, j)) ++cnt;
    }
    a.ws_off[i] = cnt;
  }
}

// exclusive prefix sum of ws_off[0 .. num_tracks) in place, the total into ws_off[num_tracks] and header[0]
__global__ __launch_bounds__(256) void k_gate_scan(StAflinkArgs a) {
  __shared__ long long part[256];
  const int tid = threadIdx.x, T = a.num_tracks;
  const int per = (T + 255) / 256, lo = tid * per < T ? tid * per : T, hi = lo + per < T ? lo + per : T;
  long long sum = 0;
  for (int i = lo; i < hi; ++i) sum += a.ws_off[i];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int t = 0; t < 256; ++t) {
      const long long v = part[t];
      part[t] = run;
      run += v;
    }
    if (run > a.capacity) atomicOr(&a.header[1], 1);
    a.header[0] = run > 0x7fffffffLL ? 0x7fffffff : (int)run;
    a.ws_off[T] = a.header[0];
  }
  __syncthreads();
  long long run = part[tid];
  for (int i = lo; i < hi; ++i) {
    const int v = a.ws_off[i];
    a.ws_off[i] = run > 0x7fffffffLL ? 0x7fffffff : (int)run;
    run += v;
  }
}

__global__ __launch_bounds__(256) void k_gate_fill(StAflinkArgs a) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.num_tracks; i += gridDim.x * blockDim.x) {
    int s0, s1;
    if (!track_ok(a, i, &s0, &s1) || !rows_ok(a, i)) continue;
    long long o = a.ws_off[i];
    for (int j = s0; j < s1; ++j) {
      if (!(rows_ok(a, j) && gate_pass(a, i, j))) continue;
      if (o < a.capacity) {
        int* c = a.cand + (size_t)o * 3;
        c[0] = a.trk_set[i];
        c[1] = i - s0;
        c[2] = j - s0;
      }
      ++o;
    }
  }
}

// ---- transform
__global__ __launch_bounds__(256) void k_transform(StAflinkArgs a) {
  int total = a.header[0];
  total = total < a.capacity ? total : a.capacity;
  const long long left = (long long)total - a.first;
  const int n = left < a.count ? (int)(left > 0 ? left : 0) : a.count;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n * 3; e += gridDim.x * blockDim.x) {
    const int q = e / 3, col = e % 3;
    const int* c = a.cand + (size_t)(a.first + q) * 3;
    float* x = a.ws_x + (size_t)q * kXFloats + col;
    const int set = c[0];
    bool ok = set >= 0 && set < a.num_sets;
    int i = 0, j = 0;
    if (ok) {
      const int s0 = a.set_off[set], s1 = a.set_off[set + 1];
      i = s0 + c[1];
      j = s0 + c[2];
      ok = s0 >= 0 && s1 <= a.num_tracks && c[1] >= 0 && c[2] >= 0 && i < s1 && j < s1 && rows_ok(a, i) && rows_ok(a, j);
    }
    if (!ok) {
      atomicOr(&a.header[1], 2);
      for (int t = 0; t < 2 * kLen; ++t) x[t * 3] = 0.f;
      continue;
    }
    const int ni = a.trk_off[i + 1] - a.trk_off[i], nj = a.trk_off[j + 1] - a.trk_off[j];
    const int li = ni < kLen ? ni : kLen, lj = nj < kLen ? nj : kLen;
    const double* pi = a.feat + (size_t)(a.trk_off[i + 1] - li) * 3 + col;      // the last li rows of i
    const double* pj = a.feat + (size_t)a.trk_off[j] * 3 + col;                  // the first lj rows of j
    double mn = pi[0], mx = pi[0];
    if (li < kLen || lj < kLen) {                  // the zero pads take part
      mn = fmin(mn, 0.0);
      mx = fmax(mx, 0.0);
    }
    for (int t = 0; t < li; ++t) {
      mn = fmin(mn, pi[t * 3]);
      mx = fmax(mx, pi[t * 3]);
    }
    for (int t = 0; t < lj; ++t) {
      mn = fmin(mn, pj[t * 3]);
      mx = fmax(mx, pj[t * 3]);
    }
    const double sub = (mx + mn) / 2.0, div = (mx - mn) / 2.0 + 1e-5;
    const int pad = kLen - li;
    for (int t = 0; t < kLen; ++t) x[t * 3] = (float)(((t < pad ? 0.0 : pi[(t - pad) * 3]) - sub) / div);
    for (int t = 0; t < kLen; ++t) x[(kLen + t) * 3] = (float)(((t < lj ? pj[t * 3] : 0.0) - sub) / div);
  }
}

int validate(const StAflinkArgs* a) {
  ST_REQUIRE(a != nullptr && a->struct_size == (int)sizeof(StAflinkArgs), "st_aflink: args missing or of another size");
  ST_REQUIRE(a->num_sets >= 0 && a->num_tracks >= 0 && a->num_rows >= 0 && a->num_rows <= 0x7fffffff / 3,
             "st_aflink: bad sizes (%d sets, %d tracks, %d rows)", a->num_sets, a->num_tracks, a->num_rows);
  ST_REQUIRE(a->capacity >= 0 && a->capacity <= kMaxCapacity, "st_aflink: %d candidate slots, at most %d are supported",
             a->capacity, kMaxCapacity);
  ST_REQUIRE(a->header != nullptr, "st_aflink: the header is missing");
  return ST_OK;
}

int validate_tables(const StAflinkArgs* a) {
  ST_REQUIRE(a->num_tracks == 0 || (a->feat && a->trk_off && a->trk_set && a->set_off),
             "st_aflink: a track table is missing");
  ST_REQUIRE(a->capacity == 0 || a->cand, "st_aflink: the candidate list is missing");
  return ST_OK;
}

int validate_range(const StAflinkArgs* a, const char* what) {
  ST_REQUIRE(a->first >= 0 && a->count >= 0 && (long long)a->first + a->count <= a->capacity,
             "%s: range [%d, %d + %d) of %d candidate slots", what, a->first, a->first, a->count, a->capacity);
  ST_REQUIRE(a->count == 0 || a->ws_x, "%s: the input buffer is missing", what);
  return ST_OK;
}

}  // namespace

extern "C" {

int st_aflink_group_pairs(void) { return kP; }
size_t st_aflink_packed_floats(void) { return (size_t)kPackedFloats; }
int st_aflink_max_candidates(void) { return kMaxCapacity; }

int st_aflink_weights_create(const float* packed_host, size_t num_floats, void** handle) {
  ST_REQUIRE(packed_host != nullptr && handle != nullptr, "st_aflink_weights_create: a pointer is missing");
  ST_REQUIRE(num_floats == (size_t)kPackedFloats, "st_aflink_weights_create: %zu floats, the packed network has %d",
             num_floats, kPackedFloats);
  float* dev = nullptr;
  ST_CHECK_HIP(hipMalloc((void**)&dev, (size_t)kPackedFloats * sizeof(float)));
  hipError_t e = hipMemcpy(dev, packed_host, (size_t)kPackedFloats * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(dev);
    return st::set_error(ST_ERR_HIP, "st_aflink_weights_create: hipMemcpy failed: %s", hipGetErrorString(e));
  }
  *handle = new AflinkWeights{dev};
  return ST_OK;
}

int st_aflink_weights_destroy(void* handle) {
  if (!handle) return ST_OK;
  AflinkWeights* w = (AflinkWeights*)handle;
  (void)hipFree(w->dev);
  delete w;
  return ST_OK;
}

int st_aflink_gate(const StAflinkArgs* a, st_stream_t stream_) {
  ST_CHECK(validate(a));
  ST_CHECK(validate_tables(a));
  ST_REQUIRE(a->ws_off != nullptr, "st_aflink_gate: the offset table is missing");
  hipStream_t stream = (hipStream_t)stream_;
  ST_CHECK_HIP(hipMemsetAsync(a->header, 0, 2 * sizeof(int), stream));
  const int blocks = a->num_tracks > 0 ? st::ceil_div(a->num_tracks, 256) : 1;
  if (a->num_tracks > 0) hipLaunchKernelGGL(k_gate_count, dim3(blocks < 4096 ? blocks : 4096), dim3(256), 0, stream, *a);
  hipLaunchKernelGGL(k_gate_scan, dim3(1), dim3(256), 0, stream, *a);
  if (a->num_tracks > 0) hipLaunchKernelGGL(k_gate_fill, dim3(blocks < 4096 ? blocks : 4096), dim3(256), 0, stream, *a);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

int st_aflink_transform(const StAflinkArgs* a, st_stream_t stream_) {
  ST_CHECK(validate(a));
  ST_CHECK(validate_tables(a));
  ST_CHECK(validate_range(a, "st_aflink_transform"));
  if (a->count == 0) return ST_OK;
  const int blocks = st::ceil_div(a->count * 3, 256);
  hipLaunchKernelGGL(k_transform, dim3(blocks < 4096 ? blocks : 4096), dim3(256), 0, (hipStream_t)stream_, *a);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

int st_aflink_score(const StAflinkArgs* a, const void* weights, st_stream_t stream_) {
  ST_CHECK(validate(a));
  ST_CHECK(validate_range(a, "st_aflink_score"));
  ST_REQUIRE(weights != nullptr && ((const AflinkWeights*)weights)->dev != nullptr, "st_aflink_score: no packed weights");
  ST_REQUIRE(a->count == 0 || a->conf, "st_aflink_score: the confidence buffer is missing");
  if (a->count == 0) return ST_OK;
  hipLaunchKernelGGL(k_score, dim3(st::ceil_div(a->count, kP)), dim3(kThreads), 0, (hipStream_t)stream_, *a,
                     (const float*)((const AflinkWeights*)weights)->dev);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

int st_aflink_run(const StAflinkArgs* a, const void* weights, st_stream_t stream) {
  ST_CHECK(validate(a));
  ST_CHECK(validate_tables(a));
  ST_REQUIRE(a->ws_off != nullptr, "st_aflink_run: the offset table is missing");
  ST_REQUIRE(weights != nullptr && ((const AflinkWeights*)weights)->dev != nullptr, "st_aflink_run: no packed weights");
  ST_REQUIRE(a->capacity == 0 || (a->chunk >= 1 && a->ws_x && a->conf), "st_aflink_run: %d candidate slots need a chunk "
             "size (%d), an input buffer and a confidence buffer", a->capacity, a->chunk);
  ST_CHECK(st_aflink_gate(a, stream));
  StAflinkArgs r = *a;
  for (int first = 0; first < a->capacity; first += a->chunk) {
    r.first = first;
    r.count = a->capacity - first < a->chunk ? a->capacity - first : a->chunk;
    ST_CHECK(st_aflink_transform(&r, stream));
    ST_CHECK(st_aflink_score(&r, weights, stream));
  }
  return ST_OK;
}

}  // extern "C"
