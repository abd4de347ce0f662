// ECC camera-motion compensation (cmc=dict(method='ecc')) of the tracker: the estimate, on the device.
//
// Behavioural spec: the reference's CameraMotionCompensation (mmtrack/models/motion/camera_motion_compensation.py) =
// cv2.findTransformECC(MOTION_EUCLIDEAN, 50 iterations, eps 1e-3, gaussFiltSize 1).  OpenCV is an un-vendored dependency
// and absent; the rules E0..E10 are restated from OpenCV 4.x ecc.cpp [upstream-memory], PARITY UNPINNED against cv2
// itself.  tests/ecc_ref.py lists the rules and restates them in numpy (float64, and fp32 per-pixel arithmetic under
// float64 sums); tests/test_ecc_gpu.py holds these kernels to it.  DESIGN.md "ECC camera-motion compensation".
//
//   front     crop, grey (R 9798 + G 19235 + B 3735 + 2^14) >> 15 of the BGR frame, s x s box mean -> fp32 (exact).
//   prepare   fixed dyadic blur {1} / {1/4, 1/2, 1/4} / {1/16, 1/4, 3/8, 1/4, 1/16} of template and input (REFLECT_101,
//             exact in fp32), central-difference gradients of the blurred input; the input and its two gradients are
//             stored interleaved (one 16-byte load per bilinear tap in the iteration).
//   iterate   ONE pass over the template per iteration for all N pairs: each pixel warps, samples, builds its Jacobian
//             row in fp32 and accumulates the RAW moments in fp64 (J^T J, J^T Iw, J^T T, J^T 1, sum Iw T, first and
//             second moments of Iw and T, n: 45 values for AFFINE, 21 for EUCLIDEAN, 14 for TRANSLATION); the zero-mean
//             sums of the rules follow from them (J^T Iz = J^T Iw - mean_I J^T 1, ...), so no second pass is needed.
//             Wave shuffles -> LDS -> one partial per workgroup, all in a fixed order; no atomics.
//   finalize  one wave per pair: sums the partials in workgroup order, then moments, rho, Cholesky solve, lambda, the
//             warp update and the stop / failure tests on lane 0 in fp64; keeps the pair's `done` word.
// All num_iters rounds (iterate + finalize) are enqueued up front; workgroups of a finished pair exit at once.  The
// order of launches on the stream is the only dependency: no workgroup waits on another.
#include <cmath>
#include <cstdint>

#include "st_common.h"

namespace {

constexpr int kMaxFrames = 32;
constexpr int kThreads = 256;
constexpr int kPixPerThread = 8;
constexpr int kWgPixels = kThreads * kPixPerThread;   // template pixels per workgroup of the iterate kernel
constexpr int kMaxVals = 45;                          // raw moments of AFFINE, the stride of a partial
constexpr int kState = 16;                            // doubles per pair: warp (6), rho, last, done, iterations
constexpr int kRho = 6, kLast = 7, kDone = 8, kIters = 9;

struct FramePtrs { const unsigned char* p[kMaxFrames]; };

constexpr int n_params(int mode) { return mode == ST_ECC_TRANSLATION ? 2 : mode == ST_ECC_EUCLIDEAN ? 3 : 6; }
constexpr int n_vals(int mode) { return n_params(mode) * (n_params(mode) + 1) / 2 + 3 * n_params(mode) + 6; }
static_assert(n_vals(ST_ECC_AFFINE) == kMaxVals, "partial stride");

// ---- E0 front: one thread per plane pixel ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ int ecc_px(const T* p) {
  if constexpr (sizeof(T) == 1) {
    return (int)*p;
  } else {
    const int v = (int)*p;          // numpy astype(uint8) of the integral values the preprocessor produces
    return min(max(v, 0), 255);
  }
}

template <typename T>
__device__ __forceinline__ void ecc_front_body(const T* src, long long plane_stride, int row_stride, int ph, int pw,
                                               int s, float* out) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= ph * pw) return;
  const int py = i / pw, px = i - py * pw;
  int sum = 0;
  for (int dy = 0; dy < s; ++dy)
    for (int dx = 0; dx < s; ++dx) {
      const T* p = src + (long long)(py * s + dy) * row_stride + (px * s + dx);
      // the batch is BGR: R = channel 2, B = channel 0
      sum += (ecc_px(p + 2 * plane_stride) * 9798 + ecc_px(p + plane_stride) * 19235 + ecc_px(p) * 3735 + (1 << 14)) >> 15;
    }
  out[i] = (float)sum / (float)(s * s);        // a multiple of 1 / s^2 below 256: exact
}

__global__ __launch_bounds__(kThreads) void ecc_front_u8_kernel(FramePtrs fp, int fh, int fw, int ph, int pw, int s,
                                                                float* planes) {
  const int n = blockIdx.y;
  ecc_front_body<unsigned char>(fp.p[n], (long long)fh * fw, fw, ph, pw, s, planes + (size_t)n * ph * pw);
}

__global__ __launch_bounds__(kThreads) void ecc_front_f32_kernel(const float* batch, int H, int W, int ph, int pw, int s,
                                                                 float* planes) {
  const int n = blockIdx.y;
  ecc_front_body<float>(batch + (size_t)n * 3 * H * W, (long long)H * W, W, ph, pw, s, planes + (size_t)n * ph * pw);
}

// ---- E1 / E2 prepare ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect101(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i;
}

struct BlurTaps { int r; float k[5]; };

// grid (ceil(P / 256), 2 N): plane z < N blurs the template of pair z, plane z >= N the input of pair z - N
__global__ __launch_bounds__(kThreads) void ecc_blur_kernel(const float* prev, const float* curr, int N, int ph, int pw,
                                                            BlurTaps t, float* Tb, float* Ib) {
  const int z = blockIdx.y, P = ph * pw;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= P) return;
  const float* src = (z < N ? prev + (size_t)z * P : curr + (size_t)(z - N) * P);
  float* dst = (z < N ? Tb + (size_t)z * P : Ib + (size_t)(z - N) * P);
  const int y = i / pw, x = i - y * pw;
  float acc = 0.f;
  for (int dy = -t.r; dy <= t.r; ++dy) {
    const float* row = src + (size_t)reflect101(y + dy, ph) * pw;
    float h = 0.f;
    for (int dx = -t.r; dx <= t.r; ++dx) h += t.k[dx + t.r] * row[reflect101(x + dx, pw)];
    acc += t.k[dy + t.r] * h;
  }
  dst[i] = acc;
}

// grid (ceil(P / 256), N): {I, gx, gy, 0} of the blurred input
__global__ __launch_bounds__(kThreads) void ecc_grad_kernel(const float* Ib, int ph, int pw, float4* IG) {
  const int n = blockIdx.y, P = ph * pw;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= P) return;
  const float* I = Ib + (size_t)n * P;
  const int y = i / pw, x = i - y * pw;
  const float gx = 0.5f * (I[y * pw + reflect101(x + 1, pw)] - I[y * pw + reflect101(x - 1, pw)]);
  const float gy = 0.5f * (I[reflect101(y + 1, ph) * pw + x] - I[reflect101(y - 1, ph) * pw + x]);
  IG[(size_t)n * P + i] = make_float4(I[i], gx, gy, 0.f);
}

// grid (ceil(P / 256), N): the interleaved planes back into three (st_cmc_ecc_prepare)
__global__ __launch_bounds__(kThreads) void ecc_unpack_kernel(const float4* IG, int P, float* Ib, float* gx, float* gy) {
  const size_t i = (size_t)blockIdx.y * P + blockIdx.x * kThreads + threadIdx.x;
  if (blockIdx.x * kThreads + threadIdx.x >= (unsigned)P) return;
  const float4 v = IG[i];
  if (Ib) Ib[i] = v.x;
  if (gx) gx[i] = v.y;
  if (gy) gy[i] = v.z;
}

// ---- state ----------------------------------------------------------------------------------------------------------
// warps_in: (N, 6) float64 plane warps or null (identity)
__global__ void ecc_init_kernel(int N, const double* warps_in, double eps, double* state) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  double* st = state + (size_t)n * kState;
  const double id[6] = {1, 0, 0, 0, 1, 0};
  for (int k = 0; k < 6; ++k) st[k] = warps_in ? warps_in[(size_t)n * 6 + k] : id[k];
  st[kRho] = -1.0;
  st[kLast] = -eps;
  st[kDone] = 0.0;
  st[kIters] = 0.0;
  for (int k = kIters + 1; k < kState; ++k) st[k] = 0.0;
}

// ---- E3 .. E6 iterate: grid (G, N), G = ceil(P / kWgPixels) -----------------------------------------------------------
// layout of the NV raw moments: H upper triangle row-major | J^T Iw | J^T T | J^T 1 | sum Iw T, sum Iw, sum T, sum Iw^2,
// sum T^2, n
template <int MODE>
__global__ __launch_bounds__(kThreads) void ecc_iterate_kernel(const float* __restrict__ Tb, const float4* __restrict__ IG,
                                                               int ph, int pw, const double* __restrict__ state,
                                                               double* __restrict__ partials) {
  constexpr int K = n_params(MODE), NH = K * (K + 1) / 2, NV = n_vals(MODE);
  const int n = blockIdx.y, G = gridDim.x;
  const double* st = state + (size_t)n * kState;
  if (st[kDone] != 0.0) return;                      // the pair has stopped or failed: uniform over the workgroup
  const float m00 = (float)st[0], m01 = (float)st[1], m02 = (float)st[2];
  const float m10 = (float)st[3], m11 = (float)st[4], m12 = (float)st[5];
  const int P = ph * pw;
  const float* T = Tb + (size_t)n * P;
  const float4* ig = IG + (size_t)n * P;
  double acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = 0.0;

#pragma unroll 1
  for (int k = 0; k < kPixPerThread; ++k) {
    const int idx = blockIdx.x * kWgPixels + k * kThreads + threadIdx.x;
    if (idx >= P) break;
    const int y = idx / pw, x = idx - y * pw;
    const float xf = (float)x, yf = (float)y;
    const float qx = (m00 * xf + m01 * yf) + m02;
    const float qy = (m10 * xf + m11 * yf) + m12;
    const float rx = floorf(qx + 0.5f), ry = floorf(qy + 0.5f);
    // E3 mask; false for a NaN.  Inside means q in [-0.5, size - 0.5): the four taps lie in [-1, size]
    if (!(rx >= 0.f && rx <= (float)(pw - 1) && ry >= 0.f && ry <= (float)(ph - 1))) continue;
    const float x0f = floorf(qx), y0f = floorf(qy);
    const float fx = qx - x0f, fy = qy - y0f;
    const float gx1 = 1.f - fx, gy1 = 1.f - fy;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const bool xa = x0 >= 0, xb = x0 + 1 < pw, ya = y0 >= 0, yb = y0 + 1 < ph;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 v00 = (xa && ya) ? ig[y0 * pw + x0] : z4;
    const float4 v01 = (xb && ya) ? ig[y0 * pw + x0 + 1] : z4;
    const float4 v10 = (xa && yb) ? ig[(y0 + 1) * pw + x0] : z4;
    const float4 v11 = (xb && yb) ? ig[(y0 + 1) * pw + x0 + 1] : z4;
    const float Iw = (v00.x * gx1 + v01.x * fx) * gy1 + (v10.x * gx1 + v11.x * fx) * fy;
    const float gxw = (v00.y * gx1 + v01.y * fx) * gy1 + (v10.y * gx1 + v11.y * fx) * fy;
    const float gyw = (v00.z * gx1 + v01.z * fx) * gy1 + (v10.z * gx1 + v11.z * fx) * fy;
    float J[K];
    if constexpr (MODE == ST_ECC_TRANSLATION) {
      J[0] = gxw;
      J[1] = gyw;
    } else if constexpr (MODE == ST_ECC_EUCLIDEAN) {
      const float hx = (-(xf * m10)) - yf * m00;
      const float hy = xf * m00 - yf * m10;
      J[0] = gxw * hx + gyw * hy;
      J[1] = gxw;
      J[2] = gyw;
    } else {
      J[0] = gxw * xf;
      J[1] = gyw * xf;
      J[2] = gxw * yf;
      J[3] = gyw * yf;
      J[4] = gxw;
      J[5] = gyw;
    }
    // products of two fp32 values are exact in fp64, so the fused form rounds exactly as multiply-then-add would
    const double Id = (double)Iw, Td = (double)T[idx];
    double Jd[K];
#pragma unroll
    for (int i = 0; i < K; ++i) Jd[i] = (double)J[i];
    int h = 0;
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
      for (int j = i; j < K; ++j) {
        acc[h] = __builtin_fma(Jd[i], Jd[j], acc[h]);
        ++h;
      }
#pragma unroll
    for (int i = 0; i < K; ++i) {
      acc[NH + i] = __builtin_fma(Jd[i], Id, acc[NH + i]);
      acc[NH + K + i] = __builtin_fma(Jd[i], Td, acc[NH + K + i]);
      acc[NH + 2 * K + i] += Jd[i];
    }
    constexpr int B = NH + 3 * K;
    acc[B + 0] = __builtin_fma(Id, Td, acc[B + 0]);
    acc[B + 1] += Id;
    acc[B + 2] += Td;
    acc[B + 3] = __builtin_fma(Id, Id, acc[B + 3]);
    acc[B + 4] = __builtin_fma(Td, Td, acc[B + 4]);
    acc[B + 5] += 1.0;
  }

  __shared__ double red[kThreads / 64][NV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    double s = acc[v];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) red[wave][v] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double s = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) s += red[w][threadIdx.x];
    partials[((size_t)n * G + blockIdx.x) * kMaxVals + threadIdx.x] = s;
  }
}

// ---- E4, E6 .. E10 finalize: grid N, one wave ---------------------------------------------------------------------------
// Cholesky H = L L^T in place of H^-1; false when a pivot is not > 0 (singular, E10)
template <int K>
__device__ bool ecc_cholesky(const double (&H)[K][K], double (&L)[K][K]) {
  for (int j = 0; j < K; ++j) {
    double d = H[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0) || !isfinite(d)) return false;
    L[j][j] = sqrt(d);
    for (int i = j + 1; i < K; ++i) {
      double s = H[i][j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / L[j][j];
    }
  }
  return true;
}

template <int K>
__device__ void ecc_solve(const double (&L)[K][K], const double (&b)[K], double (&x)[K]) {
  double y[K];
  for (int i = 0; i < K; ++i) {
    double s = b[i];
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
  for (int i = K - 1; i >= 0; --i) {
    double s = y[i];
    for (int k = i + 1; k < K; ++k) s -= L[k][i] * x[k];
    x[i] = s / L[i][i];
  }
}

__device__ void ecc_write_row(float* row, bool valid, double rho, const double* M, int s) {
  if (!row) return;
  if (!valid) {
    const float f[ST_CMC_WARP_FLOATS] = {0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    for (int k = 0; k < ST_CMC_WARP_FLOATS; ++k) row[k] = f[k];
    return;
  }
  // plane pixel i sits at image coordinate s i + c, c = (s - 1) / 2: [A | t] -> [A | s t + c - A c]
  const double c = (s - 1) / 2.0;
  row[0] = 1.f;
  row[1] = (float)rho;
  row[2] = (float)M[0];
  row[3] = (float)M[1];
  row[4] = (float)(s * M[2] + c - (M[0] * c + M[1] * c));
  row[5] = (float)M[3];
  row[6] = (float)M[4];
  row[7] = (float)(s * M[5] + c - (M[3] * c + M[4] * c));
}

template <int MODE>
__global__ __launch_bounds__(64) void ecc_finalize_kernel(double* state, const double* __restrict__ partials, int G,
                                                          int num_iters, double eps, int downscale, float* warps_out,
                                                          int* iters_out, double* step_out) {
  constexpr int K = n_params(MODE), NH = K * (K + 1) / 2, NV = n_vals(MODE), B = NH + 3 * K;
  const int n = blockIdx.x, lane = threadIdx.x;
  double* st = state + (size_t)n * kState;
  if (st[kDone] != 0.0) return;
  __shared__ double S[kMaxVals];
  if (lane < NV) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += partials[((size_t)n * G + g) * kMaxVals + lane];     // workgroup order: fixed
    S[lane] = s;
  }
  __syncthreads();
  if (lane != 0) return;

  double* d = step_out ? step_out + (size_t)n * ST_ECC_STEP_DOUBLES : nullptr;
  if (d)
    for (int k = 0; k < ST_ECC_STEP_DOUBLES; ++k) d[k] = 0.0;
  const int iters = (int)st[kIters] + 1;
  st[kIters] = (double)iters;
  float* row = warps_out ? warps_out + (size_t)n * ST_CMC_WARP_FLOATS : nullptr;
  double M[6];
  for (int k = 0; k < 6; ++k) M[k] = st[k];
  if (d)
    for (int k = 0; k < 6; ++k) d[ST_ECC_STEP_WARP + k] = M[k];

  bool ok = false;
  double rho = 0.0;
  do {
    const double cnt = S[B + 5];
    if (d) d[ST_ECC_STEP_N] = cnt;
    if (cnt == 0.0) break;
    const double sI = S[B + 1], sT = S[B + 2];
    const double mean_i = sI / cnt, mean_t = sT / cnt;
    const double std_i = sqrt((S[B + 3] - sI * mean_i) / cnt), std_t = sqrt((S[B + 4] - sT * mean_t) / cnt);
    const double img_norm = sqrt(cnt * std_i * std_i), tmp_norm = sqrt(cnt * std_t * std_t);
    const double corr = S[B + 0] - sI * mean_t;
    double H[K][K], iP[K], tP[K];
    int h = 0;
    for (int i = 0; i < K; ++i)
      for (int j = i; j < K; ++j) H[i][j] = H[j][i] = S[h++];
    for (int i = 0; i < K; ++i) {
      iP[i] = S[NH + i] - mean_i * S[NH + 2 * K + i];
      tP[i] = S[NH + K + i] - mean_t * S[NH + 2 * K + i];
    }
    rho = corr / (img_norm * tmp_norm);
    if (d) {
      d[ST_ECC_STEP_MEAN_I] = mean_i;
      d[ST_ECC_STEP_MEAN_T] = mean_t;
      d[ST_ECC_STEP_STD_I] = std_i;
      d[ST_ECC_STEP_STD_T] = std_t;
      d[ST_ECC_STEP_IMG_NORM] = img_norm;
      d[ST_ECC_STEP_TMP_NORM] = tmp_norm;
      d[ST_ECC_STEP_CORR] = corr;
      d[ST_ECC_STEP_RHO] = rho;
      for (int i = 0; i < K; ++i) {
        for (int j = 0; j < K; ++j) d[ST_ECC_STEP_H + i * 6 + j] = H[i][j];
        d[ST_ECC_STEP_IP + i] = iP[i];
        d[ST_ECC_STEP_TP + i] = tP[i];
      }
    }
    if (!isfinite(rho)) break;
    double L[K][K], a[K], b[K];
    if (!ecc_cholesky<K>(H, L)) break;
    ecc_solve<K>(L, iP, a);
    ecc_solve<K>(L, tP, b);
    double ipa = 0.0, tpa = 0.0;
    for (int i = 0; i < K; ++i) {
      ipa += iP[i] * a[i];
      tpa += tP[i] * a[i];
    }
    const double den = corr - tpa;
    if (!(den > 0.0)) break;
    const double lam = (img_norm * img_norm - ipa) / den;
    double dp[K];
    for (int i = 0; i < K; ++i) dp[i] = lam * b[i] - a[i];
    // E8
    if constexpr (MODE == ST_ECC_TRANSLATION) {
      M[2] += dp[0];
      M[5] += dp[1];
    } else if constexpr (MODE == ST_ECC_EUCLIDEAN) {
      const double th = asin(fmin(fmax(M[3], -1.0), 1.0)) + dp[0];
      M[2] += dp[1];
      M[5] += dp[2];
      M[0] = M[4] = cos(th);
      M[3] = sin(th);
      M[1] = -M[3];
    } else {
      M[0] += dp[0];
      M[3] += dp[1];
      M[1] += dp[2];
      M[4] += dp[3];
      M[2] += dp[4];
      M[5] += dp[5];
    }
    ok = true;
    if (d) {
      d[ST_ECC_STEP_LAMBDA] = lam;
      for (int i = 0; i < K; ++i) d[ST_ECC_STEP_DP + i] = dp[i];
      for (int k = 0; k < 6; ++k) d[ST_ECC_STEP_WARP + k] = M[k];
    }
  } while (false);
  if (d) d[ST_ECC_STEP_VALID] = ok ? 1.0 : 0.0;

  if (!ok) {                                         // E10
    st[kDone] = 1.0;
    ecc_write_row(row, false, 0.0, M, downscale);
    if (iters_out) iters_out[n] = iters;
    return;
  }
  const double last = st[kRho];
  st[kLast] = last;
  st[kRho] = rho;
  for (int k = 0; k < 6; ++k) st[k] = M[k];
  if (iters >= num_iters || fabs(rho - last) < eps) {   // E9: the test that would open the next iteration
    st[kDone] = 1.0;
    ecc_write_row(row, true, rho, M, downscale);
    if (iters_out) iters_out[n] = iters;
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
size_t align256(size_t b) { return (b + 255) / 256 * 256; }

struct Layout {
  int P, G;
  size_t tb, ib, ig, partials, state, total;
};

Layout layout(int N, int ph, int pw) {
  Layout l{};
  l.P = ph * pw;
  l.G = st::ceil_div(l.P, kWgPixels);
  size_t o = 0;
  l.tb = o; o += align256((size_t)N * l.P * sizeof(float));
  l.ib = o; o += align256((size_t)N * l.P * sizeof(float));
  l.ig = o; o += align256((size_t)N * l.P * sizeof(float4));
  l.partials = o; o += align256((size_t)N * l.G * kMaxVals * sizeof(double));
  l.state = o; o += align256((size_t)N * kState * sizeof(double));
  l.total = o;
  return l;
}

bool downscale_ok(int s) { return s == 1 || s == 2 || s == 4; }

int require_args(const char* who, const StEccParams* prm, int N, int img_h, int img_w, const void* a, const void* b,
                 const void* ws, size_t ws_bytes, int* ph, int* pw) {
  using namespace st;
  ST_REQUIRE(prm && prm->struct_size == (int)sizeof(StEccParams), "%s: params struct_size mismatch", who);
  ST_REQUIRE(a && b && ws, "%s: null pointer", who);
  ST_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: workspace must be 16-byte aligned", who);   // float4 gradients
  ST_REQUIRE(N > 0 && N <= 65535 && img_h > 0 && img_w > 0, "%s: bad argument", who);
  ST_REQUIRE(prm->warp_mode >= ST_ECC_TRANSLATION && prm->warp_mode <= ST_ECC_AFFINE,
             "%s: warp_mode %d is not TRANSLATION, EUCLIDEAN or AFFINE", who, prm->warp_mode);
  ST_REQUIRE(downscale_ok(prm->downscale), "%s: downscale %d must be 1, 2 or 4", who, prm->downscale);
  ST_REQUIRE(prm->gauss_filt_size == 1 || prm->gauss_filt_size == 3 || prm->gauss_filt_size == 5,
             "%s: gauss_filt_size %d must be 1, 3 or 5", who, prm->gauss_filt_size);
  ST_REQUIRE(prm->num_iters >= 1, "%s: num_iters %d must be >= 1", who, prm->num_iters);
  ST_REQUIRE(prm->stop_eps == prm->stop_eps, "%s: stop_eps is NaN", who);
  *ph = img_h / prm->downscale;
  *pw = img_w / prm->downscale;
  ST_REQUIRE(*ph >= 8 && *pw >= 8, "%s: plane %d x %d has a side under 8", who, *ph, *pw);
  ST_REQUIRE((long long)*ph * *pw <= (1LL << 30), "%s: plane too large", who);
  ST_REQUIRE(ws_bytes >= layout(N, *ph, *pw).total, "%s: workspace %zu < %zu bytes", who, ws_bytes,
             layout(N, *ph, *pw).total);
  return ST_OK;
}

int launch_prepare(const float* prev, const float* curr, int N, int ph, int pw, int gauss, unsigned char* ws,
                   hipStream_t s) {
  const Layout l = layout(N, ph, pw);
  BlurTaps t{};
  t.r = gauss / 2;
  if (gauss == 1) t.k[0] = 1.f;
  if (gauss == 3) { t.k[0] = 0.25f; t.k[1] = 0.5f; t.k[2] = 0.25f; }
  if (gauss == 5) { t.k[0] = 0.0625f; t.k[1] = 0.25f; t.k[2] = 0.375f; t.k[3] = 0.25f; t.k[4] = 0.0625f; }
  const unsigned gx = (unsigned)st::ceil_div(l.P, kThreads);
  float* Tb = reinterpret_cast<float*>(ws + l.tb);
  float* Ib = reinterpret_cast<float*>(ws + l.ib);
  hipLaunchKernelGGL(ecc_blur_kernel, dim3(gx, 2 * N), dim3(kThreads), 0, s, prev, curr, N, ph, pw, t, Tb, Ib);
  hipLaunchKernelGGL(ecc_grad_kernel, dim3(gx, N), dim3(kThreads), 0, s, Ib, ph, pw, reinterpret_cast<float4*>(ws + l.ig));
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

template <int MODE>
void launch_round(const Layout& l, int N, int ph, int pw, const StEccParams* prm, int num_iters, unsigned char* ws,
                  float* warps_out, int* iters_out, double* step_out, hipStream_t s) {
  double* state = reinterpret_cast<double*>(ws + l.state);
  double* partials = reinterpret_cast<double*>(ws + l.partials);
  hipLaunchKernelGGL(ecc_iterate_kernel<MODE>, dim3(l.G, N), dim3(kThreads), 0, s,
                     reinterpret_cast<const float*>(ws + l.tb), reinterpret_cast<const float4*>(ws + l.ig), ph, pw, state,
                     partials);
  hipLaunchKernelGGL(ecc_finalize_kernel<MODE>, dim3(N), dim3(64), 0, s, state, partials, l.G, num_iters,
                     (double)prm->stop_eps, prm->downscale, warps_out, iters_out, step_out);
}

// init + `rounds` x (iterate, finalize), all enqueued; the planes are already prepared in the workspace
int launch_rounds(int N, int ph, int pw, const StEccParams* prm, int rounds, const double* warps_in, unsigned char* ws,
                  float* warps_out, int* iters_out, double* step_out, hipStream_t s) {
  const Layout l = layout(N, ph, pw);
  hipLaunchKernelGGL(ecc_init_kernel, dim3(st::ceil_div(N, 64)), dim3(64), 0, s, N, warps_in, (double)prm->stop_eps,
                     reinterpret_cast<double*>(ws + l.state));
  for (int r = 0; r < rounds; ++r) {
    if (prm->warp_mode == ST_ECC_TRANSLATION)
      launch_round<ST_ECC_TRANSLATION>(l, N, ph, pw, prm, rounds, ws, warps_out, iters_out, step_out, s);
    else if (prm->warp_mode == ST_ECC_EUCLIDEAN)
      launch_round<ST_ECC_EUCLIDEAN>(l, N, ph, pw, prm, rounds, ws, warps_out, iters_out, step_out, s);
    else
      launch_round<ST_ECC_AFFINE>(l, N, ph, pw, prm, rounds, ws, warps_out, iters_out, step_out, s);
  }
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

}  // namespace

extern "C" int st_cmc_ecc_plane_size(int img_h, int img_w, int downscale, int* plane_h, int* plane_w) {
  using namespace st;
  ST_REQUIRE(plane_h && plane_w && img_h > 0 && img_w > 0 && downscale_ok(downscale), "st_cmc_ecc_plane_size: bad argument");
  *plane_h = img_h / downscale;
  *plane_w = img_w / downscale;
  return ST_OK;
}

extern "C" size_t st_cmc_ecc_workspace_bytes(int N, int plane_h, int plane_w) {
  return N > 0 && plane_h > 0 && plane_w > 0 ? layout(N, plane_h, plane_w).total : 0;
}

extern "C" int st_cmc_ecc_front_u8(const void* const* frames_u8_dev_ptrs_host, int N, int fh, int fw, int h, int w,
                                   int downscale, float* planes_dev, st_stream_t stream) {
  using namespace st;
  ST_REQUIRE(frames_u8_dev_ptrs_host && planes_dev && N > 0 && h > 0 && w > 0 && h <= fh && w <= fw,
             "st_cmc_ecc_front_u8: bad argument");
  ST_REQUIRE(downscale_ok(downscale) && h / downscale > 0 && w / downscale > 0,
             "st_cmc_ecc_front_u8: downscale %d must be 1, 2 or 4 and leave a plane", downscale);
  for (int i = 0; i < N; ++i)     // every frame before the first launch: a refused call has launched nothing
    ST_REQUIRE(frames_u8_dev_ptrs_host[i], "st_cmc_ecc_front_u8: frame %d is null", i);
  const int ph = h / downscale, pw = w / downscale;
  for (int base = 0; base < N; base += kMaxFrames) {
    const int k = N - base < kMaxFrames ? N - base : kMaxFrames;
    FramePtrs fp{};
    for (int i = 0; i < k; ++i) fp.p[i] = static_cast<const unsigned char*>(frames_u8_dev_ptrs_host[base + i]);
    hipLaunchKernelGGL(ecc_front_u8_kernel, dim3(ceil_div(ph * pw, kThreads), k), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), fp, fh, fw, ph, pw, downscale,
                       planes_dev + (size_t)base * ph * pw);
  }
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

extern "C" int st_cmc_ecc_front_f32(const float* batch_dev, int N, int H, int W, int h, int w, int downscale,
                                    float* planes_dev, st_stream_t stream) {
  using namespace st;
  ST_REQUIRE(batch_dev && planes_dev && N > 0 && N <= 65535 && h > 0 && w > 0 && h <= H && w <= W,
             "st_cmc_ecc_front_f32: bad argument");
  ST_REQUIRE(downscale_ok(downscale) && h / downscale > 0 && w / downscale > 0,
             "st_cmc_ecc_front_f32: downscale %d must be 1, 2 or 4 and leave a plane", downscale);
  const int ph = h / downscale, pw = w / downscale;
  hipLaunchKernelGGL(ecc_front_f32_kernel, dim3(ceil_div(ph * pw, kThreads), N), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), batch_dev, H, W, ph, pw, downscale, planes_dev);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

extern "C" int st_cmc_ecc_prepare(const float* prev_planes_dev, const float* curr_planes_dev, int N, int img_h, int img_w,
                                  const StEccParams* prm, void* ws, size_t ws_bytes, float* tmpl_out_dev,
                                  float* input_out_dev, float* gx_out_dev, float* gy_out_dev, st_stream_t stream) {
  int ph, pw;
  ST_CHECK(require_args("st_cmc_ecc_prepare", prm, N, img_h, img_w, prev_planes_dev, curr_planes_dev, ws, ws_bytes, &ph,
                        &pw));
  const hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char* w8 = static_cast<unsigned char*>(ws);
  ST_CHECK(launch_prepare(prev_planes_dev, curr_planes_dev, N, ph, pw, prm->gauss_filt_size, w8, s));
  const Layout l = layout(N, ph, pw);
  if (tmpl_out_dev)
    ST_CHECK_HIP(hipMemcpyAsync(tmpl_out_dev, w8 + l.tb, (size_t)N * l.P * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (input_out_dev || gx_out_dev || gy_out_dev) {
    hipLaunchKernelGGL(ecc_unpack_kernel, dim3(st::ceil_div(l.P, kThreads), N), dim3(kThreads), 0, s,
                       reinterpret_cast<const float4*>(w8 + l.ig), l.P, input_out_dev, gx_out_dev, gy_out_dev);
    ST_CHECK_HIP(hipGetLastError());
  }
  return ST_OK;
}

extern "C" int st_cmc_ecc_step(const float* prev_planes_dev, const float* curr_planes_dev, int N, int img_h, int img_w,
                               const StEccParams* prm, const double* warps_in_dev, void* ws, size_t ws_bytes,
                               double* step_out_dev, st_stream_t stream) {
  using namespace st;
  int ph, pw;
  ST_CHECK(require_args("st_cmc_ecc_step", prm, N, img_h, img_w, prev_planes_dev, curr_planes_dev, ws, ws_bytes, &ph, &pw));
  ST_REQUIRE(step_out_dev, "st_cmc_ecc_step: null pointer");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char* w8 = static_cast<unsigned char*>(ws);
  ST_CHECK(launch_prepare(prev_planes_dev, curr_planes_dev, N, ph, pw, prm->gauss_filt_size, w8, s));
  return launch_rounds(N, ph, pw, prm, 1, warps_in_dev, w8, nullptr, nullptr, step_out_dev, s);
}

extern "C" int st_cmc_ecc_estimate(const float* prev_planes_dev, const float* curr_planes_dev, int N, int img_h,
                                   int img_w, const StEccParams* prm, void* ws, size_t ws_bytes, float* warps_out_dev,
                                   int* iters_out_dev, st_stream_t stream) {
  using namespace st;
  int ph, pw;
  ST_CHECK(require_args("st_cmc_ecc_estimate", prm, N, img_h, img_w, prev_planes_dev, curr_planes_dev, ws, ws_bytes, &ph,
                        &pw));
  ST_REQUIRE(warps_out_dev, "st_cmc_ecc_estimate: null pointer");
  ST_REQUIRE(prm->num_iters <= 1000, "st_cmc_ecc_estimate: num_iters %d > 1000", prm->num_iters);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char* w8 = static_cast<unsigned char*>(ws);
  ST_CHECK(launch_prepare(prev_planes_dev, curr_planes_dev, N, ph, pw, prm->gauss_filt_size, w8, s));
  return launch_rounds(N, ph, pw, prm, prm->num_iters, nullptr, w8, warps_out_dev, iters_out_dev, nullptr, s);
}
