// Mesh-Affine camera-motion compensation (CMC) of the tracker: the estimate half, on the device.
//
// Behavioural spec (file:line in the reference): OCSORTTracker_Disparity.estimate_camera_motion
// (mmtrack/models/trackers/ocsort_tracker_disparity.py:87-97) -> gmc.glme_affine_warp (gmc.py:7-17) -> GLME_affine
// (utils.py:6-55): crop the uint8 cast of the preprocessed BGR batch to img_shape, swap to RGB, cv2.resize to 255 x 255
// (INTER_LINEAR, 8-bit), COLOR_RGB2GRAY + equalizeHist, calcOpticalFlowFarneback(pyr_scale 0.5, levels 5, winsize,
// iterations 3, poly_n 5, poly_sigma 1.2, flags 0), flow scaled by (w / 255, h / 255), per-component medians over
// step x step cells, estimateAffinePartial2D(RANSAC) over the cell centres.
//
// OpenCV is an un-vendored dependency and absent; every rule below is restated from the published algorithm (OpenCV
// imgproc / video sources) [upstream-memory], PARITY UNPINNED against cv2 itself.  tests/cmc_ref.py restates the same
// rules in numpy (fp32 / fp64) and tests/test_cmc_gpu.py holds these kernels to it.
//
//   front     resize: the 8-bit INTER_LINEAR arithmetic of st_resize_planes (pack_pool.hip); grey: fixed point
//             (R * 9798 + G * 19235 + B * 3735 + (1 << 14)) >> 15 [upstream-memory]; equalizeHist: first non-empty bin
//             i0, lut[i0] = 0, lut[i] = cvRound((float)cumsum(hist[i0+1..i]) * (255.f / (float)(total - hist[i0]))),
//             a single-valued image maps to its own value.  Integer output: bit-exact against the restatement.
//   pyramid   levels while 255 * 0.5^k >= 32 (OpenCV's min_size; unrounded test): k = 0, 1, 2 -> 255, 128, 64 (sizes
//             cvRound(255 * 0.5^k)).  Each level is blurred from the FULL-resolution float image (not cascaded):
//             sigma = (1 / scale - 1) / 2, ksize = max(cvRound(5 sigma) | 1, 3), separable, BORDER_REFLECT_101;
//             sigma 0 (level 0) takes cv2's fixed 3-tap kernel {1/4, 1/2, 1/4}; then float INTER_LINEAR to the level size.
//   poly exp  poly_n 5 -> 11-tap separable Gaussian (sigma 1.2) moments, 1/G from the 6 x 6 moment matrix (host, double);
//             rows and columns clamped at the border (replicate).  5 coefficients per pixel (ry, rx, ryy, rxx, rxy).
//   matrices  the second image's coefficients sampled bilinearly at x + flow when (floor) inside [0, size - 1), else
//             zero linear part / own quadratic part; averaged with the first image's; pixels within 5 of a border
//             scaled by {0.14, 0.14, 0.4472, 0.4472, 0.4472} per side.  -> G11, G12, G22, h1, h2.
//   blur      flags 0: box of winsize x winsize, rows and columns clamped at the border (replicate).
//   solve     flow = ((g11 h2 - g12 h1), (g22 h1 - g12 h2)) / (g11 g22 - g12^2 + 1e-3), in double; the matrices are
//             rebuilt from the new flow after every iteration but the last.
//   levels    flow of level k+1 resized (float INTER_LINEAR) to level k and multiplied by 1 / pyr_scale = 2.
//   mesh      per-component median of the step x step cells of the flow (np.median of an even count: the mean of the
//             two middle values), scaled in double; src = (float)((c + 0.5) * step * s), dst = (float)(src + median).
//   fit       DEVIATION (stated): OpenCV's RANSAC draws from its own RNG.  Here every two-point similarity
//             hypothesis (i < j) is scored against every point (inlier: squared residual <= thr^2, fp32), the largest
//             consensus set wins (ties: the lowest (i, j)), and the 4-DOF model [a -b tx; b a ty] is refitted to it by
//             linear least squares (closed form, double).  inlier ratio = |set| / points; valid = ratio >= min ratio.
#include <cmath>
#include <cstdint>
#include <vector>

#include "st_common.h"

namespace {

constexpr int kSide = ST_CMC_SIDE;
constexpr int kPlane = kSide * kSide;
constexpr int kMaxLevels = 4;
constexpr int kMaxBlur = 15;          // taps of the widest pyramid blur (9 at the 3 levels of a 255 image)
constexpr int kPolyN = 5;
constexpr int kMaxFrames = 32;
constexpr int kMaxPoints = 1024;

struct FramePtrs { const unsigned char* p[kMaxFrames]; };

// ---- front: crop + channel swap + 8-bit INTER_LINEAR to 255 x 255 + grey + equalizeHist, one workgroup per frame ---
__device__ __forceinline__ void cmc_tap(int d, double scale, int n, int& s, int& a0, int& a1) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int i = (int)floorf(f);
  f -= (float)i;
  if (i < 0) { f = 0.f; i = 0; }
  if (i >= n - 1) { f = 0.f; i = n - 1; }
  s = i;
  a0 = __float2int_rn((1.f - f) * 2048.f);
  a1 = __float2int_rn(f * 2048.f);
}

template <typename T>
__device__ __forceinline__ int cmc_px(const T* p) {
  if constexpr (sizeof(T) == 1) {
    return (int)*p;
  } else {
    const int v = (int)*p;          // numpy astype(uint8) of the integral values the preprocessor produces
    return min(max(v, 0), 255);
  }
}

template <typename T>
__device__ void cmc_front_body(const T* src, long long plane_stride, int row_stride, int h, int w, unsigned char* out) {
  __shared__ unsigned char grey[kPlane];
  __shared__ int hist[256];
  __shared__ unsigned char lut[256];
  const int tid = threadIdx.x;
  for (int i = tid; i < 256; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  const double sx = (double)w / kSide, sy = (double)h / kSide;
  for (int p = tid; p < kPlane; p += blockDim.x) {
    const int dy = p / kSide, dx = p - dy * kSide;
    int xs, ax0, ax1;
    cmc_tap(dx, sx, w, xs, ax0, ax1);
    float fy = (float)(((double)dy + 0.5) * sy - 0.5);
    const int ys = (int)floorf(fy);
    fy -= (float)ys;
    const int b0 = __float2int_rn((1.f - fy) * 2048.f), b1 = __float2int_rn(fy * 2048.f);
    const int y0 = min(max(ys, 0), h - 1), y1 = min(max(ys + 1, 0), h - 1);
    const int x1 = min(xs + 1, w - 1);
    int ch[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const T* pl = src + c * plane_stride;
      const T* r0 = pl + (long long)y0 * row_stride;
      const T* r1 = pl + (long long)y1 * row_stride;
      const int S0 = cmc_px(r0 + xs) * ax0 + cmc_px(r0 + x1) * ax1;
      const int S1 = cmc_px(r1 + xs) * ax0 + cmc_px(r1 + x1) * ax1;
      const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
      ch[c] = min(max(v, 0), 255);
    }
    // the batch is BGR: after the swap to RGB, R = channel 2, B = channel 0
    const int g = (ch[2] * 9798 + ch[1] * 19235 + ch[0] * 3735 + (1 << 14)) >> 15;
    grey[p] = (unsigned char)g;
    atomicAdd(&hist[g], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int i = 0;
    while (hist[i] == 0) ++i;
    if (hist[i] == kPlane) {
      for (int k = 0; k < 256; ++k) lut[k] = (unsigned char)i;
    } else {
      const float scale = 255.f / (float)(kPlane - hist[i]);
      int sum = 0;
      for (int k = 0; k <= i; ++k) lut[k] = 0;
      for (int k = i + 1; k < 256; ++k) {
        sum += hist[k];
        const int v = __float2int_rn((float)sum * scale);
        lut[k] = (unsigned char)min(max(v, 0), 255);
      }
    }
  }
  __syncthreads();
  for (int p = tid; p < kPlane; p += blockDim.x) out[p] = lut[grey[p]];
}

__global__ __launch_bounds__(1024) void cmc_front_u8_kernel(FramePtrs fp, int fh, int fw, int h, int w,
                                                            unsigned char* planes) {
  const int n = blockIdx.x;
  cmc_front_body<unsigned char>(fp.p[n], (long long)fh * fw, fw, h, w, planes + (size_t)n * kPlane);
}

__global__ __launch_bounds__(1024) void cmc_front_f32_kernel(const float* batch, int H, int W, int h, int w,
                                                             unsigned char* planes) {
  const int n = blockIdx.x;
  cmc_front_body<float>(batch + (size_t)n * 3 * H * W, (long long)H * W, W, h, w, planes + (size_t)n * kPlane);
}

// ---- Farneback ------------------------------------------------------------------------------------------------------
struct Level {
  int w, h;
  int ksize;                    // pyramid blur taps
  float kern[kMaxBlur];
  long long off;                // pixel offset of this level inside a pair's per-level arrays
};

struct FlowGeom {
  int L;                        // levels used (coarsest = L - 1)
  Level lv[kMaxLevels];
  long long S;                  // pixels of all levels of one pair
  float g[kPolyN + 1], xg[kPolyN + 1], xxg[kPolyN + 1];
  float ig11, ig03, ig33, ig55;
};

// per-pair workspace (floats): I 2S | R 10S | M 5S | V 5 * 255^2 | flow 2S
__host__ __device__ inline long long pair_floats(long long S) { return 2 * S + 10 * S + 5 * S + 5LL * kPlane + 2 * S; }

struct PairWs {
  float *I, *R, *M, *V, *F;
};
__device__ __forceinline__ PairWs pair_ws(float* ws, const FlowGeom& g, int n) {
  float* b = ws + (long long)n * pair_floats(g.S);
  PairWs p;
  p.I = b;
  p.R = p.I + 2 * g.S;
  p.M = p.R + 10 * g.S;
  p.V = p.M + 5 * g.S;
  p.F = p.V + 5LL * kPlane;
  return p;
}

__device__ __forceinline__ int reflect101(int p, int n) {
  if (p < 0) p = -p;
  if (p >= n) p = 2 * n - 2 - p;
  return p;
}

__device__ __forceinline__ void flt_tap(int d, double scale, int n, int& s, float& f) {
  f = (float)(((double)d + 0.5) * scale - 0.5);
  s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= n - 1) { f = 0.f; s = n - 1; }
}

// blurred full-resolution image at (y, x): rows filtered first, then the column (cv2 sepFilter2D order)
__device__ float blurred_at(const unsigned char* img, const Level& L, int y, int x) {
  const int r = L.ksize / 2;
  float acc = 0.f;
  for (int j = 0; j < L.ksize; ++j) {
    const unsigned char* row = img + reflect101(y + j - r, kSide) * kSide;
    float hsum = 0.f;
    for (int i = 0; i < L.ksize; ++i) hsum = hsum + L.kern[i] * (float)row[reflect101(x + i - r, kSide)];
    acc = acc + L.kern[j] * hsum;
  }
  return acc;
}

// grid (ceil(max level pixels / 256), L, 2 * N): the level-k image of both frames of every pair
__global__ __launch_bounds__(256) void cmc_pyramid_kernel(const unsigned char* prev, const unsigned char* curr,
                                                          FlowGeom g, float* ws) {
  const int l = blockIdx.y, n = blockIdx.z >> 1, im = blockIdx.z & 1;
  const Level& L = g.lv[l];
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= L.w * L.h) return;
  const int y = p / L.w, x = p - y * L.w;
  const unsigned char* img = (im ? curr : prev) + (size_t)n * kPlane;
  int xs, ys;
  float fx, fy;
  flt_tap(x, (double)kSide / L.w, kSide, xs, fx);
  // rows: fraction kept, index clamped (cv2 resize's row rule)
  fy = (float)(((double)y + 0.5) * ((double)kSide / L.h) - 0.5);
  ys = (int)floorf(fy);
  fy -= (float)ys;
  const int y0 = min(max(ys, 0), kSide - 1), y1 = min(max(ys + 1, 0), kSide - 1), x1 = min(xs + 1, kSide - 1);
  const float S0 = blurred_at(img, L, y0, xs) * (1.f - fx) + blurred_at(img, L, y0, x1) * fx;
  const float S1 = blurred_at(img, L, y1, xs) * (1.f - fx) + blurred_at(img, L, y1, x1) * fx;
  PairWs w = pair_ws(ws, g, n);
  w.I[im * g.S + L.off + p] = S0 * (1.f - fy) + S1 * fy;
}

// grid (ceil(max level pixels / 256), L, 2 * N): polynomial expansion (5 coefficients) of every level image
__global__ __launch_bounds__(256) void cmc_polyexp_kernel(FlowGeom g, float* ws) {
  const int l = blockIdx.y, n = blockIdx.z >> 1, im = blockIdx.z & 1;
  const Level& L = g.lv[l];
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= L.w * L.h) return;
  const int y = p / L.w, x = p - y * L.w;
  PairWs w = pair_ws(ws, g, n);
  const float* I = w.I + im * g.S + L.off;
  double b1 = 0, b2 = 0, b3 = 0, b4 = 0, b5 = 0, b6 = 0;
  for (int k = -kPolyN; k <= kPolyN; ++k) {
    const int xx = min(max(x + k, 0), L.w - 1);
    // vertical part at column xx: sum g, sum xg (odd), sum xxg
    float v0 = I[y * L.w + xx] * g.g[0], v1 = 0.f, v2 = 0.f;
    for (int j = 1; j <= kPolyN; ++j) {
      const float a = I[max(y - j, 0) * L.w + xx], b = I[min(y + j, L.h - 1) * L.w + xx];
      const float s = a + b;
      v0 = v0 + g.g[j] * s;
      v1 = v1 + g.xg[j] * (b - a);
      v2 = v2 + g.xxg[j] * s;
    }
    const int ak = k < 0 ? -k : k;
    const double gk = g.g[ak], xgk = (k < 0 ? -1.0 : 1.0) * (double)g.xg[ak], xxgk = g.xxg[ak];
    b1 += (double)v0 * gk;
    b2 += (double)v0 * xgk;
    b3 += (double)v1 * gk;
    b4 += (double)v0 * xxgk;
    b5 += (double)v2 * gk;
    b6 += (double)v1 * xgk;
  }
  float* R = w.R + (im * g.S + L.off + p) * 5;
  R[0] = (float)(b3 * g.ig11);
  R[1] = (float)(b2 * g.ig11);
  R[2] = (float)(b1 * g.ig03 + b5 * g.ig33);
  R[3] = (float)(b1 * g.ig03 + b4 * g.ig33);
  R[4] = (float)(b6 * g.ig55);
}

__device__ __forceinline__ float border_w(int i) {
  return i == 0 || i == 1 ? 0.14f : 0.4472f;
}

// the update matrices of one pixel from its own flow (dx, dy)
__device__ void update_matrices(const float* R0, const float* R1, int w, int h, int x, int y, float dx, float dy,
                                float* M) {
  const float* r0 = R0 + ((long long)y * w + x) * 5;
  float fx = x + dx, fy = y + dy;
  const int x1 = (int)floorf(fx), y1 = (int)floorf(fy);
  fx -= x1;
  fy -= y1;
  float r2, r3, r4, r5, r6;
  if ((unsigned)x1 < (unsigned)(w - 1) && (unsigned)y1 < (unsigned)(h - 1)) {
    const float* p = R1 + ((long long)y1 * w + x1) * 5;
    const float* q = p + (long long)w * 5;
    const float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
    r2 = a00 * p[0] + a01 * p[5] + a10 * q[0] + a11 * q[5];
    r3 = a00 * p[1] + a01 * p[6] + a10 * q[1] + a11 * q[6];
    r4 = a00 * p[2] + a01 * p[7] + a10 * q[2] + a11 * q[7];
    r5 = a00 * p[3] + a01 * p[8] + a10 * q[3] + a11 * q[8];
    r6 = a00 * p[4] + a01 * p[9] + a10 * q[4] + a11 * q[9];
    r4 = (r0[2] + r4) * 0.5f;
    r5 = (r0[3] + r5) * 0.5f;
    r6 = (r0[4] + r6) * 0.25f;
  } else {
    r2 = r3 = 0.f;
    r4 = r0[2];
    r5 = r0[3];
    r6 = r0[4] * 0.5f;
  }
  r2 = (r0[0] - r2) * 0.5f;
  r3 = (r0[1] - r3) * 0.5f;
  r2 += r4 * dy + r6 * dx;
  r3 += r6 * dy + r5 * dx;
  constexpr int B = 5;
  if ((unsigned)(x - B) >= (unsigned)(w - 2 * B) || (unsigned)(y - B) >= (unsigned)(h - 2 * B)) {
    const float s = (x < B ? border_w(x) : 1.f) * (x >= w - B ? border_w(w - x - 1) : 1.f) *
                    (y < B ? border_w(y) : 1.f) * (y >= h - B ? border_w(h - y - 1) : 1.f);
    r2 *= s; r3 *= s; r4 *= s; r5 *= s; r6 *= s;
  }
  M[0] = r4 * r4 + r6 * r6;
  M[1] = (r4 + r5) * r6;
  M[2] = r5 * r5 + r6 * r6;
  M[3] = r4 * r2 + r6 * r3;
  M[4] = r6 * r2 + r5 * r3;
}

// grid (ceil(pixels / 256), N): level l's initial flow (zero at the coarsest level, else the next coarser level's
// flow resized and doubled) and its update matrices
__global__ __launch_bounds__(256) void cmc_level_init_kernel(FlowGeom g, int l, float* ws) {
  const Level& L = g.lv[l];
  const int n = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= L.w * L.h) return;
  const int y = p / L.w, x = p - y * L.w;
  PairWs w = pair_ws(ws, g, n);
  float dx = 0.f, dy = 0.f;
  if (l + 1 < g.L) {
    const Level& C = g.lv[l + 1];
    const float* pf = w.F + 2 * C.off;
    int xs;
    float fx;
    flt_tap(x, (double)C.w / L.w, C.w, xs, fx);
    float fy = (float)(((double)y + 0.5) * ((double)C.h / L.h) - 0.5);
    const int ys = (int)floorf(fy);
    fy -= (float)ys;
    const int y0 = min(max(ys, 0), C.h - 1), y1 = min(max(ys + 1, 0), C.h - 1), x1 = min(xs + 1, C.w - 1);
    float v[2];
    for (int c = 0; c < 2; ++c) {
      const float S0 = pf[(y0 * C.w + xs) * 2 + c] * (1.f - fx) + pf[(y0 * C.w + x1) * 2 + c] * fx;
      const float S1 = pf[(y1 * C.w + xs) * 2 + c] * (1.f - fx) + pf[(y1 * C.w + x1) * 2 + c] * fx;
      v[c] = (float)((double)(S0 * (1.f - fy) + S1 * fy) * 2.0);
    }
    dx = v[0];
    dy = v[1];
  }
  w.F[2 * (L.off + p)] = dx;
  w.F[2 * (L.off + p) + 1] = dy;
  update_matrices(w.R + 5 * L.off, w.R + 5 * (g.S + L.off), L.w, L.h, x, y, dx, dy, w.M + 5 * (L.off + p));
}

// grid (ceil(pixels / 256), N): vertical half of the winsize box (rows clamped)
__global__ __launch_bounds__(256) void cmc_vblur_kernel(FlowGeom g, int l, int m, float* ws) {
  const Level& L = g.lv[l];
  const int n = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= L.w * L.h) return;
  const int y = p / L.w, x = p - y * L.w;
  PairWs w = pair_ws(ws, g, n);
  const float* M = w.M + 5 * L.off;
  float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int d = -m; d <= m; ++d) {
    const float* r = M + ((long long)min(max(y + d, 0), L.h - 1) * L.w + x) * 5;
#pragma unroll
    for (int c = 0; c < 5; ++c) s[c] += r[c];
  }
#pragma unroll
  for (int c = 0; c < 5; ++c) w.V[(long long)p * 5 + c] = s[c];
}

// grid (ceil(pixels / 256), N): horizontal half of the box (columns clamped), the regularised 2 x 2 solve, and - but
// after the last iteration - the update matrices from the new flow
__global__ __launch_bounds__(256) void cmc_hsolve_kernel(FlowGeom g, int l, int m, int update, float* ws) {
  const Level& L = g.lv[l];
  const int n = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= L.w * L.h) return;
  const int y = p / L.w, x = p - y * L.w;
  PairWs w = pair_ws(ws, g, n);
  double s[5] = {0, 0, 0, 0, 0};
  for (int d = -m; d <= m; ++d) {
    const float* r = w.V + ((long long)y * L.w + min(max(x + d, 0), L.w - 1)) * 5;
#pragma unroll
    for (int c = 0; c < 5; ++c) s[c] += (double)r[c];
  }
  const double sc = 1.0 / ((double)(2 * m + 1) * (2 * m + 1));
  const double g11 = s[0] * sc, g12 = s[1] * sc, g22 = s[2] * sc, h1 = s[3] * sc, h2 = s[4] * sc;
  const double idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3);
  const float dx = (float)((g11 * h2 - g12 * h1) * idet);
  const float dy = (float)((g22 * h1 - g12 * h2) * idet);
  w.F[2 * (L.off + p)] = dx;
  w.F[2 * (L.off + p) + 1] = dy;
  if (update)
    update_matrices(w.R + 5 * L.off, w.R + 5 * (g.S + L.off), L.w, L.h, x, y, dx, dy, w.M + 5 * (L.off + p));
}

// ---- mesh: one 64-lane workgroup per cell; median of step^2 values per component -----------------------------------
// mesh (N, P, 4): src x, src y, dst x, dst y
__global__ __launch_bounds__(64) void cmc_mesh_kernel(FlowGeom g, int step, int gw, double sfx, double sfy, float* ws,
                                                      float* mesh) {
  __shared__ float vals[2][256];
  __shared__ float mid[2][2];
  const int cell = blockIdx.x, n = blockIdx.y;
  const int cy = cell / gw, cx = cell - cy * gw;
  const int cnt = step * step;
  const float* F = pair_ws(ws, g, n).F + 2 * g.lv[0].off;
  for (int i = threadIdx.x; i < cnt; i += 64) {
    const int yy = cy * step + i / step, xx = cx * step + i % step;
    vals[0][i] = F[(yy * kSide + xx) * 2];
    vals[1][i] = F[(yy * kSide + xx) * 2 + 1];
  }
  __syncthreads();
  const int lo = (cnt - 1) / 2, hi = cnt / 2;
  for (int i = threadIdx.x; i < cnt; i += 64) {
    for (int c = 0; c < 2; ++c) {
      const float v = vals[c][i];
      int rank = 0;
      for (int j = 0; j < cnt; ++j) {
        const float u = vals[c][j];
        rank += (u < v) || (u == v && j < i);
      }
      if (rank == lo) mid[c][0] = v;
      if (rank == hi) mid[c][1] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double s[2] = {sfx, sfy};
    float* o = mesh + ((long long)n * gridDim.x + cell) * 4;
    const float src[2] = {(float)((cx + 0.5) * step * sfx), (float)((cy + 0.5) * step * sfy)};
    for (int c = 0; c < 2; ++c) {
      const double med = ((double)mid[c][0] * s[c] + (double)mid[c][1] * s[c]) / 2.0;
      o[c] = src[c];
      o[2 + c] = (float)((double)src[c] + med);
    }
  }
}

// ---- fit: exhaustive two-point hypotheses over kFitParts workgroups per pair (best key by atomicMax), then one
// workgroup per pair for the consensus set and the least-squares refit
constexpr int kFitParts = 64;

__device__ __forceinline__ void load_points(const float* mesh, int n, int P, float (*pt)[4]) {
  for (int i = threadIdx.x; i < P * 4; i += blockDim.x) pt[i / 4][i % 4] = mesh[(long long)n * P * 4 + i];
}

// key = (inlier count << 32) | ~(pair index): the largest set wins, ties go to the lowest (i, j)
__global__ __launch_bounds__(256) void cmc_fit_score_kernel(const float* mesh, int P, float thr2,
                                                            unsigned long long* keys) {
  __shared__ float pt[kMaxPoints][4];
  __shared__ unsigned long long best[4];
  const int n = blockIdx.y, tid = threadIdx.x;
  load_points(mesh, n, P, pt);
  __syncthreads();
  unsigned long long key = 0;
  const long long total = (long long)P * P;
  for (long long t = (long long)blockIdx.x * blockDim.x + tid; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int i = (int)(t / P), j = (int)(t - (long long)i * P);
    if (j <= i) continue;
    const float dpx = pt[j][0] - pt[i][0], dpy = pt[j][1] - pt[i][1];
    const float dqx = pt[j][2] - pt[i][2], dqy = pt[j][3] - pt[i][3];
    const float den = dpx * dpx + dpy * dpy;
    if (!(den > 0.f)) continue;
    const float a = (dqx * dpx + dqy * dpy) / den, b = (dqy * dpx - dqx * dpy) / den;
    const float tx = pt[i][2] - (a * pt[i][0] - b * pt[i][1]), ty = pt[i][3] - (b * pt[i][0] + a * pt[i][1]);
    int c = 0;
    for (int k = 0; k < P; ++k) {
      const float ex = a * pt[k][0] - b * pt[k][1] + tx - pt[k][2];
      const float ey = b * pt[k][0] + a * pt[k][1] + ty - pt[k][3];
      c += (ex * ex + ey * ey) <= thr2;
    }
    const unsigned long long k2 = ((unsigned long long)c << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)t);
    key = k2 > key ? k2 : key;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  if ((tid & 63) == 0) best[tid >> 6] = key;
  __syncthreads();
  if (tid == 0) {
    unsigned long long k = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) k = best[i] > k ? best[i] : k;
    atomicMax(keys + n, k);
  }
}

__global__ __launch_bounds__(256) void cmc_fit_kernel(const float* mesh, int P, float thr2, float min_ratio,
                                                     const unsigned long long* keys, float* warps,
                                                     unsigned char* inliers) {
  __shared__ float pt[kMaxPoints][4];
  __shared__ unsigned char in_set[kMaxPoints];
  const int n = blockIdx.x, tid = threadIdx.x;
  load_points(mesh, n, P, pt);
  __syncthreads();
  const unsigned long long bk = keys[n];
  const int count = (int)(bk >> 32);
  float* out = warps + (long long)n * ST_CMC_WARP_FLOATS;
  if (count == 0) {   // no usable hypothesis (every source point coincides): no warp
    if (tid < ST_CMC_WARP_FLOATS) out[tid] = 0.f;
    for (int k = tid; k < P; k += blockDim.x)
      if (inliers) inliers[(long long)n * P + k] = 0;
    return;
  }
  const long long t = (long long)(0xFFFFFFFFu - (unsigned)(bk & 0xFFFFFFFFu));
  const int i = (int)(t / P), j = (int)(t - (long long)i * P);
  {
    const float dpx = pt[j][0] - pt[i][0], dpy = pt[j][1] - pt[i][1];
    const float dqx = pt[j][2] - pt[i][2], dqy = pt[j][3] - pt[i][3];
    const float den = dpx * dpx + dpy * dpy;
    const float a = (dqx * dpx + dqy * dpy) / den, b = (dqy * dpx - dqx * dpy) / den;
    const float tx = pt[i][2] - (a * pt[i][0] - b * pt[i][1]), ty = pt[i][3] - (b * pt[i][0] + a * pt[i][1]);
    for (int k = tid; k < P; k += blockDim.x) {
      const float ex = a * pt[k][0] - b * pt[k][1] + tx - pt[k][2];
      const float ey = b * pt[k][0] + a * pt[k][1] + ty - pt[k][3];
      in_set[k] = (ex * ex + ey * ey) <= thr2;
      if (inliers) inliers[(long long)n * P + k] = in_set[k];
    }
  }
  __syncthreads();
  if (tid == 0) {
    double px = 0, py = 0, qx = 0, qy = 0;
    int m = 0;
    for (int k = 0; k < P; ++k)
      if (in_set[k]) { px += pt[k][0]; py += pt[k][1]; qx += pt[k][2]; qy += pt[k][3]; ++m; }
    px /= m; py /= m; qx /= m; qy /= m;
    double sxx = 0, sa = 0, sb = 0;
    for (int k = 0; k < P; ++k) {
      if (!in_set[k]) continue;
      const double ux = pt[k][0] - px, uy = pt[k][1] - py, vx = pt[k][2] - qx, vy = pt[k][3] - qy;
      sxx += ux * ux + uy * uy;
      sa += ux * vx + uy * vy;
      sb += ux * vy - uy * vx;
    }
    const double a = sa / sxx, b = sb / sxx;
    const double tx = qx - (a * px - b * py), ty = qy - (b * px + a * py);
    const float ratio = (float)m / (float)P;
    out[0] = ratio >= min_ratio ? 1.f : 0.f;
    out[1] = ratio;
    out[2] = (float)a; out[3] = (float)(-b); out[4] = (float)tx;
    out[5] = (float)b; out[6] = (float)a; out[7] = (float)ty;
  }
}

// ---- host-side geometry -------------------------------------------------------------------------------------------
int cv_round(double v) { return (int)std::nearbyint(v); }   // half to even (the default rounding mode)

FlowGeom make_geom() {
  FlowGeom g{};
  int L = 0;
  double scale = 1.0;
  for (; L < 5; ++L) {            // levels = 5 requested: k while 255 * 0.5^k >= 32 (and k <= 5)
    if (L > 0) {
      scale *= 0.5;
      if (kSide * scale < 32.0) break;
    }
  }
  L = L > kMaxLevels ? kMaxLevels : L;
  g.L = L;
  long long off = 0;
  for (int k = 0; k < L; ++k) {
    double sc = 1.0;
    for (int i = 0; i < k; ++i) sc *= 0.5;
    Level& lv = g.lv[k];
    lv.w = cv_round(kSide * sc);
    lv.h = lv.w;
    lv.off = off;
    off += (long long)lv.w * lv.h;
    const double sigma = (1.0 / sc - 1.0) * 0.5;
    int ks = cv_round(sigma * 5) | 1;
    ks = ks < 3 ? 3 : ks;
    lv.ksize = ks;
    if (sigma <= 0 && ks == 3) {
      lv.kern[0] = 0.25f; lv.kern[1] = 0.5f; lv.kern[2] = 0.25f;
    } else {
      double tmp[kMaxBlur], s = 0;
      for (int i = 0; i < ks; ++i) {
        const double x = i - (ks - 1) * 0.5;
        tmp[i] = std::exp(-x * x / (2 * sigma * sigma));
        s += tmp[i];
      }
      for (int i = 0; i < ks; ++i) lv.kern[i] = (float)(tmp[i] / s);
    }
  }
  g.S = off;
  // FarnebackPrepareGaussian(n = 5, sigma = 1.2)
  const double sigma = 1.2;
  float gg[2 * kPolyN + 1];
  double s = 0;
  for (int x = -kPolyN; x <= kPolyN; ++x) {
    gg[x + kPolyN] = (float)std::exp(-x * x / (2 * sigma * sigma));
    s += gg[x + kPolyN];
  }
  s = 1.0 / s;
  for (int x = -kPolyN; x <= kPolyN; ++x) gg[x + kPolyN] = (float)(gg[x + kPolyN] * s);
  for (int x = 0; x <= kPolyN; ++x) {
    g.g[x] = gg[x + kPolyN];
    g.xg[x] = (float)(x * g.g[x]);
    g.xxg[x] = (float)(x * x * g.g[x]);
  }
  double G[6][6] = {};
  for (int y = -kPolyN; y <= kPolyN; ++y)
    for (int x = -kPolyN; x <= kPolyN; ++x) {
      const double gy = gg[y + kPolyN], gx = gg[x + kPolyN];
      G[0][0] += gy * gx;
      G[1][1] += gy * gx * x * x;
      G[3][3] += gy * gx * x * x * x * x;
      G[5][5] += gy * gx * x * x * y * y;
    }
  G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1];
  G[4][4] = G[3][3];
  G[3][4] = G[4][3] = G[5][5];
  // the entries of inv(G) the expansion needs: the {0, 3, 4} block is [[a c c], [c d e], [c e d]], 1, 2, 5 diagonal
  const double a = G[0][0], c = G[0][3], d = G[3][3], e = G[3][4];
  // inverse of the 3 x 3 symmetric block by cofactors
  const double det = a * (d * d - e * e) - c * (c * d - e * c) + c * (c * e - d * c);
  g.ig03 = (float)((c * e - c * d) / det);
  g.ig33 = (float)((a * d - c * c) / det);
  g.ig11 = (float)(1.0 / G[1][1]);
  g.ig55 = (float)(1.0 / G[5][5]);
  return g;
}

const FlowGeom& geom() {
  static const FlowGeom g = make_geom();
  return g;
}

int launch_flow(const unsigned char* prev, const unsigned char* curr, int N, int winsize, float* ws, hipStream_t s) {
  const FlowGeom& g = geom();
  const int m = winsize / 2;
  const int maxpx = g.lv[0].w * g.lv[0].h;
  hipLaunchKernelGGL(cmc_pyramid_kernel, dim3((maxpx + 255) / 256, g.L, 2 * N), dim3(256), 0, s, prev, curr, g, ws);
  hipLaunchKernelGGL(cmc_polyexp_kernel, dim3((maxpx + 255) / 256, g.L, 2 * N), dim3(256), 0, s, g, ws);
  for (int l = g.L - 1; l >= 0; --l) {
    const int px = g.lv[l].w * g.lv[l].h, blocks = (px + 255) / 256;
    hipLaunchKernelGGL(cmc_level_init_kernel, dim3(blocks, N), dim3(256), 0, s, g, l, ws);
    for (int it = 0; it < 3; ++it) {
      hipLaunchKernelGGL(cmc_vblur_kernel, dim3(blocks, N), dim3(256), 0, s, g, l, m, ws);
      hipLaunchKernelGGL(cmc_hsolve_kernel, dim3(blocks, N), dim3(256), 0, s, g, l, m, it < 2 ? 1 : 0, ws);
    }
  }
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

__global__ void cmc_copy_flow_kernel(FlowGeom g, const float* ws, float* flow_out, float* levels_out) {
  const int n = blockIdx.y;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const float* F = ws + (long long)n * pair_floats(g.S) + 2 * g.S + 10 * g.S + 5 * g.S + 5LL * kPlane;
  if (flow_out && i < 2LL * kPlane) flow_out[(long long)n * 2 * kPlane + i] = F[2 * g.lv[0].off + i];
  if (levels_out && i < 2 * g.S) levels_out[(long long)n * 2 * g.S + i] = F[i];
}

}  // namespace

extern "C" int st_cmc_num_levels(int* sides) {
  const FlowGeom& g = geom();
  if (sides)
    for (int l = 0; l < g.L; ++l) sides[l] = g.lv[l].w;
  return g.L;
}

// workspace: per-pair Farneback buffers | mesh (N x kMaxPoints x 4 floats) | fit keys (N x u64, 256-byte aligned)
size_t keys_offset(int N) {
  const size_t b = ((size_t)N * (size_t)pair_floats(geom().S) + (size_t)N * kMaxPoints * 4) * sizeof(float);
  return (b + 255) / 256 * 256;
}

extern "C" size_t st_cmc_workspace_bytes(int N) {
  return N > 0 ? keys_offset(N) + (size_t)N * sizeof(unsigned long long) : 0;
}

extern "C" int st_cmc_front_u8(const void* const* frames_u8_dev_ptrs_host, int N, int fh, int fw, int h, int w,
                               void* planes_dev, st_stream_t stream) {
  using namespace st;
  ST_REQUIRE(frames_u8_dev_ptrs_host && planes_dev && N > 0 && h > 0 && w > 0 && h <= fh && w <= fw,
             "st_cmc_front_u8: bad argument");
  for (int i = 0; i < N; ++i)     // every frame before the first launch: a refused call has launched nothing
    ST_REQUIRE(frames_u8_dev_ptrs_host[i], "st_cmc_front_u8: frame %d is null", i);
  for (int base = 0; base < N; base += kMaxFrames) {
    const int k = N - base < kMaxFrames ? N - base : kMaxFrames;
    FramePtrs fp{};
    for (int i = 0; i < k; ++i) fp.p[i] = static_cast<const unsigned char*>(frames_u8_dev_ptrs_host[base + i]);
    hipLaunchKernelGGL(cmc_front_u8_kernel, dim3(k), dim3(1024), 0, static_cast<hipStream_t>(stream), fp, fh, fw, h, w,
                       static_cast<unsigned char*>(planes_dev) + (size_t)base * kPlane);
  }
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

extern "C" int st_cmc_front_f32(const float* batch_dev, int N, int H, int W, int h, int w, void* planes_dev,
                                st_stream_t stream) {
  using namespace st;
  ST_REQUIRE(batch_dev && planes_dev && N > 0 && h > 0 && w > 0 && h <= H && w <= W, "st_cmc_front_f32: bad argument");
  hipLaunchKernelGGL(cmc_front_f32_kernel, dim3(N), dim3(1024), 0, static_cast<hipStream_t>(stream), batch_dev, H, W, h,
                     w, static_cast<unsigned char*>(planes_dev));
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

extern "C" int st_cmc_flow(const void* prev_planes_dev, const void* curr_planes_dev, int N, int winsize, void* ws,
                           size_t ws_bytes, float* flow_out_dev, float* levels_out_dev, st_stream_t stream) {
  using namespace st;
  ST_REQUIRE(prev_planes_dev && curr_planes_dev && ws && N > 0, "st_cmc_flow: bad argument");
  ST_REQUIRE(winsize >= 1 && winsize % 2 == 1 && winsize <= 63, "st_cmc_flow: winsize %d must be odd, 1..63", winsize);
  ST_REQUIRE(ws_bytes >= st_cmc_workspace_bytes(N), "st_cmc_flow: workspace %zu < %zu bytes", ws_bytes,
             st_cmc_workspace_bytes(N));
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ST_CHECK(launch_flow(static_cast<const unsigned char*>(prev_planes_dev), static_cast<const unsigned char*>(curr_planes_dev),
                       N, winsize, static_cast<float*>(ws), s));
  if (flow_out_dev || levels_out_dev) {
    const FlowGeom& g = geom();
    const long long mx = 2 * g.S > 2LL * kPlane ? 2 * g.S : 2LL * kPlane;
    hipLaunchKernelGGL(cmc_copy_flow_kernel, dim3((unsigned)((mx + 255) / 256), N), dim3(256), 0, s, g,
                       static_cast<const float*>(ws), flow_out_dev, levels_out_dev);
    ST_CHECK_HIP(hipGetLastError());
  }
  return ST_OK;
}

// ---- the later stages, shared by st_cmc_estimate and the two injection points -------------------------------------
namespace {

// grid (ceil(2 * 255^2 / 256), N): a caller's flow field into the level-0 flow of every pair's workspace (the inverse of
// cmc_copy_flow_kernel), so that the mesh reads it where the Farneback launches leave theirs
__global__ void cmc_load_flow_kernel(FlowGeom g, const float* flow_in, float* ws) {
  const int n = blockIdx.y;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < 2LL * kPlane) pair_ws(ws, g, n).F[2 * g.lv[0].off + i] = flow_in[(long long)n * 2 * kPlane + i];
}

int require_estimate_args(const char* who, const StCmcParams* prm, int N, int img_h, int img_w, const void* ws,
                          size_t ws_bytes, const float* warps_out_dev) {
  using namespace st;
  ST_REQUIRE(prm && prm->struct_size == (int)sizeof(StCmcParams), "%s: params struct_size mismatch", who);
  ST_REQUIRE(warps_out_dev && ws && N > 0 && img_h > 0 && img_w > 0, "%s: bad argument", who);
  ST_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "%s: workspace must be 8-byte aligned", who);   // 64-bit fit keys
  ST_REQUIRE(prm->step >= 8 && prm->step * prm->step <= 256, "%s: step %d must be in 8..16", who, prm->step);
  ST_REQUIRE(ws_bytes >= st_cmc_workspace_bytes(N), "%s: workspace %zu < %zu bytes", who, ws_bytes,
             st_cmc_workspace_bytes(N));
  return ST_OK;
}

// points (N, P, 4) -> warps (N, ST_CMC_WARP_FLOATS), inliers (N, P; optional); the fit keys live in the workspace
int launch_fit(const float* points, int N, int P, float ransac_thr, float min_inlier_ratio, void* ws, float* warps,
               unsigned char* inliers, hipStream_t s) {
  unsigned long long* keys =
      reinterpret_cast<unsigned long long*>(static_cast<unsigned char*>(ws) + keys_offset(N));
  const float thr2 = ransac_thr * ransac_thr;
  ST_CHECK_HIP(hipMemsetAsync(keys, 0, (size_t)N * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(cmc_fit_score_kernel, dim3(kFitParts, N), dim3(256), 0, s, points, P, thr2, keys);
  hipLaunchKernelGGL(cmc_fit_kernel, dim3(N), dim3(256), 0, s, points, P, thr2, min_inlier_ratio, keys, warps, inliers);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

// the level-0 flow of every pair's workspace -> mesh (into mesh_out, else into the workspace) -> fit
int launch_mesh_fit(int N, int img_h, int img_w, const StCmcParams* prm, void* ws, float* warps, float* mesh_out,
                    unsigned char* inliers, hipStream_t s) {
  const FlowGeom& g = geom();
  const int gw = kSide / prm->step, P = gw * gw;
  float* mesh = mesh_out ? mesh_out : static_cast<float*>(ws) + (long long)N * pair_floats(g.S);
  hipLaunchKernelGGL(cmc_mesh_kernel, dim3(P, N), dim3(64), 0, s, g, prm->step, gw, (double)img_w / kSide,
                     (double)img_h / kSide, static_cast<float*>(ws), mesh);
  return launch_fit(mesh, N, P, prm->ransac_thr, prm->min_inlier_ratio, ws, warps, inliers, s);
}

}  // namespace

extern "C" int st_cmc_estimate(const void* prev_planes_dev, const void* curr_planes_dev, int N, int img_h, int img_w,
                               const StCmcParams* prm, void* ws, size_t ws_bytes, float* warps_out_dev,
                               float* mesh_out_dev, unsigned char* inliers_out_dev, st_stream_t stream) {
  ST_CHECK(require_estimate_args("st_cmc_estimate", prm, N, img_h, img_w, ws, ws_bytes, warps_out_dev));
  ST_CHECK(st_cmc_flow(prev_planes_dev, curr_planes_dev, N, prm->winsize, ws, ws_bytes, nullptr, nullptr, stream));
  return launch_mesh_fit(N, img_h, img_w, prm, ws, warps_out_dev, mesh_out_dev, inliers_out_dev,
                         static_cast<hipStream_t>(stream));
}

extern "C" int st_cmc_mesh_fit(const float* flow_dev, int N, int img_h, int img_w, const StCmcParams* prm, void* ws,
                               size_t ws_bytes, float* warps_out_dev, float* mesh_out_dev,
                               unsigned char* inliers_out_dev, st_stream_t stream) {
  using namespace st;
  ST_CHECK(require_estimate_args("st_cmc_mesh_fit", prm, N, img_h, img_w, ws, ws_bytes, warps_out_dev));
  ST_REQUIRE(flow_dev, "st_cmc_mesh_fit: flow is null");
  const FlowGeom& g = geom();
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(cmc_load_flow_kernel, dim3((unsigned)((2LL * kPlane + 255) / 256), N), dim3(256), 0, s, g, flow_dev,
                     static_cast<float*>(ws));
  return launch_mesh_fit(N, img_h, img_w, prm, ws, warps_out_dev, mesh_out_dev, inliers_out_dev, s);
}

extern "C" int st_cmc_fit(const float* points_dev, int N, int P, float ransac_thr, float min_inlier_ratio, void* ws,
                          size_t ws_bytes, float* warps_out_dev, unsigned char* inliers_out_dev, st_stream_t stream) {
  using namespace st;
  ST_REQUIRE(points_dev && warps_out_dev && ws && N > 0, "st_cmc_fit: bad argument");
  ST_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "st_cmc_fit: workspace must be 8-byte aligned");   // 64-bit fit keys
  ST_REQUIRE(P >= 2 && P <= kMaxPoints, "st_cmc_fit: %d points, must be in 2..%d", P, kMaxPoints);
  ST_REQUIRE(ws_bytes >= st_cmc_workspace_bytes(N), "st_cmc_fit: workspace %zu < %zu bytes", ws_bytes,
             st_cmc_workspace_bytes(N));
  return launch_fit(points_dev, N, P, ransac_thr, min_inlier_ratio, ws, warps_out_dev, inliers_out_dev,
                    static_cast<hipStream_t>(stream));
}
