// Left-right check of the stereo module (StereoCostVolume(lr_check=True); DESIGN.md "Left-right check of the stereo
// module").  No reference function exists, as for the module itself: the five rules below are the specification, their
// executable form is tests/lrcheck_ref.py (numpy + the C oracle's soft-argmin / upsample), held bit for bit.
//
//   1  dL = st_softargmin(V)                                   V [N][H][W][D]: the volume the left soft-argmin reads
//   2  VR[n][y][x'][d] = V[n][y][x'+d][d] if x'+d < W, else 0   the right-view volume (mirror of "cost 0 where x-d < 0")
//   3  dR = softargmin(VR), operation order of oracle_softargmin: m = max_d T*c[d]; then d ascending:
//      e = exp(T*c[d] - m), s += e, t = fmaf(d, e, t); result t / s               (st_softargmin_right: rules 2 + 3)
//   4  r = (int)floorf(dL + 0.5f), xr = x - r; pixel (y, x) is INVALID if dL is not finite, xr < 0, or
//      !(fabsf(dL - dR[y][xr]) * (float)s <= lr_max_diff)   (a NaN fails; a difference EQUAL to lr_max_diff is valid)
//   5  disp_postp = valid ? (what st_disp_upsample_pack writes) : +0;  disp_mask = valid ? 1 : 0 inside (valid_h,
//      valid_w), 0 outside; the mask of output pixel (Y, X) is that of level pixel (Y / s, X / s)
//                                                                                 (st_lr_check_pack: rules 4 + 5)
//
// st_softargmin_right.  Element d of right pixel x' sits at ((y*W + x' + d)*D + d): a diagonal of the left volume, so a
// lane walking its own diagonal in memory would touch one new 64-byte segment per level.  Instead a workgroup of
// LR_TW = 128 lanes (one right pixel each) goes through the levels in slabs of LR_DS = 16: slab [d0, d0+16) of its 128
// pixels needs the left columns x0+d0 .. x0+d0+142, levels [d0, d0+16) only - 143 contiguous 64-byte segments, fetched
// with 16-byte loads (four lanes per segment), re-fetch (128+15)/128 = 1.12.  They land in an LDS tile [column][16]
// with a row stride of 17 floats, where lane i reads tile[i+d][d] = word 17 i + 18 d: over the 32 lanes of a
// ds_read_b32 group 17 i mod 32 takes every bank once.  Rule 3 wants the maximum before the first exponential, so the
// slabs are swept twice (the second sweep re-reads what the first one left in the caches); a running-maximum rescale
// would change the bits.  The next slab's global loads are issued before the current slab's arithmetic and stored to
// the other tile buffer after it.  Every loop is bounded by D or the tile; no atomics, no spinning.
#include <algorithm>
#include <cstdint>

#include "st_common.h"

namespace st {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// The exponential of the left soft-argmin kernels (costvolume.hip: cv_expf two values per instruction, default operand
// selection only - every constant an explicit (c, c) scalar register pair), operation for operation, so
// that dR and dL come from the same arithmetic.  For arguments <= 0 (x = T c - max).
struct LrExpPk {
  f32x2 log2e, nln2hi, ln2lo, c0, c1, c2, c3, c4, c5, one;
};
__device__ __forceinline__ f32x2 lr_dup_s(float c) {
  f32x2 p = {c, c};
  asm volatile("" : "+s"(p));     // opaque: the broadcast cannot be folded into op_sel
  return p;
}
__device__ __forceinline__ LrExpPk lr_exp_pk_consts() {
  LrExpPk k;
  k.log2e = lr_dup_s(1.44269504088896341f); k.nln2hi = lr_dup_s(-0.693359375f); k.ln2lo = lr_dup_s(2.12194440e-4f);
  k.c0 = lr_dup_s(1.9875691500e-4f); k.c1 = lr_dup_s(1.3981999507e-3f); k.c2 = lr_dup_s(8.3334519073e-3f);
  k.c3 = lr_dup_s(4.1665795894e-2f); k.c4 = lr_dup_s(1.6666665459e-1f); k.c5 = lr_dup_s(5.0000001201e-1f);
  k.one = lr_dup_s(1.0f);
  return k;
}
template <int NB>
__device__ __forceinline__ void lr_expf_pk_nonpos(f32x2 (&x)[NB], const LrExpPk& k) {
  f32x2 n[NB], r[NB], p[NB];
#define LR_STAGE(body)                       \
  _Pragma("unroll") for (int b = 0; b < NB; ++b) { body; } \
  __builtin_amdgcn_sched_barrier(0);
  LR_STAGE(r[b] = x[b] * k.log2e)
  LR_STAGE((n[b] = f32x2{rintf(r[b][0]), rintf(r[b][1])}))
  LR_STAGE(r[b] = __builtin_elementwise_fma(n[b], k.nln2hi, x[b]))
  LR_STAGE(r[b] = __builtin_elementwise_fma(n[b], k.ln2lo, r[b]))
  LR_STAGE(p[b] = __builtin_elementwise_fma(k.c0, r[b], k.c1))
  LR_STAGE(p[b] = __builtin_elementwise_fma(p[b], r[b], k.c2))
  LR_STAGE(p[b] = __builtin_elementwise_fma(p[b], r[b], k.c3))
  LR_STAGE(p[b] = __builtin_elementwise_fma(p[b], r[b], k.c4))
  LR_STAGE(p[b] = __builtin_elementwise_fma(p[b], r[b], k.c5))
  LR_STAGE((p[b] = __builtin_elementwise_fma(p[b], r[b] * r[b], r[b])))
  LR_STAGE(p[b] = p[b] + k.one)
#undef LR_STAGE
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    f32x2 e = {ldexpf(p[b][0], (int)n[b][0]), ldexpf(p[b][1], (int)n[b][1])};
    if (x[b][0] < -103.0f) e[0] = 0.0f;
    if (x[b][1] < -103.0f) e[1] = 0.0f;
    x[b] = e;
  }
}

constexpr int LR_TW = 128;                      // right pixels (= lanes) per workgroup
constexpr int LR_DS = 16;                       // levels per slab: one 64-byte segment per column
constexpr int LR_COLS = LR_TW + LR_DS - 1;      // left columns a slab of the tile touches
constexpr int LR_STRIDE = LR_DS + 1;            // tile row stride in floats (odd: see the header)
constexpr int LR_TILE = LR_COLS * LR_STRIDE;

// VEC: D a multiple of 4 and a 16-byte aligned volume (16-byte loads, a level quad never straddles D); otherwise one
// float per load, any D.
template <bool VEC>
__global__ __launch_bounds__(LR_TW) void softargmin_right_kernel(const float* __restrict__ vol, int W, int D,
                                                                  float temperature, int gx,
                                                                  float* __restrict__ out_disp) {
  __shared__ __attribute__((aligned(16))) float tile[2][LR_TILE];
  const int tid = threadIdx.x;
  const int x0 = (int)(blockIdx.x % (unsigned)gx) * LR_TW;
  const size_t rowbase = (size_t)(blockIdx.x / (unsigned)gx) * W;   // (n * H + y) * W
  const int nslab = (D + LR_DS - 1) / LR_DS;
  constexpr int NLD = VEC ? (LR_COLS * (LR_DS / 4) + LR_TW - 1) / LR_TW : (LR_COLS * LR_DS + LR_TW - 1) / LR_TW;
  f32x4 st4[VEC ? NLD : 1];
  float st1[VEC ? 1 : NLD];

  // column `col` of slab `slab` is left pixel x0 + d0 + col; levels and columns past the volume read as 0 (rule 2)
  auto stage_load = [&](int slab) {
    const int d0 = slab * LR_DS;
    if (VEC) {
#pragma unroll
      for (int i = 0; i < NLD; ++i) {
        const int e = tid + LR_TW * i, col = e >> 2, d = d0 + 4 * (e & 3);
        const int x = x0 + d0 + col;
        st4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (col < LR_COLS && x < W && d < D) st4[i] = *reinterpret_cast<const f32x4*>(vol + (rowbase + x) * D + d);
      }
    } else {
#pragma unroll
      for (int i = 0; i < NLD; ++i) {
        const int e = tid + LR_TW * i, col = e >> 4, d = d0 + (e & 15);
        const int x = x0 + d0 + col;
        st1[i] = 0.f;
        if (col < LR_COLS && x < W && d < D) st1[i] = vol[(rowbase + x) * D + d];
      }
    }
  };
  auto stage_store = [&](int buf) {
    float* t = tile[buf];
    if (VEC) {
#pragma unroll
      for (int i = 0; i < NLD; ++i) {
        const int e = tid + LR_TW * i, col = e >> 2, q = e & 3;
        if (col < LR_COLS) {
#pragma unroll
          for (int k = 0; k < 4; ++k) t[col * LR_STRIDE + 4 * q + k] = st4[i][k];
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NLD; ++i) {
        const int e = tid + LR_TW * i, col = e >> 4;
        if (col < LR_COLS) t[col * LR_STRIDE + (e & 15)] = st1[i];
      }
    }
  };

  const LrExpPk ek = lr_exp_pk_consts();
  float m = -__builtin_inff(), s = 0.f, t = 0.f;
  stage_load(0);
  stage_store(0);
  __syncthreads();
  const int total = 2 * nslab;     // sweep 1: the maximum; sweep 2: exponentials and the two sums, d ascending
  for (int it = 0; it < total; ++it) {
    const int buf = it & 1;
    const bool second = it >= nslab;
    const int slab = second ? it - nslab : it;
    const bool more = it + 1 < total;
    if (more) stage_load(it + 1 >= nslab ? it + 1 - nslab : it + 1);   // in flight during the arithmetic below
    const float* tp = tile[buf] + tid * LR_STRIDE;      // this lane's diagonal: level d0 + d at tp[d * (LR_STRIDE + 1)]
    const int d0 = slab * LR_DS;
    const int nd = min(LR_DS, D - d0);                  // uniform
    float c[LR_DS];
#pragma unroll
    for (int d = 0; d < LR_DS; ++d) c[d] = temperature * tp[d * (LR_STRIDE + 1)];   // T c once, as the oracle forms it
    if (!second) {
#pragma unroll
      for (int d = 0; d < LR_DS; ++d)
        if (d < nd) m = fmaxf(m, c[d]);
    } else {
      f32x2 negm = {-m, -m};
      asm volatile("" : "+v"(negm));
      f32x2 xa[LR_DS / 4], xb[LR_DS / 4];
#pragma unroll
      for (int b = 0; b < LR_DS / 4; ++b) {
        xa[b] = f32x2{c[2 * b], c[2 * b + 1]} + negm;
        xb[b] = f32x2{c[LR_DS / 2 + 2 * b], c[LR_DS / 2 + 2 * b + 1]} + negm;
      }
      lr_expf_pk_nonpos<LR_DS / 4>(xa, ek);
      lr_expf_pk_nonpos<LR_DS / 4>(xb, ek);
#pragma unroll
      for (int d = 0; d < LR_DS; ++d) {
        if (d < nd) {
          const float e = d < LR_DS / 2 ? xa[d >> 1][d & 1] : xb[(d - LR_DS / 2) >> 1][d & 1];
          s += e;
          t = fmaf((float)(d0 + d), e, t);
        }
      }
    }
    if (more) stage_store(buf ^ 1);   // every lane finished reading that buffer before the barrier of the last turn
    __syncthreads();
  }
  const int x = x0 + tid;
  if (x < W) out_disp[rowbase + x] = t / s;
}

// rule 4 for level pixel x of one row (dl / dr: that row of dL / dR)
__device__ __forceinline__ bool lr_pixel_valid(const float* __restrict__ dl, const float* __restrict__ dr, int Wl, int x,
                                               float fscale, float max_diff) {
  const float d = dl[x];
  if (!__builtin_isfinite(d)) return false;
  const float rf = floorf(d + 0.5f);
  // xr = x - (int)rf must lie in the right image: xr < 0 is rule 4's second clause; xr >= Wl cannot happen for a
  // soft-argmin result (dL >= 0) and is refused here so that no input can make the kernel read outside dR.  Compared as
  // floats (exact for these integers), so the conversion below never overflows.
  if (!(rf <= (float)x && rf >= (float)(x - (Wl - 1)))) return false;
  const int xr = x - (int)rf;
  return fabsf(d - dr[xr]) * fscale <= max_diff;
}

// The arithmetic of st_disp_upsample_pack (costvolume.hip: disp_upsample_value, oracle_disp_upsample), copied so that a
// valid pixel keeps its bits; P = 4 consecutive pixels per thread with 16-byte stores, or 1.
template <int P>
__global__ __launch_bounds__(256) void lr_check_pack_kernel(const float* __restrict__ dl, const float* __restrict__ dr, int N,
                                                            int Hl, int Wl, int scale, int H, int W, int valid_h,
                                                            int valid_w, float max_diff, float* __restrict__ out,
                                                            float* __restrict__ mask) {
  const int WP = W / P;
  const long long total = (long long)N * H * WP;
  const float inv = 1.0f / (float)scale, fscale = (float)scale;
  const size_t plane = (size_t)H * W;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int X0 = P * (int)(idx % WP);
    const long long r = idx / WP;
    const int Y = (int)(r % H);
    const int n = (int)(r / H);
    const float* b = dl + (size_t)n * Hl * Wl;
    const size_t lrow = ((size_t)n * Hl + Y / scale) * Wl;
    float v[P], mk[P];
#pragma unroll
    for (int e = 0; e < P; ++e) {
      const int X = X0 + e;
      v[e] = 0.f;
      mk[e] = 0.f;
      if (Y < valid_h && X < valid_w && lr_pixel_valid(dl + lrow, dr + lrow, Wl, X / scale, fscale, max_diff)) {
        float sy = ((float)Y + 0.5f) * inv - 0.5f;
        float sx = ((float)X + 0.5f) * inv - 0.5f;
        sy = sy < 0.f ? 0.f : sy;
        sx = sx < 0.f ? 0.f : sx;
        const int y0 = min((int)sy, Hl - 1), x0 = min((int)sx, Wl - 1);
        const int y1 = min(y0 + 1, Hl - 1), x1 = min(x0 + 1, Wl - 1);
        const float ly = sy - (float)y0, lx = sx - (float)x0;
        const float hy = 1.0f - ly, hx = 1.0f - lx;
        const float v00 = b[(size_t)y0 * Wl + x0], v01 = b[(size_t)y0 * Wl + x1];
        const float v10 = b[(size_t)y1 * Wl + x0], v11 = b[(size_t)y1 * Wl + x1];
        v[e] = (hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11)) * fscale;
        mk[e] = 1.f;
      }
    }
    float* o = out + (size_t)n * 3 * plane + (size_t)Y * W + X0;
    if (P == 4) {
      const f32x4 v4 = {v[0], v[P > 1 ? 1 : 0], v[P > 2 ? 2 : 0], v[P > 3 ? 3 : 0]};
      *reinterpret_cast<f32x4*>(o) = v4;
      *reinterpret_cast<f32x4*>(o + plane) = v4;
      *reinterpret_cast<f32x4*>(o + 2 * plane) = v4;
      if (mask) {
        const f32x4 m4 = {mk[0], mk[P > 1 ? 1 : 0], mk[P > 2 ? 2 : 0], mk[P > 3 ? 3 : 0]};
        *reinterpret_cast<f32x4*>(mask + (size_t)n * plane + (size_t)Y * W + X0) = m4;
      }
    } else {
      o[0] = v[0];
      o[plane] = v[0];
      o[2 * plane] = v[0];
      if (mask) mask[(size_t)n * plane + (size_t)Y * W + X0] = mk[0];
    }
  }
}

}  // namespace st

extern "C" int st_softargmin_right(const float* vol_dev, int N, int H, int W, int D, float temperature,
                                   float* out_disp_right_dev, st_stream_t stream_) {
  using namespace st;
  ST_REQUIRE(vol_dev && out_disp_right_dev && N > 0 && H > 0 && W > 0 && D > 0, "st_softargmin_right: bad argument");
  const int gx = (W + LR_TW - 1) / LR_TW;
  const long long blocks = (long long)gx * H * N;
  ST_REQUIRE(blocks < (1ll << 31), "st_softargmin_right: grid too large");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (D % 4 == 0 && (reinterpret_cast<uintptr_t>(vol_dev) & 15) == 0)
    hipLaunchKernelGGL(softargmin_right_kernel<true>, dim3((unsigned)blocks), dim3(LR_TW), 0, stream, vol_dev, W, D,
                       temperature, gx, out_disp_right_dev);
  else
    hipLaunchKernelGGL(softargmin_right_kernel<false>, dim3((unsigned)blocks), dim3(LR_TW), 0, stream, vol_dev, W, D,
                       temperature, gx, out_disp_right_dev);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

extern "C" int st_lr_check_pack(const float* disp_left_dev, const float* disp_right_dev, int N, int Hl, int Wl, int scale,
                                int H, int W, int valid_h, int valid_w, float lr_max_diff, float* disp_postp_dev,
                                float* disp_mask_dev, st_stream_t stream_) {
  using namespace st;
  ST_REQUIRE(disp_left_dev && disp_right_dev && disp_postp_dev, "st_lr_check_pack: null pointer");
  ST_REQUIRE(N > 0 && Hl > 0 && Wl > 0 && scale > 0 && H == Hl * scale && W == Wl * scale,
             "st_lr_check_pack: output must be exactly scale x the level map");
  ST_REQUIRE(valid_h >= 0 && valid_h <= H && valid_w >= 0 && valid_w <= W, "st_lr_check_pack: bad valid region");
  ST_REQUIRE(lr_max_diff >= 0.0f, "st_lr_check_pack: lr_max_diff must be >= 0 (image pixels)");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const uintptr_t align = reinterpret_cast<uintptr_t>(disp_postp_dev) | reinterpret_cast<uintptr_t>(disp_mask_dev);
  if (W % 4 == 0 && (align & 15) == 0) {
    const long long total4 = (long long)N * H * (W / 4);
    const int blocks4 = (int)std::min<long long>((total4 + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(lr_check_pack_kernel<4>, dim3(blocks4), dim3(256), 0, stream, disp_left_dev, disp_right_dev, N, Hl,
                       Wl, scale, H, W, valid_h, valid_w, lr_max_diff, disp_postp_dev, disp_mask_dev);
  } else {
    const long long total = (long long)N * H * W;
    const int blocks = (int)std::min<long long>((total + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(lr_check_pack_kernel<1>, dim3(blocks), dim3(256), 0, stream, disp_left_dev, disp_right_dev, N, Hl,
                       Wl, scale, H, W, valid_h, valid_w, lr_max_diff, disp_postp_dev, disp_mask_dev);
  }
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}
