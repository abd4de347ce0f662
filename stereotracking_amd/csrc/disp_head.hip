// Disparity-completion head (DispHeadV2) on the device, and the branch average of an out_fd detector plan.
//
// Restates the forward of the reference's mmtrack/models/dense_head/disp_head_v2.py:129-176 (input_transform=None,
// out_channels=1) and the rescale of base_disp_head.py:131-139 as a fixed launch sequence:
//
//   p3 (stride 8) --conv3x3--> ELU --conv3x3--> [ELU + nearest x2 -> cat[:, :C]]
//   df (stride 4, 64 ch) --pool (sum, max)--> MLP, sigmoid --> [df * (1 - s) -> cat[:, C:C+64]]
//   cat --conv3x3--> ELU --conv3x3--> [ELU + nearest x2] --conv3x3--> [ELU + 1x1 reg + bias + ReLU] --> pred
//
// The five 3x3 convolutions (BN folded in fp64) run on the library's conv primitive with act = 0, on the Winograd
// instance wherever the layer qualifies; everything in brackets is a bandwidth kernel of this file: 16-byte accesses
// along the channel axis, no float atomics, a fixed reduction order (two runs are bit-equal, an image's result does not
// depend on its batch).  No kernel reads a channel outside the slices it is given, and every output and every
// workspace buffer is written before it is read.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "st_common.h"

namespace st {

int conv2d_launch(const StConvDesc& d, hipStream_t stream, int force_variant, int* picked_variant);
bool wino_conv_applicable(const StConvDesc& d);
bool wino_shape_ok(int Cin, int Cout);
size_t wino_packed_floats(int Cout, int Cin);
int wino_pack_weights(const float* packed, int Cout, int Cin, float* out);

namespace {

constexpr int DF_CH = 64;       // channels of the disparity features = gate channels (CBAM(64, 4), disp_head_v2.py:126)
constexpr int GATE_HID = 16;    // 64 / reduction ratio 4
constexpr int REG_CH = 128;     // input channels of `reg` = output channels of dconv3_1
constexpr int MID_CH = 256;     // dconv2_1 / dconv2_2 width (fixed in the reference, not `channels`)
constexpr int POOL_CHUNK = 128; // pixels per pooling block (16 pixel slots x 8 pixels)
constexpr int POOL_MAX_BLOCKS = 512;

__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : expm1f(x); }
__device__ __forceinline__ float4 elu4(float4 v) { return make_float4(elu1(v.x), elu1(v.y), elu1(v.z), elu1(v.w)); }

// The grid-stride loops stay scalar: vectorised two iterations wide, their index arithmetic becomes packed-fp32
// instructions with a constant broadcast by op_sel_hi - the operand form the library must not contain (DESIGN.md 5;
// tests/test_cpu_oracle_and_abi.py fences it).
#define ST_SCALAR_LOOP _Pragma("clang loop vectorize(disable) interleave(disable)")

inline unsigned grid_for(long long items, int per_block = 256) {
  const long long b = (items + per_block - 1) / per_block;
  return (unsigned)std::min<long long>(std::max<long long>(b, 1), 256ll * 32);
}

// out = (a + b) * scale over C channels of `pixels` pixels (float4 along the channels; the operation order of the conv
// epilogue (v + res) * post_scale)
__global__ __launch_bounds__(256) void avg2_kernel(const float* __restrict__ a, int a_ld, int a_off,
                                                   const float* __restrict__ b, int b_ld, int b_off,
                                                   float* __restrict__ out, int out_ld, int out_off, long long pixels,
                                                   int C4, float scale) {
  const long long total = pixels * C4;
  ST_SCALAR_LOOP
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long p = i / C4;
    const int c = (int)(i - p * C4) * 4;
    const float4 x = *reinterpret_cast<const float4*>(a + (size_t)p * a_ld + a_off + c);
    const float4 y = *reinterpret_cast<const float4*>(b + (size_t)p * b_ld + b_off + c);
    float4 r;
    r.x = (x.x + y.x) * scale; r.y = (x.y + y.y) * scale; r.z = (x.z + y.z) * scale; r.w = (x.w + y.w) * scale;
    *reinterpret_cast<float4*>(out + (size_t)p * out_ld + out_off + c) = r;
  }
}

__global__ __launch_bounds__(256) void elu_inplace_kernel(float* __restrict__ x, int ld, int off, long long pixels, int C4) {
  const long long total = pixels * C4;
  ST_SCALAR_LOOP
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long p = i / C4;
    float4* q = reinterpret_cast<float4*>(x + (size_t)p * ld + off + (int)(i - p * C4) * 4);
    *q = elu4(*q);
  }
}

// ELU of a raw [N][h][w][C] slice, stored nearest-x2 upsampled into a channel slice of an [N][2h][2w][out_ld] buffer
__global__ __launch_bounds__(256) void elu_up2_kernel(const float* __restrict__ in, int in_ld, int in_off,
                                                      float* __restrict__ out, int out_ld, int out_off, int N, int h,
                                                      int w, int C4) {
  const long long total = (long long)N * h * w * C4;
  ST_SCALAR_LOOP
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long p = i / C4;
    const int c = (int)(i - p * C4) * 4;
    const int x = (int)(p % w);
    const long long ny = p / w;             // n * h + y
    const float4 v = elu4(*reinterpret_cast<const float4*>(in + (size_t)p * in_ld + in_off + c));
    const size_t row0 = ((size_t)(2 * ny) * (2 * w) + 2 * x) * out_ld + out_off + c;   // (n, 2y, 2x): 2 * (n*h + y) = n*2h + 2y
    const size_t row1 = row0 + (size_t)(2 * w) * out_ld;
    *reinterpret_cast<float4*>(out + row0) = v;
    *reinterpret_cast<float4*>(out + row0 + out_ld) = v;
    *reinterpret_cast<float4*>(out + row1) = v;
    *reinterpret_cast<float4*>(out + row1 + out_ld) = v;
  }
}

// Per (image, block): sum and max over the block's pixel range of the 64 df channels.  256 threads = 16 pixel slots x
// 16 channel quads; the 4 slots of a wave are combined with shuffles, the 4 waves through LDS, always in the same order.
// part[((n * nblk + blk) * 2 + {0 sum, 1 max}) * 64 + c]
__global__ __launch_bounds__(256) void gate_pool_kernel(const float* __restrict__ df, int ld, int off, int HW, int chunk,
                                                        int nblk, float* __restrict__ part) {
  const int n = blockIdx.y, blk = blockIdx.x;
  const int tid = threadIdx.x, cq = tid & 15, slot = tid >> 4;
  const int p0 = blk * chunk, p1 = min(p0 + chunk, HW);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  const float* base = df + (size_t)n * HW * ld + off + cq * 4;
  ST_SCALAR_LOOP
  for (int p = p0 + slot; p < p1; p += 16) {
    const float4 v = *reinterpret_cast<const float4*>(base + (size_t)p * ld);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
  }
#pragma unroll
  for (int d = 16; d <= 32; d <<= 1) {   // lanes l, l ^ 16, l ^ 32, l ^ 48 hold the same channel quad
    s.x += __shfl_xor(s.x, d); s.y += __shfl_xor(s.y, d); s.z += __shfl_xor(s.z, d); s.w += __shfl_xor(s.w, d);
    m.x = fmaxf(m.x, __shfl_xor(m.x, d)); m.y = fmaxf(m.y, __shfl_xor(m.y, d));
    m.z = fmaxf(m.z, __shfl_xor(m.z, d)); m.w = fmaxf(m.w, __shfl_xor(m.w, d));
  }
  __shared__ float4 ls[4][16], lm[4][16];
  const int wave = tid >> 6, lane = tid & 63;
  if (lane < 16) { ls[wave][lane] = s; lm[wave][lane] = m; }
  __syncthreads();
  if (tid < 16) {
    float4 a = ls[0][tid], b = lm[0][tid];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const float4 u = ls[k][tid], v = lm[k][tid];
      a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
      b.x = fmaxf(b.x, v.x); b.y = fmaxf(b.y, v.y); b.z = fmaxf(b.z, v.z); b.w = fmaxf(b.w, v.w);
    }
    float* o = part + ((size_t)(n * nblk + blk) * 2) * DF_CH + tid * 4;
    *reinterpret_cast<float4*>(o) = a;
    *reinterpret_cast<float4*>(o + DF_CH) = b;
  }
}

// One block of 64 threads per image: combine the partials (block order), the two-layer MLP on the average and on the
// maximum, their sum through the sigmoid.  w1 [16][64], b1 [16], w2 [64][16], b2 [64] (nn.Linear layout).
__global__ __launch_bounds__(64) void gate_mlp_kernel(const float* __restrict__ part, int nblk, int HW,
                                                      const float* __restrict__ w1, const float* __restrict__ b1,
                                                      const float* __restrict__ w2, const float* __restrict__ b2,
                                                      float* __restrict__ scale) {
  const int n = blockIdx.x, c = threadIdx.x;
  __shared__ float pooled[2][DF_CH], hid[2][GATE_HID];
  float s = 0.f, m = -INFINITY;
  for (int k = 0; k < nblk; ++k) {
    const float* q = part + ((size_t)(n * nblk + k) * 2) * DF_CH + c;
    s += q[0];
    m = fmaxf(m, q[DF_CH]);
  }
  pooled[0][c] = s / (float)HW;
  pooled[1][c] = m;
  __syncthreads();
  if (c < 2 * GATE_HID) {
    const int which = c / GATE_HID, j = c % GATE_HID;
    float a = b1[j];
    for (int i = 0; i < DF_CH; ++i) a += w1[j * DF_CH + i] * pooled[which][i];
    hid[which][j] = fmaxf(a, 0.f);
  }
  __syncthreads();
  float a0 = b2[c], a1 = b2[c];
  for (int j = 0; j < GATE_HID; ++j) {
    a0 += w2[c * GATE_HID + j] * hid[0][j];
    a1 += w2[c * GATE_HID + j] * hid[1][j];
  }
  const float t = a0 + a1;
  scale[n * DF_CH + c] = 1.f / (1.f + expf(-t));
}

// out slice = df * (1 - s[n][c])
__global__ __launch_bounds__(256) void gate_apply_kernel(const float* __restrict__ df, int ld, int off,
                                                         const float* __restrict__ scale, float* __restrict__ out,
                                                         int out_ld, int out_off, int N, int HW) {
  const long long total = (long long)N * HW * (DF_CH / 4);
  ST_SCALAR_LOOP
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long p = i / (DF_CH / 4);
    const int c = (int)(i - p * (DF_CH / 4)) * 4;
    const int n = (int)(p / HW);
    const float4 v = *reinterpret_cast<const float4*>(df + (size_t)p * ld + off + c);
    const float4 s = *reinterpret_cast<const float4*>(scale + n * DF_CH + c);
    float4 r;
    r.x = v.x * (1.f - s.x); r.y = v.y * (1.f - s.y); r.z = v.z * (1.f - s.z); r.w = v.w * (1.f - s.w);
    *reinterpret_cast<float4*>(out + (size_t)p * out_ld + out_off + c) = r;
  }
}

// pred[p] = ReLU(bias + sum_c ELU(x[p][c]) * w[c]) over the 128 raw dconv3_1 channels: 32 lanes x float4 per pixel,
// two pixels per wave, butterfly over the 32 lanes.  pred2 (may be NULL) receives the same values.
__global__ __launch_bounds__(256) void elu_reg_relu_kernel(const float* __restrict__ x, int ld, int off,
                                                           const float* __restrict__ w, float bias, long long pixels,
                                                           float* __restrict__ pred, float* __restrict__ pred2) {
  const int lane32 = threadIdx.x & 31;
  const float4 wv = *reinterpret_cast<const float4*>(w + lane32 * 4);
  const long long groups = (long long)gridDim.x * (blockDim.x >> 5);
  const long long rounds = (pixels + groups - 1) / groups;     // every lane runs every round: the shuffles stay convergent
  long long p = (long long)blockIdx.x * (blockDim.x >> 5) + (threadIdx.x >> 5);
  ST_SCALAR_LOOP
  for (long long r = 0; r < rounds; ++r, p += groups) {
    float a = 0.f;
    if (p < pixels) {
      const float4 v = elu4(*reinterpret_cast<const float4*>(x + (size_t)p * ld + off + lane32 * 4));
      a = (v.x * wv.x + v.y * wv.y) + (v.z * wv.z + v.w * wv.w);
    }
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) a += __shfl_xor(a, d);
    if (lane32 == 0 && p < pixels) {
      const float y = fmaxf(a + bias, 0.f);
      pred[p] = y;
      if (pred2) pred2[p] = y;
    }
  }
}

// torch's bilinear rule with align_corners=False: src = (dst + 0.5) * in / out - 0.5, clamped at 0
__global__ __launch_bounds__(256) void bilinear_kernel(const float* __restrict__ in, int N, int h, int w,
                                                       float* __restrict__ out, int H, int W, float sy, float sx) {
  const long long total = (long long)N * H * W;
  ST_SCALAR_LOOP
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int X = (int)(i % W);
    const long long t = i / W;
    const int Y = (int)(t % H), n = (int)(t / H);
    const float fy = fmaxf(sy * ((float)Y + 0.5f) - 0.5f, 0.f), fx = fmaxf(sx * ((float)X + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly = fminf(fmaxf(fy - (float)y0, 0.f), 1.f), lx = fminf(fmaxf(fx - (float)x0, 0.f), 1.f);
    const float* q = in + (size_t)n * h * w;
    const float top = (1.f - lx) * q[(size_t)y0 * w + x0] + lx * q[(size_t)y0 * w + x1];
    const float bot = (1.f - lx) * q[(size_t)y1 * w + x0] + lx * q[(size_t)y1 * w + x1];
    out[i] = (1.f - ly) * top + ly * bot;
  }
}

// The map the per-box depth stage reads (st_disp_fuse): up2 = the head's half-resolution prediction at [H][W] by the
// arithmetic of bilinear_kernel, expression for expression (mode 1 is bit-equal to it), or - mode 2 - the input disparity
// wherever that is valid (> 0).  A thread owns 4 output columns of one row: one 16-byte load of disp and one 16-byte
// store where the quad is whole and 16-byte aligned, scalar accesses otherwise (unaligned rows, the tail of a width that
// is no multiple of 4).  With the source at exactly half the size (sx = sy = 0.5) its 4 pixels interpolate between the
// source columns a - 1 .. a + 2 (a = X0 / 2), clamped to the map: 4 loads per source row, not 8.  blockIdx.y = frame.
// The count of head-filled pixels: a shuffle reduction per wave, the 16 waves of the workgroup through 64 bytes of LDS,
// then ONE integer atomic per workgroup.  The N counters share a cache line and atomics on one line are served one
// after the other, about 10 ns each on an MI355X: with one atomic per WAVE (8192 at 8 x 736 x 1280) the counter alone
// cost 85 us next to a 24 us kernel, which is why the workgroup is as large as it can be - 512 atomics.
constexpr int FUSE_THREADS = 1024;
__global__ __launch_bounds__(FUSE_THREADS) void disp_fuse_kernel(const float* __restrict__ dense,
                                                                 const float* __restrict__ disp, size_t disp_stride, int H,
                                                                 int W, int ext_h, int ext_w, int mode, float sy, float sx,
                                                                 float* __restrict__ out, int* __restrict__ filled) {
  const int n = blockIdx.y, h = H >> 1, w = W >> 1, W4 = (W + 3) >> 2;
  const int items = H * W4;
  const float* q = dense + (size_t)n * h * w;
  const float* dn = disp + (size_t)n * disp_stride;
  float* on = out + (size_t)n * H * W;
  int count = 0;
  ST_SCALAR_LOOP
  for (int i = blockIdx.x * FUSE_THREADS + threadIdx.x; i < items; i += gridDim.x * FUSE_THREADS) {
    const int Y = i / W4, X0 = (i - Y * W4) * 4;
    const float fy = fmaxf(sy * ((float)Y + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)fy, h - 1);
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0);
    const float ly = fminf(fmaxf(fy - (float)y0, 0.f), 1.f);
    const float* r0 = q + (size_t)y0 * w;
    const float* r1 = q + (size_t)y1 * w;
    // the 8 source values, loaded unconditionally and independently of each other (one wait for all of them); every
    // x0 / x1 below is one of these four clamped columns, picked by index with selects - the same cell, so the same bits
    const int a = X0 >> 1;
    const int c0 = max(a - 1, 0), c1 = min(a, w - 1), c2 = min(a + 1, w - 1), c3 = min(a + 2, w - 1);
    const float t_0 = r0[c0], t_1 = r0[c1], t_2 = r0[c2], t_3 = r0[c3];
    const float b_0 = r1[c0], b_1 = r1[c1], b_2 = r1[c2], b_3 = r1[c3];
    float up[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {                // (columns past W - the tail quad - clamp like any other; never stored)
      const float fx = fmaxf(sx * ((float)(X0 + j) + 0.5f) - 0.5f, 0.f);
      const int x0 = min((int)fx, w - 1);
      const int x1 = x0 + (x0 < w - 1 ? 1 : 0);
      const float lx = fminf(fmaxf(fx - (float)x0, 0.f), 1.f);
      const float t0 = x0 == c0 ? t_0 : x0 == c1 ? t_1 : x0 == c2 ? t_2 : t_3;
      const float b0 = x0 == c0 ? b_0 : x0 == c1 ? b_1 : x0 == c2 ? b_2 : b_3;
      const float t1 = x1 == c0 ? t_0 : x1 == c1 ? t_1 : x1 == c2 ? t_2 : t_3;
      const float b1 = x1 == c0 ? b_0 : x1 == c1 ? b_1 : x1 == c2 ? b_2 : b_3;
      const float top = (1.f - lx) * t0 + lx * t1;
      const float bot = (1.f - lx) * b0 + lx * b1;
      up[j] = (1.f - ly) * top + ly * bot;
    }
    const size_t o = (size_t)Y * W + X0;
    const bool whole = X0 + 4 <= W;
    float v[4] = {up[0], up[1], up[2], up[3]};
    bool head[4] = {true, true, true, true};
    if (mode == 2) {
      float d[4] = {0.f, 0.f, 0.f, 0.f};
      if (whole && ((reinterpret_cast<uintptr_t>(dn + o) & 15) == 0)) {
        const float4 dv = *reinterpret_cast<const float4*>(dn + o);
        d[0] = dv.x; d[1] = dv.y; d[2] = dv.z; d[3] = dv.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (X0 + j < W) d[j] = dn[o + j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        head[j] = !(d[j] > 0.f);                 // 0, -0.0, negatives and NaN take the head's value; +Inf is kept
        v[j] = head[j] ? up[j] : d[j];
      }
    }
    if (Y < ext_h) {
#pragma unroll
      for (int j = 0; j < 4; ++j) count += (head[j] && X0 + j < ext_w) ? 1 : 0;
    }
    if (whole && ((reinterpret_cast<uintptr_t>(on + o) & 15) == 0)) {
      *reinterpret_cast<float4*>(on + o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (X0 + j < W) on[o + j] = v[j];
    }
  }
  if (filled) {                                  // (uniform) every thread arrives here: full waves, a full barrier
    __shared__ int part[FUSE_THREADS / 64];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) count += __shfl_xor(count, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
      int total = 0;
#pragma unroll
      for (int k = 0; k < FUSE_THREADS / 64; ++k) total += part[k];
      if (total) atomicAdd(filled + n, total);
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int avg2_launch(const float* a, int a_ld, int a_off, const float* b, int b_ld, int b_off, float* out, int out_ld,
                int out_off, long long pixels, int C, float scale, hipStream_t stream) {
  ST_REQUIRE(a && b && out && pixels > 0 && C > 0, "avg2: null pointer or empty tensor");
  ST_REQUIRE(((C | a_ld | a_off | b_ld | b_off | out_ld | out_off) & 3) == 0 && aligned16(a) && aligned16(b) && aligned16(out),
             "avg2: channel counts, strides and offsets must be multiples of 4, tensors 16-byte aligned");
  ST_REQUIRE(a_off + C <= a_ld && b_off + C <= b_ld && out_off + C <= out_ld, "avg2: channel slice exceeds ld");
  hipLaunchKernelGGL(avg2_kernel, dim3(grid_for(pixels * (C / 4))), dim3(256), 0, stream, a, a_ld, a_off, b, b_ld, b_off,
                     out, out_ld, out_off, pixels, C / 4, scale);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

}  // namespace st

using namespace st;

namespace {

struct HeadParam {
  std::string name;
  std::vector<int64_t> shape;
  std::vector<float> data;
  bool set = false;
  int64_t numel() const {
    int64_t n = 1;
    for (auto s : shape) n *= s;
    return n;
  }
};

struct HeadConv {
  std::string prefix;
  int cin = 0, cout = 0;
  size_t wgt_off = 0, bias_off = 0, wino_off = 0;
  bool wino = false;
};

constexpr int HEAD_LAUNCHES = 13;
const char* const kLaunchNames[HEAD_LAUNCHES] = {
    "dconv1_1", "elu_inplace(dconv1_1)", "dconv1_2", "elu_up2(dconv1_2)", "gate_pool", "gate_mlp", "gate_apply",
    "dconv2_1", "elu_inplace(dconv2_1)", "dconv2_2", "elu_up2(dconv2_2)", "dconv3_1", "elu_reg_relu"};

struct HeadTap {
  size_t off;
  int N, H, W, C, ld;
};

}  // namespace

struct StDispHead {
  StDispHeadConfig cfg{};
  std::vector<HeadParam> params;
  std::map<std::string, int> pindex;
  HeadConv convs[5];
  size_t w1_off = 0, b1_off = 0, w2_off = 0, b2_off = 0, reg_off = 0;   // float offsets in the weight arena
  float reg_bias = 0.f;
  size_t wgt_floats = 0;
  float* wgt_dev = nullptr;
  bool finalized = false;
  // workspace layout (float offsets)
  size_t o_a = 0, o_b = 0, o_cat = 0, o_d = 0, o_e = 0, o_f = 0, o_g = 0, o_pred = 0, o_part = 0, o_scale = 0, ws_floats = 0;
  int nblk = 1, chunk = POOL_CHUNK;
  std::map<std::string, HeadTap> taps;
  // optional per-launch timing (tools only): events on the caller's stream around every launch of a forward
  bool timing = false;
  std::vector<hipEvent_t> events;   // HEAD_LAUNCHES + 1

  void add_param(const std::string& name, std::vector<int64_t> shape) {
    HeadParam p;
    p.name = name;
    p.shape = std::move(shape);
    params.push_back(std::move(p));
    pindex[name] = (int)params.size() - 1;
  }
  const float* get(const std::string& n) const { return params[pindex.at(n)].data.data(); }
};

extern "C" int st_disp_head_create(const StDispHeadConfig* cfg, StDispHead** out) {
  if (!cfg || !out) return set_error(ST_ERR_INVALID, "st_disp_head_create: null argument");
  ST_REQUIRE(cfg->struct_size == (int)sizeof(StDispHeadConfig), "st_disp_head_create: struct_size mismatch (%d vs %zu)",
             cfg->struct_size, sizeof(StDispHeadConfig));
  ST_REQUIRE(cfg->batch > 0 && cfg->p3_height > 0 && cfg->p3_width > 0, "st_disp_head_create: batch and map size must be positive");
  ST_REQUIRE(cfg->in_channels > 0 && cfg->in_channels % 4 == 0, "st_disp_head_create: in_channels must be a positive multiple of 4 (got %d)",
             cfg->in_channels);
  ST_REQUIRE(cfg->channels > 0 && cfg->channels % 32 == 0 && cfg->channels <= 1024,
             "st_disp_head_create: channels must be a multiple of 32, at most 1024 (got %d)", cfg->channels);
  const long long top = (long long)cfg->batch * 16 * cfg->p3_height * cfg->p3_width;   // pixels of the half-resolution maps
  ST_REQUIRE(top * MID_CH < (1ll << 40) && (long long)cfg->p3_height * cfg->p3_width * 16 < (1ll << 30),
             "st_disp_head_create: maps too large");
  auto h = std::make_unique<StDispHead>();
  h->cfg = *cfg;
  if (h->cfg.bn_eps <= 0) h->cfg.bn_eps = 1e-3;
  const int C = cfg->channels;
  const char* names[5] = {"dconv1_1", "dconv1_2", "dconv2_1", "dconv2_2", "dconv3_1"};
  const int cins[5] = {cfg->in_channels, C, C + DF_CH, MID_CH, MID_CH}, couts[5] = {C, C, MID_CH, MID_CH, REG_CH};
  size_t wf = 0;
  auto bump = [&](size_t n) { size_t o = wf; wf = (wf + n + 63) & ~(size_t)63; return o; };
  for (int i = 0; i < 5; ++i) {   // the reference's state_dict order
    HeadConv& c = h->convs[i];
    c.prefix = names[i]; c.cin = cins[i]; c.cout = couts[i];
    h->add_param(c.prefix + ".conv.weight", {c.cout, c.cin, 3, 3});
    h->add_param(c.prefix + ".bn.weight", {c.cout});
    h->add_param(c.prefix + ".bn.bias", {c.cout});
    h->add_param(c.prefix + ".bn.running_mean", {c.cout});
    h->add_param(c.prefix + ".bn.running_var", {c.cout});
    c.wgt_off = bump((size_t)round_up(c.cout, 32) * round_up(9 * c.cin, 32));
    c.bias_off = bump((size_t)round_up(c.cout, 32));
    c.wino = wino_shape_ok(c.cin, c.cout);
    if (c.wino) c.wino_off = bump(wino_packed_floats(c.cout, c.cin));
  }
  h->add_param("reg.conv.weight", {1, REG_CH, 1, 1});
  h->add_param("reg.conv.bias", {1});
  h->add_param("cbam.ChannelGate.mlp.1.weight", {GATE_HID, DF_CH});
  h->add_param("cbam.ChannelGate.mlp.1.bias", {GATE_HID});
  h->add_param("cbam.ChannelGate.mlp.3.weight", {DF_CH, GATE_HID});
  h->add_param("cbam.ChannelGate.mlp.3.bias", {DF_CH});
  h->reg_off = bump(REG_CH);
  h->w1_off = bump(GATE_HID * DF_CH); h->b1_off = bump(GATE_HID);
  h->w2_off = bump(DF_CH * GATE_HID); h->b2_off = bump(DF_CH);
  h->wgt_floats = wf;

  const int N = cfg->batch, ph = cfg->p3_height, pw = cfg->p3_width;
  const size_t px8 = (size_t)N * ph * pw, px4 = 4 * px8, px2 = 16 * px8;
  const int HW4 = 4 * ph * pw;
  h->nblk = std::min(ceil_div(HW4, POOL_CHUNK), POOL_MAX_BLOCKS);
  h->chunk = ceil_div(HW4, h->nblk);
  size_t ws = 0;
  auto wbump = [&](size_t n) { size_t o = ws; ws = (ws + n + 63) & ~(size_t)63; return o; };
  h->o_b = wbump(px8 * C);                  // dconv1_2, raw
  h->o_cat = wbump(px4 * (C + DF_CH));      // [ELU(dconv1_2) x2 | gated df]
  h->o_e = wbump(px4 * MID_CH);             // dconv2_2, raw
  h->o_g = wbump(px2 * REG_CH);             // dconv3_1, raw
  h->o_pred = wbump(px2);
  h->o_part = wbump((size_t)N * h->nblk * 2 * DF_CH);
  h->o_scale = wbump((size_t)N * DF_CH);
  h->o_f = wbump(px2 * MID_CH);             // ELU(dconv2_2) x2; until it is written its memory holds ...
  h->o_a = h->o_f;                          // ... dconv1_1 (ELU in place) and
  h->o_d = h->o_f + ((px8 * C + 63) & ~(size_t)63);   // ... dconv2_1 (ELU in place): C + 4 * 256 <= 16 * 256 floats per p3 pixel
  h->ws_floats = ws;
  h->taps["dconv1_2"] = {h->o_b, N, ph, pw, C, C};
  h->taps["gate_scale"] = {h->o_scale, N, 1, 1, DF_CH, DF_CH};
  h->taps["cat"] = {h->o_cat, N, 2 * ph, 2 * pw, C + DF_CH, C + DF_CH};
  h->taps["dconv2_2"] = {h->o_e, N, 2 * ph, 2 * pw, MID_CH, MID_CH};
  h->taps["dconv3_1_raw"] = {h->o_g, N, 4 * ph, 4 * pw, REG_CH, REG_CH};
  h->taps["pred"] = {h->o_pred, N, 4 * ph, 4 * pw, 1, 1};
  *out = h.release();
  return ST_OK;
}

extern "C" int st_disp_head_destroy(StDispHead* head) {
  if (!head) return ST_OK;
  if (head->wgt_dev) (void)hipFree(head->wgt_dev);
  for (auto& e : head->events) (void)hipEventDestroy(e);
  delete head;
  return ST_OK;
}

extern "C" int st_disp_head_num_params(const StDispHead* head) { return head ? (int)head->params.size() : 0; }

extern "C" int st_disp_head_param_info(const StDispHead* head, int idx, char* name, int name_cap, int64_t shape[4],
                                       int* ndim) {
  if (!head || idx < 0 || idx >= (int)head->params.size())
    return set_error(ST_ERR_INVALID, "st_disp_head_param_info: bad index %d", idx);
  const HeadParam& p = head->params[idx];
  if (name && name_cap > 0) {
    std::strncpy(name, p.name.c_str(), (size_t)name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (ndim) *ndim = (int)p.shape.size();
  if (shape)
    for (size_t i = 0; i < 4; ++i) shape[i] = i < p.shape.size() ? p.shape[i] : 1;
  return ST_OK;
}

extern "C" int st_disp_head_set_param(StDispHead* head, const char* name, const float* host, int64_t numel) {
  if (!head || !name || !host) return set_error(ST_ERR_INVALID, "st_disp_head_set_param: null argument");
  auto it = head->pindex.find(name);
  if (it == head->pindex.end()) return set_error(ST_ERR_NOTFOUND, "st_disp_head_set_param: unknown parameter '%s'", name);
  HeadParam& p = head->params[it->second];
  ST_REQUIRE(numel == p.numel(), "st_disp_head_set_param: '%s' expects %lld values, got %lld", name, (long long)p.numel(),
             (long long)numel);
  p.data.assign(host, host + numel);
  p.set = true;
  head->finalized = false;
  return ST_OK;
}

extern "C" int st_disp_head_finalize(StDispHead* head) {
  if (!head) return set_error(ST_ERR_INVALID, "st_disp_head_finalize: null head");
  for (const HeadParam& p : head->params)
    if (!p.set) return set_error(ST_ERR_STATE, "st_disp_head_finalize: parameter '%s' was never set", p.name.c_str());
  std::vector<float> host(head->wgt_floats, 0.f);
  for (const HeadConv& c : head->convs) {
    ST_CHECK(st_conv_pack_weights(head->get(c.prefix + ".conv.weight"), nullptr, head->get(c.prefix + ".bn.weight"),
                                  head->get(c.prefix + ".bn.bias"), head->get(c.prefix + ".bn.running_mean"),
                                  head->get(c.prefix + ".bn.running_var"), head->cfg.bn_eps, c.cout, c.cin, 3, 3,
                                  host.data() + c.wgt_off, host.data() + c.bias_off));
    if (c.wino) ST_CHECK(wino_pack_weights(host.data() + c.wgt_off, c.cout, c.cin, host.data() + c.wino_off));
  }
  std::memcpy(host.data() + head->reg_off, head->get("reg.conv.weight"), sizeof(float) * REG_CH);
  head->reg_bias = head->get("reg.conv.bias")[0];
  std::memcpy(host.data() + head->w1_off, head->get("cbam.ChannelGate.mlp.1.weight"), sizeof(float) * GATE_HID * DF_CH);
  std::memcpy(host.data() + head->b1_off, head->get("cbam.ChannelGate.mlp.1.bias"), sizeof(float) * GATE_HID);
  std::memcpy(host.data() + head->w2_off, head->get("cbam.ChannelGate.mlp.3.weight"), sizeof(float) * DF_CH * GATE_HID);
  std::memcpy(host.data() + head->b2_off, head->get("cbam.ChannelGate.mlp.3.bias"), sizeof(float) * DF_CH);
  if (!head->wgt_dev) ST_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&head->wgt_dev), head->wgt_floats * sizeof(float)));
  ST_CHECK_HIP(hipMemcpy(head->wgt_dev, host.data(), head->wgt_floats * sizeof(float), hipMemcpyHostToDevice));
  head->finalized = true;
  return ST_OK;
}

extern "C" size_t st_disp_head_workspace_bytes(const StDispHead* head) { return head ? head->ws_floats * sizeof(float) : 0; }

namespace {

int head_conv(const StDispHead* h, int i, const float* in, int N, int H, int W, int in_ld, int in_off, float* out,
              hipStream_t stream) {
  const HeadConv& c = h->convs[i];
  StConvDesc d{};
  d.in_dev = in; d.N = N; d.Hi = H; d.Wi = W; d.Cin = c.cin; d.in_ld = in_ld; d.in_off = in_off;
  d.wgt_dev = h->wgt_dev + c.wgt_off; d.bias_dev = h->wgt_dev + c.bias_off;
  d.Cout = c.cout; d.KH = d.KW = 3; d.stride = 1; d.pad = 1;
  d.out1_dev = out; d.out1_ld = c.cout; d.out1_off = 0; d.split = c.cout;
  d.post_scale = 1.f; d.act = 0;
  d.wgt_wino_dev = c.wino ? h->wgt_dev + c.wino_off : nullptr;
  // the Winograd instance wherever the layer qualifies (shape, alignment, tensors below 2 GiB), else the implicit GEMM
  // at the library's own tile choice: a function of the shapes alone, so two contexts of one shape run the same kernels
  return conv2d_launch(d, stream, wino_conv_applicable(d) ? 43 : -1, nullptr);
}

}  // namespace

extern "C" int st_disp_head_forward(StDispHead* head, const float* p3_dev, int p3_ld, int p3_off, const float* df_dev,
                                    int df_ld, int df_off, void* workspace_dev, size_t workspace_bytes,
                                    st_stream_t stream_, float* pred_out_dev) {
  if (!head) return set_error(ST_ERR_INVALID, "st_disp_head_forward: null head");
  if (!head->finalized) return set_error(ST_ERR_STATE, "st_disp_head_forward: call st_disp_head_finalize first");
  ST_REQUIRE(p3_dev && df_dev && workspace_dev, "st_disp_head_forward: null pointer");
  if (workspace_bytes < head->ws_floats * sizeof(float))
    return set_error(ST_ERR_WORKSPACE, "st_disp_head_forward: workspace %zu < required %zu", workspace_bytes,
                     head->ws_floats * sizeof(float));
  const StDispHeadConfig& cfg = head->cfg;
  ST_REQUIRE(((p3_ld | p3_off | df_ld | df_off) & 3) == 0 && aligned16(p3_dev) && aligned16(df_dev) && aligned16(workspace_dev),
             "st_disp_head_forward: strides and offsets must be multiples of 4, tensors 16-byte aligned");
  ST_REQUIRE(p3_off >= 0 && p3_off + cfg.in_channels <= p3_ld && df_off >= 0 && df_off + DF_CH <= df_ld,
             "st_disp_head_forward: channel slice exceeds ld");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  float* ws = static_cast<float*>(workspace_dev);
  const int N = cfg.batch, ph = cfg.p3_height, pw = cfg.p3_width, C = cfg.channels, CC = C + DF_CH;
  const long long px8 = (long long)N * ph * pw, px4 = 4 * px8, px2 = 16 * px8;
  float *A = ws + head->o_a, *B = ws + head->o_b, *cat = ws + head->o_cat, *D = ws + head->o_d, *E = ws + head->o_e,
        *F = ws + head->o_f, *G = ws + head->o_g, *pred = ws + head->o_pred, *part = ws + head->o_part,
        *scale = ws + head->o_scale;
  const float* wd = head->wgt_dev;
  if (head->timing && head->events.empty()) {
    head->events.resize(HEAD_LAUNCHES + 1);
    for (auto& e : head->events) ST_CHECK_HIP(hipEventCreate(&e));
  }
  int tick = 0;
#define ST_HEAD_TICK() do { if (head->timing) ST_CHECK_HIP(hipEventRecord(head->events[tick++], stream)); } while (0)
  // 1/8
  ST_HEAD_TICK();
  ST_CHECK(head_conv(head, 0, p3_dev, N, ph, pw, p3_ld, p3_off, A, stream));
  ST_HEAD_TICK();
  hipLaunchKernelGGL(elu_inplace_kernel, dim3(grid_for(px8 * (C / 4))), dim3(256), 0, stream, A, C, 0, px8, C / 4);
  ST_HEAD_TICK();
  ST_CHECK(head_conv(head, 1, A, N, ph, pw, C, 0, B, stream));
  ST_HEAD_TICK();
  hipLaunchKernelGGL(elu_up2_kernel, dim3(grid_for(px8 * (C / 4))), dim3(256), 0, stream, B, C, 0, cat, CC, 0, N, ph, pw, C / 4);
  ST_HEAD_TICK();
  // channel gate on the disparity features, into the other slice of the concat
  hipLaunchKernelGGL(gate_pool_kernel, dim3(head->nblk, N), dim3(256), 0, stream, df_dev, df_ld, df_off, 4 * ph * pw,
                     head->chunk, head->nblk, part);
  ST_HEAD_TICK();
  hipLaunchKernelGGL(gate_mlp_kernel, dim3(N), dim3(64), 0, stream, part, head->nblk, 4 * ph * pw, wd + head->w1_off,
                     wd + head->b1_off, wd + head->w2_off, wd + head->b2_off, scale);
  ST_HEAD_TICK();
  hipLaunchKernelGGL(gate_apply_kernel, dim3(grid_for(px4 * (DF_CH / 4))), dim3(256), 0, stream, df_dev, df_ld, df_off, scale,
                     cat, CC, C, N, 4 * ph * pw);
  ST_HEAD_TICK();
  // 1/4
  ST_CHECK(head_conv(head, 2, cat, N, 2 * ph, 2 * pw, CC, 0, D, stream));
  ST_HEAD_TICK();
  hipLaunchKernelGGL(elu_inplace_kernel, dim3(grid_for(px4 * (MID_CH / 4))), dim3(256), 0, stream, D, MID_CH, 0, px4, MID_CH / 4);
  ST_HEAD_TICK();
  ST_CHECK(head_conv(head, 3, D, N, 2 * ph, 2 * pw, MID_CH, 0, E, stream));
  ST_HEAD_TICK();
  hipLaunchKernelGGL(elu_up2_kernel, dim3(grid_for(px4 * (MID_CH / 4))), dim3(256), 0, stream, E, MID_CH, 0, F, MID_CH, 0, N,
                     2 * ph, 2 * pw, MID_CH / 4);
  ST_HEAD_TICK();
  // 1/2
  ST_CHECK(head_conv(head, 4, F, N, 4 * ph, 4 * pw, MID_CH, 0, G, stream));
  ST_HEAD_TICK();
  hipLaunchKernelGGL(elu_reg_relu_kernel, dim3(grid_for(px2, 8)), dim3(256), 0, stream, G, REG_CH, 0, wd + head->reg_off,
                     head->reg_bias, px2, pred, pred_out_dev);
  ST_HEAD_TICK();
#undef ST_HEAD_TICK
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

extern "C" int st_disp_head_set_timing(StDispHead* head, int enable) {
  if (!head) return set_error(ST_ERR_INVALID, "st_disp_head_set_timing: null head");
  head->timing = enable != 0;
  return ST_OK;
}

extern "C" int st_disp_head_num_launches(void) { return HEAD_LAUNCHES; }

extern "C" const char* st_disp_head_launch_name(int i) { return i >= 0 && i < HEAD_LAUNCHES ? kLaunchNames[i] : ""; }

extern "C" int st_disp_head_launch_times(StDispHead* head, int cap, float* ms) {
  if (!head || !ms) return set_error(ST_ERR_INVALID, "st_disp_head_launch_times: null argument");
  ST_REQUIRE(head->timing && (int)head->events.size() == HEAD_LAUNCHES + 1, "st_disp_head_launch_times: no timed forward has run");
  ST_REQUIRE(cap >= HEAD_LAUNCHES, "st_disp_head_launch_times: capacity %d < %d launches", cap, HEAD_LAUNCHES);
  ST_CHECK_HIP(hipEventSynchronize(head->events[HEAD_LAUNCHES]));
  for (int i = 0; i < HEAD_LAUNCHES; ++i) ST_CHECK_HIP(hipEventElapsedTime(&ms[i], head->events[i], head->events[i + 1]));
  return ST_OK;
}

extern "C" int st_disp_head_tap(const StDispHead* head, const char* name, const void* workspace_dev, const float** ptr_dev,
                                int* N, int* C, int* H, int* W, int* ld) {
  if (!head || !name) return set_error(ST_ERR_INVALID, "st_disp_head_tap: null argument");
  auto it = head->taps.find(name);
  if (it == head->taps.end()) return set_error(ST_ERR_NOTFOUND, "st_disp_head_tap: unknown tap '%s'", name);
  const HeadTap& t = it->second;
  if (ptr_dev) *ptr_dev = static_cast<const float*>(workspace_dev) + t.off;
  if (N) *N = t.N;
  if (C) *C = t.C;
  if (H) *H = t.H;
  if (W) *W = t.W;
  if (ld) *ld = t.ld;
  return ST_OK;
}

extern "C" int st_disp_head_resize(const float* pred_dev, int N, int h, int w, float* out_dev, int H, int W,
                                   st_stream_t stream) {
  ST_REQUIRE(pred_dev && out_dev, "st_disp_head_resize: null pointer");
  ST_REQUIRE(N > 0 && h > 0 && w > 0 && H > 0 && W > 0, "st_disp_head_resize: sizes must be positive");
  ST_REQUIRE((long long)h * w < (1ll << 31) && (long long)H * W < (1ll << 31), "st_disp_head_resize: map too large");
  hipLaunchKernelGGL(bilinear_kernel, dim3(grid_for((long long)N * H * W)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     pred_dev, N, h, w, out_dev, H, W, (float)h / (float)H, (float)w / (float)W);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

extern "C" int st_disp_fuse(const float* dense_dev, const float* disp_dev, size_t disp_frame_stride, int N, int H, int W,
                            int ext_h, int ext_w, int mode, float* out_dev, int32_t* filled_dev, st_stream_t stream_) {
  ST_REQUIRE(dense_dev && disp_dev && out_dev, "st_disp_fuse: null pointer");
  ST_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "st_disp_fuse: sizes must be positive (at most 65535 frames)");
  ST_REQUIRE((H & 1) == 0 && (W & 1) == 0, "st_disp_fuse: H and W must be even (the head predicts at H/2 x W/2), got %d x %d", H, W);
  ST_REQUIRE((long long)H * W < (1ll << 31), "st_disp_fuse: map too large");
  ST_REQUIRE(ext_h >= 1 && ext_h <= H && ext_w >= 1 && ext_w <= W, "st_disp_fuse: extent %d x %d outside the %d x %d map",
             ext_h, ext_w, H, W);
  ST_REQUIRE(mode == 1 || mode == 2, "st_disp_fuse: mode must be 1 (completed) or 2 (fused), got %d", mode);
  ST_REQUIRE(disp_frame_stride >= (size_t)H * W, "st_disp_fuse: disp_frame_stride %zu < H * W = %zu", disp_frame_stride,
             (size_t)H * W);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (filled_dev) ST_CHECK_HIP(hipMemsetAsync(filled_dev, 0, sizeof(int32_t) * (size_t)N, stream));
  const int h = H / 2, w = W / 2;
  const long long items = (long long)H * ((W + 3) / 4);
  // 512 workgroups (8192 waves, two workgroups per CU) at most; the grid-stride loop takes the rest
  const unsigned gx = (unsigned)std::min<long long>((items + FUSE_THREADS - 1) / FUSE_THREADS, std::max(1, 512 / N));
  hipLaunchKernelGGL(disp_fuse_kernel, dim3(gx, (unsigned)N), dim3(FUSE_THREADS), 0, stream, dense_dev, disp_dev,
                     disp_frame_stride, H, W, ext_h, ext_w, mode, (float)h / (float)H, (float)w / (float)W, out_dev,
                     filled_dev);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}
