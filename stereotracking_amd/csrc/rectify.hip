// StereoRectify on the device: st_rectify_remap (include/stereotrack.h section 2) - undistort + rectify F raw frames through
// fixed-point maps in ONE launch.  The rule is cv2.remap's 8-bit INTER_LINEAR on CV_16SC2 maps (5 fractional bits)
// restated as exact integer arithmetic (published algorithm, cv2 un-vendored: parity unpinned); host restatement:
// stereotracking_amd/rectify.py::remap_host, independent one: tests/rectify_ref.py.
//
//   map cell (qx, qy) in 1/32 px;  x0 = qx >> 5, a = qx & 31, y0 = qy >> 5, b = qy & 31 (arithmetic shifts)
//   bilinear: out = ((32-a)(32-b) p00 + a(32-b) p01 + (32-a)b p10 + ab p11 + 512) >> 10
//             a tap outside the raw image = border; a tap of weight 0 is NOT READ (a map cell that is exactly the last
//             column / row never touches the element behind it: a frame may end with its allocation)
//   nearest:  the element at ((qx + 16) >> 5, (qy + 16) >> 5); outside: border (1-byte elements) or 0
//
// Shape: one thread owns 4 adjacent output pixels of one row of one MAP and walks every frame that uses this map: the
// 32 bytes of map cells, the tap offsets, weights and bounds are computed once and serve F/M frames x P planes; one
// packed 4-byte store per plane and frame (bytewise on the tail columns / unaligned rows).  Taps are byte gathers: a
// wave covers 256 output pixels of a row, whose taps lie in a few source rows of a narrow window (rectification is
// smooth), served by L2.  No workspace, no atomics, nothing written outside [0, h2) x [0, w2).
#include "st_common.h"

namespace st {

constexpr int RECT_MAX_FRAMES = 32;

struct RectifyArgs {
  const void* src[RECT_MAX_FRAMES];
  void* dst[RECT_MAX_FRAMES];
  unsigned char map_index[RECT_MAX_FRAMES];
  const int2* maps;      // [M][h2][w2] (qx, qy)
  int F, P, h, w, h2, w2, border;
};

// floor((q + 16) / 32) without the overflow of q + 16
__device__ __forceinline__ int rect_round(int q) { return (q >> 5) + ((q & 31) >= 16 ? 1 : 0); }

__global__ __launch_bounds__(256) void rectify_bilinear_u8_kernel(const RectifyArgs a) {
  const int chunks = (a.w2 + 3) >> 2;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)chunks * a.h2) return;
  const int y = (int)(t / chunks), x = (int)(t % chunks) * 4;
  const int m = blockIdx.y;
  const int n = min(4, a.w2 - x);
  const int2* __restrict__ cell = a.maps + ((long long)m * a.h2 + y) * a.w2 + x;
  int off[4];            // element offset of tap (x0, y0) inside a plane (meaningful only where a tap is read)
  unsigned wgt[4];       // w00 | w01 << 16 (a weight is at most 32 * 32 = 1024)
  unsigned wlo[4];       // w10 | w11 << 16
  unsigned rd[4];        // bit k: tap k is read (inside the image AND weight != 0)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    off[i] = 0; wgt[i] = 0; wlo[i] = 0; rd[i] = 0;
    if (i < n) {
      const int2 q = cell[i];
      const int x0 = q.x >> 5, fa = q.x & 31, y0 = q.y >> 5, fb = q.y & 31;
      const unsigned w00 = (32 - fa) * (32 - fb), w01 = fa * (32 - fb), w10 = (32 - fa) * fb, w11 = fa * fb;
      const bool ix0 = x0 >= 0 && x0 < a.w, ix1 = x0 >= -1 && x0 < a.w - 1;
      const bool iy0 = y0 >= 0 && y0 < a.h, iy1 = y0 >= -1 && y0 < a.h - 1;
      rd[i] = (ix0 && iy0 && w00 ? 1u : 0u) | (ix1 && iy0 && w01 ? 2u : 0u) | (ix0 && iy1 && w10 ? 4u : 0u) |
              (ix1 && iy1 && w11 ? 8u : 0u);
      if (rd[i]) off[i] = y0 * a.w + x0;      // |y0| <= h, |x0| <= w here: a tap is inside, P * h * w < 2^31
      wgt[i] = w00 | (w01 << 16);
      wlo[i] = w10 | (w11 << 16);
    }
  }
  const long long plane_in = (long long)a.h * a.w, plane_out = (long long)a.h2 * a.w2;
  const unsigned bd = (unsigned)a.border;
  for (int f = 0; f < a.F; ++f) {
    if (a.map_index[f] != m) continue;      // wave-uniform
    const unsigned char* __restrict__ src = static_cast<const unsigned char*>(a.src[f]);
    unsigned char* __restrict__ dst = static_cast<unsigned char*>(a.dst[f]) + (long long)y * a.w2 + x;
    for (int p = 0; p < a.P; ++p, src += plane_in, dst += plane_out) {
      unsigned v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned char* s = src + off[i];
        const unsigned p00 = (rd[i] & 1u) ? s[0] : bd;
        const unsigned p01 = (rd[i] & 2u) ? s[1] : bd;
        const unsigned p10 = (rd[i] & 4u) ? s[a.w] : bd;
        const unsigned p11 = (rd[i] & 8u) ? s[a.w + 1] : bd;
        v[i] = ((wgt[i] & 0xffffu) * p00 + (wgt[i] >> 16) * p01 + (wlo[i] & 0xffffu) * p10 + (wlo[i] >> 16) * p11 + 512u) >> 10;
      }
      if (n == 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        *reinterpret_cast<unsigned*>(dst) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < n) dst[i] = (unsigned char)v[i];
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void rectify_nearest_kernel(const RectifyArgs a) {
  const int chunks = (a.w2 + 3) >> 2;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)chunks * a.h2) return;
  const int y = (int)(t / chunks), x = (int)(t % chunks) * 4;
  const int m = blockIdx.y;
  const int n = min(4, a.w2 - x);
  const int2* __restrict__ cell = a.maps + ((long long)m * a.h2 + y) * a.w2 + x;
  int off[4];
  bool in[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    off[i] = 0; in[i] = false;
    if (i < n) {
      const int2 q = cell[i];
      const int sx = rect_round(q.x), sy = rect_round(q.y);
      in[i] = sx >= 0 && sx < a.w && sy >= 0 && sy < a.h;
      if (in[i]) off[i] = sy * a.w + sx;
    }
  }
  const long long plane_in = (long long)a.h * a.w, plane_out = (long long)a.h2 * a.w2;
  const T outside = sizeof(T) == 1 ? (T)a.border : (T)0;
  for (int f = 0; f < a.F; ++f) {
    if (a.map_index[f] != m) continue;
    const T* __restrict__ src = static_cast<const T*>(a.src[f]);
    T* __restrict__ dst = static_cast<T*>(a.dst[f]) + (long long)y * a.w2 + x;
    for (int p = 0; p < a.P; ++p, src += plane_in, dst += plane_out) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < n) dst[i] = in[i] ? src[off[i]] : outside;
    }
  }
}

}  // namespace st

extern "C" int st_rectify_remap(const void* const* src_dev_ptrs_host, int F, int P, int h, int w, const int* maps_dev,
                                int M, const int* map_index_host, void* const* dst_dev_ptrs_host, void* dst_block_dev,
                                int h2, int w2, int elem_bytes, int bilinear, int border, st_stream_t stream) {
  using namespace st;
  ST_REQUIRE(src_dev_ptrs_host && maps_dev && map_index_host && F > 0 && F <= RECT_MAX_FRAMES,
             "st_rectify_remap: bad argument (1..%d frames)", RECT_MAX_FRAMES);
  ST_REQUIRE((dst_dev_ptrs_host != nullptr) != (dst_block_dev != nullptr),
             "st_rectify_remap: give the destination pointers OR one contiguous (F, P, h2, w2) block");
  ST_REQUIRE((P == 1 || P == 3) && h > 0 && w > 0 && h2 > 0 && w2 > 0 && M > 0 && M <= 256,
             "st_rectify_remap: P must be 1 or 3, sizes positive, 1..256 maps");
  ST_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4, "st_rectify_remap: elem_bytes must be 1, 2 or 4");
  ST_REQUIRE(!bilinear || elem_bytes == 1,
             "st_rectify_remap: bilinear is the 8-bit image path (cv2.remap INTER_LINEAR, uint8); fp32 maps take bilinear = 0");
  ST_REQUIRE(border >= 0 && border <= 255, "st_rectify_remap: border must be in [0, 255]");
  ST_REQUIRE((long long)P * h * w < (1ll << 31) && (long long)P * h2 * w2 < (1ll << 31) &&
             (long long)M * h2 * w2 < (1ll << 31), "st_rectify_remap: image too large");
  ST_REQUIRE((reinterpret_cast<uintptr_t>(maps_dev) & 7) == 0, "st_rectify_remap: maps must be 8-byte aligned");
  RectifyArgs a;
  const size_t frame_bytes = (size_t)P * h2 * w2 * elem_bytes;
  for (int f = 0; f < RECT_MAX_FRAMES; ++f) {
    a.src[f] = nullptr; a.dst[f] = nullptr; a.map_index[f] = 0;
    if (f >= F) continue;
    a.src[f] = src_dev_ptrs_host[f];
    a.dst[f] = dst_block_dev ? static_cast<void*>(static_cast<char*>(dst_block_dev) + f * frame_bytes) : dst_dev_ptrs_host[f];
    ST_REQUIRE(a.src[f] && a.dst[f], "st_rectify_remap: frame %d: null source or destination", f);
    ST_REQUIRE((reinterpret_cast<uintptr_t>(a.src[f]) % elem_bytes) == 0 && (reinterpret_cast<uintptr_t>(a.dst[f]) % elem_bytes) == 0,
               "st_rectify_remap: frame %d not aligned to its element size", f);
    ST_REQUIRE(map_index_host[f] >= 0 && map_index_host[f] < M, "st_rectify_remap: map_index[%d] = %d outside [0, %d)", f,
               map_index_host[f], M);
    a.map_index[f] = (unsigned char)map_index_host[f];
  }
  a.maps = reinterpret_cast<const int2*>(maps_dev);
  a.F = F; a.P = P; a.h = h; a.w = w; a.h2 = h2; a.w2 = w2; a.border = border;
  const long long threads = (long long)((w2 + 3) / 4) * h2;
  const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)M);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (bilinear) hipLaunchKernelGGL(rectify_bilinear_u8_kernel, grid, dim3(256), 0, s, a);
  else if (elem_bytes == 1) hipLaunchKernelGGL(rectify_nearest_kernel<unsigned char>, grid, dim3(256), 0, s, a);
  else if (elem_bytes == 2) hipLaunchKernelGGL(rectify_nearest_kernel<unsigned short>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(rectify_nearest_kernel<unsigned int>, grid, dim3(256), 0, s, a);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}
