// Device half of the JPEG reader (include/stereotrack_jpeg.h): quantised coefficients of N
// images of one geometry -> uint8 planar BGR (or RGB) frames, the layout RawFrames and the raw stem kernels take.  The
// entropy decode stays on the host (jpeg_io.cpp); what is dense and regular runs here, in two launches:
//
//   A  jpeg_idct_kernel   dequantise, inverse DCT (columns, then rows), clamp -> uint8 component planes in caller work
//                         memory, at component resolution.  8 threads per 8x8 block, 32 blocks per workgroup: thread
//                         (b, r) loads ROW r of block b with one 16-byte load (a wave reads 1 KiB of consecutive
//                         coefficients per instruction), dequantises it into LDS, takes COLUMN r through pass 1 in
//                         place, then row r through pass 2, and stores 8 samples with one 8-byte store.  A block's tile
//                         is 72 words apart from the next (64 + 8): the column reads of the four blocks of a 32-lane
//                         half then fall on four different groups of 8 banks.
//   B  jpeg_color_kernel  per thread 4 neighbouring pixels of one row: the luma quad (one 4-byte load), chroma upsampled
//                         from the component plane's columns a - 1 .. a + 2 (clamped; 4 loads per chroma row for the quad,
//                         not 2 per pixel: DESIGN.md 25 has the measurement), colour conversion, one 4-byte store per
//                         plane where the quad is whole and its address 4-byte aligned, scalar stores otherwise
//                         (unaligned rows, the tail of a width that is no multiple of 4).  blockIdx.y = image.
//
// Integer VALU only; the arithmetic is jpeg_core.h, the text st_jpeg_reconstruct_host runs.  The padded MCU area is
// computed and dropped: A stores only comp_w x comp_h of each plane, B reads only that and stores only width x height.
#include <algorithm>
#include <cstdint>

#include "../../include/stereotrack_jpeg.h"
#include "jpeg_core.h"
#include "st_common.h"

namespace st {
bool jpeg_geometry_ok(const StJpegInfo& info);      // jpeg_io.cpp
}

namespace {

namespace J = st::jpeg;

constexpr int IDCT_THREADS = 256, IDCT_BLOCKS = IDCT_THREADS / 8, TILE_WORDS = 72;
constexpr int COLOR_THREADS = 256;

struct JpegGeom {
  int ncomp, hs, vs;
  int width, height;
  int bw[3], cw[3], ch[3];
  long long first_block[3];     // index of each component's first block within an image (absent components: blocks_per_image)
  long long plane_off[3];       // byte offset of each component plane within an image's work memory
  long long blocks_per_image, work_per_image;
};

__global__ __launch_bounds__(IDCT_THREADS) void jpeg_idct_kernel(const int16_t* __restrict__ coef,
                                                                 const uint16_t* __restrict__ quant, long long total_blocks,
                                                                 JpegGeom g, uint8_t* __restrict__ work) {
  __shared__ __attribute__((aligned(16))) int32_t tile[IDCT_BLOCKS * TILE_WORDS];
  const int b = threadIdx.x >> 3, r = threadIdx.x & 7;
  const long long blk = (long long)blockIdx.x * IDCT_BLOCKS + b;
  const bool live = blk < total_blocks;
  int32_t* t = tile + b * TILE_WORDS;
  long long n = 0, idx = 0;
  int c = 0;
  if (live) {
    n = blk / g.blocks_per_image;
    const long long rem = blk - n * g.blocks_per_image;
    c = rem >= g.first_block[2] ? 2 : (rem >= g.first_block[1] ? 1 : 0);
    idx = rem - g.first_block[c];
    const int4 cv = *reinterpret_cast<const int4*>(coef + blk * 64 + r * 8);
    const uint4 qv = *reinterpret_cast<const uint4*>(quant + (n * 3 + c) * 64 + r * 8);
    const uint32_t cw_[4] = {(uint32_t)cv.x, (uint32_t)cv.y, (uint32_t)cv.z, (uint32_t)cv.w};
    const uint32_t qw_[4] = {qv.x, qv.y, qv.z, qv.w};
    int32_t d[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      d[2 * j] = J::dequant((int16_t)(cw_[j] & 0xffffu), (uint16_t)(qw_[j] & 0xffffu));
      d[2 * j + 1] = J::dequant((int16_t)(cw_[j] >> 16), (uint16_t)(qw_[j] >> 16));
    }
    *reinterpret_cast<int4*>(t + r * 8) = make_int4(d[0], d[1], d[2], d[3]);
    *reinterpret_cast<int4*>(t + r * 8 + 4) = make_int4(d[4], d[5], d[6], d[7]);
  }
  __syncthreads();
  if (live) {                       // pass 1 on column r, in place: no other thread touches this column
    int32_t col[8], res[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) col[k] = t[k * 8 + r];
    J::idct_1d(col, res, J::PASS1_SHIFT);
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k * 8 + r] = res[k];
  }
  __syncthreads();
  if (!live) return;
  const int4 lo = *reinterpret_cast<const int4*>(t + r * 8), hi = *reinterpret_cast<const int4*>(t + r * 8 + 4);
  const int32_t row[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  int32_t res[8];
  J::idct_1d(row, res, J::PASS2_SHIFT);
  uint8_t s[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = J::idct_sample(res[k]);
  const int bw = g.bw[c];
  const int by = (int)(idx / bw), bx = (int)(idx - (long long)by * bw);
  const int y = by * 8 + r, x0 = bx * 8;
  if (y >= g.ch[c] || x0 >= g.cw[c]) return;       // padded MCU area: computed, never stored
  uint8_t* dst = work + n * g.work_per_image + g.plane_off[c] + (long long)y * (bw * 8) + x0;
  if (x0 + 8 <= g.cw[c]) {
    uint2 v;
    v.x = s[0] | (s[1] << 8) | (s[2] << 16) | ((uint32_t)s[3] << 24);
    v.y = s[4] | (s[5] << 8) | (s[6] << 16) | ((uint32_t)s[7] << 24);
    *reinterpret_cast<uint2*>(dst) = v;            // plane pitch and x0 are multiples of 8, the base of 16
  } else {
    for (int k = 0; k < 8; ++k)
      if (x0 + k < g.cw[c]) dst[k] = s[k];
  }
}

__global__ __launch_bounds__(COLOR_THREADS) void jpeg_color_kernel(const uint8_t* __restrict__ work, JpegGeom g,
                                                                   uint8_t* __restrict__ out, long long image_stride,
                                                                   long long plane_stride, long long row_stride, int rgb) {
  const int W4 = (g.width + 3) >> 2;
  const long long item = (long long)blockIdx.x * COLOR_THREADS + threadIdx.x;
  if (item >= (long long)W4 * g.height) return;
  const int y = (int)(item / W4), x0 = (int)(item - (long long)y * W4) * 4;
  const uint8_t* wn = work + (long long)blockIdx.y * g.work_per_image;
  // the luma quad: inside the plane's pitch (a multiple of 8 >= width); columns >= width are stale and never stored
  const uint32_t yq = *reinterpret_cast<const uint32_t*>(wn + g.plane_off[0] + (long long)y * (g.bw[0] * 8) + x0);
  int cc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  if (g.ncomp == 3) {
#pragma unroll
    for (int c = 1; c < 3; ++c) {
      const uint8_t* pl = wn + g.plane_off[c];
      const int pitch = g.bw[c] * 8;
      if (!g.hs) {       // 4:4:4: the chroma quad like the luma quad, one aligned 4-byte load (columns >= width never stored)
        const uint32_t q = *reinterpret_cast<const uint32_t*>(pl + (long long)y * pitch + x0);
#pragma unroll
        for (int j = 0; j < 4; ++j) cc[c - 1][j] = (q >> (8 * j)) & 255;
      } else {
        J::chroma_quad([pl, pitch](int cx, int cy) { return (int)pl[(long long)cy * pitch + cx]; }, x0, y, g.cw[c], g.ch[c],
                       g.hs, g.vs, cc[c - 1]);
      }
    }
  }
  uint8_t px[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int Y = (yq >> (8 * j)) & 255;
    uint8_t r, gg, b;
    if (g.ncomp == 1)
      r = gg = b = (uint8_t)Y;
    else
      J::ycc_to_rgb(Y, cc[0][j], cc[1][j], r, gg, b);
    px[0][j] = rgb ? r : b;          // selects, not indexed stores: px stays in registers
    px[1][j] = gg;
    px[2][j] = rgb ? b : r;
  }
  uint8_t* o = out + (long long)blockIdx.y * image_stride + (long long)y * row_stride + x0;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    uint8_t* op = o + p * plane_stride;
    if (x0 + 4 <= g.width && (reinterpret_cast<uintptr_t>(op) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(op) = px[p][0] | (px[p][1] << 8) | (px[p][2] << 16) | ((uint32_t)px[p][3] << 24);
    } else {
      for (int j = 0; j < 4; ++j)
        if (x0 + j < g.width) op[j] = px[p][j];
    }
  }
}

// The kernels index memory with the struct's grids, so a struct that is not what st_jpeg_info makes of its width /
// height / components / sampling is refused before any launch (st::jpeg_geometry_ok, jpeg_io.cpp: the one text of it).
bool make_geom(const StJpegInfo& I, JpegGeom& g) {
  if (!st::jpeg_geometry_ok(I)) return false;
  g.ncomp = I.components;
  g.hs = I.sampling >= ST_JPEG_422;
  g.vs = I.sampling == ST_JPEG_420;
  g.width = I.width;
  g.height = I.height;
  long long blocks = 0;
  for (int c = 0; c < 3; ++c) {
    g.first_block[c] = blocks;                 // absent components: blocks_per_image
    g.plane_off[c] = blocks * 64;
    g.bw[c] = c < I.components ? I.blocks_w[c] : 0;
    g.cw[c] = c < I.components ? I.comp_w[c] : 0;
    g.ch[c] = c < I.components ? I.comp_h[c] : 0;
    if (c < I.components) blocks += (long long)I.blocks_w[c] * I.blocks_h[c];
  }
  g.blocks_per_image = blocks;
  g.work_per_image = (long long)I.work_bytes;
  return true;
}

}  // namespace

extern "C" size_t st_jpeg_work_bytes(const StJpegInfo* info, int N) {
  JpegGeom g;
  if (!info || info->struct_size != (int)sizeof(StJpegInfo) || N < 1 || !make_geom(*info, g)) return 0;
  return (size_t)g.work_per_image * (size_t)N;
}

extern "C" int st_jpeg_reconstruct(const int16_t* coef_dev, const uint16_t* quant_dev, int N, const StJpegInfo* info,
                                   void* work_dev, size_t work_bytes, uint8_t* out_dev, ptrdiff_t image_stride,
                                   ptrdiff_t plane_stride, ptrdiff_t row_stride, int rgb_order, st_stream_t stream_) {
  ST_REQUIRE(coef_dev && quant_dev && info && work_dev && out_dev, "st_jpeg_reconstruct: null pointer");
  ST_REQUIRE(info->struct_size == (int)sizeof(StJpegInfo), "st_jpeg_reconstruct: StJpegInfo.struct_size %d, this library has %d",
             info->struct_size, (int)sizeof(StJpegInfo));
  ST_REQUIRE(N >= 1 && N <= 65535, "st_jpeg_reconstruct: N must be 1..65535, got %d", N);
  JpegGeom g;
  ST_REQUIRE(make_geom(*info, g), "st_jpeg_reconstruct: StJpegInfo is not what st_jpeg_info returns for its width / height / sampling");
  ST_REQUIRE((reinterpret_cast<uintptr_t>(coef_dev) & 15) == 0 && (reinterpret_cast<uintptr_t>(quant_dev) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(work_dev) & 15) == 0,
             "st_jpeg_reconstruct: coef_dev, quant_dev and work_dev must be 16-byte aligned");
  if (work_bytes < (size_t)g.work_per_image * (size_t)N)
    return st::set_error(ST_ERR_WORKSPACE, "st_jpeg_reconstruct: work memory of %zu bytes, %zu needed", work_bytes,
                         (size_t)g.work_per_image * (size_t)N);
  ST_REQUIRE(row_stride >= info->width && plane_stride > 0 && image_stride > 0, "st_jpeg_reconstruct: bad output strides");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const long long total = g.blocks_per_image * N;
  const long long groups = (total + IDCT_BLOCKS - 1) / IDCT_BLOCKS;
  const long long items = (long long)((g.width + 3) / 4) * g.height;
  const long long tiles = (items + COLOR_THREADS - 1) / COLOR_THREADS;
  ST_REQUIRE(groups < (1ll << 31) && tiles < (1ll << 31), "st_jpeg_reconstruct: batch too large for one launch");
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)groups), dim3(IDCT_THREADS), 0, stream, coef_dev, quant_dev, total, g,
                     static_cast<uint8_t*>(work_dev));
  ST_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)tiles, (unsigned)N), dim3(COLOR_THREADS), 0, stream,
                     static_cast<const uint8_t*>(work_dev), g, out_dev, (long long)image_stride, (long long)plane_stride,
                     (long long)row_stride, rgb_order ? 1 : 0);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}
