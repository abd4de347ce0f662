// Device half of the JPEG writer (include/stereotrack_vis.h): uint8 planar frames of N images of
// one geometry -> quantised int16 coefficients in the reader's layout.  The entropy encode stays on the host
// (jpeg_encode.cpp); what is dense and regular runs here, in ONE launch and without work memory: every component sample
// is a pure function of the pixels (jpeg_fwd_core.h), so colour conversion, edge replication and chroma downsampling
// happen in the load of a block's row.
//
//   jpeg_forward_kernel   the mirror of jpeg_idct_kernel: 8 threads per 8x8 block, 32 blocks per workgroup.  Thread
//                         (b, r) builds ROW r of block b from the pixels (8, 16 or 32 pixels of three planes, byte loads:
//                         the planes carry no alignment), takes it through the row pass into LDS, takes COLUMN r
//                         through the column pass and the quantisation, writes the results back into LDS, and stores
//                         row r of the quantised block with one 16-byte store (a wave writes 1 KiB of consecutive
//                         coefficients per instruction).  A block's tile is 72 words apart from the next, as in the
//                         inverse kernel.  A dummy block runs the block whose DC it carries and stores that DC over
//                         zeros: no block waits for another.
//
// Integer VALU only; the arithmetic is jpeg_fwd_core.h, the text st_jpeg_forward_host runs.
#include <cstdint>

#include "../../include/stereotrack_vis.h"
#include "jpeg_fwd_core.h"
#include "st_common.h"

namespace st {
bool jpeg_fwd_geom(const StJpegInfo& I, jpeg::FwdGeom& g);      // jpeg_encode.cpp
}

namespace {

namespace J = st::jpeg;

constexpr int FWD_THREADS = 256, FWD_BLOCKS = FWD_THREADS / 8, TILE_WORDS = 72;

__global__ __launch_bounds__(FWD_THREADS) void jpeg_forward_kernel(const uint8_t* __restrict__ in, long long image_stride,
                                                                   long long plane_stride, long long row_stride, int rgb,
                                                                   const uint16_t* __restrict__ quant, long long total_blocks,
                                                                   J::FwdGeom g, int16_t* __restrict__ coef) {
  __shared__ __attribute__((aligned(16))) int32_t tile[FWD_BLOCKS * TILE_WORDS];
  const int b = threadIdx.x >> 3, r = threadIdx.x & 7;
  const long long blk = (long long)blockIdx.x * FWD_BLOCKS + b;
  const bool live = blk < total_blocks;
  int32_t* t = tile + b * TILE_WORDS;
  int c = 0;
  bool dummy = false;
  if (live) {
    const long long n = blk / g.blocks_per_image;
    const long long rem = blk - n * g.blocks_per_image;
    c = rem >= g.first_block[2] ? 2 : (rem >= g.first_block[1] ? 1 : 0);
    const long long idx = rem - g.first_block[c];
    const int bw = g.bw[c];
    const int by = (int)(idx / bw), bx = (int)(idx - (long long)by * bw);
    int sy, sx;
    dummy = J::fwd_dummy_source(g, c, by, bx, sy, sx);
    const uint8_t* img = in + n * image_stride;
    const int ncomp = g.ncomp;
    auto ld = [img, plane_stride, row_stride, rgb, ncomp](int p, int y, int x) {
      const int plane = ncomp == 1 ? 0 : (rgb ? p : 2 - p);
      return (int)img[plane * plane_stride + y * row_stride + x];
    };
    int32_t row[8], res[8];
    J::fwd_row(ld, g, c, sy * 8 + r, sx * 8, row);
    J::fdct_1d(row, res, false);
    *reinterpret_cast<int4*>(t + r * 8) = make_int4(res[0], res[1], res[2], res[3]);
    *reinterpret_cast<int4*>(t + r * 8 + 4) = make_int4(res[4], res[5], res[6], res[7]);
  }
  __syncthreads();
  if (live) {                       // the column pass on column r, in place: no other thread touches this column
    int32_t col[8], res[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) col[k] = t[k * 8 + r];
    J::fdct_1d(col, res, true);
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k * 8 + r] = (int32_t)J::fwd_quantise(res[k], quant[c * 64 + k * 8 + r]);
  }
  __syncthreads();
  if (!live) return;
  const int4 lo = *reinterpret_cast<const int4*>(t + r * 8), hi = *reinterpret_cast<const int4*>(t + r * 8 + 4);
  uint4 v;
  v.x = ((uint32_t)lo.x & 0xffffu) | ((uint32_t)lo.y << 16);
  v.y = ((uint32_t)lo.z & 0xffffu) | ((uint32_t)lo.w << 16);
  v.z = ((uint32_t)hi.x & 0xffffu) | ((uint32_t)hi.y << 16);
  v.w = ((uint32_t)hi.z & 0xffffu) | ((uint32_t)hi.w << 16);
  if (dummy) v = make_uint4(r == 0 ? ((uint32_t)lo.x & 0xffffu) : 0u, 0u, 0u, 0u);
  *reinterpret_cast<uint4*>(coef + blk * 64 + r * 8) = v;       // the base is 16-byte aligned, a row is 16 bytes
}

}  // namespace

extern "C" int st_jpeg_forward(const uint8_t* in_dev, ptrdiff_t image_stride, ptrdiff_t plane_stride, ptrdiff_t row_stride,
                               int rgb_order, const uint16_t* quant_dev, int N, const StJpegInfo* info, int16_t* coef_dev,
                               st_stream_t stream_) {
  ST_REQUIRE(in_dev && quant_dev && info && coef_dev, "st_jpeg_forward: null pointer");
  ST_REQUIRE(info->struct_size == (int)sizeof(StJpegInfo), "st_jpeg_forward: StJpegInfo.struct_size %d, this library has %d",
             info->struct_size, (int)sizeof(StJpegInfo));
  ST_REQUIRE(N >= 1 && N <= 65535, "st_jpeg_forward: N must be 1..65535, got %d", N);
  J::FwdGeom g;
  ST_REQUIRE(st::jpeg_fwd_geom(*info, g), "st_jpeg_forward: StJpegInfo is not what st_jpeg_encode_geometry returns for its width / height / sampling");
  ST_REQUIRE((reinterpret_cast<uintptr_t>(quant_dev) & 15) == 0 && (reinterpret_cast<uintptr_t>(coef_dev) & 15) == 0,
             "st_jpeg_forward: quant_dev and coef_dev must be 16-byte aligned");
  ST_REQUIRE(row_stride >= info->width && (info->components == 1 || plane_stride > 0) && (N == 1 || image_stride > 0),
             "st_jpeg_forward: bad input strides");
  const long long total = g.blocks_per_image * N;
  const long long groups = (total + FWD_BLOCKS - 1) / FWD_BLOCKS;
  ST_REQUIRE(groups < (1ll << 31), "st_jpeg_forward: batch too large for one launch");
  hipLaunchKernelGGL(jpeg_forward_kernel, dim3((unsigned)groups), dim3(FWD_THREADS), 0, static_cast<hipStream_t>(stream_),
                     in_dev, (long long)image_stride, (long long)plane_stride, (long long)row_stride, rgb_order ? 1 : 0,
                     quant_dev, total, g, coef_dev);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}
