// The track overlay (include/stereotrack_vis.h): box outlines and id tags painted in place into
// uint8 planar frames on the device, in front of the JPEG forward launch.
//
//   draw_tracks_kernel    one thread owns ONE pixel (its three planes) and walks the frame's boxes in list order,
//                         applying to its own pixel whatever each box paints there: outline blend, tag blend, ink.  A
//                         pixel several boxes touch gets the sequential result whatever the launch geometry - no thread
//                         writes another's pixel, no atomics, no order between threads.  The box fields are read with
//                         wave-uniform addresses (scalar loads); a box that misses the thread's pixel costs a few
//                         compares.  blockIdx.y = frame.
//
// Integer arithmetic apart from the rounding of the four coordinates (floorf(v + 0.5f), one IEEE add); tests/draw_ref.py
// restates the rules in numpy and the kernel equals it byte for byte.
#include <cstdint>

#include "../../include/stereotrack_vis.h"
#include "st_common.h"

namespace {

constexpr int DRAW_THREADS = 256;

// 5x7 glyphs, one byte per row, bit 4 = leftmost column: 0-9, space, '.', '|', '-'
__constant__ uint8_t kFont[14][7] = {
    {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E},
    {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F}, {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E},
    {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},
    {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08},
    {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E}, {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C},
    {0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00}, {0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C},
    {0x04, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04}, {0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00}};

__device__ inline int glyph_index(int ch) {
  if (ch >= '0' && ch <= '9') return ch - '0';
  return ch == '.' ? 11 : (ch == '|' ? 12 : (ch == '-' ? 13 : 10));
}

// nearest pixel of a finite coordinate, kept inside +-2^20 so that the sums below stay in int
__device__ inline int round_px(float v) {
  const float r = floorf(v + 0.5f);
  return (int)fminf(fmaxf(r, -1048576.0f), 1048576.0f);
}

__device__ inline int blend(int a256, int colour, int pixel) { return (a256 * colour + (256 - a256) * pixel + 128) >> 8; }

__global__ __launch_bounds__(DRAW_THREADS) void draw_tracks_kernel(uint8_t* __restrict__ frames, int height, int width,
                                                                   long long image_stride, long long plane_stride,
                                                                   long long row_stride, const StDrawBox* __restrict__ boxes,
                                                                   const int32_t* __restrict__ counts, int max_boxes,
                                                                   int lw, int a256) {
  const long long item = (long long)blockIdx.x * DRAW_THREADS + threadIdx.x;
  if (item >= (long long)height * width) return;
  const int y = (int)(item / width), x = (int)(item - (long long)y * width);
  const int n = blockIdx.y;
  int count = counts[n];
  count = count < 0 ? 0 : (count > max_boxes ? max_boxes : count);
  uint8_t* px = frames + n * image_stride + y * row_stride + x;
  int v[3] = {0, 0, 0};
  bool loaded = false, dirty = false;
  const int half = lw / 2;
  for (int k = 0; k < count; ++k) {
    const StDrawBox& B = boxes[(long long)n * max_boxes + k];
    const float fx1 = B.x1, fy1 = B.y1, fx2 = B.x2, fy2 = B.y2;
    if (!(isfinite(fx1) && isfinite(fy1) && isfinite(fx2) && isfinite(fy2))) continue;
    const int x1 = round_px(fx1), y1 = round_px(fy1), x2 = round_px(fx2), y2 = round_px(fy2);
    if (x2 < x1 || y2 < y1) continue;
    // outline: inside the outer rectangle and not inside the inner one
    const int ox1 = x1 - half, oy1 = y1 - half, ox2 = x2 - half + lw - 1, oy2 = y2 - half + lw - 1;
    const bool outer = x >= ox1 && x <= ox2 && y >= oy1 && y <= oy2;
    const bool inner = x >= ox1 + lw && x <= ox2 - lw && y >= oy1 + lw && y <= oy2 - lw;
    // tag
    const int len = B.label_len > ST_DRAW_LABEL_MAX ? ST_DRAW_LABEL_MAX : B.label_len;
    const int zoom = B.zoom < 1 ? 1 : (B.zoom > 8 ? 8 : B.zoom);
    const int tx = x1 + lw, ty = y1 + lw;
    const bool tag = len > 0 && x >= tx && y >= ty && x < tx + (6 * len + 1) * zoom && y < ty + 9 * zoom;
    if (!((outer && !inner) || tag)) continue;
    if (!loaded) {
#pragma unroll
      for (int p = 0; p < 3; ++p) v[p] = px[p * plane_stride];
      loaded = true;
    }
    dirty = true;
    if (outer && !inner) {
#pragma unroll
      for (int p = 0; p < 3; ++p) v[p] = blend(a256, B.colour[p], v[p]);
    }
    if (tag) {
      const int u = (x - tx) / zoom - 1, w = (y - ty) / zoom - 1;       // font cell, the margin taken off
      bool ink = false;
      if (u >= 0 && w >= 0 && w < 7 && u % 6 < 5 && u / 6 < len) {
        const int gi = glyph_index(B.label[u / 6]);
        ink = (kFont[gi][w] >> (4 - u % 6)) & 1;
      }
#pragma unroll
      for (int p = 0; p < 3; ++p) v[p] = ink ? 0 : blend(a256, B.colour[p], v[p]);
    }
  }
  if (dirty) {
#pragma unroll
    for (int p = 0; p < 3; ++p) px[p * plane_stride] = (uint8_t)v[p];
  }
}

}  // namespace

extern "C" int st_draw_tracks(uint8_t* frames_dev, int N, int height, int width, ptrdiff_t image_stride,
                              ptrdiff_t plane_stride, ptrdiff_t row_stride, const StDrawBox* boxes_dev,
                              const int32_t* counts_dev, int max_boxes, int line_width, int alpha256, st_stream_t stream_) {
  ST_REQUIRE(N >= 1 && N <= 65535, "st_draw_tracks: N must be 1..65535, got %d", N);
  ST_REQUIRE(height >= 1 && height <= 65535 && width >= 1 && width <= 65535, "st_draw_tracks: frame sizes are 1..65535, got %d x %d",
             height, width);
  ST_REQUIRE(max_boxes >= 0 && max_boxes <= 65535, "st_draw_tracks: max_boxes must be 0..65535, got %d", max_boxes);
  ST_REQUIRE(line_width >= 1 && line_width <= 64, "st_draw_tracks: line_width must be 1..64, got %d", line_width);
  ST_REQUIRE(alpha256 >= 0 && alpha256 <= 256, "st_draw_tracks: alpha256 must be 0..256, got %d", alpha256);
  ST_REQUIRE(row_stride >= width && plane_stride > 0 && (N == 1 || image_stride > 0), "st_draw_tracks: bad frame strides");
  if (max_boxes == 0) return ST_OK;                  // nothing to draw: no launch, the pointers are not looked at
  ST_REQUIRE(frames_dev && boxes_dev && counts_dev, "st_draw_tracks: null pointer");
  ST_REQUIRE((reinterpret_cast<uintptr_t>(boxes_dev) & 3) == 0 && (reinterpret_cast<uintptr_t>(counts_dev) & 3) == 0,
             "st_draw_tracks: boxes_dev and counts_dev must be 4-byte aligned");
  const long long tiles = ((long long)height * width + DRAW_THREADS - 1) / DRAW_THREADS;
  hipLaunchKernelGGL(draw_tracks_kernel, dim3((unsigned)tiles, (unsigned)N), dim3(DRAW_THREADS), 0,
                     static_cast<hipStream_t>(stream_), frames_dev, height, width, (long long)image_stride,
                     (long long)plane_stride, (long long)row_stride, boxes_dev, counts_dev, max_boxes, line_width, alpha256);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}
