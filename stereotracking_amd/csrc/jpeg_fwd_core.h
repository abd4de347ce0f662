// The JPEG forward core: the ONE copy of the arithmetic that the host routine (jpeg_encode.cpp, st_jpeg_forward_host)
// and the kernel (jpeg_forward.hip, st_jpeg_forward) must agree on to the coefficient - colour conversion, edge
// replication and chroma downsampling in libjpeg's order, the forward DCT and the quantisation.  It restates
// libjpeg-turbo's default compress path [upstream-memory; pinned against Pillow's files by tests/golden/jpeg_write]:
//   jccolor.c   rgb_ycc_convert      16-bit fixed point, the rounding terms folded into the sums
//   jcprepct.c  pre_process_data     rows replicated to the luma vertical factor BEFORE downsampling, the DOWNSAMPLED
//                                    plane's last row replicated after it
//   jcsample.c  h2v1 / h2v2_downsample, fullsize_downsample   columns replicated to width_in_blocks * 8 * h_factor,
//                                    alternating bias 0,1 / 1,2
//   jfdctint.c  jpeg_fdct_islow      CONST_BITS 13, PASS1_BITS 2, rows then columns
//   jcdctmgr.c  quantize             divisor 8 * table entry, rounded half away from zero
//   jccoefct.c  compress_data        dummy blocks: AC 0, DC of the previous block of the MCU
// Integer only.  Every sample is a pure function of (component, row, column) of the pixels, so neither side keeps a
// component plane.  Also a plain C++ header (tests/native/jpeg_write_check.cpp builds it on the CPU under sanitizers).
#pragma once
#include <cstdint>

#include "jpeg_core.h"

namespace st {
namespace jpeg {

// The block grids of one geometry.  bw / bh: the grid padded to whole MCUs (StJpegInfo.blocks_w / blocks_h, the layout
// of the coefficient array); wib / hib: libjpeg's width_in_blocks / height_in_blocks, ceil(true size / 8) - a block of
// the padded grid at or beyond them is a dummy block.
struct FwdGeom {
  int ncomp, hs, vs;
  int width, height;
  int bw[3], bh[3], wib[3], hib[3], ch[3];
  long long first_block[3];     // index of each component's first block within an image (absent: blocks_per_image)
  long long blocks_per_image;
};

ST_JPEG_HD int rgb_to_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
ST_JPEG_HD int rgb_to_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
ST_JPEG_HD int rgb_to_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// component c of the pixel (y, x), both inside the image; ld(plane, y, x) reads plane 0, 1, 2 = R, G, B
template <typename Load>
ST_JPEG_HD int fwd_pixel(Load ld, int ncomp, int c, int y, int x) {
  if (ncomp == 1) return ld(0, y, x);
  const int r = ld(0, y, x), g = ld(1, y, x), b = ld(2, y, x);
  return c == 0 ? rgb_to_y(r, g, b) : (c == 1 ? rgb_to_cb(r, g, b) : rgb_to_cr(r, g, b));
}

// Sample (cy, cx) of component c over the padded grid, as libjpeg's preprocessing leaves it in front of the DCT.
// The row of the DOWNSAMPLED plane is clamped first (its last row is what gets replicated), then the source rows and
// columns are clamped into the image (replication in front of the downsampler).  The bias alternates with the output
// column as given, also beyond the component's true width.
template <typename Load>
ST_JPEG_HD int fwd_sample(Load ld, const FwdGeom& g, int c, int cy, int cx) {
  const int hs = c ? g.hs : 0, vs = c ? g.vs : 0;
  if (cy >= g.ch[c]) cy = g.ch[c] - 1;
  const int H1 = g.height - 1, W1 = g.width - 1;
  if (!hs) {
    return fwd_pixel(ld, g.ncomp, c, cy < H1 ? cy : H1, cx < W1 ? cx : W1);
  }
  const int x0 = 2 * cx < W1 ? 2 * cx : W1, x1 = 2 * cx + 1 < W1 ? 2 * cx + 1 : W1;
  if (!vs) {
    const int y = cy < H1 ? cy : H1;
    return (fwd_pixel(ld, g.ncomp, c, y, x0) + fwd_pixel(ld, g.ncomp, c, y, x1) + (cx & 1)) >> 1;
  }
  const int y0 = 2 * cy < H1 ? 2 * cy : H1, y1 = 2 * cy + 1 < H1 ? 2 * cy + 1 : H1;
  return (fwd_pixel(ld, g.ncomp, c, y0, x0) + fwd_pixel(ld, g.ncomp, c, y0, x1) + fwd_pixel(ld, g.ncomp, c, y1, x0) +
          fwd_pixel(ld, g.ncomp, c, y1, x1) + 1 + (cx & 1)) >> 2;
}

// row `cy`, columns x0 .. x0 + 7 of component c, level shifted
template <typename Load>
ST_JPEG_HD void fwd_row(Load ld, const FwdGeom& g, int c, int cy, int x0, int32_t out[8]) {
  for (int k = 0; k < 8; ++k) out[k] = fwd_sample(ld, g, c, cy, x0 + k) - 128;
}

ST_JPEG_HD int32_t fdescale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }

// One 1-D pass of jpeg_fdct_islow over 8 values: a row of level-shifted samples (pass2 = false: results scaled up by
// 2^PASS1_BITS) or a column of the row pass's results (pass2 = true: that scaling and the constants' removed).
ST_JPEG_HD void fdct_1d(const int32_t in[8], int32_t out[8], bool pass2) {
  const int32_t F298 = 2446, F390 = 3196, F541 = 4433, F765 = 6270, F899 = 7373, F1175 = 9633, F1501 = 12299,
                F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
  const int sh = pass2 ? CONST_BITS + PASS1_BITS : CONST_BITS - PASS1_BITS;
  int32_t tmp0 = in[0] + in[7], tmp7 = in[0] - in[7], tmp1 = in[1] + in[6], tmp6 = in[1] - in[6];
  int32_t tmp2 = in[2] + in[5], tmp5 = in[2] - in[5], tmp3 = in[3] + in[4], tmp4 = in[3] - in[4];
  const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  if (pass2) {
    out[0] = fdescale(tmp10 + tmp11, PASS1_BITS);
    out[4] = fdescale(tmp10 - tmp11, PASS1_BITS);
  } else {
    out[0] = (tmp10 + tmp11) * (1 << PASS1_BITS);
    out[4] = (tmp10 - tmp11) * (1 << PASS1_BITS);
  }
  int32_t z1 = (tmp12 + tmp13) * F541;
  out[2] = fdescale(z1 + tmp13 * F765, sh);
  out[6] = fdescale(z1 - tmp12 * F1847, sh);
  z1 = tmp4 + tmp7;
  int32_t z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int32_t z5 = (z3 + z4) * F1175;
  tmp4 *= F298;
  tmp5 *= F2053;
  tmp6 *= F3072;
  tmp7 *= F1501;
  z1 *= -F899;
  z2 *= -F2562;
  z3 *= -F1961;
  z4 *= -F390;
  z3 += z5;
  z4 += z5;
  out[7] = fdescale(tmp4 + z1 + z3, sh);
  out[5] = fdescale(tmp5 + z2 + z4, sh);
  out[3] = fdescale(tmp6 + z2 + z3, sh);
  out[1] = fdescale(tmp7 + z1 + z4, sh);
}

// DCT output (8 x the true coefficient) -> quantised coefficient.  A table entry of 0 counts as 1 on both sides.
ST_JPEG_HD int16_t fwd_quantise(int32_t c, uint16_t q) {
  const int32_t qv = 8 * (q ? (int32_t)q : 1);
  const int32_t a = c < 0 ? -c : c;
  const int32_t v = (a + (qv >> 1)) / qv;
  return (int16_t)(c < 0 ? -v : v);
}

// Is block (by, bx) of component c a dummy block?  (sy, sx): the block whose DC it carries - the last real block in
// front of it in the MCU's block order (row-major within the MCU); the MCU's first block is always real.
ST_JPEG_HD bool fwd_dummy_source(const FwdGeom& g, int c, int by, int bx, int& sy, int& sx) {
  sy = by;
  sx = bx;
  if (bx < g.wib[c] && by < g.hib[c]) return false;
  const int fh = (c == 0 && g.hs) ? 2 : 1, fv = (c == 0 && g.vs) ? 2 : 1;
  const int my = by - by % fv, mx = bx - bx % fh;
  for (int k = (by - my) * fh + (bx - mx) - 1; k >= 0; --k) {
    sy = my + k / fh;
    sx = mx + k % fh;
    if (sx < g.wib[c] && sy < g.hib[c]) break;
  }
  return true;
}

// The whole of one real block: the host's text; the kernel runs the same pieces with a block's rows spread over threads.
template <typename Load>
ST_JPEG_HD void fwd_block(Load ld, const FwdGeom& g, int c, int by, int bx, const uint16_t* quant, int16_t out[64]) {
  int32_t t[64];
  for (int r = 0; r < 8; ++r) {
    int32_t row[8];
    fwd_row(ld, g, c, by * 8 + r, bx * 8, row);
    fdct_1d(row, t + r * 8, false);
  }
  for (int k = 0; k < 8; ++k) {
    int32_t col[8], res[8];
    for (int r = 0; r < 8; ++r) col[r] = t[r * 8 + k];
    fdct_1d(col, res, true);
    for (int r = 0; r < 8; ++r) out[r * 8 + k] = fwd_quantise(res[r], quant[r * 8 + k]);
  }
}

}  // namespace jpeg
}  // namespace st
