// The JPEG reconstruction core: the ONE copy of the arithmetic that the host routine (jpeg_io.cpp,
// st_jpeg_reconstruct_host) and the kernels (jpeg_decode.hip, st_jpeg_reconstruct) must agree on to the byte - the 1-D
// pass of the inverse DCT, the IDCT's output sample, the chroma upsampling expressions and the colour conversion.  It
// restates libjpeg-turbo's default decode path [upstream-memory; pinned by tests/golden/jpeg]:
//   jidctint.c  jpeg_idct_islow     CONST_BITS 13, PASS1_BITS 2, twelve FIX_* constants, columns then rows, DESCALE
//   jdsample.c  h2v1_fancy_upsample / h2v2_fancy_upsample ("fancy", triangle filter; not merged upsampling)
//   jdcolor.c   ycc_rgb_convert     16-bit fixed point, ONE_HALF folded into the tables
// Integer only.  Every sum and product is taken modulo 2^32 (unsigned arithmetic, read back as two's complement), so
// coefficients no encoder emits have a defined result too - the same one on both sides - and the final sample is
// CLAMPED to [0, 255]: libjpeg's range-limit table wraps there, which is not reproduced.
// Also a plain C++ header (tests/native/jpeg_check.cpp builds it on the CPU under sanitizers, without HIP).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define ST_JPEG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ST_JPEG_HD inline
#endif

namespace st {
namespace jpeg {

constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int PASS1_SHIFT = CONST_BITS - PASS1_BITS;        // DESCALE of the column pass
constexpr int PASS2_SHIFT = CONST_BITS + PASS1_BITS + 3;    // DESCALE of the row pass
constexpr uint32_t FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270,
                   FIX_0_899976223 = 7373, FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137,
                   FIX_1_961570560 = 16069, FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

// arithmetic shift of the two's-complement reading of x, after adding the rounding half: libjpeg's DESCALE
ST_JPEG_HD int32_t descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }

// One 1-D pass of jpeg_idct_islow over 8 values (a column of dequantised coefficients with shift = PASS1_SHIFT, a row
// of the work array with shift = PASS2_SHIFT).  libjpeg's shortcuts for all-zero AC terms give the same numbers.
ST_JPEG_HD void idct_1d(const int32_t in[8], int32_t out[8], int shift) {
  const uint32_t i0 = (uint32_t)in[0], i1 = (uint32_t)in[1], i2 = (uint32_t)in[2], i3 = (uint32_t)in[3],
                 i4 = (uint32_t)in[4], i5 = (uint32_t)in[5], i6 = (uint32_t)in[6], i7 = (uint32_t)in[7];
  // even part
  uint32_t z1 = (i2 + i6) * FIX_0_541196100;
  uint32_t tmp2 = z1 - i6 * FIX_1_847759065;
  uint32_t tmp3 = z1 + i2 * FIX_0_765366865;
  uint32_t tmp0 = (i0 + i4) << CONST_BITS;
  uint32_t tmp1 = (i0 - i4) << CONST_BITS;
  const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  // odd part
  tmp0 = i7; tmp1 = i5; tmp2 = i3; tmp3 = i1;
  z1 = tmp0 + tmp3;
  uint32_t z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
  const uint32_t z5 = (z3 + z4) * FIX_1_175875602;
  tmp0 *= FIX_0_298631336;
  tmp1 *= FIX_2_053119869;
  tmp2 *= FIX_3_072711026;
  tmp3 *= FIX_1_501321110;
  z1 = 0u - z1 * FIX_0_899976223;
  z2 = 0u - z2 * FIX_2_562915447;
  z3 = 0u - z3 * FIX_1_961570560;
  z4 = 0u - z4 * FIX_0_390180644;
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  out[0] = descale(tmp10 + tmp3, shift);
  out[7] = descale(tmp10 - tmp3, shift);
  out[1] = descale(tmp11 + tmp2, shift);
  out[6] = descale(tmp11 - tmp2, shift);
  out[2] = descale(tmp12 + tmp1, shift);
  out[5] = descale(tmp12 - tmp1, shift);
  out[3] = descale(tmp13 + tmp0, shift);
  out[4] = descale(tmp13 - tmp0, shift);
}

// dequantisation: coefficient * table entry in int32 (|product| < 2^31 for every int16 x uint16)
ST_JPEG_HD int32_t dequant(int16_t c, uint16_t q) { return (int32_t)c * (int32_t)q; }

ST_JPEG_HD int clamp255(int32_t v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// a row-pass result -> the sample: + CENTERJSAMPLE, range limit (a plain clamp)
ST_JPEG_HD uint8_t idct_sample(int32_t v) { return (uint8_t)clamp255((int32_t)((uint32_t)v + 128u)); }

// h2v1_fancy_upsample: output 2i from sample i and its left neighbour, output 2i+1 from sample i and its right one.
// The first and the last column of libjpeg's loop are these with the neighbour index clamped into the row.
ST_JPEG_HD int up_h2v1_even(int c, int left) { return (3 * c + left + 1) >> 2; }
ST_JPEG_HD int up_h2v1_odd(int c, int right) { return (3 * c + right + 2) >> 2; }

// h2v2_fancy_upsample: the column sum of the nearer and the farther chroma row, then the horizontal step.  Rows and
// columns beyond the component's true size are the edge sample (jdmainct's replicated context rows).
ST_JPEG_HD int up_h2v2_colsum(int near, int far) { return 3 * near + far; }
ST_JPEG_HD int up_h2v2_even(int sum, int left_sum) { return (3 * sum + left_sum + 8) >> 4; }
ST_JPEG_HD int up_h2v2_odd(int sum, int right_sum) { return (3 * sum + right_sum + 7) >> 4; }

// libjpeg takes the fancy upsamplers only for components wider than two samples; narrower ones are replicated
ST_JPEG_HD bool fancy_width(int comp_w) { return comp_w > 2; }

// ycc_rgb_convert: SCALEBITS 16, FIX(x) = (int)(x * 65536 + 0.5)
constexpr int32_t FIX_1_40200 = 91881, FIX_1_77200 = 116130, FIX_0_71414 = 46802, FIX_0_34414 = 22554,
                  ONE_HALF = 1 << 15;
ST_JPEG_HD void ycc_to_rgb(int y, int cb, int cr, uint8_t& r, uint8_t& g, uint8_t& b) {
  cb -= 128;
  cr -= 128;
  r = (uint8_t)clamp255(y + ((FIX_1_40200 * cr + ONE_HALF) >> 16));
  g = (uint8_t)clamp255(y + ((-FIX_0_34414 * cb + ONE_HALF - FIX_0_71414 * cr) >> 16));
  b = (uint8_t)clamp255(y + ((FIX_1_77200 * cb + ONE_HALF) >> 16));
}

// The chroma samples (cb or cr - called once for each) of the 4 luma positions x0 .. x0 + 3 (x0 % 4 == 0) of row y,
// from a component plane of true size cw x ch read through ld(column, row).  hs / vs: 1 when the component is
// subsampled in that direction.  The 4 positions interpolate between the component's columns a - 1 .. a + 2 (a = x0 / 2),
// clamped into the plane: 4 loads per chroma row, not 8.  Positions at or beyond the image width get defined values
// from clamped columns; the callers do not store them.
template <typename Load>
ST_JPEG_HD void chroma_quad(Load ld, int x0, int y, int cw, int ch, int hs, int vs, int out[4]) {
  if (!hs) {                                         // 4:4:4
    for (int j = 0; j < 4; ++j) out[j] = ld(x0 + j < cw ? x0 + j : cw - 1, y);
    return;
  }
  const int a = x0 >> 1, cy = vs ? y >> 1 : y;
  if (!fancy_width(cw)) {                            // replicated
    for (int j = 0; j < 4; ++j) out[j] = ld(a + (j >> 1) < cw ? a + (j >> 1) : cw - 1, cy);
    return;
  }
  int col[4], v[4];
  for (int k = 0; k < 4; ++k) {
    const int c = a - 1 + k;
    col[k] = c < 0 ? 0 : (c < cw ? c : cw - 1);
  }
  if (!vs) {
    for (int k = 0; k < 4; ++k) v[k] = ld(col[k], y);
    out[0] = up_h2v1_even(v[1], v[0]);
    out[1] = up_h2v1_odd(v[1], v[2]);
    out[2] = up_h2v1_even(v[2], v[1]);
    out[3] = up_h2v1_odd(v[2], v[3]);
    return;
  }
  const int fy = (y & 1) ? (cy + 1 < ch ? cy + 1 : ch - 1) : (cy > 0 ? cy - 1 : 0);
  for (int k = 0; k < 4; ++k) v[k] = up_h2v2_colsum(ld(col[k], cy), ld(col[k], fy));
  out[0] = up_h2v2_even(v[1], v[0]);
  out[1] = up_h2v2_odd(v[1], v[2]);
  out[2] = up_h2v2_even(v[2], v[1]);
  out[3] = up_h2v2_odd(v[2], v[3]);
}

}  // namespace jpeg
}  // namespace st
