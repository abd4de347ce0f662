// Stand-alone host check of the JPEG writer's host routines (stereotracking_amd/csrc/jpeg_encode.cpp on
// jpeg_fwd_core.h), built as plain host code with -fsanitize=address,undefined and run by hand (no pytest wrapper, no GPU):
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__
//       -I<rocm>/include tests/native/jpeg_write_check.cpp stereotracking_amd/csrc/jpeg_encode.cpp
//       stereotracking_amd/csrc/jpeg_io.cpp stereotracking_amd/csrc/st_common.cpp -o jpeg_write_check
//   ./jpeg_write_check
//
// Every (h, w) in 1..18 x 1..18 plus (31, 33) and (48, 80), gray and the three samplings, qualities 1 / 30 / 85 / 100,
// with and without a restart per MCU row, both channel orders: seeded noise in a pixel buffer of EXACTLY h * w * planes
// bytes goes through st_jpeg_encode_geometry / st_jpeg_quant_tables / st_jpeg_forward_host / st_jpeg_entropy_encode
// with buffers of exactly coef_count elements and exactly st_jpeg_encode_bound bytes, and back through the reader
// (st_jpeg_info / st_jpeg_entropy_decode), which must return the same geometry, tables and coefficients.  Then the
// refusals: a capacity one byte short, a struct that is not the geometry, coefficients outside the baseline range.
// The sanitizers must have nothing to report.  Exit status 0 and a summary line on success.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/stereotrack_vis.h"

namespace {

uint32_t lcg_state = 20261021u;
uint32_t lcg() {
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return lcg_state >> 8;
}

int fail(const char* what, int h, int w, int s, int q) {
  std::fprintf(stderr, "jpeg_write_check: %s at %dx%d sampling %d quality %d: %s\n", what, h, w, s, q, st_last_error());
  return 1;
}

int run(int h, int w, int sampling, int quality, int rst_rows, int rgb_order, bool full) {
  const int nc = sampling == ST_JPEG_GRAY ? 1 : 3;
  StJpegInfo info;
  std::memset(&info, 0, sizeof(info));
  info.struct_size = (int)sizeof(info);
  if (st_jpeg_encode_geometry(h, w, nc, sampling, 0, &info) != ST_OK) return fail("geometry", h, w, sampling, quality);
  if (rst_rows && st_jpeg_encode_geometry(h, w, nc, sampling, rst_rows * info.mcus_x, &info) != ST_OK)
    return fail("geometry with restarts", h, w, sampling, quality);
  std::vector<uint8_t> px((size_t)h * w * nc);
  const int base = (int)(lcg() & 255), amp = full ? 127 : 40;
  for (auto& v : px) {
    int s = (full ? 128 : base) + (int)(lcg() % (2 * amp + 1)) - amp;
    v = (uint8_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
  }
  std::vector<uint16_t> quant(192), quant2(192);
  if (st_jpeg_quant_tables(quality, quant.data()) != ST_OK) return fail("tables", h, w, sampling, quality);
  std::vector<int16_t> coef(info.coef_count), coef2(info.coef_count);
  // planar here, so that the last byte read is the last byte of the buffer
  if (st_jpeg_forward_host(px.data(), (ptrdiff_t)h * w, w, 1, rgb_order, quant.data(), &info, coef.data()) != ST_OK)
    return fail("forward", h, w, sampling, quality);
  const size_t bound = st_jpeg_encode_bound(&info);
  std::vector<uint8_t> out(bound);
  size_t n = 0;
  if (st_jpeg_entropy_encode(coef.data(), quant.data(), &info, out.data(), out.size(), &n) != ST_OK || n > bound)
    return fail("entropy encode", h, w, sampling, quality);
  StJpegInfo back;
  std::memset(&back, 0, sizeof(back));
  back.struct_size = (int)sizeof(back);
  if (st_jpeg_info(out.data(), n, &back) != ST_OK || std::memcmp(&back, &info, sizeof(info)) != 0)
    return fail("the reader's geometry of the written file", h, w, sampling, quality);
  if (st_jpeg_entropy_decode(out.data(), n, coef2.data(), quant2.data()) != ST_OK || coef != coef2 ||
      std::memcmp(quant.data(), quant2.data(), (size_t)nc * 128) != 0)
    return fail("the reader's coefficients of the written file", h, w, sampling, quality);
  if (h == 17 && w == 13) {                                    // refusals, once per sampling / quality
    if (st_jpeg_entropy_encode(coef.data(), quant.data(), &info, out.data(), bound - 1, &n) != ST_ERR_WORKSPACE)
      return fail("a capacity one byte short was not refused", h, w, sampling, quality);
    StJpegInfo bad = info;
    bad.blocks_h[0] += 1;
    if (st_jpeg_forward_host(px.data(), (ptrdiff_t)h * w, w, 1, rgb_order, quant.data(), &bad, coef2.data()) != ST_ERR_INVALID ||
        st_jpeg_entropy_encode(coef.data(), quant.data(), &bad, out.data(), out.size(), &n) != ST_ERR_INVALID ||
        st_jpeg_encode_bound(&bad) != 0)
      return fail("a struct that is not the geometry was not refused", h, w, sampling, quality);
    coef2 = coef;
    coef2[coef2.size() - 1] = 1024;
    if (st_jpeg_entropy_encode(coef2.data(), quant.data(), &info, out.data(), out.size(), &n) != ST_ERR_INVALID)
      return fail("an AC coefficient of 11 bits was not refused", h, w, sampling, quality);
    std::fill(coef2.begin(), coef2.end(), (int16_t)-1023);      // the longest codes in every position: fits the bound
    for (size_t i = 0; i < coef2.size(); i += 2) coef2[i] = 1023;
    if (st_jpeg_entropy_encode(coef2.data(), quant.data(), &info, out.data(), out.size(), &n) != ST_OK || n > bound)
      return fail("worst-case coefficients", h, w, sampling, quality);
  }
  return 0;
}

}  // namespace

int main() {
  static const int qualities[4] = {1, 30, 85, 100};
  int cases = 0, k = 0;
  for (int h = 1; h <= 20; ++h)
    for (int w = 1; w <= 20; ++w) {
      int hh = h, ww = w;
      if (h > 18 || w > 18) {                                   // the two larger geometries stand in the sweep's last cells
        if (h == 19 && w == 19) { hh = 31; ww = 33; }
        else if (h == 20 && w == 20) { hh = 48; ww = 80; }
        else continue;
      }
      for (int s = ST_JPEG_GRAY; s <= ST_JPEG_420; ++s) {
        ++k;
        const int q = qualities[k & 3];
        if (run(hh, ww, s, q, (k >> 2) & 1, (k >> 3) & 1, q == 100)) return 1;
        ++cases;
      }
    }
  std::printf("jpeg_write_check: %d cases written, read back and equal; refusals as documented\n", cases);
  return 0;
}
