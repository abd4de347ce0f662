// Host routines of the JPEG writer (include/stereotrack_vis.h): geometry and tables, the forward
// path in plain C++ (the CPU product path and the executable specification of jpeg_forward.hip) and the Huffman entropy
// encode with the file layout - a serial bit loop, host work like the reader's entropy decode.  No GPU call, no global
// state, no allocation: Python runs the entropy encode on several threads out of page-locked staging memory.
//
// The file is what libjpeg-turbo's jpeg_write_* calls emit with jpeg_set_defaults + jpeg_set_quality (force_baseline)
// [upstream-memory; pinned against Pillow's files by tests/golden/jpeg_write]: jcmarker.c write_file_header /
// write_frame_header / write_scan_header for the segment order, jchuff.c encode_one_block / emit_restart for the scan,
// jcparam.c for the tables.  ITU-T T.81 is the format: B.2 segments, F.1.2 Huffman encoding, Annex K tables.
#include <cstdint>
#include <cstring>

#include "../../include/stereotrack_vis.h"
#include "jpeg_fwd_core.h"
#include "st_common.h"

namespace st {
void jpeg_fill_geometry(StJpegInfo& I);             // jpeg_io.cpp
bool jpeg_geometry_ok(const StJpegInfo& I);

bool jpeg_fwd_geom(const StJpegInfo& I, jpeg::FwdGeom& g) {
  if (!jpeg_geometry_ok(I)) return false;
  g.ncomp = I.components;
  g.hs = I.sampling >= ST_JPEG_422;
  g.vs = I.sampling == ST_JPEG_420;
  g.width = I.width;
  g.height = I.height;
  long long blocks = 0;
  for (int c = 0; c < 3; ++c) {
    const bool have = c < I.components;
    g.first_block[c] = blocks;
    g.bw[c] = have ? I.blocks_w[c] : 0;
    g.bh[c] = have ? I.blocks_h[c] : 0;
    g.wib[c] = have ? (I.comp_w[c] + 7) / 8 : 0;
    g.hib[c] = have ? (I.comp_h[c] + 7) / 8 : 0;
    g.ch[c] = have ? I.comp_h[c] : 0;
    if (have) blocks += (long long)I.blocks_w[c] * I.blocks_h[c];
  }
  g.blocks_per_image = blocks;
  return true;
}
}  // namespace st

namespace {

namespace J = st::jpeg;

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// ITU-T T.81 Annex K.1, natural order
const uint8_t kLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                           14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                           18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                           49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                             99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                             99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K.3: code counts per length 1 .. 16, then the symbols in code order
const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

struct Codes {            // on the caller's stack: 2 KiB for the four tables
  uint16_t code[256];
  uint8_t len[256];
};

void build_codes(Codes& t, const uint8_t* bits, const uint8_t* vals) {     // Annex C
  std::memset(&t, 0, sizeof(t));
  unsigned code = 0;
  int k = 0;
  for (int length = 1; length <= 16; ++length) {
    for (int i = 0; i < bits[length - 1]; ++i) {
      t.code[vals[k]] = (uint16_t)code++;
      t.len[vals[k]] = (uint8_t)length;
      ++k;
    }
    code <<= 1;
  }
}

struct BitWriter {        // the capacity was checked against st_jpeg_encode_bound before the first byte
  uint8_t* p;
  uint64_t acc = 0;
  int n = 0;
  void put(unsigned v, int bits) {
    acc = (acc << bits) | (v & ((1u << bits) - 1u));
    n += bits;
    while (n >= 8) {
      const uint8_t b = (uint8_t)(acc >> (n - 8));
      *p++ = b;
      if (b == 0xFF) *p++ = 0;
      n -= 8;
    }
  }
  void flush() {          // pad with 1-bits to the byte
    if (n) put(0x7F, 8 - n);
    acc = 0;
    n = 0;
  }
};

int bit_size(int v) {
  int s = 0;
  while (v) {
    ++s;
    v >>= 1;
  }
  return s;
}

bool encode_block(BitWriter& w, const int16_t* blk, int& pred, const Codes& dc, const Codes& ac) {
  int diff = blk[0] - pred;
  pred = blk[0];
  int mag = diff < 0 ? -diff : diff, bits = diff < 0 ? diff - 1 : diff;
  int s = bit_size(mag);
  if (s > 11) return false;
  w.put(dc.code[s], dc.len[s]);
  if (s) w.put((unsigned)bits, s);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = blk[kZigzag[k]];
    if (v == 0) {
      ++run;
      continue;
    }
    while (run > 15) {
      w.put(ac.code[0xF0], ac.len[0xF0]);
      run -= 16;
    }
    mag = v < 0 ? -v : v;
    bits = v < 0 ? v - 1 : v;
    s = bit_size(mag);
    if (s > 10) return false;
    const int sym = (run << 4) | s;
    w.put(ac.code[sym], ac.len[sym]);
    w.put((unsigned)bits, s);
    run = 0;
  }
  if (run) w.put(ac.code[0], ac.len[0]);
  return true;
}

uint8_t* put_segment(uint8_t* p, int marker, const uint8_t* payload, int n) {
  *p++ = 0xFF;
  *p++ = (uint8_t)marker;
  *p++ = (uint8_t)((n + 2) >> 8);
  *p++ = (uint8_t)((n + 2) & 255);
  std::memcpy(p, payload, (size_t)n);
  return p + n;
}

uint8_t* put_dht(uint8_t* p, int tc_th, const uint8_t* bits, const uint8_t* vals, int nvals) {
  uint8_t buf[1 + 16 + 162];
  buf[0] = (uint8_t)tc_th;
  std::memcpy(buf + 1, bits, 16);
  std::memcpy(buf + 17, vals, (size_t)nvals);
  return put_segment(p, 0xC4, buf, 17 + nvals);
}

int check_info(const StJpegInfo* info, J::FwdGeom& g, const char* who) {
  ST_REQUIRE(info, "%s: null pointer", who);
  ST_REQUIRE(info->struct_size == (int)sizeof(StJpegInfo), "%s: StJpegInfo.struct_size %d, this library has %d", who,
             info->struct_size, (int)sizeof(StJpegInfo));
  ST_REQUIRE(st::jpeg_fwd_geom(*info, g), "%s: StJpegInfo is not what st_jpeg_encode_geometry returns for its width / height / sampling",
             who);
  ST_REQUIRE(info->restart_interval >= 0 && info->restart_interval <= 65535, "%s: restart_interval must be 0..65535, got %d", who,
             info->restart_interval);
  return ST_OK;
}

}  // namespace

extern "C" int st_jpeg_encode_geometry(int height, int width, int components, int sampling, int restart_interval,
                                       StJpegInfo* info) {
  ST_REQUIRE(info, "st_jpeg_encode_geometry: null pointer");
  ST_REQUIRE(info->struct_size == (int)sizeof(StJpegInfo), "st_jpeg_encode_geometry: StJpegInfo.struct_size %d, this library has %d",
             info->struct_size, (int)sizeof(StJpegInfo));
  ST_REQUIRE(height >= 1 && height <= 65535 && width >= 1 && width <= 65535,
             "st_jpeg_encode_geometry: JPEG sizes are 1..65535, got %d x %d", height, width);
  ST_REQUIRE((components == 1 && sampling == ST_JPEG_GRAY) ||
                 (components == 3 && sampling >= ST_JPEG_444 && sampling <= ST_JPEG_420),
             "st_jpeg_encode_geometry: unknown sampling %d for %d component(s)", sampling, components);
  ST_REQUIRE(restart_interval >= 0 && restart_interval <= 65535, "st_jpeg_encode_geometry: restart_interval must be 0..65535, got %d",
             restart_interval);
  StJpegInfo I;
  std::memset(&I, 0, sizeof(I));
  I.struct_size = (int)sizeof(StJpegInfo);
  I.height = height;
  I.width = width;
  I.components = components;
  I.sampling = sampling;
  I.restart_interval = restart_interval;
  st::jpeg_fill_geometry(I);
  *info = I;
  return ST_OK;
}

extern "C" int st_jpeg_quant_tables(int quality, uint16_t* quant_out) {
  ST_REQUIRE(quant_out, "st_jpeg_quant_tables: null pointer");
  const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
  const int scale = q < 50 ? 5000 / q : 200 - 2 * q;          // jpeg_quality_scaling
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < 64; ++k) {
      int v = ((c ? kChroma[k] : kLuma[k]) * scale + 50) / 100;
      quant_out[c * 64 + k] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
  return ST_OK;
}

extern "C" int st_jpeg_forward_host(const uint8_t* pixels, ptrdiff_t plane_stride, ptrdiff_t row_stride,
                                    ptrdiff_t pixel_stride, int rgb_order, const uint16_t* quant, const StJpegInfo* info,
                                    int16_t* coef_out) {
  ST_REQUIRE(pixels && quant && coef_out, "st_jpeg_forward_host: null pointer");
  J::FwdGeom g;
  ST_CHECK(check_info(info, g, "st_jpeg_forward_host"));
  auto ld = [=](int p, int y, int x) {
    const int plane = rgb_order ? p : 2 - p;                  // ld's planes are R, G, B
    return (int)pixels[(g.ncomp == 1 ? 0 : plane) * plane_stride + y * row_stride + x * pixel_stride];
  };
  for (int c = 0; c < g.ncomp; ++c) {
    int16_t* base = coef_out + info->coef_offset[c];
    const uint16_t* q = quant + c * 64;
    for (int by = 0; by < g.bh[c]; ++by)                      // real blocks first: a dummy block copies a DC
      for (int bx = 0; bx < g.bw[c]; ++bx)
        if (bx < g.wib[c] && by < g.hib[c]) J::fwd_block(ld, g, c, by, bx, q, base + ((size_t)by * g.bw[c] + bx) * 64);
    for (int by = 0; by < g.bh[c]; ++by)
      for (int bx = 0; bx < g.bw[c]; ++bx) {
        int sy, sx;
        if (!J::fwd_dummy_source(g, c, by, bx, sy, sx)) continue;
        int16_t* blk = base + ((size_t)by * g.bw[c] + bx) * 64;
        std::memset(blk, 0, 64 * sizeof(int16_t));
        blk[0] = base[((size_t)sy * g.bw[c] + sx) * 64];
      }
  }
  return ST_OK;
}

extern "C" size_t st_jpeg_encode_bound(const StJpegInfo* info) {
  J::FwdGeom g;
  if (!info || info->struct_size != (int)sizeof(StJpegInfo) || !st::jpeg_fwd_geom(*info, g)) return 0;
  return (size_t)1024 + (size_t)416 * (size_t)g.blocks_per_image + (size_t)4 * info->mcus_x * info->mcus_y;
}

extern "C" int st_jpeg_entropy_encode(const int16_t* coef, const uint16_t* quant, const StJpegInfo* info, uint8_t* out,
                                      size_t capacity, size_t* out_bytes) {
  ST_REQUIRE(coef && quant && out && out_bytes, "st_jpeg_entropy_encode: null pointer");
  J::FwdGeom g;
  ST_CHECK(check_info(info, g, "st_jpeg_entropy_encode"));
  const size_t bound = st_jpeg_encode_bound(info);
  if (capacity < bound)
    return st::set_error(ST_ERR_WORKSPACE, "st_jpeg_entropy_encode: capacity of %zu bytes, %zu needed (st_jpeg_encode_bound)",
                         capacity, bound);
  const int nc = g.ncomp, ntab = nc == 1 ? 1 : 2;
  for (int c = 0; c < nc; ++c)
    for (int k = 0; k < 64; ++k)
      ST_REQUIRE(quant[c * 64 + k] >= 1 && quant[c * 64 + k] <= 255,
                 "st_jpeg_entropy_encode: quantisation table entry %d of component %d is %d, baseline takes 1..255", k, c,
                 (int)quant[c * 64 + k]);
  if (nc == 3)
    ST_REQUIRE(std::memcmp(quant + 64, quant + 128, 128) == 0, "st_jpeg_entropy_encode: Cb and Cr share one table in the file; theirs differ");
  uint8_t* p = out;
  *p++ = 0xFF;
  *p++ = 0xD8;
  static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  p = put_segment(p, 0xE0, jfif, 14);
  for (int t = 0; t < ntab; ++t) {
    uint8_t buf[65];
    buf[0] = (uint8_t)t;
    for (int k = 0; k < 64; ++k) buf[1 + k] = (uint8_t)quant[t * 64 + kZigzag[k]];
    p = put_segment(p, 0xDB, buf, 65);
  }
  const int fh = g.hs ? 2 : 1, fv = g.vs ? 2 : 1;
  {
    uint8_t buf[6 + 9];
    buf[0] = 8;
    buf[1] = (uint8_t)(g.height >> 8);
    buf[2] = (uint8_t)(g.height & 255);
    buf[3] = (uint8_t)(g.width >> 8);
    buf[4] = (uint8_t)(g.width & 255);
    buf[5] = (uint8_t)nc;
    for (int c = 0; c < nc; ++c) {
      buf[6 + 3 * c] = (uint8_t)(c + 1);
      buf[7 + 3 * c] = (uint8_t)(c == 0 ? (fh << 4 | fv) : 0x11);
      buf[8 + 3 * c] = (uint8_t)(c ? 1 : 0);
    }
    p = put_segment(p, 0xC0, buf, 6 + 3 * nc);
  }
  p = put_dht(p, 0x00, kDcLumaBits, kDcVals, 12);
  p = put_dht(p, 0x10, kAcLumaBits, kAcLumaVals, 162);
  if (ntab == 2) {
    p = put_dht(p, 0x01, kDcChromaBits, kDcVals, 12);
    p = put_dht(p, 0x11, kAcChromaBits, kAcChromaVals, 162);
  }
  const int ri = info->restart_interval;
  if (ri) {
    const uint8_t buf[2] = {(uint8_t)(ri >> 8), (uint8_t)(ri & 255)};
    p = put_segment(p, 0xDD, buf, 2);
  }
  {
    uint8_t buf[1 + 6 + 3];
    buf[0] = (uint8_t)nc;
    for (int c = 0; c < nc; ++c) {
      buf[1 + 2 * c] = (uint8_t)(c + 1);
      buf[2 + 2 * c] = (uint8_t)(c ? 0x11 : 0x00);
    }
    buf[1 + 2 * nc] = 0;
    buf[2 + 2 * nc] = 63;
    buf[3 + 2 * nc] = 0;
    p = put_segment(p, 0xDA, buf, 4 + 2 * nc);
  }
  Codes dc[2], ac[2];
  build_codes(dc[0], kDcLumaBits, kDcVals);
  build_codes(ac[0], kAcLumaBits, kAcLumaVals);
  build_codes(dc[1], kDcChromaBits, kDcVals);
  build_codes(ac[1], kAcChromaBits, kAcChromaVals);
  BitWriter w;
  w.p = p;
  int pred[3] = {0, 0, 0};
  int left = ri, rst = 0;
  for (int my = 0; my < info->mcus_y; ++my)
    for (int mx = 0; mx < info->mcus_x; ++mx) {
      if (ri && left == 0) {
        w.flush();
        *w.p++ = 0xFF;
        *w.p++ = (uint8_t)(0xD0 + rst);
        rst = (rst + 1) & 7;
        pred[0] = pred[1] = pred[2] = 0;
        left = ri;
      }
      --left;
      for (int c = 0; c < nc; ++c) {
        const int ch = c == 0 ? fh : 1, cv = c == 0 ? fv : 1, t = c ? 1 : 0;
        for (int ly = 0; ly < cv; ++ly)
          for (int lx = 0; lx < ch; ++lx) {
            const size_t b = (size_t)(my * cv + ly) * g.bw[c] + (size_t)(mx * ch + lx);
            if (!encode_block(w, coef + info->coef_offset[c] + b * 64, pred[c], dc[t], ac[t]))
              return st::set_error(ST_ERR_INVALID, "st_jpeg_entropy_encode: a coefficient of component %d, block %zu is outside the "
                                   "baseline range (DC difference of 11 bits, AC of 10)", c, b);
          }
      }
    }
  w.flush();
  p = w.p;
  *p++ = 0xFF;
  *p++ = 0xD9;
  *out_bytes = (size_t)(p - out);
  return ST_OK;
}
