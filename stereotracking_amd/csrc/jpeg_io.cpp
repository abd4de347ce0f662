// Host routines of the JPEG reader (include/stereotrack_jpeg.h): the marker parse, the Huffman
// entropy decode - a serial bit loop, host work like st_png_unfilter - and the reconstruction in plain C++ (the CPU
// product path of the dataset readers and the executable specification of jpeg_decode.hip).  No GPU call, no global
// state, no allocation in the entropy decode: Python runs it on several threads into page-locked staging memory.
//
// The reference decodes every image with OpenCV behind mmcv.imfrombytes (cv2 / mmcv are absent here); OpenCV's JPEG
// reader is libjpeg-turbo with its defaults, whose arithmetic jpeg_core.h restates [upstream-memory; pinned against
// Pillow's libjpeg-turbo by tests/golden/jpeg].  ITU-T T.81 is the format: B.2 segments, F.2.2 Huffman decoding,
// Annex C table generation, E.2.4 restart handling.
#include <cstdint>
#include <cstring>
#include <exception>
#include <vector>

#include "../../include/stereotrack_jpeg.h"
#include "jpeg_core.h"
#include "st_common.h"

namespace st {

// The ONE text of the geometry: MCU grid, block grids padded to whole MCUs, true component sizes, offsets and byte
// sizes, from width / height / components / sampling.  st_jpeg_info fills the struct with it; the reconstruction
// entries (host and device) index memory with these fields, so they refuse a struct that is not what this makes.
void jpeg_fill_geometry(StJpegInfo& I) {
  const int fh = I.sampling >= ST_JPEG_422 ? 2 : 1, fv = I.sampling == ST_JPEG_420 ? 2 : 1;
  I.mcus_x = (I.width + 8 * fh - 1) / (8 * fh);
  I.mcus_y = (I.height + 8 * fv - 1) / (8 * fv);
  size_t off = 0;
  for (int c = 0; c < 3; ++c) {
    I.blocks_w[c] = I.blocks_h[c] = I.comp_w[c] = I.comp_h[c] = 0;
    I.coef_offset[c] = 0;
    if (c >= I.components) continue;
    const int ch = c == 0 ? fh : 1, cv = c == 0 ? fv : 1;
    I.blocks_w[c] = I.mcus_x * ch;
    I.blocks_h[c] = I.mcus_y * cv;
    I.comp_w[c] = (I.width * ch + fh - 1) / fh;
    I.comp_h[c] = (I.height * cv + fv - 1) / fv;
    I.coef_offset[c] = off;
    off += (size_t)64 * I.blocks_w[c] * I.blocks_h[c];
  }
  I.coef_count = off;
  I.coef_bytes = off * sizeof(int16_t);
  I.work_bytes = (off + 15) / 16 * 16;       // one byte per sample of the padded component planes
}

bool jpeg_geometry_ok(const StJpegInfo& I) {
  if (I.width < 1 || I.width > 65535 || I.height < 1 || I.height > 65535) return false;
  if (!((I.components == 1 && I.sampling == ST_JPEG_GRAY) ||
        (I.components == 3 && I.sampling >= ST_JPEG_444 && I.sampling <= ST_JPEG_420)))
    return false;
  StJpegInfo want = I;
  jpeg_fill_geometry(want);
  bool same = I.mcus_x == want.mcus_x && I.mcus_y == want.mcus_y && I.coef_count == want.coef_count &&
              I.coef_bytes == want.coef_bytes && I.work_bytes == want.work_bytes;
  for (int c = 0; c < I.components; ++c)
    same = same && I.blocks_w[c] == want.blocks_w[c] && I.blocks_h[c] == want.blocks_h[c] && I.comp_w[c] == want.comp_w[c] &&
           I.comp_h[c] == want.comp_h[c] && I.coef_offset[c] == want.coef_offset[c];
  return same;
}

}  // namespace st

namespace {

using st::set_error;

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
  bool defined = false;
  uint8_t vals[256];
  int32_t maxcode[18];     // largest code of each length (left-aligned compare is not used: plain code values), -1 = none
  int32_t valptr[17], mincode[17];
  uint16_t fast[512];      // 9-bit prefix -> (length << 8) | symbol, 0 = longer than 9 bits
};

struct Header {
  StJpegInfo info;
  uint16_t quant[4][64];   // natural order
  bool quant_defined[4] = {false, false, false, false};
  Huff dc[4], ac[4];
  int tq[3], td[3], ta[3];
  size_t scan_pos = 0;     // first byte of the entropy-coded segment
};

int build_huff(Huff& h, const uint8_t* counts, const uint8_t* vals, int nvals, int is_dc) {
  int code = 0, k = 0;
  std::memset(h.fast, 0, sizeof(h.fast));
  for (int len = 1; len <= 16; ++len) {
    h.valptr[len] = k;
    h.mincode[len] = code;
    // the Kraft bound, BEFORE an entry of this length is written: more codes than fit would index past `fast`
    if (code + counts[len - 1] > (1 << len))
      return set_error(ST_ERR_INVALID, "JPEG: a DHT segment defines more codes of length %d than fit", len);
    for (int i = 0; i < counts[len - 1]; ++i, ++k, ++code) {
      if (len <= 9) {
        const int first = code << (9 - len);
        for (int j = 0; j < (1 << (9 - len)); ++j) h.fast[first + j] = (uint16_t)((len << 8) | vals[k]);
      }
    }
    h.maxcode[len] = counts[len - 1] ? code - 1 : -1;
    code <<= 1;
  }
  h.maxcode[17] = 0x7fffffff;
  for (int i = 0; i < nvals; ++i) {
    h.vals[i] = vals[i];
    if (is_dc && vals[i] > 11) return set_error(ST_ERR_INVALID, "JPEG: DC Huffman table holds category %d (8-bit data has 0..11)", vals[i]);
  }
  h.defined = true;
  return ST_OK;
}

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Segments up to and including the scan header: the geometry into H.info, the DQT / DHT contents into H.
int parse_header(const uint8_t* d, size_t n, Header& H) {
  StJpegInfo& I = H.info;
  const int struct_size = I.struct_size;
  std::memset(&I, 0, sizeof(I));
  I.struct_size = struct_size;
  if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return set_error(ST_ERR_INVALID, "not a JPEG file (no SOI marker)");
  size_t pos = 2;
  bool have_sof = false, jfif = false, adobe = false;
  int adobe_transform = -1, comp_id[3] = {0, 0, 0}, hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1};
  for (;;) {
    while (pos < n && d[pos] != 0xFF) ++pos;          // garbage between segments is skipped, as libjpeg does
    while (pos < n && d[pos] == 0xFF) ++pos;          // fill bytes
    if (pos >= n) return set_error(ST_ERR_INVALID, "JPEG: the file ends before the scan header");
    const int m = d[pos++];
    if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;        // stand-alone markers
    if (m == 0xD8) continue;
    if (m == 0xD9) return set_error(ST_ERR_INVALID, "JPEG: EOI before any scan");
    if (pos + 2 > n) return set_error(ST_ERR_INVALID, "JPEG: truncated segment header");
    const int len = be16(d + pos);
    if (len < 2 || pos + (size_t)len > n) return set_error(ST_ERR_INVALID, "JPEG: segment 0x%02X runs past the end of the file", m);
    const uint8_t* s = d + pos + 2;
    const int sl = len - 2;
    pos += len;
    switch (m) {
      case 0xC0: case 0xC1: {
        if (have_sof) return set_error(ST_ERR_INVALID, "JPEG: two frame headers");
        if (sl < 6) return set_error(ST_ERR_INVALID, "JPEG: short frame header");
        const int prec = s[0], nf = s[5];
        if (prec == 12) return set_error(ST_ERR_UNSUPPORTED, "12-bit JPEG is not supported");
        if (prec != 8) return set_error(ST_ERR_UNSUPPORTED, "%d-bit JPEG is not supported", prec);
        I.height = be16(s + 1);
        I.width = be16(s + 3);
        if (I.height == 0) return set_error(ST_ERR_UNSUPPORTED, "JPEG height given by a DNL marker is not supported");
        if (I.width == 0) return set_error(ST_ERR_INVALID, "JPEG: zero width");
        if (nf == 4) return set_error(ST_ERR_UNSUPPORTED, "4-component (CMYK / YCCK) JPEG is not supported");
        if (nf != 1 && nf != 3) return set_error(ST_ERR_UNSUPPORTED, "%d-component JPEG is not supported", nf);
        if (sl < 6 + 3 * nf) return set_error(ST_ERR_INVALID, "JPEG: short frame header");
        I.components = nf;
        for (int c = 0; c < nf; ++c) {
          comp_id[c] = s[6 + 3 * c];
          hs[c] = s[7 + 3 * c] >> 4;
          vs[c] = s[7 + 3 * c] & 15;
          H.tq[c] = s[8 + 3 * c];
          if (hs[c] < 1 || hs[c] > 4 || vs[c] < 1 || vs[c] > 4 || H.tq[c] > 3)
            return set_error(ST_ERR_INVALID, "JPEG: bad sampling factors or table number in the frame header");
        }
        have_sof = true;
        break;
      }
      case 0xC2: return set_error(ST_ERR_UNSUPPORTED, "progressive JPEG (SOF2) is not supported");
      case 0xC3: case 0xC7: case 0xCB: case 0xCF: return set_error(ST_ERR_UNSUPPORTED, "lossless JPEG (SOF%d) is not supported", m - 0xC0);
      case 0xC5: case 0xC6: return set_error(ST_ERR_UNSUPPORTED, "hierarchical (differential) JPEG (SOF%d) is not supported", m - 0xC0);
      case 0xC9: case 0xCA: case 0xCD: case 0xCE: case 0xCC:
        return set_error(ST_ERR_UNSUPPORTED, "arithmetic-coded JPEG is not supported");
      case 0xC8: return set_error(ST_ERR_INVALID, "JPEG: reserved marker 0xC8");
      case 0xC4: {                                                    // DHT, several tables per segment
        int o = 0;
        while (o < sl) {
          if (o + 17 > sl) return set_error(ST_ERR_INVALID, "JPEG: short DHT segment");
          const int tc = s[o] >> 4, th = s[o] & 15;
          if (tc > 1 || th > 3) return set_error(ST_ERR_INVALID, "JPEG: bad Huffman table class / number");
          int total = 0;
          for (int i = 0; i < 16; ++i) total += s[o + 1 + i];
          if (total > 256 || o + 17 + total > sl) return set_error(ST_ERR_INVALID, "JPEG: bad DHT symbol count");
          const int rc = build_huff(tc ? H.ac[th] : H.dc[th], s + o + 1, s + o + 17, total, tc == 0);
          if (rc != ST_OK) return rc;
          o += 17 + total;
        }
        break;
      }
      case 0xDB: {                                                    // DQT, 8- or 16-bit entries, several tables
        int o = 0;
        while (o < sl) {
          const int pq = s[o] >> 4, tq = s[o] & 15;
          if (pq > 1 || tq > 3) return set_error(ST_ERR_INVALID, "JPEG: bad quantisation table precision / number");
          if (o + 1 + 64 * (pq + 1) > sl) return set_error(ST_ERR_INVALID, "JPEG: short DQT segment");
          for (int k = 0; k < 64; ++k)
            H.quant[tq][kZigzag[k]] = pq ? (uint16_t)be16(s + o + 1 + 2 * k) : s[o + 1 + k];
          H.quant_defined[tq] = true;
          o += 1 + 64 * (pq + 1);
        }
        break;
      }
      case 0xDD:
        if (sl < 2) return set_error(ST_ERR_INVALID, "JPEG: short DRI segment");
        I.restart_interval = be16(s);
        break;
      case 0xE0:
        if (sl >= 5 && !std::memcmp(s, "JFIF", 5)) jfif = true;
        break;
      case 0xEE:
        if (sl >= 12 && !std::memcmp(s, "Adobe", 5)) {
          adobe = true;
          adobe_transform = s[11];
        }
        break;
      case 0xDA: {
        if (!have_sof) return set_error(ST_ERR_INVALID, "JPEG: scan header before the frame header");
        if (sl < 1) return set_error(ST_ERR_INVALID, "JPEG: short scan header");
        const int ns = s[0];
        if (ns != I.components)
          return set_error(ST_ERR_UNSUPPORTED, "multi-scan JPEG (a scan of %d of %d components) is not supported", ns, I.components);
        if (sl < 4 + 2 * ns) return set_error(ST_ERR_INVALID, "JPEG: short scan header");
        for (int c = 0; c < ns; ++c) {
          if (s[1 + 2 * c] != comp_id[c]) return set_error(ST_ERR_INVALID, "JPEG: scan components out of frame order");
          H.td[c] = s[2 + 2 * c] >> 4;
          H.ta[c] = s[2 + 2 * c] & 15;
          if (H.td[c] > 3 || H.ta[c] > 3) return set_error(ST_ERR_INVALID, "JPEG: bad Huffman table number in the scan header");
        }
        if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0)
          return set_error(ST_ERR_UNSUPPORTED, "progressive JPEG scan parameters are not supported");
        // colour space (jdapimin.c default_decompress_parms): 3 components are YCbCr unless Adobe says transform 0 or,
        // without JFIF / Adobe, the component ids spell RGB
        if (I.components == 3) {
          if (adobe && adobe_transform == 0) return set_error(ST_ERR_UNSUPPORTED, "Adobe APP14 transform 0 (RGB JPEG) is not supported");
          if (!jfif && !adobe && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')
            return set_error(ST_ERR_UNSUPPORTED, "RGB JPEG (component ids R, G, B) is not supported");
          if (hs[1] != 1 || vs[1] != 1 || hs[2] != 1 || vs[2] != 1 ||
              !((hs[0] == 1 && vs[0] == 1) || (hs[0] == 2 && vs[0] == 1) || (hs[0] == 2 && vs[0] == 2)))
            return set_error(ST_ERR_UNSUPPORTED, "JPEG sampling factors %dx%d,%dx%d,%dx%d are not supported (4:4:4, 4:2:2, 4:2:0 only)",
                             hs[0], vs[0], hs[1], vs[1], hs[2], vs[2]);
          I.sampling = hs[0] == 1 ? ST_JPEG_444 : (vs[0] == 1 ? ST_JPEG_422 : ST_JPEG_420);
        } else {
          I.sampling = ST_JPEG_GRAY;          // a one-component scan is not interleaved: its factors do not matter
          hs[0] = vs[0] = 1;
        }
        st::jpeg_fill_geometry(I);
        H.scan_pos = pos;
        return ST_OK;
      }
      default: break;                                                 // APPn, COM and everything else: skipped
    }
  }
}

// Bit reader over the entropy-coded segment: removes FF00 stuffing, stops at a marker.  Past the data it feeds zero
// bits and counts them; a decoder that consumes one of those has run off the data (`overrun`).
struct Bits {
  const uint8_t* d;
  size_t n, pos;
  uint64_t buf = 0;
  int bits = 0, pad = 0;
  bool at_marker = false, overrun = false;

  void fill() {
    while (bits <= 48) {
      uint32_t b = 0;
      if (!at_marker) {
        if (pos >= n) {
          at_marker = true;
        } else if (d[pos] != 0xFF) {
          b = d[pos++];
        } else if (pos + 1 >= n) {
          at_marker = true;
        } else if (d[pos + 1] == 0x00) {                    // stuffed FF
          b = 0xFF;
          pos += 2;
        } else if (d[pos + 1] == 0xFF) {                    // fill byte
          ++pos;
          continue;
        } else {
          at_marker = true;                                 // pos stays on the marker's FF
        }
      }
      if (at_marker) pad += 8;
      buf = (buf << 8) | b;
      bits += 8;
    }
  }
  inline uint32_t peek(int k) {            // k <= 16
    if (bits < k) fill();
    return (uint32_t)(buf >> (bits - k)) & ((1u << k) - 1);
  }
  inline void skip(int k) {
    bits -= k;
    if (bits < pad) overrun = true;
  }
  inline uint32_t get(int k) {
    if (k == 0) return 0;
    const uint32_t v = peek(k);
    skip(k);
    return v;
  }
};

inline int decode_symbol(Bits& br, const Huff& h) {
  const uint32_t look = br.peek(16);
  const uint16_t f = h.fast[look >> 7];
  if (f) {
    br.skip(f >> 8);
    return f & 255;
  }
  for (int len = 10; len <= 16; ++len) {
    const int32_t code = (int32_t)(look >> (16 - len));
    if (code <= h.maxcode[len]) {
      if (code < h.mincode[len]) return -1;
      br.skip(len);
      return h.vals[h.valptr[len] + code - h.mincode[len]];
    }
  }
  return -1;
}

inline int extend(uint32_t v, int s) { return s && v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

int decode_block(Bits& br, const Huff& dc, const Huff& ac, int& pred, int16_t* blk) {
  std::memset(blk, 0, 64 * sizeof(int16_t));
  int s = decode_symbol(br, dc);
  if (s < 0) return -1;
  pred += extend(br.get(s), s);
  if (pred < -32768 || pred > 32767) return -1;
  blk[0] = (int16_t)pred;
  for (int k = 1; k < 64;) {
    const int rs = decode_symbol(br, ac);
    if (rs < 0) return -1;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;                  // EOB
      k += 16;
      if (k > 64) return -1;
      continue;
    }
    k += r;
    if (k > 63) return -1;
    blk[kZigzag[k++]] = (int16_t)extend(br.get(s), s);
  }
  return br.overrun ? -1 : 0;
}

}  // namespace

extern "C" int st_jpeg_info(const uint8_t* data, size_t nbytes, StJpegInfo* info) {
  ST_REQUIRE(data && info, "st_jpeg_info: null argument");
  ST_REQUIRE(info->struct_size == (int)sizeof(StJpegInfo), "st_jpeg_info: StJpegInfo.struct_size %d, this library has %d",
             info->struct_size, (int)sizeof(StJpegInfo));
  Header H;
  H.info.struct_size = info->struct_size;
  const int rc = parse_header(data, nbytes, H);
  if (rc == ST_OK) *info = H.info;
  return rc;
}

extern "C" int st_jpeg_entropy_decode(const uint8_t* data, size_t nbytes, int16_t* coef_out, uint16_t* quant_out) {
  ST_REQUIRE(data && coef_out && quant_out, "st_jpeg_entropy_decode: null argument");
  Header H;
  H.info.struct_size = (int)sizeof(StJpegInfo);
  ST_CHECK(parse_header(data, nbytes, H));
  const StJpegInfo& I = H.info;
  std::memset(quant_out, 0, 3 * 64 * sizeof(uint16_t));
  for (int c = 0; c < I.components; ++c) {
    ST_REQUIRE(H.quant_defined[H.tq[c]], "JPEG: component %d uses quantisation table %d, which the file does not define", c, H.tq[c]);
    ST_REQUIRE(H.dc[H.td[c]].defined && H.ac[H.ta[c]].defined, "JPEG: component %d uses a Huffman table the file does not define", c);
    std::memcpy(quant_out + 64 * c, H.quant[H.tq[c]], 64 * sizeof(uint16_t));
  }
  Bits br{data, nbytes, H.scan_pos};
  const int bh = I.sampling >= ST_JPEG_422 ? 2 : 1, bv = I.sampling == ST_JPEG_420 ? 2 : 1;
  int pred[3] = {0, 0, 0};
  const long long total = (long long)I.mcus_x * I.mcus_y;
  long long done = 0;
  int next_rst = 0;
  for (int my = 0; my < I.mcus_y; ++my)
    for (int mx = 0; mx < I.mcus_x; ++mx, ++done) {
      if (I.restart_interval && done && done % I.restart_interval == 0) {
        // E.2.4: the interval ends on a byte boundary; what is left in the reader is padding bits only
        ST_REQUIRE(br.bits - br.pad < 8, "JPEG: entropy data left over before restart marker %lld", done / I.restart_interval);
        size_t p = br.pos;
        while (p + 1 < nbytes && data[p] == 0xFF && data[p + 1] == 0xFF) ++p;
        ST_REQUIRE(p + 1 < nbytes && data[p] == 0xFF && data[p + 1] == 0xD0 + next_rst,
                   "JPEG: restart marker RST%d not found after MCU %lld (corrupt or truncated data)", next_rst, done);
        next_rst = (next_rst + 1) & 7;
        br = Bits{data, nbytes, p + 2};
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < I.components; ++c) {
        const int nh = c == 0 ? bh : 1, nv = c == 0 ? bv : 1;
        for (int v = 0; v < nv; ++v)
          for (int h = 0; h < nh; ++h) {
            const size_t b = (size_t)(my * nv + v) * I.blocks_w[c] + (size_t)(mx * nh + h);
            if (decode_block(br, H.dc[H.td[c]], H.ac[H.ta[c]], pred[c], coef_out + I.coef_offset[c] + 64 * b) != 0)
              return set_error(ST_ERR_INVALID, "JPEG: corrupt or truncated entropy data in MCU %lld of %lld", done, total);
          }
      }
    }
  return ST_OK;
}

// The host half of the device entropy decode (jpeg_entropy.hip): the header parse and the table checks of
// st_jpeg_entropy_decode, written out as one fixed-size descriptor.  The entropy-coded bytes are not looked at.
extern "C" int st_jpeg_entropy_prepare(const uint8_t* data, size_t nbytes, StJpegEntropyDesc* desc) {
  ST_REQUIRE(data && desc, "st_jpeg_entropy_prepare: null argument");
  ST_REQUIRE(desc->struct_size == (int)sizeof(StJpegEntropyDesc),
             "st_jpeg_entropy_prepare: StJpegEntropyDesc.struct_size %d, this library has %d", desc->struct_size,
             (int)sizeof(StJpegEntropyDesc));
  Header H;
  H.info.struct_size = (int)sizeof(StJpegInfo);
  ST_CHECK(parse_header(data, nbytes, H));
  const StJpegInfo& I = H.info;
  ST_REQUIRE(nbytes < ((size_t)1 << 28), "st_jpeg_entropy_prepare: files of 256 MiB and more are not decoded on the device");
  StJpegEntropyDesc& D = *desc;
  std::memset(&D, 0, sizeof(D));
  D.struct_size = (int)sizeof(D);
  D.components = I.components;
  D.sampling = I.sampling;
  D.restart_interval = I.restart_interval;
  D.mcus_x = I.mcus_x;
  D.mcus_y = I.mcus_y;
  D.scan_offset = (unsigned)H.scan_pos;
  D.scan_bytes = (unsigned)(nbytes - H.scan_pos);
  auto fill = [](StJpegHuffLut& L, const Huff& h) {
    std::memcpy(L.fast, h.fast, sizeof(L.fast));
    std::memcpy(L.maxcode, h.maxcode, sizeof(L.maxcode));
    std::memcpy(L.valptr + 1, h.valptr + 1, 16 * sizeof(int32_t));
    std::memcpy(L.mincode + 1, h.mincode + 1, 16 * sizeof(int32_t));
    L.maxcode[0] = -1;
    std::memcpy(L.vals, h.vals, sizeof(L.vals));
  };
  for (int c = 0; c < I.components; ++c) {
    ST_REQUIRE(H.quant_defined[H.tq[c]], "JPEG: component %d uses quantisation table %d, which the file does not define", c, H.tq[c]);
    ST_REQUIRE(H.dc[H.td[c]].defined && H.ac[H.ta[c]].defined, "JPEG: component %d uses a Huffman table the file does not define", c);
    std::memcpy(D.quant[c], H.quant[H.tq[c]], 64 * sizeof(uint16_t));
    D.dc_slot[c] = D.ac_slot[c] = c;
    for (int e = c - 1; e >= 0; --e) {                  // components that name one table share its slot
      if (H.td[e] == H.td[c]) D.dc_slot[c] = D.dc_slot[e];
      if (H.ta[e] == H.ta[c]) D.ac_slot[c] = D.ac_slot[e];
    }
    if (D.dc_slot[c] == c) fill(D.dc[c], H.dc[H.td[c]]);
    if (D.ac_slot[c] == c) fill(D.ac[c], H.ac[H.ta[c]]);
  }
  return ST_OK;
}

extern "C" int st_jpeg_reconstruct_host(const int16_t* coef, const uint16_t* quant, const StJpegInfo* info, uint8_t* out,
                                        ptrdiff_t plane_stride, ptrdiff_t row_stride, ptrdiff_t pixel_stride, int rgb_order) {
  namespace J = st::jpeg;
  ST_REQUIRE(coef && quant && info && out, "st_jpeg_reconstruct_host: null argument");
  ST_REQUIRE(info->struct_size == (int)sizeof(StJpegInfo), "st_jpeg_reconstruct_host: StJpegInfo.struct_size mismatch");
  const StJpegInfo& I = *info;
  ST_REQUIRE(st::jpeg_geometry_ok(I),
             "st_jpeg_reconstruct_host: StJpegInfo is not what st_jpeg_info returns for its width / height / sampling");
  std::vector<uint8_t> planes[3];
  try {
    for (int c = 0; c < I.components; ++c) planes[c].resize((size_t)64 * I.blocks_w[c] * I.blocks_h[c]);
  } catch (const std::exception&) {          // nothing may leave an extern "C" function
    return set_error(ST_ERR_INVALID, "st_jpeg_reconstruct_host: out of memory");
  }
  for (int c = 0; c < I.components; ++c) {
    const int pitch = 8 * I.blocks_w[c];
    const uint16_t* q = quant + 64 * c;
    for (int by = 0; by < I.blocks_h[c]; ++by)
      for (int bx = 0; bx < I.blocks_w[c]; ++bx) {
        const int16_t* blk = coef + I.coef_offset[c] + 64 * ((size_t)by * I.blocks_w[c] + bx);
        int32_t ws[64], col[8], res[8];
        for (int x = 0; x < 8; ++x) {                 // pass 1: columns
          for (int k = 0; k < 8; ++k) col[k] = J::dequant(blk[8 * k + x], q[8 * k + x]);
          J::idct_1d(col, res, J::PASS1_SHIFT);
          for (int k = 0; k < 8; ++k) ws[8 * k + x] = res[k];
        }
        for (int y = 0; y < 8; ++y) {                 // pass 2: rows
          J::idct_1d(ws + 8 * y, res, J::PASS2_SHIFT);
          uint8_t* dst = planes[c].data() + (size_t)(8 * by + y) * pitch + 8 * bx;
          for (int x = 0; x < 8; ++x) dst[x] = J::idct_sample(res[x]);
        }
      }
  }
  const int hs = I.sampling >= ST_JPEG_422, vs = I.sampling == ST_JPEG_420;
  const int p_r = rgb_order ? 0 : 2, p_b = rgb_order ? 2 : 0;
  for (int y = 0; y < I.height; ++y)
    for (int x0 = 0; x0 < I.width; x0 += 4) {
      int cc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
      for (int c = 1; c < I.components; ++c) {
        const uint8_t* pl = planes[c].data();
        const int pitch = 8 * I.blocks_w[c];
        J::chroma_quad([pl, pitch](int cx, int cy) { return (int)pl[(size_t)cy * pitch + cx]; }, x0, y, I.comp_w[c],
                       I.comp_h[c], hs, vs, cc[c - 1]);
      }
      for (int j = 0; j < 4 && x0 + j < I.width; ++j) {
        const int x = x0 + j;
        const int Y = planes[0][(size_t)y * 8 * I.blocks_w[0] + x];
        uint8_t r, g, b;
        if (I.components == 1)
          r = g = b = (uint8_t)Y;
        else
          J::ycc_to_rgb(Y, cc[0][j], cc[1][j], r, g, b);
        uint8_t* o = out + y * row_stride + x * pixel_stride;
        o[p_r * plane_stride] = r;
        o[1 * plane_stride] = g;
        o[p_b * plane_stride] = b;
      }
    }
  return ST_OK;
}
