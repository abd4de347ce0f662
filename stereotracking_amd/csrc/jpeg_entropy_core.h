// The device entropy decoder's core (include/stereotrack_jpeg.h, DESIGN.md section 25 "Entropy decode on the device"):
// the ONE text of the byte reader, the symbol decode, the state step, the count scan's operator and the DC chain's
// addressing, compiled by the kernels (jpeg_entropy.hip) and, as plain C++ without HIP, by the CPU emulation of
// tests/native/jpeg_entropy_check.cpp.  The specification is st_jpeg_entropy_decode (jpeg_io.cpp); what is restated
// here is its reader's byte rules and its decode_block, cut so that any thread can run it from any bit position.
//
// Positions are RAW: (byte index in the scan) * 8 + bit.  A raw FF is never plain data: FF 00 is the data byte FF,
// FF FF makes the first FF a fill byte, FF xx is a marker - so one byte of look-behind tells what a byte is, and every
// decoder, synchronised or not, finds every marker.  The decoder state at a position is (block within the MCU, zigzag
// index); crossing a marker resets it to (0, 0) and continues two bytes behind the marker's FF.
//
// The host counts MCUs and looks for RSTn where it expects one; a decoder here is driven by the markers it meets and
// counts (markers crossed, blocks completed since the last one).  In the write pass those counts are true, so a thread
// knows which restart interval `kseg` and which block `jblk` of it it is decoding: blocks beyond the interval's MCUs
// (garbage a decoder reads from padding bits or behind the last MCU) are dropped without a verdict, as the host never
// looks at those bits; a marker met, or the data's end reached, before the interval's blocks are complete is the
// host's overrun; and the thread that completes an interval's last block checks what the host checks there: fewer
// than 8 bits left, then RST(kseg mod 8).
#pragma once
#include <cstdint>

#include "../../include/stereotrack_jpeg.h"

#ifdef __HIPCC__
#define ST_JE_HD __host__ __device__ inline
#else
#define ST_JE_HD inline
#endif

namespace st {
namespace jent {

#ifdef __HIP_DEVICE_COMPILE__
__constant__ static const uint8_t kZigzag[64] =
#else
static const uint8_t kZigzag[64] =
#endif
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr uint32_t MAX_SCAN_BYTES = 1u << 28;      // raw bit positions fit 31 bits

// What a decode needs of one image: the descriptor (tables; an LDS copy in the kernel) and the derived counts.
struct Ctx {
  const StJpegEntropyDesc* d;
  uint32_t n;                  // scan bytes
  int bpm, ny, nh, nv;         // blocks per MCU, luma blocks per MCU (nh x nv)
  int mcus_x;
  uint32_t ri_blocks;          // blocks of a full restart interval (0: no DRI)
  uint32_t ri;                 // MCUs of it
  uint32_t K;                  // number of intervals (1 without DRI)
  uint32_t last_blocks;        // blocks of interval K - 1
  int blocks_w[3];
  uint64_t coef_offset[3];
};

ST_JE_HD void make_ctx(Ctx& cx, const StJpegEntropyDesc* d, const int blocks_w[3], const uint64_t coef_offset[3]) {
  cx.d = d;
  cx.n = d->scan_bytes;
  cx.nh = d->sampling >= ST_JPEG_422 ? 2 : 1;
  cx.nv = d->sampling == ST_JPEG_420 ? 2 : 1;
  cx.ny = cx.nh * cx.nv;
  cx.bpm = d->components == 1 ? 1 : cx.ny + 2;
  cx.mcus_x = d->mcus_x;
  const uint32_t total = (uint32_t)d->mcus_x * (uint32_t)d->mcus_y;
  cx.ri = (uint32_t)d->restart_interval;
  cx.ri_blocks = cx.ri * (uint32_t)cx.bpm;
  cx.K = cx.ri ? (total + cx.ri - 1) / cx.ri : 1;
  cx.last_blocks = (total - (cx.K - 1) * cx.ri) * (uint32_t)cx.bpm;
  for (int c = 0; c < 3; ++c) {
    cx.blocks_w[c] = blocks_w[c];
    cx.coef_offset[c] = coef_offset[c];
  }
}

// blocks the host decodes from interval k (k < K)
ST_JE_HD uint32_t need_blocks(const Ctx& cx, uint32_t k) { return k + 1 < cx.K ? cx.ri_blocks : cx.last_blocks; }

ST_JE_HD int comp_of_block(const Ctx& cx, int blk) { return blk < cx.ny ? 0 : blk - cx.ny + 1; }

// first coefficient of block j of interval k in the component layout [component][block_row][block_col][64]
ST_JE_HD uint64_t block_base(const Ctx& cx, uint32_t k, uint32_t j) {
  const uint32_t mcu = k * cx.ri + j / (uint32_t)cx.bpm;
  const int sub = (int)(j % (uint32_t)cx.bpm);
  const uint32_t my = mcu / (uint32_t)cx.mcus_x, mx = mcu - my * (uint32_t)cx.mcus_x;
  const int c = comp_of_block(cx, sub);
  uint64_t row = my, col = mx;
  if (c == 0) {
    row = (uint64_t)my * cx.nv + sub / cx.nh;
    col = (uint64_t)mx * cx.nh + sub % cx.nh;
  }
  return cx.coef_offset[c] + 64 * (row * (uint64_t)cx.blocks_w[c] + col);
}

// ---- the byte reader -------------------------------------------------------------------------------------------------
// Up to 5 data bytes from raw position p on (fill bytes skipped, stuffing removed), left-aligned in `bits`; idx[k] is the
// raw index of data byte k, and for k >= nb the raw index of what ends the data: term 1 = a marker (its FF; `code` its
// second byte), term 2 = the end of the bytes (a lone FF as the last byte included), term 0 = more data.
struct Window {
  uint64_t bits;
  uint32_t idx[6];
  int nb, term, code;
};

template <class Load>
ST_JE_HD void gather(const Load& ld, uint32_t n, uint32_t p, Window& w) {
  w.bits = 0;
  w.nb = w.term = w.code = 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    uint32_t v = 0;
    if (!w.term) {
      for (;;) {                          // ends at a data byte, a marker or the end: p only grows, p < n inside
        if (p >= n) { w.term = 2; break; }
        v = ld(p);
        if (v != 0xFF) break;
        if (p + 1 >= n) { w.term = 2; break; }
        const uint32_t v2 = ld(p + 1);
        if (v2 == 0x00) break;
        if (v2 != 0xFF) { w.term = 1; w.code = (int)v2; break; }
        ++p;                              // a fill byte
      }
    }
    w.idx[k] = p;
    if (!w.term) {
      w.bits |= (uint64_t)v << (56 - 8 * k);
      w.nb = k + 1;
      p += v == 0xFF ? 2 : 1;
    }
  }
  w.idx[5] = p;
}

ST_JE_HD uint32_t pick(const Window& w, int q) {
  return q == 0 ? w.idx[0] : q == 1 ? w.idx[1] : q == 2 ? w.idx[2] : q == 3 ? w.idx[3] : q == 4 ? w.idx[4] : w.idx[5];
}

// Where a decoder that knows nothing starts in the subsequence that begins at raw byte p (0 < p < n): behind a
// stuffing 00 or a marker's second byte, told from the byte in front.
template <class Load>
ST_JE_HD uint32_t speculative_start(const Load& ld, uint32_t p) {
  return (ld(p - 1) == 0xFF && ld(p) != 0xFF) ? p + 1 : p;
}

// ---- the symbol decode (decode_symbol of jpeg_io.cpp) ------------------------------------------------------------------
ST_JE_HD int huff_symbol(const StJpegHuffLut& h, uint32_t look, int& len) {          // look: 16 bits
  const uint32_t f = h.fast[look >> 7];
  if (f) {
    len = (int)(f >> 8);
    return (int)(f & 255);
  }
  for (int l = 10; l <= 16; ++l) {
    const int32_t code = (int32_t)(look >> (16 - l));
    if (code <= h.maxcode[l]) {
      if (code < h.mincode[l]) return -1;
      len = l;
      return h.vals[h.valptr[l] + code - h.mincode[l]];
    }
  }
  return -1;
}

ST_JE_HD int extend(uint32_t v, int s) { return s && v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// ---- the state step ----------------------------------------------------------------------------------------------------
struct Entry {
  uint32_t pos;        // raw byte * 8 + bit
  uint32_t state;      // block within the MCU << 8 | zigzag index (0 = the DC symbol is next)
};
ST_JE_HD bool same(const Entry& a, const Entry& b) { return a.pos == b.pos && a.state == b.state; }

// (markers crossed, blocks completed since the last of them - or at all if none): the scan's element and operator
struct Count {
  uint32_t m, c;
};
ST_JE_HD Count combine(const Count& l, const Count& r) { return Count{l.m + r.m, r.m ? r.c : l.c + r.c}; }

struct NoSink {
  ST_JE_HD void store(uint64_t, int16_t) const {}
  ST_JE_HD void error(uint32_t) const {}
};

// Decode every symbol whose first bit lies in raw bytes [.., end) from entry `e`; returns the exit.  cnt: what this
// piece crossed and completed.  WRITE: kseg / jblk are the true interval and block index at the entry; coefficients of
// the blocks the host decodes go to sink.store(element, value) - each zigzag position exactly once, by the thread that
// owns the symbol covering it (skipped positions as zeros, the DC as its difference) - and the host's refusals to
// sink.error(bits).  Bounded: every round consumes a bit of [.., end), crosses a marker or ends.
template <bool WRITE, class Load, class Sink>
ST_JE_HD Entry decode_piece(const Ctx& cx, const Load& ld, Entry e, uint32_t end, Count& cnt, uint32_t kseg, uint32_t jblk,
                            Sink& sink) {
  uint32_t p = e.pos >> 3;
  int b = (int)(e.pos & 7), blk = (int)(e.state >> 8), k = (int)(e.state & 255);
  cnt = Count{0, 0};
  bool live = false;
  uint64_t base = 0;
  if (WRITE) {
    live = kseg < cx.K && jblk < need_blocks(cx, kseg);
    if (live) base = block_base(cx, kseg, jblk);
  }
  Window w;
  for (uint32_t rounds = 9 * (end - (p < end ? p : end)) + 16; rounds && p < end; --rounds) {
    gather(ld, cx.n, p, w);
    const int avail = 8 * w.nb - b;
    const int c = comp_of_block(cx, blk);
    const StJpegHuffLut& h = k == 0 ? cx.d->dc[cx.d->dc_slot[c]] : cx.d->ac[cx.d->ac_slot[c]];
    int len = 16, s = 0, r = 0;
    const int sym = huff_symbol(h, (uint32_t)((w.bits << b) >> 48), len);
    if (sym >= 0) {
      s = k == 0 ? sym : (sym & 15);
      r = k == 0 ? 0 : (sym >> 4);
      len += s;
    }
    if (len > avail) {                                  // the data ends inside this symbol: on to what ends it
      const uint32_t t = pick(w, w.nb);
      if (w.term != 1) {                                // the end of the bytes: nothing more, for anyone
        p = cx.n;
        b = 0;
        break;
      }
      if (WRITE && live) sink.error(ST_JPEG_E_SHORT);   // the interval's blocks are not complete
      ++cnt.m;
      cnt.c = 0;
      ++kseg;
      jblk = 0;
      blk = k = 0;
      p = t + 2;
      b = 0;
      if (WRITE) {
        live = kseg < cx.K;
        if (live) base = block_base(cx, kseg, 0);
      }
      continue;
    }
    bool done = false;
    if (sym < 0) {                                      // fixed rule: 16 bits, the block ends
      if (WRITE && live) sink.error(ST_JPEG_E_CODE);
      done = true;
    } else {
      const int v = s ? extend((uint32_t)((w.bits << (b + len - s)) >> (64 - s)), s) : 0;
      if (k == 0) {
        if (WRITE && live) sink.store(base, (int16_t)v);
        k = 1;
      } else if (s == 0 && r != 15) {                   // EOB
        if (WRITE && live)
          for (int z = k; z < 64; ++z) sink.store(base + kZigzag[z], 0);
        done = true;
      } else {
        const int k2 = s ? k + r : k + 16;
        if (s ? k2 > 63 : k2 > 64) {
          if (WRITE && live) sink.error(ST_JPEG_E_RUN);
          done = true;
        } else {
          if (WRITE && live) {
            for (int z = k; z < k2; ++z) sink.store(base + kZigzag[z], 0);
            if (s) sink.store(base + kZigzag[k2], (int16_t)v);
          }
          k = s ? k2 + 1 : k2;
          done = k >= 64;
        }
      }
    }
    const int nb_ = b + len;
    p = pick(w, nb_ >> 3);
    b = nb_ & 7;
    if (done) {
      ++cnt.c;
      k = 0;
      blk = blk + 1 == cx.bpm ? 0 : blk + 1;
      if (WRITE) {
        const bool was_live = live;
        ++jblk;
        live = kseg < cx.K && jblk < need_blocks(cx, kseg);
        if (live) base = block_base(cx, kseg, jblk);
        if (was_live && !live && kseg + 1 < cx.K) {     // the interval's last block: what the host checks before RSTn
          gather(ld, cx.n, p, w);
          if (8 * w.nb - b >= 8) sink.error(ST_JPEG_E_LEFTOVER);
          else if (w.term != 1 || w.code != 0xD0 + (int)(kseg & 7)) sink.error(ST_JPEG_E_MARKER);
        }
      }
    }
  }
  return Entry{p * 8 + (uint32_t)b, (uint32_t)(blk << 8 | k)};
}

// after the last piece: the counts at the end of the bytes
ST_JE_HD uint32_t final_check(const Ctx& cx, const Count& at_end) {
  return (at_end.m + 1 < cx.K || (at_end.m + 1 == cx.K && at_end.c < cx.last_blocks)) ? (uint32_t)ST_JPEG_E_SHORT : 0u;
}

// ---- the DC chain ------------------------------------------------------------------------------------------------------
// Item t of component c in scan order (MCU by MCU, within a luma MCU row by row): its DC element, and whether the
// predictor restarts in front of it.  per = blocks of c in one MCU.
ST_JE_HD int dc_per(const Ctx& cx, int c) { return c == 0 ? cx.ny : 1; }
ST_JE_HD uint64_t dc_element(const Ctx& cx, int c, uint32_t t) {
  const uint32_t per = (uint32_t)dc_per(cx, c), mcu = t / per, sub = t % per;
  const uint32_t my = mcu / (uint32_t)cx.mcus_x, mx = mcu - my * (uint32_t)cx.mcus_x;
  uint64_t row = my, col = mx;
  if (c == 0) {
    row = (uint64_t)my * cx.nv + sub / (uint32_t)cx.nh;
    col = (uint64_t)mx * cx.nh + sub % (uint32_t)cx.nh;
  }
  return cx.coef_offset[c] + 64 * (row * (uint64_t)cx.blocks_w[c] + col);
}
ST_JE_HD bool dc_restarts(const Ctx& cx, int c, uint32_t t) { return cx.ri && t % (cx.ri * (uint32_t)dc_per(cx, c)) == 0; }

// (sum since the last restart, a restart seen): the segmented scan's element; sums wrap modulo 2^32 - the first
// excursion out of int16 is exact and raises the verdict, what follows it no longer matters
struct DcSum {
  uint32_t sum;
  uint32_t restart;
};
ST_JE_HD DcSum dc_combine(const DcSum& l, const DcSum& r) { return DcSum{r.restart ? r.sum : l.sum + r.sum, l.restart | r.restart}; }
ST_JE_HD bool dc_in_range(uint32_t pred) { return (int32_t)pred >= -32768 && (int32_t)pred <= 32767; }

}  // namespace jent
}  // namespace st
