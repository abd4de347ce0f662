// Exact-fp32 MFMA implicit-GEMM convolution for gfx950 (MI355X), NHWC.
//
//   out[m][j] = epilogue( sum_k A[m][k] * W[j][k] + bias[j] )
//   m = (n, oy, ox) output pixel, k = (kh, kw, ci), j = output channel.
//
// One ConvModule of the reference (Conv2d no-bias -> BatchNorm2d(eps=1e-3) ->
// SiLU; reference mmtrack/models/backbones/csp_darknet_disparity_v1.py:126-135)
// is ONE launch of this kernel: BN is folded into W/bias on the host in fp64,
// SiLU, the bottleneck residual, the two-branch average (a+b)/2
// (csp_darknet_disparity_v1.py:184), CSP/PAFPN channel concat (channel-offset
// stores) and PAFPN nearest x2 upsample (replicated stores) all live in the
// epilogue, so no separate elementwise kernel touches HBM.
//
// Machine mapping (MI355X_MICROARCH.md): v_mfma_f32_32x32x2_f32 (exact fp32,
// 64 cycles/SIMD, 157 TFLOP/s chip peak).  A wave owns a (32*TM)x(32*TN)
// output tile in 16*TM*TN accumulator registers.  A and W tiles of BK=32 are
// staged global -> registers (16 B/lane, im2col gather with zero fill) ->
// LDS rows of 36 floats (conflict-free ds_read_b128: 36*i mod 64 distinct for
// any 16 rows) and double buffered, one barrier per K-chunk.  Lane (i, h)
// reads k = 8g+4h .. 8g+4h+3 with one ds_read_b128; MFMA step s pairs
// A[i][8g+4h+s] with W[j][8g+4h+s] for h = 0,1 - a k permutation, which a
// sum over k does not care about.
#include <algorithm>

#include <type_traits>

#include "st_common.h"

namespace st {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct ConvKArgs {
  const float* in;
  const float* wgt;
  const float* bias;
  float* out1;
  float* out2;
  float* up;
  const float* res;
  int Hi, Wi, Cin, in_ld, in_off;
  int Ho, Wo, HoWo, Cout;
  int KH, KW, stride, pad;
  int K, Kpad, M;
  unsigned in_bytes, wgt_bytes;  // buffer-descriptor extents (range-checked loads)
  int out1_ld, out1_off, split;
  int out2_ld, out2_off;
  int up_ld, up_off;
  int res_ld, res_off;
  float post_scale;
  int act;
  int n_tiles;  // tiles along Cout
};

constexpr int BK = 32;
constexpr int LDK = 36;  // padded LDS row (floats)

__device__ __forceinline__ float silu_f32(float v) {
  // v * sigmoid(v) with v_exp_f32 / v_rcp_f32 (1 ulp each): v * rcp(1 + exp(-v)); exp(-v) = inf for
  // v << 0 gives v * 0 = -0
  return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v));
}

// Fused epilogue shared by all conv kernels: bias, SiLU, residual / branch average, split and
// channel-offset stores, nearest x2 upsampled store.
template <int TM, int TN>
__device__ __forceinline__ void conv_epilogue(const ConvKArgs& p, f32x16 (&acc)[TM][TN], int m0, int n0, int wm,
                                              int wn, int l31, int lh, int BM, int BN) {
  // ---- epilogue: lane holds column j = lane&31, rows (r&3) + 8*(r>>2) + 4*(lane>>5)
  // All element offsets fit 32 bits (checked on the host), bases are wave-uniform: stores/loads use
  // the SGPR-base + 32-bit VGPR-offset form.  The common case (tile fully inside, no split / upsample)
  // runs without per-element predicates.
  const bool full_tile = (m0 + BM <= p.M) && (n0 + BN <= p.Cout);
  // a tile that lies on ONE side of the split stores through one (pointer, stride, offset) triple chosen once per
  // workgroup (CSP main|short convs: split = Cout / 2 is a multiple of the tile width)
  const bool side1 = !p.out2 || n0 + BN <= p.split, side2 = p.out2 && n0 >= p.split;
  const bool simple = full_tile && !p.up && (side1 || side2);
  if (simple) {
    float* __restrict__ o1 = side1 ? p.out1 + p.out1_off : p.out2 + p.out2_off - p.split;
    const unsigned o_ld = side1 ? (unsigned)p.out1_ld : (unsigned)p.out2_ld;
    const float* __restrict__ rs = p.res ? p.res + p.res_off : nullptr;
#pragma unroll
    for (int tj = 0; tj < TN; ++tj) {
      const unsigned j = n0 + wn * 32 * TN + tj * 32 + l31;
      const float bj = p.bias[j];
#pragma unroll
      for (int ti = 0; ti < TM; ++ti) {
        const unsigned mb = m0 + wm * 32 * TM + ti * 32 + 4 * lh;
        float rv[16];
        if (rs) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            rv[r] = rs[(mb + (r & 3) + 8 * (r >> 2)) * (unsigned)p.res_ld + j];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = acc[ti][tj][r] + bj;
          if (p.act) v = silu_f32(v);
          if (rs) v = (v + rv[r]) * p.post_scale;
          o1[(mb + (r & 3) + 8 * (r >> 2)) * o_ld + j] = v;
        }
      }
    }
    return;
  }
#pragma unroll
  for (int tj = 0; tj < TN; ++tj) {
    const int j = n0 + wn * 32 * TN + tj * 32 + l31;
    const float bj = p.bias[j];  // bias is padded to the tile grid
    const bool vj = j < p.Cout;
#pragma unroll
    for (int ti = 0; ti < TM; ++ti) {
      // residual: issue all 16 loads of this 32x32 tile before the first use (one wait, not 16
      // dependent HBM round trips)
      float rv[16];
      if (p.res) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * 32 * TM + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          rv[r] = (m < p.M && vj) ? p.res[(unsigned)m * (unsigned)p.res_ld + p.res_off + j] : 0.f;
        }
      }
      // (n, oy, ox) of the lane's rows for the upsampled store: ONE division pair per 32x32 tile, then the 16 rows
      // (m + 0,1,2,3, 8,9,10,11, ...) by stepping - the per-element divisions were ~1300 vector instructions per wave
      int un = 0, uy = 0, ux = 0;
      if (p.up) {
        const int mfirst = m0 + wm * 32 * TM + ti * 32 + 4 * lh;
        un = mfirst / p.HoWo;
        const int rem = mfirst - un * p.HoWo;
        uy = rem / p.Wo;
        ux = rem - uy * p.Wo;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 * TM + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (p.up && r > 0) {   // step from row r-1: +1 inside a group of 4, +5 to the next group
          ux += (r & 3) ? 1 : 5;
          while (ux >= p.Wo) {
            ux -= p.Wo;
            if (++uy == p.Ho) { uy = 0; ++un; }
          }
        }
        if (m < p.M && vj) {
          float v = acc[ti][tj][r] + bj;
          if (p.act) v = silu_f32(v);
          if (p.res) v = (v + rv[r]) * p.post_scale;
          if (j < p.split)
            p.out1[(unsigned)m * (unsigned)p.out1_ld + p.out1_off + j] = v;
          else
            p.out2[(unsigned)m * (unsigned)p.out2_ld + p.out2_off + (j - p.split)] = v;
          if (p.up) {
            const unsigned W2 = 2u * p.Wo;
            const unsigned base = ((unsigned)un * 2u * p.Ho + 2u * uy) * W2 + 2u * ux;
            float* u = p.up + p.up_off + j;
            u[base * (unsigned)p.up_ld] = v;
            u[(base + 1) * (unsigned)p.up_ld] = v;
            u[(base + W2) * (unsigned)p.up_ld] = v;
            u[(base + W2 + 1) * (unsigned)p.up_ld] = v;
          }
        }
      }
    }
  }
}

// NBUF = 2: LDS double buffer, one barrier per K-chunk (multi-wave blocks).
// NBUF = 1: single-wave blocks (WM = WN = 1) only - the wave's own in-order LDS queue orders the
//           write of chunk k+1 behind the reads of chunk k, so there is no cross-wave barrier at all and
//           half the LDS (2 such waves per SIMD fit in 160 KiB).
// DMA = 1: tiles go global -> LDS directly (`buffer_load_dwordx4 ... lds`, 1 KiB per wave-instruction):
//          no staging VGPRs, no ds_write, no address math between load and store.  The LDS image must be
//          lane-linear (8 rows x 128 B per instruction, unpadded), so bank conflicts are removed by an XOR
//          swizzle applied on the SOURCE side (lane (row, q) fetches k-group q ^ ((row>>1)&7)) and undone
//          by the same XOR in the fragment reads (cdna_hip_programming.md rule 21): conflict-free for the
//          ds_read_b128 lane groups.
// PW = 1: the layer is POINTWISE (1x1, stride 1, no padding - half of the launches of the network).  Input pixel =
//         output pixel and k = channel: no divisions or tap masks in the set-up, and the per-chunk address update of
//         the staging loads is one add.  The general set-up is ~300 vector instructions per lane and the general
//         update ~20 per chunk; on the fp32 matrix path VALU time adds to MFMA time (tools/micro/mfma_peak.hip), and a
//         K = 128 layer has only 64 MFMAs per wave to hide them behind.
template <int TM, int TN, int WM, int WN, int NBUF, int ILV = 1, int DMA = 0, int PW = 0>
__global__ __launch_bounds__(64 * WM * WN) void conv_igemm_kernel(ConvKArgs p) {
  static_assert(NBUF == 2 || (WM == 1 && WN == 1), "single LDS buffer needs a single-wave block");
  static_assert(!DMA || (NBUF == 2 && 64 * WM * WN >= 128), "LDS-DMA variant: double buffer, >= 2 waves");
  constexpr int LDK = DMA ? 32 : st::LDK;  // LDS row length in floats (DMA image is unpadded)
  constexpr int NT = 64 * WM * WN;
  constexpr int BM = 32 * TM * WM;
  constexpr int BN = 32 * TN * WN;
  constexpr int ROWS = NT / 8;  // tile rows covered by one staging pass
  constexpr int AP = BM / ROWS;
  constexpr int BP = BN / ROWS;
  static_assert(BM % ROWS == 0 && BN % ROWS == 0, "tile/thread mismatch");

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                    // [NBUF][BM][LDK]
  float* Bs = smem + NBUF * BM * LDK;  // [NBUF][BN][LDK]

  // XCD-aware tile order: blocks b and b+8 share an XCD (and its L2); give each XCD a
  // contiguous run of tiles so Cout-tiles of one pixel tile and neighbouring pixel
  // tiles (3x3 halo rows) hit the same L2.  Bijective for any grid size.
  const int nblk = gridDim.x, bid = blockIdx.x;
  const int q = nblk >> 3, r8 = nblk & 7, xcd = bid & 7, slot = bid >> 3;
  const int logical = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + slot;
  const int mt = logical / p.n_tiles;
  const int nt = logical - mt * p.n_tiles;
  const int m0 = mt * BM, n0 = nt * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave - wm * WN;
  const int l31 = lane & 31, lh = lane >> 5;

  // ---- staging geometry: thread owns 4-float group kq of rows r0 + ROWS*pass.
  // Loads are raw buffer loads: the hardware range check returns 0 for an out-of-range offset, so the
  // im2col zero fill (padding, ragged M, K tail) costs one v_cndmask instead of an exec-masked branch.
  // Per row: the byte offset of its window's (0,0) tap (may be "negative" at the border: only added to
  // in-range taps) and a bit mask of the KH*KW taps that fall inside the image.
  const int r0 = tid >> 3;
  // DMA: lane (row, q) stages k-group q ^ ((row >> 1) & 7); (row >> 1) & 7 is the same for every pass
  // because ROWS is a multiple of 16
  const int kq = DMA ? ((tid & 7) ^ ((r0 >> 1) & 7)) : (tid & 7);
  const __amdgpu_buffer_rsrc_t rsrcA =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, p.in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrcB =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wgt), 0, p.wgt_bytes, 0x00020000);
  int rowoff[AP];
  unsigned vmask[AP];
#pragma unroll
  for (int a = 0; a < AP; ++a) {
    const int m = m0 + r0 + a * ROWS;
    const bool vm = m < p.M;
    const int mm = vm ? m : 0;
    if (PW) {
      rowoff[a] = (mm * p.in_ld + p.in_off) * 4;
      vmask[a] = vm ? 1u : 0u;
      continue;
    }
    const int n = mm / p.HoWo;
    const int rem = mm - n * p.HoWo;
    const int oy = rem / p.Wo;
    const int ox = rem - oy * p.Wo;
    const int iy0 = oy * p.stride - p.pad, ix0 = ox * p.stride - p.pad;
    rowoff[a] = (((n * p.Hi + iy0) * p.Wi + ix0) * p.in_ld + p.in_off) * 4;
    unsigned msk = 0;
    for (int kh = 0; kh < p.KH; ++kh)
      for (int kw = 0; kw < p.KW; ++kw)
        if (vm && (unsigned)(iy0 + kh) < (unsigned)p.Hi && (unsigned)(ix0 + kw) < (unsigned)p.Wi)
          msk |= 1u << (kh * p.KW + kw);
    vmask[a] = msk;
  }
  unsigned woff[BP];
#pragma unroll
  for (int b = 0; b < BP; ++b) woff[b] = ((unsigned)(n0 + r0 + b * ROWS) * (unsigned)p.Kpad + kq * 4) * 4u;

  // running (tap, c) of this lane's 4-float group and the tap's byte offset; advanced by 32 per chunk
  int kc_c = kq * 4, kc_kh = 0, kc_kw = 0, kc_k = kq * 4;
  if (!PW) {
    while (kc_c >= p.Cin) {
      kc_c -= p.Cin;
      if (++kc_kw == p.KW) { kc_kw = 0; ++kc_kh; }
    }
  }
  int kc_tap = PW ? 0 : kc_kh * p.KW + kc_kw;
  int kc_off = PW ? kc_k * 4 : ((kc_kh * p.Wi + kc_kw) * p.in_ld + kc_c) * 4;

  f32x4 areg[AP], breg[BP];
  // one 16-B staging item of this thread: A row `a` (im2col gather, zero fill) / W row `b`
  auto load_a = [&](int a, bool vk) {
    const bool v = vk && ((vmask[a] >> kc_tap) & 1u);
    const unsigned off = v ? (unsigned)(rowoff[a] + kc_off) : 0x80000000u;
    areg[a] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrcA, off, 0, 0));
  };
  auto load_b = [&](int b, int kc) {
    breg[b] = __builtin_bit_cast(
        f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrcB, woff[b], kc * (BK * 4), 0));
  };
  auto advance = [&]() {  // move this lane's (kh, kw, c) to the next K-chunk
    kc_k += BK;
    if (PW) {   // k = channel: the lane's group moves 32 channels on
      kc_off += BK * 4;
      return;
    }
    kc_c += BK;
    while (kc_c >= p.Cin) {
      kc_c -= p.Cin;
      if (++kc_kw == p.KW) { kc_kw = 0; ++kc_kh; }
    }
    kc_tap = kc_kh * p.KW + kc_kw;
    kc_off = ((kc_kh * p.Wi + kc_kw) * p.in_ld + kc_c) * 4;
  };
  auto store_a = [&](int a, int buf) {
    *reinterpret_cast<f32x4*>(As + buf * BM * LDK + (r0 + a * ROWS) * LDK + kq * 4) = areg[a];
  };
  auto store_b = [&](int b, int buf) {
    *reinterpret_cast<f32x4*>(Bs + buf * BN * LDK + (r0 + b * ROWS) * LDK + kq * 4) = breg[b];
  };
  // LDS-DMA items: wave-uniform LDS base (the hardware adds lane * 16 B), per-lane range-checked source
  auto dma_a = [&](int a, bool vk, int buf) {
    const bool v = vk && ((vmask[a] >> kc_tap) & 1u);
    const unsigned off = v ? (unsigned)(rowoff[a] + kc_off) : 0x80000000u;
#if defined(__HIP_DEVICE_COMPILE__)  // device-only builtin; the host pass only needs the kernel stub
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        rsrcA, (__attribute__((address_space(3))) void*)(As + buf * BM * LDK + (wave * 8 + a * ROWS) * LDK), 16, off,
        0, 0, 0);
#else
    (void)off; (void)buf;
#endif
  };
  auto dma_b = [&](int b, int kc, int buf) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        rsrcB, (__attribute__((address_space(3))) void*)(Bs + buf * BN * LDK + (wave * 8 + b * ROWS) * LDK), 16,
        woff[b], kc * (BK * 4), 0, 0);
#else
    (void)b; (void)kc; (void)buf;
#endif
  };
  auto dma_chunk = [&](int kc, int buf) {
    const bool vk = kc_k < p.K;
#pragma unroll
    for (int a = 0; a < AP; ++a) dma_a(a, vk, buf);
#pragma unroll
    for (int b = 0; b < BP; ++b) dma_b(b, kc, buf);
    advance();
  };
  auto load_chunk = [&](int kc) {
    const bool vk = kc_k < p.K;
#pragma unroll
    for (int a = 0; a < AP; ++a) load_a(a, vk);
#pragma unroll
    for (int b = 0; b < BP; ++b) load_b(b, kc);
    advance();
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int a = 0; a < AP; ++a) store_a(a, buf);
#pragma unroll
    for (int b = 0; b < BP; ++b) store_b(b, buf);
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nchunks = p.Kpad / BK;
  if (DMA) {
    dma_chunk(0, 0);
  } else {
    load_chunk(0);
    store_chunk(0);
  }
  // LDS-DMA data is only ordered behind the ISSUING wave's vmcnt; other waves read it after the barrier, so every
  // wave drains its own DMA explicitly before joining it (not left to the compiler's waitcnt insertion)
  if (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // Main loop.  A K-chunk is 16 MFMA "slots" (4 fragment groups x 4 k-steps) per accumulator tile.  The
  // staging of chunk k+1 is threaded through the MFMA stream of chunk k, one 16-B item per slot: global
  // loads in the first 8 slots, LDS stores (into the other buffer) in the last 8.  Issued between MFMAs
  // they ride in the shadow of the 64-cycle matrix instructions instead of forming a load burst at the
  // top and a vmcnt-wait + ds_write burst at the bottom of every chunk.
  constexpr int NI = AP + BP;
  // One K-chunk.  MORE = "a chunk follows" is a compile-time tag: the steady-state body is straight-line code
  // (no uniform branches around the staging items, no K-tail test), only the final chunk looks at the K tail.
  // The A/W fragments of k-group g+1 are read from LDS BEFORE the 4*TM*TN MFMAs of group g are issued
  // (two fragment register sets), so the ds_read latency is covered by a full group of MFMAs instead of being
  // exposed four times per chunk.
  auto do_chunk = [&](int kc, auto more_tag) {
    constexpr bool MORE = decltype(more_tag)::value;
    const int buf = NBUF == 2 ? (kc & 1) : 0;
    const int nbuf = NBUF == 2 ? (buf ^ 1) : 0;
    constexpr bool more = MORE;
    const bool vk = kc_k < p.K;  // the lane state already describes chunk kc + 1
    if (!DMA && !ILV && more) load_chunk(kc + 1);
    if (DMA && !ILV && more) dma_chunk(kc + 1, nbuf);

    const float* Ab = As + buf * BM * LDK + (wm * 32 * TM + l31) * LDK + (DMA ? 0 : 4 * lh);
    const float* Bb = Bs + buf * BN * LDK + (wn * 32 * TN + l31) * LDK + (DMA ? 0 : 4 * lh);
    const int sw = (l31 >> 1) & 7;  // DMA image: k-group g of a row lives in 16-B slot g ^ sw
    // k-groups of this chunk that hold real data (K tail): only the final chunk can be short
    const int gmax = MORE ? 4 : (p.K - kc * BK + 7) >> 3;
    f32x4 a[2][TM], b[2][TN];
    auto read_frags = [&](int g, int set) {
      const int koff = DMA ? (((2 * g + lh) ^ sw) * 4) : g * 8;
#pragma unroll
      for (int i = 0; i < TM; ++i)
        a[set][i] = *reinterpret_cast<const f32x4*>(Ab + i * 32 * LDK + koff);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        b[set][j] = *reinterpret_cast<const f32x4*>(Bb + j * 32 * LDK + koff);
    };
    read_frags(0, 0);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (!MORE && g >= gmax) break;
      const int set = g & 1;
      if (g + 1 < 4) read_frags(g + 1, set ^ 1);   // (zero padding beyond the K tail: harmless to read)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[set][i][s], b[set][j][s], acc[i][j], 0, 0, 0);
        if (DMA && ILV) {
          const int slot = g * 4 + s;
          if (more) {  // one DMA item per slot, all issued in the first half of the chunk
#pragma unroll
            for (int it = 0; it < NI; ++it) {
              if ((it * 8) / NI == slot) {
                if (it < AP) dma_a(it, vk, nbuf); else dma_b(it - AP, kc + 1, nbuf);
              }
            }
            if (slot == 7) advance();
          }
        }
        if (!DMA && ILV && NBUF == 2) {
          const int slot = g * 4 + s;
          if (more) {
#pragma unroll
            for (int it = 0; it < NI; ++it) {
              if ((it * 8) / NI == slot) {
                if (it < AP) load_a(it, vk); else load_b(it - AP, kc + 1);
              }
              if (8 + (it * 8) / NI == slot) {
                if (it < AP) store_a(it, nbuf); else store_b(it - AP, nbuf);
              }
            }
            if (slot == 7) advance();
          }
        }
      }
    }

    if (!DMA && (!ILV || NBUF != 2) && more) {
      if (ILV) load_chunk(kc + 1);  // single-buffer blocks: stage after the reads of this chunk
      store_chunk(nbuf);
    }
    if (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA of chunk kc + 1 has landed
    __syncthreads();
  };
  for (int kc = 0; kc + 1 < nchunks; ++kc) do_chunk(kc, std::true_type{});
  do_chunk(nchunks - 1, std::false_type{});

  conv_epilogue<TM, TN>(p, acc, m0, n0, wm, wn, l31, lh, BM, BN);
}

// ==== TOOLS-ONLY from here to the matching #endif (make ABLATION=1; round-5 decision) ====================
// The split-operand instances below did not pass the round's frozen parity gate (`ST_SPLIT_BF16=1 pytest -m gpu`:
// profiles/r05_gpu_tests_split_plan.log - the two white-noise configs[2] cases read 1.59e-3 from float64 against a bound
// of 1.29e-3) and bought +0.7 % under the in-flight loop: they are PARKED.  The product library contains no bf16 MFMA
// and no way to select one; tools/split_*.py and the split tests run against the tools build (ST_LIBRARY=...ablation.so).
#ifdef ST_ABLATION
// ---- split-operand instance ("bf16x3"): the same implicit GEMM on the BF16 matrix pipes ------------------------------
// fp32 operands are split into three bf16 terms, x = hi + mid + lo (3 x 8 = 24 mantissa bits: the split is error-free),
// and the product is assembled from 6 of the 9 term products (hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid; the dropped
// ones are below 2^-24 relative), every term product exact in the fp32 accumulator of v_mfma_f32_32x32x16_bf16.  gfx950
// runs that instruction at 16x the rate of v_mfma_f32_32x32x2_f32 per multiply-add, so 6 of them per 16 k replace 8 of
// the fp32-input form at a quarter of the cycles: 2.67x the fp32 matrix rate.  Inputs, weights, accumulators and
// outputs stay fp32; measured on MI355X (tools/micro/bf16x3_gemm.hip, profiles/r04_bf16x3_microbench.txt) the result
// is CLOSER to a float64 evaluation than the fp32-input MFMA's (max error 3.2e-7 vs 5.2e-7 of the output scale).
// Structure = the register-staged kernel above: the split happens once per staged element on the way into LDS (three
// bf16 images per tile, rows of 32 k padded to 80 bytes: conflict-free 16-byte fragment reads), weights included -
// the packed fp32 weights are used as they are.  One LDS buffer (61 KB for a 128 x 128 tile: two workgroups per CU),
// the next chunk's global loads in flight during the MFMAs of the current one.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// x = hi + mid + lo, every term ROUNDED to nearest-even bf16 (v_cvt_pk_bf16_f32, two values per instruction): hi =
// bf16(x), r = x - hi (exact), mid = bf16(r), lo = bf16(r - mid).  Rounding (not truncation) keeps the representation
// error of the triple unbiased - a truncating split was measured 1.3x further from float64 end to end than the fp32
// plan on the white-noise sequence (its residuals all have the sign of x and add up along K).  Written with the
// instructions it should compile to (from generic casts the compiler emitted ~12 vector instructions per element,
// which made the kernel VALU-bound): per PAIR of elements 3 v_cvt_pk + 4 shift/mask + 4 v_sub = 5.5 per element.
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned sp_cvt_pk_bf16(float lo, float hi) {   // [bf16(hi) : bf16(lo)], round to nearest even
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ float sp_lo_f32(unsigned pk) { return __builtin_bit_cast(float, pk << 16); }
__device__ __forceinline__ float sp_hi_f32(unsigned pk) { return __builtin_bit_cast(float, pk & 0xFFFF0000u); }
__device__ __forceinline__ void split3_f32x4(const f32x4 x, u32x2& hi, u32x2& mid, u32x2& lo) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float x0 = x[2 * e], x1 = x[2 * e + 1];
    const unsigned h = sp_cvt_pk_bf16(x0, x1);
    const float r0 = x0 - sp_lo_f32(h), r1 = x1 - sp_hi_f32(h);        // exact
    const unsigned m = sp_cvt_pk_bf16(r0, r1);
    const float q0 = r0 - sp_lo_f32(m), q1 = r1 - sp_hi_f32(m);        // exact
    hi[e] = h; mid[e] = m; lo[e] = sp_cvt_pk_bf16(q0, q1);
  }
}

// SBK = k per chunk: 32 (two k16 steps, one workgroup of 128 x 128 per CU) or 16 (one step, half the LDS: two
// co-resident workgroups cover each other's barrier and fragment-read latency)
template <int TM, int TN, int WM, int WN, int PW, int SBK, bool SACC>
__global__ __launch_bounds__(64 * WM * WN, (SBK == 16 ? 2 : 1)) void conv_split_kernel(ConvKArgs p) {
  constexpr int NT = 64 * WM * WN;
  constexpr int BM = 32 * TM * WM;
  constexpr int BN = 32 * TN * WN;
  constexpr int KQ = SBK / 4;          // 16-byte staging groups per row
  constexpr int SP_LDK = SBK + 8;      // bf16 per LDS row: 80 B (SBK 32) / 48 B (SBK 16), conflict-free 16-byte reads
  constexpr int NSTEP = SBK / 16;
  constexpr int ROWS = NT / KQ;
  constexpr int AP = BM / ROWS;
  constexpr int BP = BN / ROWS;
  static_assert(BM % ROWS == 0 && BN % ROWS == 0, "tile/thread mismatch");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __bf16* As = reinterpret_cast<__bf16*>(smem);   // [2 buffers]{[3 parts][BM][SP_LDK] | [3 parts][BN][SP_LDK]}
  __bf16* Bs = As + 3 * BM * SP_LDK;

  const int nblk = gridDim.x, bid = blockIdx.x;   // XCD-aware tile order (as above)
  const int q = nblk >> 3, r8 = nblk & 7, xcd = bid & 7, slot = bid >> 3;
  const int logical = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + slot;
  const int mt = logical / p.n_tiles;
  const int nt = logical - mt * p.n_tiles;
  const int m0 = mt * BM, n0 = nt * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave - wm * WN;
  const int l31 = lane & 31, lh = lane >> 5;
  const int r0 = tid / KQ, kq = tid % KQ;
  const __amdgpu_buffer_rsrc_t rsrcA =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, p.in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrcB =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wgt), 0, p.wgt_bytes, 0x00020000);
  int rowoff[AP];
  unsigned vmask[AP];
#pragma unroll
  for (int a = 0; a < AP; ++a) {
    const int m = m0 + r0 + a * ROWS;
    const bool vm = m < p.M;
    const int mm = vm ? m : 0;
    if (PW) {
      rowoff[a] = (mm * p.in_ld + p.in_off) * 4;
      vmask[a] = vm ? 1u : 0u;
      continue;
    }
    const int n = mm / p.HoWo;
    const int rem = mm - n * p.HoWo;
    const int oy = rem / p.Wo;
    const int ox = rem - oy * p.Wo;
    const int iy0 = oy * p.stride - p.pad, ix0 = ox * p.stride - p.pad;
    rowoff[a] = (((n * p.Hi + iy0) * p.Wi + ix0) * p.in_ld + p.in_off) * 4;
    unsigned msk = 0;
    for (int kh = 0; kh < p.KH; ++kh)
      for (int kw = 0; kw < p.KW; ++kw)
        if (vm && (unsigned)(iy0 + kh) < (unsigned)p.Hi && (unsigned)(ix0 + kw) < (unsigned)p.Wi)
          msk |= 1u << (kh * p.KW + kw);
    vmask[a] = msk;
  }
  unsigned woff[BP];
#pragma unroll
  for (int b = 0; b < BP; ++b) woff[b] = ((unsigned)(n0 + r0 + b * ROWS) * (unsigned)p.Kpad + kq * 4) * 4u;
  int kc_c = kq * 4, kc_kh = 0, kc_kw = 0, kc_k = kq * 4;
  if (!PW) {
    while (kc_c >= p.Cin) {
      kc_c -= p.Cin;
      if (++kc_kw == p.KW) { kc_kw = 0; ++kc_kh; }
    }
  }
  int kc_tap = PW ? 0 : kc_kh * p.KW + kc_kw;
  int kc_off = PW ? kc_k * 4 : ((kc_kh * p.Wi + kc_kw) * p.in_ld + kc_c) * 4;

  // Pipeline, distance 2: during the MFMAs of chunk kc the lane (1) issues the global loads of chunk kc + 2 into the
  // register set chunk kc was staged from, and (2) splits chunk kc + 1 (loaded one chunk ago: landed) into its three
  // bf16 images and writes them to the OTHER LDS buffer, one 16-byte item per MFMA slot - the bf16 MFMA leaves the
  // vector issue free for 24 of its 32 cycles, so the ~22 vector instructions of an item ride beside the 6 MFMAs of
  // a slot.  One barrier per chunk.
  constexpr int NI = AP + BP;
  f32x4 stg[2][NI];
  auto load_chunk = [&](int kc, int set) {
    const bool vk = kc_k < p.K;
#pragma unroll
    for (int a = 0; a < AP; ++a) {
      const bool v = vk && ((vmask[a] >> kc_tap) & 1u);
      const unsigned off = v ? (unsigned)(rowoff[a] + kc_off) : 0x80000000u;
      stg[set][a] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrcA, off, 0, 0));
    }
#pragma unroll
    for (int b = 0; b < BP; ++b)
      stg[set][AP + b] =
          __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrcB, woff[b], kc * (SBK * 4), 0));
    kc_k += SBK;   // advance this lane's (kh, kw, c) to the next K-chunk
    if (PW) {
      kc_off += SBK * 4;
    } else {
      kc_c += SBK;
      while (kc_c >= p.Cin) {
        kc_c -= p.Cin;
        if (++kc_kw == p.KW) { kc_kw = 0; ++kc_kh; }
      }
      kc_tap = kc_kh * p.KW + kc_kw;
      kc_off = ((kc_kh * p.Wi + kc_kw) * p.in_ld + kc_c) * 4;
    }
  };
  constexpr int IMG = 3 * (BM + BN) * SP_LDK;   // bf16 elements of one LDS buffer (A images, then W images)
  auto store_item = [&](int it, int set, int buf) {   // split one staged 4-float group into its three bf16 images
    u32x2 h, m, l;
    split3_f32x4(stg[set][it], h, m, l);
    if (it < AP) {
      __bf16* d = As + buf * IMG + (r0 + it * ROWS) * SP_LDK + kq * 4;
      *reinterpret_cast<u32x2*>(d) = h;
      *reinterpret_cast<u32x2*>(d + BM * SP_LDK) = m;
      *reinterpret_cast<u32x2*>(d + 2 * BM * SP_LDK) = l;
    } else {
      __bf16* d = Bs + buf * IMG + (r0 + (it - AP) * ROWS) * SP_LDK + kq * 4;
      *reinterpret_cast<u32x2*>(d) = h;
      *reinterpret_cast<u32x2*>(d + BN * SP_LDK) = m;
      *reinterpret_cast<u32x2*>(d + 2 * BN * SP_LDK) = l;
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  // SACC: the five small term products accumulate in a register set of their own and join the leading products once, at
  // the end - their low bits are not rounded away against a running sum 2^8..2^16 times larger.  Measured against float64
  // at the path's layer shapes (tools/split_check.py): rms distance 0.37 x that of the exact-fp32 MFMA instance (one
  // accumulator for all six products: 0.86 x); same speed wherever the second set fits in registers (every instance but
  // the 128x128 k16 one, which keeps the single chain).
  f32x16 accS[SACC ? TM : 1][SACC ? TN : 1];
  if (SACC) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) accS[SACC ? i : 0][SACC ? j : 0][r] = 0.f;
  }

  const int nchunks = p.Kpad / SBK;
  load_chunk(0, 0);
  if (nchunks > 1) load_chunk(1, 1);
#pragma unroll
  for (int it = 0; it < NI; ++it) store_item(it, 0, 0);
  __syncthreads();
  constexpr int NSLOT = NSTEP * TM * TN;
  constexpr int IPS = (NI + NSLOT - 1) / NSLOT;   // staging items per MFMA slot
  constexpr int VPG = (22 * IPS + 5) / 6;         // vector instructions per MFMA gap (an item's split is ~22)
  // MORE1 / MORE2 ("chunk kc + 1 / kc + 2 exists") are compile-time tags: the body is straight-line code, so the
  // scheduler may weave the staging work between the MFMAs (a branch would split the scheduling region)
  auto do_chunk = [&](int kc, auto set_tag, auto more1_tag, auto more2_tag) {
    constexpr int SET = decltype(set_tag)::value;   // register set chunk kc was staged from = kc & 1 = LDS buffer
    constexpr bool more1 = decltype(more1_tag)::value, more2 = decltype(more2_tag)::value;
    if (more2) load_chunk(kc + 2, SET);
    const __bf16* Ab = As + SET * IMG + (wm * 32 * TM + l31) * SP_LDK + 8 * lh;
    const __bf16* Bb = Bs + SET * IMG + (wn * 32 * TN + l31) * SP_LDK + 8 * lh;
#pragma unroll
    for (int st = 0; st < NSTEP; ++st) {   // k16 steps of the chunk; lane (row, lh) holds k = 16 st + 8 lh .. + 7
      bf16x8 fa[TM][3], fb[TN][3];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int pt = 0; pt < 3; ++pt)
          fa[i][pt] = *reinterpret_cast<const bf16x8*>(Ab + (pt * BM + i * 32) * SP_LDK + 16 * st);
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int pt = 0; pt < 3; ++pt)
          fb[j][pt] = *reinterpret_cast<const bf16x8*>(Bb + (pt * BN + j * 32) * SP_LDK + 16 * st);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {   // smallest terms first, the leading product last
          if (SACC) {
            f32x16 c = accS[SACC ? i : 0][SACC ? j : 0];
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][1], fb[j][1], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][2], fb[j][0], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[j][2], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][1], fb[j][0], c, 0, 0, 0);
            accS[SACC ? i : 0][SACC ? j : 0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[j][1], c, 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[j][0], acc[i][j], 0, 0, 0);
          } else {
            f32x16 c = acc[i][j];
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][1], fb[j][1], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][2], fb[j][0], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[j][2], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][1], fb[j][0], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[j][1], c, 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][0], fb[j][0], c, 0, 0, 0);
          }
          if (more1) {
            const int slot = (st * TM + i) * TN + j;
#pragma unroll
            for (int it = 0; it < NI; ++it)
              if ((it * NSLOT) / NI == slot) store_item(it, SET ^ 1, SET ^ 1);
          }
          // issue order of this slot: the six MFMAs are a dependent chain, and an in-order wave cannot reach the vector
          // instructions behind them until the last one has issued - so the split is woven BETWEEN them: one MFMA,
          // then four vector instructions, six times (then the LDS writes).  The compiler clusters the MFMAs otherwise.
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // 1 MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, VPG, 0);   // VALU
          }
          __builtin_amdgcn_sched_group_barrier(0x200, 3 * IPS, 0);   // the item's LDS writes
        }
    }
    __syncthreads();   // chunk kc + 1's images are complete, and every wave is done reading chunk kc's buffer
  };
  using T = std::true_type;
  using F = std::false_type;
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  int kc = 0;
  for (; kc + 3 < nchunks; kc += 2) {   // steady state: both look-aheads exist for kc and kc + 1
    do_chunk(kc, S0{}, T{}, T{});
    do_chunk(kc + 1, S1{}, T{}, T{});
  }
  for (; kc < nchunks; ++kc) {          // the last one to three chunks
    const bool m1 = kc + 1 < nchunks, m2 = kc + 2 < nchunks;
    if (kc & 1) {
      if (m2) do_chunk(kc, S1{}, T{}, T{}); else if (m1) do_chunk(kc, S1{}, T{}, F{}); else do_chunk(kc, S1{}, F{}, F{});
    } else {
      if (m2) do_chunk(kc, S0{}, T{}, T{}); else if (m1) do_chunk(kc, S0{}, T{}, F{}); else do_chunk(kc, S0{}, F{}, F{});
    }
  }
  if (SACC) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] += accS[SACC ? i : 0][SACC ? j : 0];
  }
  conv_epilogue<TM, TN>(p, acc, m0, n0, wm, wn, l31, lh, BM, BN);
}

template <int TM, int TN, int WM, int WN, int PW, int SBK>
static int launch_split(const ConvKArgs& a, int m_tiles, hipStream_t stream) {
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
  constexpr size_t lds = (size_t)2 * 3 * (BM + BN) * (SBK + 8) * 2;   // two buffers of three bf16 images
  static bool attr_set = false;
  constexpr bool SACC = !(TM == 2 && TN == 2 && SBK == 16);   // the 128x128 k16 instance has no registers for it
  auto kern = conv_split_kernel<TM, TN, WM, WN, PW, SBK, SACC>;
  if (!attr_set) {
    ST_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set = true;
  }
  dim3 grid((unsigned)(m_tiles * a.n_tiles)), block(64 * WM * WN);
  hipLaunchKernelGGL(kern, grid, block, lds, stream, a);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

#endif   // ST_ABLATION: split-operand instances

#ifdef ST_ABLATION   // tools-only build: the wave-specialised experiment (instances 22..29) lives in its own file
#include "experiments/conv_igemm_ws.inc"
#endif

template <int TM, int TN, int WM, int WN, int NBUF = 2, int ILV = 1, int DMA = 0, int PW = 0>
static int launch_variant(const ConvKArgs& a, int m_tiles, hipStream_t stream) {
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
  constexpr size_t lds = (size_t)NBUF * (BM + BN) * (DMA ? 32 : LDK) * sizeof(float);
  static bool attr_set = false;
  auto kern = conv_igemm_kernel<TM, TN, WM, WN, NBUF, ILV, DMA, PW>;
  if (!attr_set) {
    ST_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set = true;
  }
  dim3 grid((unsigned)(m_tiles * a.n_tiles)), block(64 * WM * WN);
  hipLaunchKernelGGL(kern, grid, block, lds, stream, a);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

// Tile variants {BM, BN, threads}: id -> <TM,TN,WM,WN> in the switch of conv2d_launch.
//  0 128x128 (4 waves 64x64)   1 128x64 (2 waves 64x64)   2 128x32 (2 waves 64x32)
//  3  64x64  (4 waves 32x32)   4  64x32 (2 waves 32x32)   5 128x64 (4 waves 32x64)
//  6 128x32  (4 waves 32x32)   7  64x128 (4 waves 32x64)  8 256x64 (4 waves 64x64)
//  9  64x64  (1 wave, barrier-free, single LDS buffer)   10 64x32 (1 wave)   11 32x64 (1 wave)
// 12..16: LDS-DMA staging of 0 / 3 / 7 / 6 / 5 (DMA issue threaded through the MFMA stream);
// 17, 18: LDS-DMA 128x128 / 64x64 with the DMA burst at the top of the chunk
// 19..21: 256x128 tiles, 8 waves of 64x64 (LDS-DMA threaded / LDS-DMA burst / register staging)
// 22..26: wave-specialised (4 MFMA waves + 1 LDS-DMA loader wave): 128x128, 64x64, 64x128, 128x32, 128x64
struct ConvVariant { int bm, bn, threads; };
static const ConvVariant kVariants[] = {{128, 128, 256}, {128, 64, 128}, {128, 32, 128}, {64, 64, 256},
                                        {64, 32, 128},   {128, 64, 256}, {128, 32, 256}, {64, 128, 256},
                                        {256, 64, 256},  {64, 64, 64},   {64, 32, 64},   {32, 64, 64},
                                        {128, 128, 256}, {64, 64, 256},  {64, 128, 256}, {128, 32, 256},
                                        {128, 64, 256},  {128, 128, 256}, {64, 64, 256},
                                        {256, 128, 512}, {256, 128, 512}, {256, 128, 512},
                                        {128, 128, 320}, {64, 64, 320},   {64, 128, 320}, {128, 32, 320},
                                        {128, 64, 320},  {128, 128, 384}, {64, 128, 384}, {128, 128, 512}};
#ifdef ST_ABLATION
constexpr int kNumVariants = 30;   // + the wave-specialised experiments 22..29
#else
constexpr int kNumVariants = 22;
#endif

int conv_variant_count() { return kNumVariants; }
bool conv_variant_valid(int id, int cout) {
  return id >= 0 && id < kNumVariants && round_up(cout, 32) % kVariants[id].bn == 0;
}
const char* conv_variant_name(int id) {
  static const char* names[] = {"128x128", "128x64w2", "128x32w2", "64x64", "64x32w2",
                                "128x64", "128x32", "64x128", "256x64", "64x64w1", "64x32w1", "32x64w1",
                                "128x128dma", "64x64dma", "64x128dma", "128x32dma", "128x64dma",
                                "128x128dmab", "64x64dmab", "256x128dma", "256x128dmab", "256x128",
                                "128x128ws", "64x64ws", "64x128ws", "128x32ws", "128x64ws", "128x128ws2",
                                "64x128ws2", "128x128ws4"};
  return id >= 0 && id < kNumVariants ? names[id] : "-";
}

// template arguments <TM, TN, WM, WN, NBUF, ILV, DMA> of each variant's kernel instance (so profiler
// rows "st::conv_igemm_kernel<...>" can be matched to variants)
const char* conv_variant_signature(int id) {
  static const char* sigs[] = {"2, 2, 2, 2, 2, 1, 0", "2, 2, 2, 1, 2, 1, 0", "2, 1, 2, 1, 2, 1, 0",
                               "1, 1, 2, 2, 2, 1, 0", "1, 1, 2, 1, 2, 1, 0", "1, 2, 4, 1, 2, 1, 0",
                               "1, 1, 4, 1, 2, 1, 0", "1, 2, 2, 2, 2, 1, 0", "2, 2, 4, 1, 2, 1, 0",
                               "2, 2, 1, 1, 1, 1, 0", "2, 1, 1, 1, 1, 1, 0", "1, 2, 1, 1, 1, 1, 0",
                               "2, 2, 2, 2, 2, 1, 1", "1, 1, 2, 2, 2, 1, 1", "1, 2, 2, 2, 2, 1, 1",
                               "1, 1, 4, 1, 2, 1, 1", "1, 2, 4, 1, 2, 1, 1", "2, 2, 2, 2, 2, 0, 1",
                               "1, 1, 2, 2, 2, 0, 1", "2, 2, 4, 2, 2, 1, 1", "2, 2, 4, 2, 2, 0, 1",
                               "2, 2, 4, 2, 2, 1, 0", "ws 2, 2, 2, 2", "ws 1, 1, 2, 2", "ws 1, 2, 2, 2",
                               "ws 1, 1, 4, 1", "ws 1, 2, 4, 1", "ws 2, 2, 2, 2, 2", "ws 1, 2, 2, 2, 2",
                               "ws 2, 2, 2, 2, 4"};
  return id >= 0 && id < kNumVariants ? sigs[id] : "";
}

bool pw_conv_applicable(const StConvDesc& d);          // pointwise_conv.hip (tile variant 41)
int pw_conv_launch(const StConvDesc& d, hipStream_t stream, const StConvDesc* chain);
int pwr_conv_launch(const StConvDesc& d, hipStream_t stream, const StConvDesc* chain);
bool pwr_chain_applicable(const StConvDesc& d, const StConvDesc& c);
bool dc_conv_applicable(const StConvDesc& d);          // direct_conv.hip (tile variant 42)
int dc_conv_launch(const StConvDesc& d, hipStream_t stream);
bool wino_conv_applicable(const StConvDesc& d);        // wino_conv.hip (tile variant 43)
int wino_conv_launch(const StConvDesc& d, hipStream_t stream, bool narrow, bool parent_sched);
int wino_persist_launch(const StConvDesc& d, hipStream_t stream);   // wino_conv.hip (tile variant 57)

int conv2d_launch(const StConvDesc& d, hipStream_t stream, int force_variant, int* picked_variant) {
  ST_REQUIRE(d.in_dev && d.wgt_dev && d.bias_dev && d.out1_dev, "conv: null pointer");
  if (force_variant == 41) {   // streaming 1x1 kernel for narrow layers
    if (picked_variant) *picked_variant = 41;
    return pw_conv_launch(d, stream, nullptr);
  }
  if (force_variant == 46) {   // 1x1 kernel with LDS-resident weights, pixels register-fed
    if (picked_variant) *picked_variant = 46;
    return pwr_conv_launch(d, stream, nullptr);
  }
  if (force_variant == 42) {   // direct 3x3 kernel for narrow layers
    if (picked_variant) *picked_variant = 42;
    return dc_conv_launch(d, stream);
  }
  if (force_variant == 43 || force_variant == 44) {   // Winograd F(2x2,3x3) kernel (44: 32-cout workgroups)
    if (picked_variant) *picked_variant = force_variant;
    return wino_conv_launch(d, stream, force_variant == 44, false);
  }
#ifdef ST_ABLATION
  if (force_variant == 58 || force_variant == 59) {   // tools build: 43 / 44 on the K-loop schedule before the weight ring
    if (picked_variant) *picked_variant = force_variant;
    return wino_conv_launch(d, stream, force_variant == 59, true);
  }
  if (force_variant == 57) {   // tools build: persistent Winograd kernel (bit-identical to 43, not faster: wino_conv.hip)
    if (picked_variant) *picked_variant = 57;
    return wino_persist_launch(d, stream);
  }
#endif
  ST_REQUIRE(d.Cin % 4 == 0 && d.in_ld % 4 == 0 && d.in_off % 4 == 0,
             "conv: Cin/in_ld/in_off must be multiples of 4 (got %d/%d/%d)", d.Cin, d.in_ld,
             d.in_off);
  // every tile stages its operands in 16-byte buffer loads (into registers or straight into LDS)
  ST_REQUIRE(((reinterpret_cast<uintptr_t>(d.in_dev) | reinterpret_cast<uintptr_t>(d.wgt_dev)) & 15) == 0,
             "st_conv2d_nhwc: in_dev and wgt_dev must be 16-byte aligned");
  ST_REQUIRE(d.N > 0 && d.Hi > 0 && d.Wi > 0 && d.Cout > 0 && d.KH > 0 && d.KW > 0 &&
                 d.stride > 0 && d.pad >= 0,
             "conv: bad geometry");
  ST_REQUIRE(d.in_off + d.Cin <= d.in_ld, "conv: input channel slice exceeds in_ld");
  const int Ho = (d.Hi + 2 * d.pad - d.KH) / d.stride + 1;
  const int Wo = (d.Wi + 2 * d.pad - d.KW) / d.stride + 1;
  ST_REQUIRE(Ho > 0 && Wo > 0, "conv: empty output");
  const int split = (d.out2_dev ? d.split : d.Cout);
  ST_REQUIRE(split >= 0 && split <= d.Cout, "conv: bad split");
  ST_REQUIRE(d.out1_off + split <= d.out1_ld, "conv: out1 slice exceeds out1_ld");
  if (d.out2_dev)
    ST_REQUIRE(d.out2_off + (d.Cout - split) <= d.out2_ld, "conv: out2 slice exceeds out2_ld");
  if (d.up_dev) ST_REQUIRE(d.up_off + d.Cout <= d.up_ld, "conv: up slice exceeds up_ld");
  if (d.res_dev) ST_REQUIRE(d.res_off + d.Cout <= d.res_ld, "conv: res slice exceeds res_ld");
  const long long M_ll = (long long)d.N * Ho * Wo;
  // the kernel addresses every tensor with 32-bit element offsets
  ST_REQUIRE(M_ll * (long long)std::max(std::max(d.out1_ld, d.out2_ld), d.res_dev ? d.res_ld : 1) < (1ll << 31) &&
                 (long long)d.N * d.Hi * d.Wi * d.in_ld < (1ll << 29) &&   // bytes < 2^31: offset bit 31 = "invalid"
                 d.KH * d.KW <= 32 &&
                 (!d.up_dev || 4 * M_ll * d.up_ld < (1ll << 31)),
             "conv: tensor exceeds 2^31 elements");
  ST_REQUIRE((long long)d.N * d.Hi * d.Wi < (1ll << 31) && M_ll < (1ll << 31),
             "conv: pixel count exceeds int32");

  ConvKArgs a;
  a.in = d.in_dev; a.wgt = d.wgt_dev; a.bias = d.bias_dev;
  a.out1 = d.out1_dev; a.out2 = d.out2_dev; a.up = d.up_dev; a.res = d.res_dev;
  a.Hi = d.Hi; a.Wi = d.Wi; a.Cin = d.Cin; a.in_ld = d.in_ld; a.in_off = d.in_off;
  a.Ho = Ho; a.Wo = Wo; a.HoWo = Ho * Wo; a.Cout = d.Cout;
  a.KH = d.KH; a.KW = d.KW; a.stride = d.stride; a.pad = d.pad;
  a.K = d.KH * d.KW * d.Cin; a.Kpad = round_up(a.K, BK); a.M = (int)M_ll;
  a.in_bytes = (unsigned)((long long)d.N * d.Hi * d.Wi * d.in_ld * 4);
  a.wgt_bytes = (unsigned)((long long)round_up(d.Cout, 32) * a.Kpad * 4);
  a.out1_ld = d.out1_ld; a.out1_off = d.out1_off; a.split = split;
  a.out2_ld = d.out2_ld; a.out2_off = d.out2_off;
  a.up_ld = d.up_ld; a.up_off = d.up_off;
  a.res_ld = d.res_ld; a.res_off = d.res_off;
  a.post_scale = d.res_dev ? d.post_scale : 1.0f;
  a.act = d.act;

  const int cout_pad = round_up(d.Cout, 32);
  if (force_variant >= 50 && force_variant <= 55) {   // split-operand (bf16x3) instances of the same implicit GEMM
    // 50 128x128 k32 | 51 64x64 k32 | 52 128x64 k32 | 53 128x128 k16 | 54 64x64 k16 | 55 128x64 k16
    static const int sbm[3] = {128, 64, 128}, sbn[3] = {128, 64, 64};
    const int vi = (force_variant - 50) % 3, k16 = (force_variant - 50) / 3;
    ST_REQUIRE(cout_pad % sbn[vi] == 0, "conv: split variant %d does not divide Cout=%d", force_variant, d.Cout);
#ifndef ST_ABLATION
    (void)sbm; (void)k16;
    return set_error(ST_ERR_INVALID, "conv: the split-operand (bf16x3) instances 50-55 are parked in the tools-only build "
                                     "(make ABLATION=1, ST_LIBRARY=...libstereotrack_hip_ablation.so)");
#else
    if (picked_variant) *picked_variant = force_variant;
    a.n_tiles = cout_pad / sbn[vi];
    const int m_tiles = ceil_div(a.M, sbm[vi]);
    const bool pw = d.KH == 1 && d.KW == 1 && d.stride == 1 && d.pad == 0;
    switch (vi + 3 * k16) {
      case 0: return pw ? launch_split<2, 2, 2, 2, 1, 32>(a, m_tiles, stream) : launch_split<2, 2, 2, 2, 0, 32>(a, m_tiles, stream);
      case 1: return pw ? launch_split<1, 1, 2, 2, 1, 32>(a, m_tiles, stream) : launch_split<1, 1, 2, 2, 0, 32>(a, m_tiles, stream);
      case 2: return pw ? launch_split<1, 2, 4, 1, 1, 32>(a, m_tiles, stream) : launch_split<1, 2, 4, 1, 0, 32>(a, m_tiles, stream);
      case 3: return pw ? launch_split<2, 2, 2, 2, 1, 16>(a, m_tiles, stream) : launch_split<2, 2, 2, 2, 0, 16>(a, m_tiles, stream);
      case 4: return pw ? launch_split<1, 1, 2, 2, 1, 16>(a, m_tiles, stream) : launch_split<1, 1, 2, 2, 0, 16>(a, m_tiles, stream);
      default: return pw ? launch_split<1, 2, 4, 1, 1, 16>(a, m_tiles, stream) : launch_split<1, 2, 4, 1, 0, 16>(a, m_tiles, stream);
    }
#endif
  }
  int pick = -1;
  if (force_variant >= 0) {
    ST_REQUIRE(conv_variant_valid(force_variant % 100, d.Cout), "conv: variant %d does not divide Cout=%d",
               force_variant, d.Cout);
    pick = force_variant % 100;
  } else {
    // untuned default: the largest tile that still gives >= 2 blocks per CU (the detector
    // replaces this guess by a measured choice, st_detector_autotune)
    static const int order[] = {0, 5, 6, 3, 4};
    long long best_blocks = -1;
    for (int id : order) {
      if (!conv_variant_valid(id, d.Cout)) continue;
      const long long blocks = (long long)ceil_div(a.M, kVariants[id].bm) * (cout_pad / kVariants[id].bn);
      if (blocks >= 512) { pick = id; break; }
      if (blocks > best_blocks) { best_blocks = blocks; pick = id; }
    }
  }
  const ConvVariant& v = kVariants[pick];
  if (picked_variant) *picked_variant = pick;
  a.n_tiles = cout_pad / v.bn;
  const int m_tiles = ceil_div(a.M, v.bm);
  ST_REQUIRE(force_variant < 100, "conv: no such instance %d", force_variant);
  // pointwise layers run the PW instance of the picked tile variant (same tiles, shorter address code)
  const bool pw = d.KH == 1 && d.KW == 1 && d.stride == 1 && d.pad == 0;
  switch (pick) {
    case 0: return pw ? launch_variant<2, 2, 2, 2, 2, 1, 0, 1>(a, m_tiles, stream) : launch_variant<2, 2, 2, 2, 2, 1, 0, 0>(a, m_tiles, stream);
    case 1: return pw ? launch_variant<2, 2, 2, 1, 2, 1, 0, 1>(a, m_tiles, stream) : launch_variant<2, 2, 2, 1, 2, 1, 0, 0>(a, m_tiles, stream);
    case 2: return pw ? launch_variant<2, 1, 2, 1, 2, 1, 0, 1>(a, m_tiles, stream) : launch_variant<2, 1, 2, 1, 2, 1, 0, 0>(a, m_tiles, stream);
    case 3: return pw ? launch_variant<1, 1, 2, 2, 2, 1, 0, 1>(a, m_tiles, stream) : launch_variant<1, 1, 2, 2, 2, 1, 0, 0>(a, m_tiles, stream);
    case 4: return pw ? launch_variant<1, 1, 2, 1, 2, 1, 0, 1>(a, m_tiles, stream) : launch_variant<1, 1, 2, 1, 2, 1, 0, 0>(a, m_tiles, stream);
    case 5: return pw ? launch_variant<1, 2, 4, 1, 2, 1, 0, 1>(a, m_tiles, stream) : launch_variant<1, 2, 4, 1, 2, 1, 0, 0>(a, m_tiles, stream);
    case 6: return pw ? launch_variant<1, 1, 4, 1, 2, 1, 0, 1>(a, m_tiles, stream) : launch_variant<1, 1, 4, 1, 2, 1, 0, 0>(a, m_tiles, stream);
    case 7: return pw ? launch_variant<1, 2, 2, 2, 2, 1, 0, 1>(a, m_tiles, stream) : launch_variant<1, 2, 2, 2, 2, 1, 0, 0>(a, m_tiles, stream);
    case 8: return pw ? launch_variant<2, 2, 4, 1, 2, 1, 0, 1>(a, m_tiles, stream) : launch_variant<2, 2, 4, 1, 2, 1, 0, 0>(a, m_tiles, stream);
    case 9: return pw ? launch_variant<2, 2, 1, 1, 1, 1, 0, 1>(a, m_tiles, stream) : launch_variant<2, 2, 1, 1, 1, 1, 0, 0>(a, m_tiles, stream);
    case 10: return pw ? launch_variant<2, 1, 1, 1, 1, 1, 0, 1>(a, m_tiles, stream) : launch_variant<2, 1, 1, 1, 1, 1, 0, 0>(a, m_tiles, stream);
    case 11: return pw ? launch_variant<1, 2, 1, 1, 1, 1, 0, 1>(a, m_tiles, stream) : launch_variant<1, 2, 1, 1, 1, 1, 0, 0>(a, m_tiles, stream);
    case 12: return pw ? launch_variant<2, 2, 2, 2, 2, 1, 1, 1>(a, m_tiles, stream) : launch_variant<2, 2, 2, 2, 2, 1, 1, 0>(a, m_tiles, stream);
    case 13: return pw ? launch_variant<1, 1, 2, 2, 2, 1, 1, 1>(a, m_tiles, stream) : launch_variant<1, 1, 2, 2, 2, 1, 1, 0>(a, m_tiles, stream);
    case 14: return pw ? launch_variant<1, 2, 2, 2, 2, 1, 1, 1>(a, m_tiles, stream) : launch_variant<1, 2, 2, 2, 2, 1, 1, 0>(a, m_tiles, stream);
    case 15: return pw ? launch_variant<1, 1, 4, 1, 2, 1, 1, 1>(a, m_tiles, stream) : launch_variant<1, 1, 4, 1, 2, 1, 1, 0>(a, m_tiles, stream);
    case 16: return pw ? launch_variant<1, 2, 4, 1, 2, 1, 1, 1>(a, m_tiles, stream) : launch_variant<1, 2, 4, 1, 2, 1, 1, 0>(a, m_tiles, stream);
    case 17: return pw ? launch_variant<2, 2, 2, 2, 2, 0, 1, 1>(a, m_tiles, stream) : launch_variant<2, 2, 2, 2, 2, 0, 1, 0>(a, m_tiles, stream);
    case 18: return pw ? launch_variant<1, 1, 2, 2, 2, 0, 1, 1>(a, m_tiles, stream) : launch_variant<1, 1, 2, 2, 2, 0, 1, 0>(a, m_tiles, stream);
    case 19: return pw ? launch_variant<2, 2, 4, 2, 2, 1, 1, 1>(a, m_tiles, stream) : launch_variant<2, 2, 4, 2, 2, 1, 1, 0>(a, m_tiles, stream);
    case 20: return pw ? launch_variant<2, 2, 4, 2, 2, 0, 1, 1>(a, m_tiles, stream) : launch_variant<2, 2, 4, 2, 2, 0, 1, 0>(a, m_tiles, stream);
    case 21: return pw ? launch_variant<2, 2, 4, 2, 2, 1, 0, 1>(a, m_tiles, stream) : launch_variant<2, 2, 4, 2, 2, 1, 0, 0>(a, m_tiles, stream);
#ifdef ST_ABLATION
    case 22: return launch_ws<2, 2, 2, 2>(a, m_tiles, stream);
    case 23: return launch_ws<1, 1, 2, 2>(a, m_tiles, stream);
    case 24: return launch_ws<1, 2, 2, 2>(a, m_tiles, stream);
    case 25: return launch_ws<1, 1, 4, 1>(a, m_tiles, stream);
    case 26: return launch_ws<1, 2, 4, 1>(a, m_tiles, stream);
    case 27: return launch_ws<2, 2, 2, 2, 2>(a, m_tiles, stream);
    case 28: return launch_ws<1, 2, 2, 2, 2>(a, m_tiles, stream);
    case 29: return launch_ws<2, 2, 2, 2, 4>(a, m_tiles, stream);
#endif
    default: return set_error(ST_ERR_INVALID, "conv: unknown tile variant %d", pick);
  }
}

}  // namespace st

extern "C" int st_conv2d_nhwc(const StConvDesc* d, st_stream_t stream) {
  if (!d) return st::set_error(ST_ERR_INVALID, "st_conv2d_nhwc: null desc");
  return st::conv2d_launch(*d, static_cast<hipStream_t>(stream), -1, nullptr);
}

// Fused pair of 1x1 convs on the streaming kernel: `b` consumes output channels [0, 32) of `a` (the CSP
// main_conv -> bottleneck conv1 pair) straight from registers; a's own outputs are still written.
extern "C" int st_conv1x1_chain(const StConvDesc* a, const StConvDesc* b, st_stream_t stream) {
  if (!a || !b) return st::set_error(ST_ERR_INVALID, "st_conv1x1_chain: null desc");
  if (st::pwr_chain_applicable(*a, *b)) return st::pwr_conv_launch(*a, static_cast<hipStream_t>(stream), b);
  return st::pw_conv_launch(*a, static_cast<hipStream_t>(stream), b);
}

// The same convolution with the tile variant chosen by the caller (include/stereotrack.h: ids 0..21 = tile
// instances of conv_igemm_kernel, 41 = streaming 1x1 kernel, 42 = direct 3x3 kernel, -1 = library heuristic);
// how callers that autotune per layer (StereoCostVolume.autotune) apply their choice.
extern "C" int st_conv2d_nhwc_variant(const StConvDesc* d, st_stream_t stream, int variant) {
  if (!d) return st::set_error(ST_ERR_INVALID, "st_conv2d_nhwc_variant: null desc");
  return st::conv2d_launch(*d, static_cast<hipStream_t>(stream), variant, nullptr);
}
