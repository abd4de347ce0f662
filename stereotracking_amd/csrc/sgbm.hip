// OpenCV StereoSGBM, mode SGBM_3WAY, on the device: uint8 stereo pairs -> the disparity map the detector's disparity
// branch was trained on (reference reproducibility.md section 3: the AirDrone PNGs are StereoSGBM results).
//
// OpenCV is absent: every rule is restated from OpenCV 4.x stereosgbm.cpp [upstream-memory], PARITY UNPINNED against
// cv2 itself.  tests/sgbm_ref.py restates the same rules in numpy (its header lists them, with the uncertain ones) and
// tests/test_sgbm_gpu.py holds these kernels to it bit for bit: every stage is integer arithmetic.
//
//   prefilter  per pair, image and channel: x-Sobel clipped to [-ftzero, ftzero] + ftzero, rows replicated, columns 0 and
//              w-1 = ftzero in the prefiltered AND the raw-intensity rows; packed per pixel with the min / max of its
//              half-sample envelope (value | min << 8 | max << 16), planar [n][image][2 cn][h][w] u32.
//   levels     D in {16, 32, 48, 64}: one level per lane (K = 1, the lanes >= D idle).  D in {128, 192, 256}: K = D / 64
//              levels per lane, all 64 lanes busy, BLOCKED: lane l holds d = K l + k, k = 0..K-1, in register k.  So d
//              ascends with (lane, k) in lexicographic order, d +- 1 is the neighbour register except at k = 0 / K - 1
//              (one __shfl_up of register K - 1, one __shfl_down of register 0, whatever K), and the K int16 levels of a
//              lane are 2 K contiguous bytes of the (.., d) volumes, whose layout does not depend on K.
//   tb         one wave per (pair, column x in [D, w)), walking the rows: Birchfield-Tomasi cost
//              of left x against right x - d (cn prefiltered channels + cn raw channels >> 2), the horizontal box sum
//              (columns clamped to [D, w)), a rolling vertical sum over a ring of the last block_size row sums (rows
//              clamped), and the top->bottom path.  Writes C and L_tb (int16, [n][y][x - D][d]).
//   rows       one wave per (pair, row): left->right path, S1 = L_lr + L_tb in place; right->left path, S = S1 + L_rl,
//              then per x (descending) the min (in-lane over k, then across the wave), the argmin (one ballot per
//              register k: its first set lane l gives the candidate K l + k, the lowest candidate wins = the lowest d
//              of the tied minima), uniqueness as a ballot of a per-level test, subpixel from S[best -+ 1] (register
//              (best -+ 1) % K of lane (best -+ 1) / K), and the disp2 scatter in LDS (strict test in descending x =
//              ties to the highest x); then the left-right check from LDS.  -> int16 map (-16 invalid, x < D invalid).
//   median     3 x 3 median, replicated borders.
//   speckle    union-find over the 4-neighbour graph (edges where |a - b| <= maxDiff, pixels != -16): lock-free link of
//              the larger root under the smaller by atomicCAS (parents only ever decrease, so every chain ends), every
//              find / retry loop bounded by the pair's pixel count; a loop that reaches its bound sets a bit of the
//              status word instead of spinning.  Sizes by atomicAdd at the roots, then relabel fused with the pack to
//              disp_postp (N, 3, H, W) = max(d16, 0) / 16, 0 in the padding.
#include <climits>
#include <cstdint>

#include "st_common.h"

namespace {

constexpr int kInvalid = -16;
constexpr int kMaxFrames = 32;
constexpr int kMaxBlock = 9;      // the int16 bound admits block_size <= 9 (cn 1, ftzero 15)
constexpr int kMaxWidth = 4096;   // LDS of the row pass: 8 bytes per column
constexpr int kBig = 1 << 28;
constexpr int kTbWaves = 4;

struct FramePtrs { const unsigned char* p[kMaxFrames]; };

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

// ---- prefilter ------------------------------------------------------------------------------------------------------
// source pixel (0..255) of channel c (or the fixed-point BGR2GRAY of the three, cn == 1) at (y, x) of the h x w crop
struct SrcU8 {
  const unsigned char* f;
  int fh, fw;
  __device__ int px(int c, int y, int x) const { return f[((long long)c * fh + y) * fw + x]; }
};
struct SrcF32 {
  const float* f;
  int H, W;
  __device__ int px(int c, int y, int x) const {
    const int v = (int)f[((long long)c * H + y) * W + x];   // integral values; the uint8 cast of the batch
    return min(max(v, 0), 255);
  }
};

template <typename Src>
__device__ __forceinline__ int src_val(const Src& s, int cn, int c, int y, int x) {
  if (cn == 3) return s.px(c, y, x);
  // BGR batch: channel 2 = R
  return (s.px(2, y, x) * 9798 + s.px(1, y, x) * 19235 + s.px(0, y, x) * 3735 + (1 << 14)) >> 15;
}

// value of row c2 (< cn: prefiltered, else raw intensity) at (y, x)
template <typename Src>
__device__ __forceinline__ int pf_val(const Src& s, int cn, int c2, int y, int x, int h, int w, int ftzero) {
  if (x == 0 || x == w - 1) return ftzero;
  const int c = c2 < cn ? c2 : c2 - cn;
  if (c2 >= cn) return src_val(s, cn, c, y, x);
  const int ym = max(y - 1, 0), yp = min(y + 1, h - 1);
  const int sob = 2 * (src_val(s, cn, c, y, x + 1) - src_val(s, cn, c, y, x - 1)) +
                  (src_val(s, cn, c, ym, x + 1) - src_val(s, cn, c, ym, x - 1)) +
                  (src_val(s, cn, c, yp, x + 1) - src_val(s, cn, c, yp, x - 1));
  return min(max(sob, -ftzero), ftzero) + ftzero;
}

template <typename Src>
__device__ void prefilter_body(const Src& s, int cn, int h, int w, int ftzero, uint32_t* out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= w) return;
  for (int c2 = 0; c2 < 2 * cn; ++c2) {
    const int u = pf_val(s, cn, c2, y, x, h, w, ftzero);
    const int ul = x > 0 ? (u + pf_val(s, cn, c2, y, x - 1, h, w, ftzero)) / 2 : u;
    const int ur = x < w - 1 ? (u + pf_val(s, cn, c2, y, x + 1, h, w, ftzero)) / 2 : u;
    const int lo = min(u, min(ul, ur)), hi = max(u, max(ul, ur));
    out[((long long)c2 * h + y) * w + x] = (uint32_t)u | ((uint32_t)lo << 8) | ((uint32_t)hi << 16);
  }
}

// grid (ceil(w / 256), h, 2 * frames): z = 2 * pair + image (0 left, 1 right)
__global__ void __launch_bounds__(256) sgbm_prefilter_u8_kernel(FramePtrs L, FramePtrs R, int base, int fh, int fw,
                                                                int cn, int h, int w, int ftzero, uint32_t* pf) {
  const int k = blockIdx.z >> 1, img = blockIdx.z & 1;
  const SrcU8 s{img ? R.p[k] : L.p[k], fh, fw};
  prefilter_body(s, cn, h, w, ftzero, pf + ((long long)(base + k) * 2 + img) * 2 * cn * h * w);
}

__global__ void __launch_bounds__(256) sgbm_prefilter_f32_kernel(const float* left, const float* right, int H, int W,
                                                                 int cn, int h, int w, int ftzero, uint32_t* pf) {
  const int n = blockIdx.z >> 1, img = blockIdx.z & 1;
  const SrcF32 s{(img ? right : left) + (long long)n * 3 * H * W, H, W};
  prefilter_body(s, cn, h, w, ftzero, pf + ((long long)n * 2 + img) * 2 * cn * h * w);
}

// ---- cost + top->bottom path ------------------------------------------------------------------------------------------
struct SgbmGeom {
  int h, w, D, cn, r, P1, P2;
};

// the K int16 levels of one lane, d = K lane + k: 2 K contiguous bytes at p[i], moved as one word where they are
// aligned (4-byte for K = 2, 8-byte for K = 4: D is a multiple of 64 there and the volumes start 256-byte aligned)
struct Levels3 { int a, b, c; };
template <int K> struct LevelsOf;
template <> struct LevelsOf<2> { using type = uint32_t; };
template <> struct LevelsOf<3> { using type = Levels3; };
template <> struct LevelsOf<4> { using type = uint2; };
template <int K> using Levels = typename LevelsOf<K>::type;

// as loaded, 0 where !ok
template <int K>
__device__ __forceinline__ Levels<K> load_levels(bool ok, const int16_t* p, long long i) {
  if constexpr (K == 2) {
    return ok ? *reinterpret_cast<const uint32_t*>(p + i) : 0u;
  } else if constexpr (K == 3) {
    return ok ? Levels3{p[i], p[i + 1], p[i + 2]} : Levels3{0, 0, 0};
  } else {
    return ok ? *reinterpret_cast<const uint2*>(p + i) : make_uint2(0u, 0u);
  }
}

template <int K>
__device__ __forceinline__ void unpack_levels(const Levels<K>& l, int (&v)[K]) {
  if constexpr (K == 2) {
    v[0] = (int16_t)(l & 0xffff);
    v[1] = (int)l >> 16;
  } else if constexpr (K == 3) {
    v[0] = l.a;
    v[1] = l.b;
    v[2] = l.c;
  } else {
    v[0] = (int16_t)(l.x & 0xffff);
    v[1] = (int)l.x >> 16;
    v[2] = (int16_t)(l.y & 0xffff);
    v[3] = (int)l.y >> 16;
  }
}

template <int K>
__device__ __forceinline__ void store_levels(int16_t* p, const int (&v)[K]) {
  if constexpr (K == 2) {
    *reinterpret_cast<uint32_t*>(p) = (uint32_t)(v[0] & 0xffff) | ((uint32_t)v[1] << 16);
  } else if constexpr (K == 4) {
    *reinterpret_cast<uint2*>(p) = make_uint2((uint32_t)(v[0] & 0xffff) | ((uint32_t)v[1] << 16),
                                              (uint32_t)(v[2] & 0xffff) | ((uint32_t)v[3] << 16));
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) p[k] = (int16_t)v[k];
  }
}

// one step of a path (rule 4) for the K levels of a lane: Lp = L(p - r), c = C(p); m = min over all levels of Lp.
// L(d - 1) of register 0 is register K - 1 of the lane below, L(d + 1) of register K - 1 is register 0 of the lane above;
// beyond d = 0 and d = D - 1 there is kBig.
template <int K>
__device__ __forceinline__ void path_step(const int (&c)[K], const int (&Lp)[K], int m, int lane, int D, int P1, int P2,
                                          int (&L)[K]) {
  const int below = __shfl_up(Lp[K - 1], 1), above = __shfl_down(Lp[0], 1);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int lm = k > 0 ? Lp[k > 0 ? k - 1 : 0] : (lane > 0 ? below : kBig);
    const int lp = k < K - 1 ? Lp[k < K - 1 ? k + 1 : 0] : (K * lane + K < D ? above : kBig);
    L[k] = c[k] + min(min(Lp[k], min(lm, lp) + P1), m + P2) - m;
  }
}

template <int K>
__device__ __forceinline__ int lane_min(const int (&v)[K]) {
  int lo = v[0];
#pragma unroll
  for (int k = 1; k < K; ++k) lo = min(lo, v[k]);
  return lo;
}

// horizontal box sums of the BT cost at row y, column x, levels d0 .. d0 + K - 1 (columns clamped to [D, w))
template <int CN2, int K>
__device__ __forceinline__ void hsum_bt(const uint32_t* pl, const uint32_t* pr, const SgbmGeom& g, int y, int x, int d0,
                                        int (&s)[K]) {
  const long long plane = (long long)g.h * g.w;
  const long long row = (long long)y * g.w;
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0;
  for (int dx = -g.r; dx <= g.r; ++dx) {
    const int xx = min(max(x + dx, g.D), g.w - 1);
#pragma unroll
    for (int c2 = 0; c2 < CN2; ++c2) {
      const uint32_t a = pl[c2 * plane + row + xx];
      const int u = a & 255, u0 = (a >> 8) & 255, u1 = a >> 16;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const uint32_t b = pr[c2 * plane + row + xx - d0 - k];
        const int v = b & 255, v0 = (b >> 8) & 255, v1 = b >> 16;
        int c = min(max(max(0, u - v1), v0 - u), max(max(0, v - u1), u0 - v));
        if (c2 >= CN2 / 2) c >>= 2;
        s[k] += c;
      }
    }
  }
}

// grid (ceil((w - D) / kTbWaves), N), block 64 * kTbWaves; K levels per lane (D <= 64: K = 1, else D = 64 K)
template <int CN2, int K>
__global__ void __launch_bounds__(64 * kTbWaves) sgbm_tb_kernel(const uint32_t* pf, SgbmGeom g, int16_t* cost,
                                                               int16_t* ltb) {
  __shared__ int ring[kTbWaves][kMaxBlock][64 * K];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = blockIdx.y, x = g.D + blockIdx.x * kTbWaves + wv;
  if (x >= g.w) return;                       // whole waves only; no barrier below
  const int wp = g.w - g.D, bs = 2 * g.r + 1;
  const bool act = K > 1 || lane < g.D;
  const int d0 = act ? K * lane : g.D - 1;    // idle lanes read a valid column, their values are discarded
  const long long plane = (long long)g.h * g.w;
  const uint32_t* pl = pf + (long long)n * 2 * CN2 * plane;
  const uint32_t* pr = pl + CN2 * plane;
  int* rg = ring[wv][0] + lane;               // slot s, register k at rg[64 (K s + k)], private to this lane
  // window of row 0: rows -r..r clamped
  int V[K], hn[K];
#pragma unroll
  for (int k = 0; k < K; ++k) V[k] = 0;
  for (int j = -g.r; j <= g.r; ++j) {
    hsum_bt<CN2, K>(pl, pr, g, min(max(j, 0), g.h - 1), x, d0, hn);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      rg[64 * (K * (j + g.r) + k)] = hn[k];
      V[k] += hn[k];
    }
  }
  int Lp[K];
#pragma unroll
  for (int k = 0; k < K; ++k) Lp[k] = 0;
  int slot = 0;                               // slot of row y - r - 1 (leaving) = slot of row y + r (entering)
  for (int y = 0; y < g.h; ++y) {
    if (y > 0) {
      hsum_bt<CN2, K>(pl, pr, g, min(y + g.r, g.h - 1), x, d0, hn);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        V[k] += hn[k] - rg[64 * (K * slot + k)];
        rg[64 * (K * slot + k)] = hn[k];
      }
      slot = slot + 1 == bs ? 0 : slot + 1;
    }
    int L[K];
    if (y == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) L[k] = V[k];
    } else {
      const int m = wave_min(act ? lane_min<K>(Lp) : kBig);
      path_step<K>(V, Lp, m, lane, g.D, g.P1, g.P2, L);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) Lp[k] = L[k];
    if (act) {
      const long long o = (((long long)n * g.h + y) * wp + (x - g.D)) * g.D + K * lane;
      store_levels<K>(cost + o, V);
      store_levels<K>(ltb + o, Lp);
    }
  }
}

// ---- horizontal paths, decision, left-right check ----------------------------------------------------------------------
// S at level d, for every lane: the lane that holds d selects its register by comparing its own levels with d (no
// indexed register file: a wave-uniform index into v[] would go through scratch), then the wave reads that lane
template <int K>
__device__ __forceinline__ int level_of(const int (&v)[K], int lane, int d) {
  int mine = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) mine = K * lane + k == d ? v[k] : mine;
  return __shfl(mine, d / K);
}

// K = 2, 3, 4 levels per lane (D = 64 K, every lane busy): grid (h, N), block 64, dynamic LDS 8 w bytes
template <int K>
__global__ void __launch_bounds__(64) sgbm_rows_kernel(const int16_t* cost, int16_t* s1, SgbmGeom g, int uniq,
                                                       int lr_tol, int16_t* disp_out) {
  static_assert(K >= 2 && K <= 4, "K = 1 is the specialisation below");
  extern __shared__ int lds[];
  int* d2cost = lds;
  int16_t* disp1 = reinterpret_cast<int16_t*>(lds + g.w);
  int16_t* disp2 = disp1 + g.w;
  const int lane = threadIdx.x, y = blockIdx.x, n = blockIdx.y;
  const int D = g.D, w = g.w, wp = w - D;
  for (int x = lane; x < w; x += 64) {
    d2cost[x] = INT_MAX;
    disp1[x] = (int16_t)kInvalid;
    disp2[x] = (int16_t)-1;
  }
  __syncthreads();
  const long long base = ((long long)n * g.h + y) * wp * D + K * lane;
  // as for K = 1, C and S1 are loaded kChunk columns ahead of the serial recursion; the 3- and 4-level lanes take half
  // the chunk (about the same registers, more work per step to cover the latency)
  constexpr int kChunk = 8;
  auto step = [&](const Levels<K>& cl, int (&Lp)[K], bool first) {
    int c[K], L[K];
    unpack_levels<K>(cl, c);
    if (first) {                                      // wave-uniform: L = C at the start of a path
#pragma unroll
      for (int k = 0; k < K; ++k) L[k] = c[k];
    } else {
      path_step<K>(c, Lp, wave_min(lane_min<K>(Lp)), lane, D, g.P1, g.P2, L);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) Lp[k] = L[k];
  };
  // left -> right: S1 = L_lr + L_tb
  int Lp[K];
  for (int x0 = 0; x0 < wp; x0 += kChunk) {
    Levels<K> cc[kChunk], ss[kChunk];
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const int xi = x0 + k;
      cc[k] = load_levels<K>(xi < wp, cost, base + (long long)xi * D);
      ss[k] = load_levels<K>(xi < wp, s1, base + (long long)xi * D);
    }
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const int xi = x0 + k;
      if (xi >= wp) break;
      step(cc[k], Lp, xi == 0);
      int S1[K];
      unpack_levels<K>(ss[k], S1);
#pragma unroll
      for (int j = 0; j < K; ++j) S1[j] += Lp[j];
      store_levels<K>(s1 + base + (long long)xi * D, S1);
    }
  }
  // right -> left: S = S1 + L_rl, decision per x
  for (int x0 = wp - 1; x0 >= 0; x0 -= kChunk) {
    Levels<K> cc[kChunk], ss[kChunk];
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const int xi = x0 - k;
      cc[k] = load_levels<K>(xi >= 0, cost, base + (long long)xi * D);
      ss[k] = load_levels<K>(xi >= 0, s1, base + (long long)xi * D);
    }
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const int xi = x0 - k;
      if (xi < 0) break;
      step(cc[k], Lp, xi == wp - 1);
      int S[K];
      unpack_levels<K>(ss[k], S);
#pragma unroll
      for (int j = 0; j < K; ++j) S[j] += Lp[j];
      const int minS = wave_min(lane_min<K>(S));
      // the lowest d of the tied minima: the first lane l of register j's ballot holds that register's lowest tied
      // level K l + j, and the lowest of the K candidates is the lowest tied level of all
      int best = INT_MAX;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const unsigned long long at = __ballot(S[j] == minS);
        if (at) best = min(best, K * (__ffsll(at) - 1) + j);
      }
      bool unique = true;
      if (uniq > 0) {
        const int thresh = (100 * minS) / (100 - uniq);
        bool rival = false;                           // per level, not per lane
#pragma unroll
        for (int j = 0; j < K; ++j) rival |= S[j] <= thresh && abs(K * lane + j - best) > 1;
        unique = __ballot(rival) == 0ull;
      }
      if (unique) {                                   // wave-uniform
        const int sm = level_of<K>(S, lane, max(best - 1, 0)), sp = level_of<K>(S, lane, min(best + 1, D - 1));
        int d16 = 16 * best;
        if (best > 0 && best < D - 1) {
          const int denom2 = max(sm + sp - 2 * minS, 1);
          d16 += ((sm - sp) * 16 + denom2) / (2 * denom2);   // C division: truncation toward zero
        }
        if (lane == 0) {
          const int x = xi + D, x2 = x - best;
          disp1[x] = (int16_t)d16;
          if (minS < d2cost[x2]) {
            d2cost[x2] = minS;
            disp2[x2] = (int16_t)best;
          }
        }
      }
    }
  }
  __syncthreads();
  int16_t* out = disp_out + ((long long)n * g.h + y) * w;
  for (int x = lane; x < w; x += 64) {
    int d1 = disp1[x];
    if (d1 != kInvalid) {
      const int fl = d1 >> 4, ce = (d1 + 15) >> 4;
      const int xa = x - fl, xb = x - ce;
      if (xa >= 0 && xa < w && disp2[xa] >= 0 && abs(disp2[xa] - fl) > lr_tol && xb >= 0 && xb < w &&
          disp2[xb] >= 0 && abs(disp2[xb] - ce) > lr_tol)
        d1 = kInvalid;
    }
    out[x] = (int16_t)d1;
  }
}

// One level per lane (D <= 64, the lanes >= D idle): grid (h, N), block 64, dynamic LDS 8 w bytes
template <>
__global__ void __launch_bounds__(64) sgbm_rows_kernel<1>(const int16_t* cost, int16_t* s1, SgbmGeom g, int uniq,
                                                       int lr_tol, int16_t* disp_out) {
  extern __shared__ int lds[];
  int* d2cost = lds;
  int16_t* disp1 = reinterpret_cast<int16_t*>(lds + g.w);
  int16_t* disp2 = disp1 + g.w;
  const int lane = threadIdx.x, y = blockIdx.x, n = blockIdx.y;
  const int D = g.D, w = g.w, wp = w - D;
  const bool act = lane < D;
  for (int x = lane; x < w; x += 64) {
    d2cost[x] = INT_MAX;
    disp1[x] = (int16_t)kInvalid;
    disp2[x] = (int16_t)-1;
  }
  __syncthreads();
  const long long base = ((long long)n * g.h + y) * wp * D + lane;
  // the path recursions are serial in x: C and S1 are loaded kChunk columns at a time so that one memory latency
  // covers kChunk steps
  constexpr int kChunk = 16;
  auto step = [&](int c, int& Lp, bool first) {
    if (first) return act ? c : kBig;
    const int m = wave_min(Lp);
    const int lm = __shfl_up(Lp, 1), lp = __shfl_down(Lp, 1);
    const int nb = min(lane > 0 ? lm : kBig, lane + 1 < D ? lp : kBig);
    return act ? c + min(min(Lp, nb + g.P1), m + g.P2) - m : kBig;
  };
  // left -> right: S1 = L_lr + L_tb
  int Lp = kBig;
  for (int x0 = 0; x0 < wp; x0 += kChunk) {
    int cc[kChunk], ss[kChunk];
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const int xi = x0 + k;
      cc[k] = act && xi < wp ? cost[base + (long long)xi * D] : 0;
      ss[k] = act && xi < wp ? s1[base + (long long)xi * D] : 0;
    }
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const int xi = x0 + k;
      if (xi >= wp) break;
      Lp = step(cc[k], Lp, xi == 0);
      if (act) s1[base + (long long)xi * D] = (int16_t)(ss[k] + Lp);
    }
  }
  // right -> left: S = S1 + L_rl, decision per x
  Lp = kBig;
  for (int x0 = wp - 1; x0 >= 0; x0 -= kChunk) {
    int cc[kChunk], ss[kChunk];
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const int xi = x0 - k;
      cc[k] = act && xi >= 0 ? cost[base + (long long)xi * D] : 0;
      ss[k] = act && xi >= 0 ? s1[base + (long long)xi * D] : 0;
    }
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const int xi = x0 - k;
      if (xi < 0) break;
      Lp = step(cc[k], Lp, xi == wp - 1);
      const int S = act ? ss[k] + Lp : kBig;
      const int minS = wave_min(S);
      const unsigned long long at = __ballot(S == minS);
      const int best = __ffsll(at) - 1;
      bool unique = true;
      if (uniq > 0) {
        const int thresh = (100 * minS) / (100 - uniq);
        unique = __ballot(act && S <= thresh && abs(lane - best) > 1) == 0ull;
      }
      if (unique) {                                   // wave-uniform
        const int sm = __shfl(S, max(best - 1, 0)), sp = __shfl(S, min(best + 1, D - 1));
        int d16 = 16 * best;
        if (best > 0 && best < D - 1) {
          const int denom2 = max(sm + sp - 2 * minS, 1);
          d16 += ((sm - sp) * 16 + denom2) / (2 * denom2);   // C division: truncation toward zero
        }
        if (lane == 0) {
          const int x = xi + D, x2 = x - best;
          disp1[x] = (int16_t)d16;
          if (minS < d2cost[x2]) {
            d2cost[x2] = minS;
            disp2[x2] = (int16_t)best;
          }
        }
      }
    }
  }
  __syncthreads();
  int16_t* out = disp_out + ((long long)n * g.h + y) * w;
  for (int x = lane; x < w; x += 64) {
    int d1 = disp1[x];
    if (d1 != kInvalid) {
      const int fl = d1 >> 4, ce = (d1 + 15) >> 4;
      const int xa = x - fl, xb = x - ce;
      if (xa >= 0 && xa < w && disp2[xa] >= 0 && abs(disp2[xa] - fl) > lr_tol && xb >= 0 && xb < w &&
          disp2[xb] >= 0 && abs(disp2[xb] - ce) > lr_tol)
        d1 = kInvalid;
    }
    out[x] = (int16_t)d1;
  }
}

// ---- median 3 x 3 -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sgbm_median_kernel(const int16_t* in, int h, int w, int16_t* out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
  if (x >= w) return;
  const int16_t* p = in + (long long)n * h * w;
  int v[9];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int yy = min(max(y + dy - 1, 0), h - 1), xx = min(max(x + dx - 1, 0), w - 1);
      v[dy * 3 + dx] = p[(long long)yy * w + xx];
    }
#pragma unroll
  for (int i = 1; i < 9; ++i)
#pragma unroll
    for (int j = i; j > 0; --j) {
      const int a = min(v[j - 1], v[j]), b = max(v[j - 1], v[j]);
      v[j - 1] = a;
      v[j] = b;
    }
  out[(long long)n * h * w + (long long)y * w + x] = (int16_t)v[4];
}

// ---- speckle filter ------------------------------------------------------------------------------------------------------
// parent / size indices are global over the N maps (no edge crosses two maps); -1 = a pixel equal to newVal
__device__ __forceinline__ int uf_find(const int* parent, int i, int bound, int* status) {
  const volatile int* par = parent;
  for (int k = 0; k < bound; ++k) {
    const int p = par[i];
    if (p == i) return i;
    i = p;
  }
  atomicOr(status, 1);
  return i;
}

__global__ void __launch_bounds__(256) sgbm_uf_init_kernel(const int16_t* disp, long long total, int* parent, int* size) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  parent[i] = disp[i] != kInvalid ? (int)i : -1;
  size[i] = 0;
}

__global__ void __launch_bounds__(256) sgbm_uf_union_kernel(const int16_t* disp, int h, int w, int max_diff,
                                                            int* parent, int* status) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
  if (x >= w) return;
  const int hw = h * w;
  const int i = n * hw + y * w + x;
  const int v = disp[i];
  if (v == kInvalid) return;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    if (e == 0 ? x + 1 >= w : y + 1 >= h) continue;
    const int j = e == 0 ? i + 1 : i + w;
    const int u = disp[j];
    if (u == kInvalid || abs(u - v) > max_diff) continue;
    int a = i, b = j, k = 0;
    for (; k < hw; ++k) {
      a = uf_find(parent, a, hw, status);
      b = uf_find(parent, b, hw, status);
      if (a == b) break;
      if (a > b) { const int t = a; a = b; b = t; }
      if (atomicCAS(&parent[b], b, a) == b) break;   // link the larger root under the smaller
    }
    if (k == hw) atomicOr(status, 2);
  }
}

__global__ void __launch_bounds__(256) sgbm_uf_count_kernel(long long total, int hw, int* parent, int* size,
                                                            int* status) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total || parent[i] < 0) return;
  const int r = uf_find(parent, (int)i, hw, status);
  atomicAdd(&size[r], 1);
}

// relabel + pack: grid (ceil(W / 256), H, N)
__global__ void __launch_bounds__(256) sgbm_pack_kernel(const int16_t* disp, const int* parent, const int* size, int h,
                                                        int w, int max_size, int H, int W, int* status,
                                                        int16_t* final_out, float* postp) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y, n = blockIdx.z;
  if (X >= W) return;
  float o = 0.f;
  if (Y < h && X < w) {
    const int i = n * h * w + Y * w + X;
    int v = disp[i];
    if (v != kInvalid && parent && size[uf_find(parent, i, h * w, status)] <= max_size) v = kInvalid;
    if (final_out) final_out[i] = (int16_t)v;
    o = (float)max(v, 0) * (1.f / 16.f);
  }
  if (postp) {
    const long long plane = (long long)H * W;
    float* p = postp + (long long)n * 3 * plane + (long long)Y * W + X;
    p[0] = o;
    p[plane] = o;
    p[2 * plane] = o;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
size_t align256(size_t b) { return (b + 255) / 256 * 256; }

struct Layout {
  size_t pf, cost, s1, raw, med, parent, size, status, total;
};

Layout layout(int N, int h, int w, int D) {
  Layout L{};
  const size_t px = (size_t)N * h * w, cells = (size_t)N * h * (w - D) * D;
  size_t o = 0;
  L.pf = o;     o += align256(px * 2 * 6 * sizeof(uint32_t));
  L.cost = o;   o += align256(cells * sizeof(int16_t));
  L.s1 = o;     o += align256(cells * sizeof(int16_t));
  L.raw = o;    o += align256(px * sizeof(int16_t));
  L.med = o;    o += align256(px * sizeof(int16_t));
  L.parent = o; o += align256(px * sizeof(int));
  L.size = o;   o += align256(px * sizeof(int));
  L.status = o; o += 256;
  L.total = o;
  return L;
}

template <typename T>
T* at(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<unsigned char*>(ws) + off); }

// every refusal of an entry point that depends on the parameters, the geometry or the workspace address: before any launch
int check_params(const StSgbmParams* p, int N, int h, int w, const void* ws, const char* who) {
  ST_REQUIRE(p && p->struct_size == (int)sizeof(StSgbmParams), "%s: params struct_size mismatch", who);
  const int D = p->num_disparities;
  ST_REQUIRE(D == 16 || D == 32 || D == 48 || D == 64 || D == 128 || D == 192 || D == 256,
             "%s: num_disparities %d must be 16, 32, 48, 64, 128, 192 or 256", who, D);
  ST_REQUIRE(h >= 1 && w > D && w <= kMaxWidth, "%s: image %d x %d: need num_disparities < w <= %d", who, h, w,
             kMaxWidth);
  ST_REQUIRE(p->block_size >= 1 && p->block_size % 2 == 1 && p->block_size <= kMaxBlock,
             "%s: block_size %d must be odd, 1..%d", who, p->block_size, kMaxBlock);
  ST_REQUIRE(p->pre_filter_cap >= 1 && p->pre_filter_cap <= 127, "%s: pre_filter_cap %d must be in 1..127", who,
             p->pre_filter_cap);
  ST_REQUIRE(p->P1 >= 0 && p->P2 >= 0 && p->uniqueness_ratio >= 0 && p->uniqueness_ratio < 100 &&
                 p->speckle_window_size >= 0 && p->speckle_range >= 0 && (p->color == 0 || p->color == 1),
             "%s: bad parameter", who);
  const long long ft = (p->pre_filter_cap > 15 ? p->pre_filter_cap : 15) | 1;
  const long long p2 = p->P2 > p->P1 + 1 ? p->P2 : p->P1 + 1, cn = p->color ? 3 : 1;
  const long long worst = 3 * ((long long)p->block_size * p->block_size * cn * (2 * ft + 63) + p2);
  ST_REQUIRE(worst <= 32767, "%s: worst-case aggregated cost %lld leaves int16", who, worst);
  // the cost volumes are indexed in 64 bits (8 pairs of 1600 x 576 at D = 256: 1.6e9 cells each); pixels in int
  ST_REQUIRE((long long)N * h * w < INT_MAX, "%s: %d maps of %d x %d exceed int indices", who, N, h, w);
  // 2 / 4 levels per lane move as one 4- / 8-byte word (the volumes sit at 256-byte offsets of ws)
  ST_REQUIRE(D <= 64 || reinterpret_cast<uintptr_t>(ws) % 8 == 0, "%s: workspace must be 8-byte aligned", who);
  return ST_OK;
}

SgbmGeom geom_of(const StSgbmParams* p, int h, int w) {
  return SgbmGeom{h, w, p->num_disparities, p->color ? 3 : 1, p->block_size / 2, p->P1,
                  p->P2 > p->P1 + 1 ? p->P2 : p->P1 + 1};
}

template <int K>
void launch_tb(const SgbmGeom& g, int N, const uint32_t* pf, int16_t* cost, int16_t* ltb, hipStream_t s) {
  const dim3 tb(st::ceil_div(g.w - g.D, kTbWaves), N);
  if (g.cn == 3)
    hipLaunchKernelGGL((sgbm_tb_kernel<6, K>), tb, dim3(64 * kTbWaves), 0, s, pf, g, cost, ltb);
  else
    hipLaunchKernelGGL((sgbm_tb_kernel<2, K>), tb, dim3(64 * kTbWaves), 0, s, pf, g, cost, ltb);
}

template <int K>
void launch_rows(const SgbmGeom& g, int N, const int16_t* cost, int16_t* s1, int uniq, int tol, int16_t* raw_out,
                 hipStream_t s) {
  hipLaunchKernelGGL(sgbm_rows_kernel<K>, dim3(g.h, N), dim3(64), (size_t)8 * g.w, s, cost, s1, g, uniq, tol, raw_out);
}

// prefiltered planes -> int16 map before the median (cost_out: optional copy of C)
int launch_match(const SgbmGeom& g, int N, const StSgbmParams* p, void* ws, const Layout& L, int16_t* cost_out,
                 int16_t* raw_out, hipStream_t s) {
  const uint32_t* pf = at<uint32_t>(ws, L.pf);
  int16_t* cost = at<int16_t>(ws, L.cost);
  int16_t* s1 = at<int16_t>(ws, L.s1);
  const int wp = g.w - g.D;
  const int K = g.D <= 64 ? 1 : g.D / 64;     // levels per lane (check_params admits whole 64-level slots only)
  switch (K) {
    case 1: launch_tb<1>(g, N, pf, cost, s1, s); break;
    case 2: launch_tb<2>(g, N, pf, cost, s1, s); break;
    case 3: launch_tb<3>(g, N, pf, cost, s1, s); break;
    default: launch_tb<4>(g, N, pf, cost, s1, s); break;
  }
  if (cost_out)
    ST_CHECK_HIP(hipMemcpyAsync(cost_out, cost, (size_t)N * g.h * wp * g.D * sizeof(int16_t),
                                hipMemcpyDeviceToDevice, s));
  if (raw_out) {
    const int tol = p->disp12_max_diff > 0 ? p->disp12_max_diff : 1;
    switch (K) {
      case 1: launch_rows<1>(g, N, cost, s1, p->uniqueness_ratio, tol, raw_out, s); break;
      case 2: launch_rows<2>(g, N, cost, s1, p->uniqueness_ratio, tol, raw_out, s); break;
      case 3: launch_rows<3>(g, N, cost, s1, p->uniqueness_ratio, tol, raw_out, s); break;
      default: launch_rows<4>(g, N, cost, s1, p->uniqueness_ratio, tol, raw_out, s); break;
    }
  }
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

int launch_median(const int16_t* in, int N, int h, int w, int16_t* out, hipStream_t s) {
  hipLaunchKernelGGL(sgbm_median_kernel, dim3(st::ceil_div(w, 256), h, N), dim3(256), 0, s, in, h, w, out);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

int launch_speckle(const int16_t* in, int N, int h, int w, int max_size, int max_diff, int* parent, int* size,
                   int* status, int16_t* final_out, float* postp, int H, int W, hipStream_t s) {
  const long long total = (long long)N * h * w;
  const unsigned blocks = (unsigned)((total + 255) / 256);
  ST_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
  const bool filter = max_size > 0;      // speckle_window_size 0: OpenCV skips filterSpeckles
  if (filter) {
    hipLaunchKernelGGL(sgbm_uf_init_kernel, dim3(blocks), dim3(256), 0, s, in, total, parent, size);
    hipLaunchKernelGGL(sgbm_uf_union_kernel, dim3(st::ceil_div(w, 256), h, N), dim3(256), 0, s, in, h, w, max_diff,
                       parent, status);
    hipLaunchKernelGGL(sgbm_uf_count_kernel, dim3(blocks), dim3(256), 0, s, total, h * w, parent, size, status);
  }
  const int PH = postp ? H : h, PW = postp ? W : w;
  hipLaunchKernelGGL(sgbm_pack_kernel, dim3(st::ceil_div(PW, 256), PH, N), dim3(256), 0, s, in,
                     filter ? parent : nullptr, size, h, w, max_size, PH, PW, status, final_out, postp);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

int launch_tail(const SgbmGeom& g, int N, const StSgbmParams* p, void* ws, const Layout& L, float* postp, int H, int W,
                int* status, hipStream_t s) {
  int16_t* raw = at<int16_t>(ws, L.raw);
  int16_t* med = at<int16_t>(ws, L.med);
  ST_CHECK(launch_match(g, N, p, ws, L, nullptr, raw, s));
  ST_CHECK(launch_median(raw, N, g.h, g.w, med, s));
  return launch_speckle(med, N, g.h, g.w, p->speckle_window_size, 16 * p->speckle_range, at<int>(ws, L.parent),
                        at<int>(ws, L.size), status ? status : at<int>(ws, L.status), nullptr, postp, H, W, s);
}

int prefilter_u8(const void* const* lp, const void* const* rp, int N, int fh, int fw, int h, int w, const SgbmGeom& g,
                 int ftzero, void* ws, const Layout& L, hipStream_t s) {
  for (int base = 0; base < N; base += kMaxFrames) {
    const int k = N - base < kMaxFrames ? N - base : kMaxFrames;
    FramePtrs fl{}, fr{};
    for (int i = 0; i < k; ++i) {
      fl.p[i] = static_cast<const unsigned char*>(lp[base + i]);
      fr.p[i] = static_cast<const unsigned char*>(rp[base + i]);
      ST_REQUIRE(fl.p[i] && fr.p[i], "st_sgbm_u8: frame %d is null", base + i);
    }
    hipLaunchKernelGGL(sgbm_prefilter_u8_kernel, dim3(st::ceil_div(w, 256), h, 2 * k), dim3(256), 0, s, fl, fr, base,
                       fh, fw, g.cn, h, w, ftzero, at<uint32_t>(ws, L.pf));
  }
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

int prefilter_f32(const float* left, const float* right, int N, int H, int W, int h, int w, const SgbmGeom& g,
                  int ftzero, void* ws, const Layout& L, hipStream_t s) {
  hipLaunchKernelGGL(sgbm_prefilter_f32_kernel, dim3(st::ceil_div(w, 256), h, 2 * N), dim3(256), 0, s, left, right, H,
                     W, g.cn, h, w, ftzero, at<uint32_t>(ws, L.pf));
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

int ftzero_of(const StSgbmParams* p) { return (p->pre_filter_cap > 15 ? p->pre_filter_cap : 15) | 1; }

}  // namespace

extern "C" size_t st_sgbm_workspace_bytes(int N, int h, int w, int D) {
  if (N <= 0 || h <= 0 || D <= 0 || w <= D) return 0;
  return layout(N, h, w, D).total;
}

extern "C" int st_sgbm_u8(const void* const* left_ptrs_host, const void* const* right_ptrs_host, int N, int fh, int fw,
                          int h, int w, const StSgbmParams* params, void* ws, size_t ws_bytes, float* disp_postp_dev,
                          int H, int W, int* status_dev, st_stream_t stream) {
  ST_CHECK(check_params(params, N, h, w, ws, "st_sgbm_u8"));
  ST_REQUIRE(left_ptrs_host && right_ptrs_host && ws && disp_postp_dev && N > 0 && h <= fh && w <= fw && h <= H &&
                 w <= W,
             "st_sgbm_u8: bad argument");
  const size_t need = st_sgbm_workspace_bytes(N, h, w, params->num_disparities);
  ST_REQUIRE(ws_bytes >= need, "st_sgbm_u8: workspace %zu < %zu bytes", ws_bytes, need);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const SgbmGeom g = geom_of(params, h, w);
  const Layout L = layout(N, h, w, g.D);
  ST_CHECK(prefilter_u8(left_ptrs_host, right_ptrs_host, N, fh, fw, h, w, g, ftzero_of(params), ws, L, s));
  return launch_tail(g, N, params, ws, L, disp_postp_dev, H, W, status_dev, s);
}

extern "C" int st_sgbm_f32(const float* left_dev, const float* right_dev, int N, int H, int W, int h, int w,
                           const StSgbmParams* params, void* ws, size_t ws_bytes, float* disp_postp_dev,
                           int* status_dev, st_stream_t stream) {
  ST_CHECK(check_params(params, N, h, w, ws, "st_sgbm_f32"));
  ST_REQUIRE(left_dev && right_dev && ws && disp_postp_dev && N > 0 && h <= H && w <= W, "st_sgbm_f32: bad argument");
  const size_t need = st_sgbm_workspace_bytes(N, h, w, params->num_disparities);
  ST_REQUIRE(ws_bytes >= need, "st_sgbm_f32: workspace %zu < %zu bytes", ws_bytes, need);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const SgbmGeom g = geom_of(params, h, w);
  const Layout L = layout(N, h, w, g.D);
  ST_CHECK(prefilter_f32(left_dev, right_dev, N, H, W, h, w, g, ftzero_of(params), ws, L, s));
  return launch_tail(g, N, params, ws, L, disp_postp_dev, H, W, status_dev, s);
}

extern "C" int st_sgbm_match_f32(const float* left_dev, const float* right_dev, int N, int H, int W, int h, int w,
                                 const StSgbmParams* params, void* ws, size_t ws_bytes, int16_t* cost_out_dev,
                                 int16_t* disp_out_dev, st_stream_t stream) {
  ST_CHECK(check_params(params, N, h, w, ws, "st_sgbm_match_f32"));
  ST_REQUIRE(left_dev && right_dev && ws && N > 0 && h <= H && w <= W, "st_sgbm_match_f32: bad argument");
  const size_t need = st_sgbm_workspace_bytes(N, h, w, params->num_disparities);
  ST_REQUIRE(ws_bytes >= need, "st_sgbm_match_f32: workspace %zu < %zu bytes", ws_bytes, need);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const SgbmGeom g = geom_of(params, h, w);
  const Layout L = layout(N, h, w, g.D);
  ST_CHECK(prefilter_f32(left_dev, right_dev, N, H, W, h, w, g, ftzero_of(params), ws, L, s));
  return launch_match(g, N, params, ws, L, cost_out_dev, disp_out_dev, s);
}

extern "C" int st_sgbm_median(const int16_t* in_dev, int N, int h, int w, int16_t* out_dev, st_stream_t stream) {
  ST_REQUIRE(in_dev && out_dev && in_dev != out_dev && N > 0 && h > 0 && w > 0, "st_sgbm_median: bad argument");
  return launch_median(in_dev, N, h, w, out_dev, static_cast<hipStream_t>(stream));
}

extern "C" int st_sgbm_speckle(const int16_t* in_dev, int N, int h, int w, int max_size, int max_diff, void* ws,
                               size_t ws_bytes, int16_t* out_dev, float* disp_postp_dev, int H, int W, int* status_dev,
                               st_stream_t stream) {
  ST_REQUIRE(in_dev && ws && status_dev && N > 0 && h > 0 && w > 0 && max_size >= 0 && max_diff >= 0,
             "st_sgbm_speckle: bad argument");
  ST_REQUIRE(!disp_postp_dev || (h <= H && w <= W), "st_sgbm_speckle: output %d x %d smaller than the map", H, W);
  const size_t px = (size_t)N * h * w, need = 2 * align256(px * sizeof(int));
  ST_REQUIRE(ws_bytes >= need, "st_sgbm_speckle: workspace %zu < %zu bytes", ws_bytes, need);
  ST_REQUIRE((long long)N * h * w < INT_MAX, "st_sgbm_speckle: %d maps of %d x %d exceed int indices", N, h, w);
  int* parent = at<int>(ws, 0);
  int* size = at<int>(ws, align256(px * sizeof(int)));
  return launch_speckle(in_dev, N, h, w, max_size, max_diff, parent, size, status_dev, out_dev, disp_postp_dev, H, W,
                        static_cast<hipStream_t>(stream));
}
