// Huffman entropy decode of baseline JPEG scans on the device (include/stereotrack_jpeg.h, DESIGN.md section 25
// "Entropy decode on the device"): the self-synchronising decode of Weissenberger and Schmidt (ICPP 2018) over the
// text of jpeg_entropy_core.h.  Two launches per call of N images:
//
//   A  jpeg_entropy_kernel   one workgroup per image walks the scan tile by tile (`tile` subsequences of `subseq_bytes`
//                            raw bytes, one thread each; the tile's bytes, one byte in front and a 64-byte halo staged in
//                            LDS, beside the image's descriptor).  Per tile: (1) every thread decodes its subsequence
//                            from its first bit with state (0, 0) - thread 0 from the previous tile's true exit - and
//                            stores its exit; (2) thread i re-decodes from thread i - 1's exit while that differs from
//                            what it last started from, until a pass changes nothing: after pass p the first p exits are
//                            final, so at most `tile` passes; (3) an exclusive scan of (markers crossed, blocks completed)
//                            carried from tile to tile tells every thread its restart interval and block index;
//                            (4) the write pass decodes once more from the true entries and stores coefficients (DC as
//                            the difference, skipped positions as zeros) and raises the status bits.  Thread 0 then
//                            checks the counts at the end of the bytes.  The order between tiles is this one workgroup's
//                            loop: no workgroup waits on another.
//   B  jpeg_dc_kernel        one workgroup per (component, image): the segmented inclusive scan of the DC differences in
//                            scan order, restarted at interval starts, in 32 bits with the int16 range check.
//
// Every loop is bounded: the passes by `tile`, a thread's decode by the bits of its subsequence (core: decode_piece), the
// fill-byte walk by the scan's length.  Reads stay inside the blob (the entry refuses descriptors whose scan does not);
// writes go to block_base() / dc_element() of blocks the host would decode, which lie inside the image's extent.
#include <cstdint>
#include <cstring>

#include "../../include/stereotrack_jpeg.h"
#include "jpeg_entropy_core.h"
#include "st_common.h"

namespace st {
bool jpeg_geometry_ok(const StJpegInfo& info);      // jpeg_io.cpp
}

namespace {

namespace E = st::jent;

constexpr int THREADS = 256, HALO = 64, MAX_TILE_BYTES = 32768;
constexpr int DESC_WORDS = (int)(sizeof(StJpegEntropyDesc) / 16);
static_assert(sizeof(StJpegEntropyDesc) % 16 == 0, "descriptors are copied and placed in 16-byte units");
static_assert(sizeof(StJpegEntropyStats) == 16, "one stats record is four ints");

struct EntGeom {
  int blocks_w[3];
  unsigned long long coef_offset[3];
  unsigned long long coef_count;
  int ncomp, sampling, mcus_x, mcus_y;
};

// a byte of the scan: from the staged window where it covers the index, from the blob otherwise (a symbol that runs
// past the halo through fill bytes)
struct StagedLoad {
  const uint8_t* lds;
  uint32_t lo, hi;
  const uint8_t* g;
  __device__ uint32_t operator()(uint32_t p) const { return p >= lo && p < hi ? lds[p - lo] : g[p]; }
};

struct CoefSink {
  int16_t* coef;
  uint32_t* err;
  __device__ void store(uint64_t element, int16_t v) const { coef[element] = v; }
  __device__ void error(uint32_t bits) const { atomicOr(err, bits); }
};

__global__ __launch_bounds__(THREADS) void jpeg_entropy_kernel(const uint8_t* __restrict__ blob, EntGeom g, int S, int T,
                                                               int16_t* __restrict__ coef, uint16_t* __restrict__ quant,
                                                               int32_t* __restrict__ status, StJpegEntropyStats* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) uint4 desc_words[DESC_WORDS];
  __shared__ __attribute__((aligned(16))) uint8_t bytes[MAX_TILE_BYTES + HALO + 16];
  __shared__ E::Entry exits[THREADS];
  __shared__ E::Count counts[2][THREADS];
  __shared__ uint32_t err;
  const int tid = threadIdx.x, img = blockIdx.x;
  const uint4* src = reinterpret_cast<const uint4*>(blob) + (size_t)img * DESC_WORDS;
  for (int i = tid; i < DESC_WORDS; i += THREADS) desc_words[i] = src[i];
  if (tid == 0) err = 0;
  __syncthreads();
  const StJpegEntropyDesc* d = reinterpret_cast<const StJpegEntropyDesc*>(desc_words);
  if (tid < 192) quant[(size_t)img * 192 + tid] = d->quant[tid >> 6][tid & 63];
  E::Ctx cx;
  {
    const uint64_t off[3] = {g.coef_offset[0], g.coef_offset[1], g.coef_offset[2]};
    E::make_ctx(cx, d, g.blocks_w, off);
  }
  const uint8_t* scan = blob + d->blob_offset;
  const uint32_t n = cx.n;
  const uint32_t nsub = (n + (uint32_t)S - 1) / (uint32_t)S, ntiles = (nsub + (uint32_t)T - 1) / (uint32_t)T;
  CoefSink sink{coef + (size_t)img * g.coef_count, &err};
  E::NoSink none;
  E::Entry carry_entry{0, 0};
  E::Count carry_count{0, 0};
  int max_passes = 0, sum_passes = 0;
  for (uint32_t tile = 0; tile < ntiles; ++tile) {
    const uint32_t t0 = tile * (uint32_t)(T * S);
    const uint32_t lo = t0 ? t0 - 1 : 0, hi = min(n, t0 + (uint32_t)(T * S + HALO));
    __syncthreads();                                   // the last tile's reads of `bytes`, `exits`, `counts` are over
    for (uint32_t i = lo + tid; i < hi; i += THREADS) bytes[i - lo] = scan[i];
    __syncthreads();
    const StagedLoad ld{bytes, lo, hi, scan};
    const uint32_t sub = tile * (uint32_t)T + tid;
    const bool active = tid < T && sub < nsub;
    const int last = (int)min((uint32_t)T, nsub - tile * (uint32_t)T) - 1;
    const uint32_t start = sub * (uint32_t)S, end = min(n, start + (uint32_t)S);
    E::Entry entry = carry_entry, exit_{0, 0};
    E::Count cnt{0, 0};
    if (active) {
      if (tid) entry = E::Entry{E::speculative_start(ld, start) * 8, 0};
      exit_ = E::decode_piece<false>(cx, ld, entry, end, cnt, 0, 0, none);
      exits[tid] = exit_;
    }
    int passes = 1;
    while (passes < T) {                               // at most `tile` passes: pass p makes the first p exits final
      __syncthreads();
      E::Entry e = entry;
      if (active && tid) e = exits[tid - 1];
      __syncthreads();                                 // every exit is read before any is replaced
      const bool changed = !E::same(e, entry);
      if (changed) {
        entry = e;
        exit_ = E::decode_piece<false>(cx, ld, entry, end, cnt, 0, 0, none);
        exits[tid] = exit_;
      }
      if (!__syncthreads_or(changed)) break;
      ++passes;
    }
    max_passes = max(max_passes, passes);
    sum_passes += passes;
    // inclusive scan of the counts (Hillis-Steele over T entries, two buffers)
    int cur = 0;
    counts[0][tid] = active ? cnt : E::Count{0, 0};
    __syncthreads();
    for (int step = 1; step < T; step <<= 1) {
      E::Count v = counts[cur][tid];
      if (tid >= step) v = E::combine(counts[cur][tid - step], v);
      counts[cur ^ 1][tid] = v;
      cur ^= 1;
      __syncthreads();
    }
    if (active) {
      const E::Count before = tid ? E::combine(carry_count, counts[cur][tid - 1]) : carry_count;
      E::Count again;
      E::decode_piece<true>(cx, ld, entry, end, again, before.m, before.c, sink);
    }
    carry_entry = exits[last];                         // uniform: every thread keeps the carry
    carry_count = E::combine(carry_count, counts[cur][last]);
  }
  __syncthreads();
  if (tid == 0) {
    status[img] = (int32_t)(err | E::final_check(cx, carry_count));
    stats[img] = StJpegEntropyStats{(int)ntiles, (int)nsub, max_passes, sum_passes};
  }
}

constexpr int DC_THREADS = 256;

__global__ __launch_bounds__(DC_THREADS) void jpeg_dc_kernel(const uint8_t* __restrict__ blob, EntGeom g, int16_t* __restrict__ coef,
                                                             int32_t* __restrict__ status) {
  __shared__ E::DcSum sums[2][DC_THREADS];
  __shared__ StJpegEntropyDesc head;       // only the first 64 bytes (the scalars) are filled and read
  const int tid = threadIdx.x, c = blockIdx.x, img = blockIdx.y;
  if (c >= g.ncomp || status[img] != 0) return;        // uniform; a refused image's coefficients are unspecified
  if (tid < 16) reinterpret_cast<uint32_t*>(&head)[tid] = reinterpret_cast<const uint32_t*>(blob + (size_t)img * sizeof(StJpegEntropyDesc))[tid];
  __syncthreads();
  E::Ctx cx;
  {
    const uint64_t off[3] = {g.coef_offset[0], g.coef_offset[1], g.coef_offset[2]};
    E::make_ctx(cx, &head, g.blocks_w, off);
  }
  int16_t* cf = coef + (size_t)img * g.coef_count;
  const uint32_t items = (uint32_t)g.mcus_x * (uint32_t)g.mcus_y * (uint32_t)E::dc_per(cx, c);
  const uint32_t chunk = (items + DC_THREADS - 1) / DC_THREADS;
  const uint32_t a = min(items, (uint32_t)tid * chunk), b = min(items, a + chunk);
  E::DcSum mine{0, 0};
  for (uint32_t t = a; t < b; ++t)
    mine = E::dc_combine(mine, E::DcSum{(uint32_t)(int32_t)cf[E::dc_element(cx, c, t)], E::dc_restarts(cx, c, t) ? 1u : 0u});
  int cur = 0;
  sums[0][tid] = mine;
  __syncthreads();
  for (int step = 1; step < DC_THREADS; step <<= 1) {
    E::DcSum v = sums[cur][tid];
    if (tid >= step) v = E::dc_combine(sums[cur][tid - step], v);
    sums[cur ^ 1][tid] = v;
    cur ^= 1;
    __syncthreads();
  }
  uint32_t pred = tid ? sums[cur][tid - 1].sum : 0u;
  bool bad = false;
  for (uint32_t t = a; t < b; ++t) {
    const uint64_t el = E::dc_element(cx, c, t);
    if (E::dc_restarts(cx, c, t)) pred = 0;
    pred += (uint32_t)(int32_t)cf[el];
    bad = bad || !E::dc_in_range(pred);
    cf[el] = (int16_t)pred;
  }
  if (bad) atomicOr(reinterpret_cast<unsigned int*>(status + img), (unsigned int)ST_JPEG_E_DC);
}

bool make_geom(const StJpegInfo& I, EntGeom& g) {
  if (!st::jpeg_geometry_ok(I)) return false;
  for (int c = 0; c < 3; ++c) {
    g.blocks_w[c] = c < I.components ? I.blocks_w[c] : 0;
    g.coef_offset[c] = c < I.components ? (unsigned long long)I.coef_offset[c] : 0ull;
  }
  g.coef_count = (unsigned long long)I.coef_count;
  g.ncomp = I.components;
  g.sampling = I.sampling;
  g.mcus_x = I.mcus_x;
  g.mcus_y = I.mcus_y;
  return true;
}

}  // namespace

extern "C" size_t st_jpeg_entropy_work_bytes(const StJpegInfo* info, int N) {
  EntGeom g;
  if (!info || info->struct_size != (int)sizeof(StJpegInfo) || N < 1 || N > 65535 || !make_geom(*info, g)) return 0;
  return ((size_t)N * sizeof(StJpegEntropyStats) + 255) / 256 * 256;
}

extern "C" int st_jpeg_entropy_decode_dev(const uint8_t* blob_host, const uint8_t* blob_dev, size_t blob_bytes, int N,
                                          const StJpegInfo* info, const StJpegEntropyTuning* tuning, int16_t* coef_dev,
                                          uint16_t* quant_dev, int32_t* status_dev, void* work_dev, size_t work_bytes,
                                          st_stream_t stream_) {
  ST_REQUIRE(blob_host && blob_dev && info && coef_dev && quant_dev && status_dev && work_dev,
             "st_jpeg_entropy_decode_dev: null pointer");
  ST_REQUIRE(info->struct_size == (int)sizeof(StJpegInfo), "st_jpeg_entropy_decode_dev: StJpegInfo.struct_size %d, this library has %d",
             info->struct_size, (int)sizeof(StJpegInfo));
  ST_REQUIRE(N >= 1 && N <= 65535, "st_jpeg_entropy_decode_dev: N must be 1..65535, got %d", N);
  EntGeom g;
  ST_REQUIRE(make_geom(*info, g), "st_jpeg_entropy_decode_dev: StJpegInfo is not what st_jpeg_info returns for its width / height / sampling");
  int S = 32, T = 256;
  if (tuning) {
    ST_REQUIRE(tuning->struct_size == (int)sizeof(StJpegEntropyTuning), "st_jpeg_entropy_decode_dev: StJpegEntropyTuning.struct_size mismatch");
    if (tuning->subseq_bytes) S = tuning->subseq_bytes;
    if (tuning->tile) T = tuning->tile;
  }
  ST_REQUIRE(S >= 8 && S <= 512 && T >= 1 && T <= THREADS && S * T <= MAX_TILE_BYTES,
             "st_jpeg_entropy_decode_dev: subseq_bytes %d (8..512) x tile %d (1..256) must not exceed 32768", S, T);
  ST_REQUIRE((reinterpret_cast<uintptr_t>(blob_dev) & 15) == 0 && (reinterpret_cast<uintptr_t>(work_dev) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(quant_dev) & 1) == 0 && (reinterpret_cast<uintptr_t>(coef_dev) & 1) == 0 &&
                 (reinterpret_cast<uintptr_t>(status_dev) & 3) == 0,
             "st_jpeg_entropy_decode_dev: blob_dev and work_dev must be 16-byte aligned, the outputs to their element size");
  const size_t need = st_jpeg_entropy_work_bytes(info, N);
  if (work_bytes < need)
    return st::set_error(ST_ERR_WORKSPACE, "st_jpeg_entropy_decode_dev: work memory of %zu bytes, %zu needed", work_bytes, need);
  const size_t head = (size_t)N * sizeof(StJpegEntropyDesc);
  ST_REQUIRE(blob_bytes >= head, "st_jpeg_entropy_decode_dev: a blob of %zu bytes does not hold %d descriptors", blob_bytes, N);
  for (int i = 0; i < N; ++i) {
    StJpegEntropyDesc hd;                                // the scalars only: the tables are the kernel's to read
    std::memcpy(&hd, blob_host + (size_t)i * sizeof(StJpegEntropyDesc), 64);
    ST_REQUIRE(hd.struct_size == (int)sizeof(StJpegEntropyDesc), "st_jpeg_entropy_decode_dev: descriptor %d has struct_size %d", i, hd.struct_size);
    ST_REQUIRE(hd.components == info->components && hd.sampling == info->sampling && hd.mcus_x == info->mcus_x &&
                   hd.mcus_y == info->mcus_y,
               "st_jpeg_entropy_decode_dev: descriptor %d does not match the StJpegInfo geometry (one call decodes one geometry and sampling class)", i);
    ST_REQUIRE(hd.restart_interval >= 0 && hd.restart_interval <= 65535, "st_jpeg_entropy_decode_dev: descriptor %d: bad restart interval", i);
    for (int c = 0; c < 3; ++c)
      ST_REQUIRE(hd.dc_slot[c] >= 0 && hd.dc_slot[c] <= 2 && hd.ac_slot[c] >= 0 && hd.ac_slot[c] <= 2,
                 "st_jpeg_entropy_decode_dev: descriptor %d: bad table slot", i);
    ST_REQUIRE(hd.scan_bytes < E::MAX_SCAN_BYTES && (hd.blob_offset & 15) == 0 && hd.blob_offset >= head &&
                   (size_t)hd.blob_offset + hd.scan_bytes <= blob_bytes,
               "st_jpeg_entropy_decode_dev: descriptor %d: its scan (offset %u, %u bytes) does not lie inside the blob behind the descriptors", i,
               hd.blob_offset, hd.scan_bytes);
  }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)N), dim3(THREADS), 0, stream, blob_dev, g, S, T, coef_dev, quant_dev,
                     status_dev, static_cast<StJpegEntropyStats*>(work_dev));
  ST_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(jpeg_dc_kernel, dim3(3u, (unsigned)N), dim3(DC_THREADS), 0, stream, blob_dev, g, coef_dev, status_dev);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}
