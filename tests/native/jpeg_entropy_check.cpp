// Stand-alone host check of the device entropy decoder's algorithm (stereotracking_amd/csrc/jpeg_entropy_core.h, the
// text jpeg_entropy.hip compiles) against its specification, st_jpeg_entropy_decode.  Plain host code, no HIP, built
// with -fsanitize=address,undefined (tests/test_cpu_jpeg_entropy.py builds and runs it):
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__
//       -I<rocm>/include tests/native/jpeg_entropy_check.cpp stereotracking_amd/csrc/jpeg_io.cpp
//       stereotracking_amd/csrc/st_common.cpp -o jpeg_entropy_check
//   ./jpeg_entropy_check tests/golden/jpeg/*.jpg
//
// emulate() is jpeg_entropy_kernel + jpeg_dc_kernel with the threads of a workgroup as serial loops: per tile the
// speculative pass, the re-decode passes until no exit changes, the count scan, the write pass; then the final count
// check and the chunked segmented DC scan.  The scan bytes sit in a buffer of exactly their length, and the
// coefficients in one of exactly coef_count elements, so that the sanitizer sees any access outside them.
// Inputs: every file named on the command line, then 200 seeded corruptions of them (byte flips, truncations, both),
// at several (subseq_bytes, tile) settings.  For each the verdict must equal st_jpeg_entropy_decode's, and where both
// accept every coefficient and table value must be equal.  With --probe FILE S T it prints one file's stats instead.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/stereotrack_jpeg.h"
#include "../../stereotracking_amd/csrc/jpeg_entropy_core.h"

namespace {

namespace E = st::jent;

uint32_t lcg_state = 20241021u;
uint32_t lcg() {
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return lcg_state >> 8;
}

struct PlainLoad {
  const uint8_t* d;
  uint32_t n;
  uint32_t operator()(uint32_t p) const {
    if (p >= n) std::abort();              // the core never asks for a byte outside the scan
    return d[p];
  }
};

struct VecSink {
  std::vector<int16_t>* coef;
  std::vector<uint8_t>* written;
  uint32_t* err;
  void store(uint64_t el, int16_t v) const {
    coef->at(el) = v;
    if (written->at(el)++) {
      std::fprintf(stderr, "jpeg_entropy_check: element %llu stored twice\n", (unsigned long long)el);
      std::abort();
    }
  }
  void error(uint32_t bits) const { *err |= bits; }
};

struct Result {
  uint32_t status = 0;
  StJpegEntropyStats stats = {0, 0, 0, 0};
  bool all_written = false;
};

Result emulate(const StJpegEntropyDesc& desc, const uint8_t* file, const StJpegInfo& info, int S, int T, std::vector<int16_t>& coef) {
  Result res;
  std::vector<uint8_t> scan(file + desc.scan_offset, file + desc.scan_offset + desc.scan_bytes);
  E::Ctx cx;
  const uint64_t off[3] = {info.coef_offset[0], info.coef_offset[1], info.coef_offset[2]};
  E::make_ctx(cx, &desc, info.blocks_w, off);
  const uint32_t n = cx.n;
  const PlainLoad ld{scan.data(), n};
  std::vector<uint8_t> written(coef.size(), 0);
  uint32_t err = 0;
  VecSink sink{&coef, &written, &err};
  E::NoSink none;
  const uint32_t nsub = (n + S - 1) / S, ntiles = (nsub + T - 1) / T;
  E::Entry carry_entry{0, 0};
  E::Count carry_count{0, 0};
  std::vector<E::Entry> entry(T), exits(T), seen(T);
  std::vector<E::Count> cnt(T), incl(T);
  for (uint32_t tile = 0; tile < ntiles; ++tile) {
    const int live = (int)std::min<uint32_t>(T, nsub - tile * T);
    auto end_of = [&](int i) { return std::min<uint32_t>(n, (tile * T + i + 1) * (uint32_t)S); };
    for (int i = 0; i < live; ++i) {                                            // pass 1
      const uint32_t start = (tile * T + i) * (uint32_t)S;
      entry[i] = i ? E::Entry{E::speculative_start(ld, start) * 8, 0} : carry_entry;
      exits[i] = E::decode_piece<false>(cx, ld, entry[i], end_of(i), cnt[i], 0, 0, none);
    }
    int passes = 1;
    while (passes < T) {
      for (int i = 1; i < live; ++i) seen[i] = exits[i - 1];                    // every exit read before any is replaced
      bool changed = false;
      for (int i = 1; i < live; ++i)
        if (!E::same(seen[i], entry[i])) {
          entry[i] = seen[i];
          exits[i] = E::decode_piece<false>(cx, ld, entry[i], end_of(i), cnt[i], 0, 0, none);
          changed = true;
        }
      if (!changed) break;
      ++passes;
    }
    res.stats.max_passes = std::max(res.stats.max_passes, passes);
    res.stats.sum_passes += passes;
    for (int i = 0; i < live; ++i) incl[i] = i ? E::combine(incl[i - 1], cnt[i]) : cnt[i];
    for (int i = 0; i < live; ++i) {                                            // write pass
      const E::Count before = i ? E::combine(carry_count, incl[i - 1]) : carry_count;
      E::Count again;
      const E::Entry x = E::decode_piece<true>(cx, ld, entry[i], end_of(i), again, before.m, before.c, sink);
      if (!E::same(x, exits[i]) || again.m != cnt[i].m || again.c != cnt[i].c) {
        std::fprintf(stderr, "jpeg_entropy_check: the write pass left a piece elsewhere than the settled pass\n");
        std::abort();
      }
      if (i + 1 < live && !E::same(x, entry[i + 1])) {
        std::fprintf(stderr, "jpeg_entropy_check: tile %u settled on entries that are not a chain\n", tile);
        std::abort();
      }
    }
    carry_entry = exits[live - 1];
    carry_count = E::combine(carry_count, incl[live - 1]);
  }
  res.status = err | E::final_check(cx, carry_count);
  res.stats.tiles = (int)ntiles;
  res.stats.subsequences = (int)nsub;
  res.all_written = std::all_of(written.begin(), written.end(), [](uint8_t w) { return w == 1; });
  if (res.status) return res;
  // jpeg_dc_kernel: 256 chunks per component, a segmented scan over the chunk sums, the chunks again
  const int threads = 256;
  for (int c = 0; c < info.components; ++c) {
    const uint32_t items = (uint32_t)info.mcus_x * info.mcus_y * E::dc_per(cx, c), chunk = (items + threads - 1) / threads;
    std::vector<E::DcSum> sums(threads);
    for (int i = 0; i < threads; ++i) {
      const uint32_t a = std::min(items, i * chunk), b = std::min(items, a + chunk);
      E::DcSum mine{0, 0};
      for (uint32_t t = a; t < b; ++t)
        mine = E::dc_combine(mine, E::DcSum{(uint32_t)(int32_t)coef.at(E::dc_element(cx, c, t)), E::dc_restarts(cx, c, t) ? 1u : 0u});
      sums[i] = i ? E::dc_combine(sums[i - 1], mine) : mine;
    }
    for (int i = 0; i < threads; ++i) {
      const uint32_t a = std::min(items, i * chunk), b = std::min(items, a + chunk);
      uint32_t pred = i ? sums[i - 1].sum : 0u;
      for (uint32_t t = a; t < b; ++t) {
        const uint64_t el = E::dc_element(cx, c, t);
        if (E::dc_restarts(cx, c, t)) pred = 0;
        pred += (uint32_t)(int32_t)coef.at(el);
        if (!E::dc_in_range(pred)) res.status |= ST_JPEG_E_DC;
        coef.at(el) = (int16_t)pred;
      }
    }
  }
  return res;
}

const int kSettings[][2] = {{16, 4}, {16, 64}, {32, 256}, {8, 1}, {24, 7}, {512, 64}};
int counts[3] = {0, 0, 0};   // accepted, refused by the entropy decode, refused by the header parse

// 0 = the emulation agrees with the host routine at every setting
int run(const std::vector<uint8_t>& d, const char* name) {
  StJpegInfo info;
  std::memset(&info, 0, sizeof(info));
  info.struct_size = (int)sizeof(info);
  StJpegEntropyDesc desc;
  desc.struct_size = (int)sizeof(desc);
  const int rc_info = st_jpeg_info(d.data(), d.size(), &info);
  const int rc_prep = st_jpeg_entropy_prepare(d.data(), d.size(), &desc);
  if (rc_info != ST_OK) {
    if (rc_prep != rc_info) {
      std::fprintf(stderr, "jpeg_entropy_check: %s: st_jpeg_info returns %d, st_jpeg_entropy_prepare %d\n", name, rc_info, rc_prep);
      return 1;
    }
    ++counts[2];
    return 0;
  }
  if (info.coef_count > (size_t)1 << 24) {   // a flipped size byte: not worth the memory here
    ++counts[2];
    return 0;
  }
  std::vector<int16_t> want(info.coef_count);
  std::vector<uint16_t> quant(3 * 64);
  const int rc = st_jpeg_entropy_decode(d.data(), d.size(), want.data(), quant.data());
  if (rc_prep != ST_OK) {                     // an undefined table: the host routine refuses it with the same words
    if (rc != rc_prep) {
      std::fprintf(stderr, "jpeg_entropy_check: %s: prepare returns %d, the host decode %d\n", name, rc_prep, rc);
      return 1;
    }
    ++counts[2];
    return 0;
  }
  if (desc.scan_offset + (size_t)desc.scan_bytes != d.size() || desc.mcus_x != info.mcus_x || desc.mcus_y != info.mcus_y ||
      desc.components != info.components || desc.sampling != info.sampling || desc.restart_interval != info.restart_interval) {
    std::fprintf(stderr, "jpeg_entropy_check: %s: the descriptor does not describe the file\n", name);
    return 1;
  }
  for (const auto& st : kSettings) {
    std::vector<int16_t> coef(info.coef_count, (int16_t)0x5a5a);
    const Result r = emulate(desc, d.data(), info, st[0], st[1], coef);
    if ((r.status != 0) != (rc != ST_OK)) {
      std::fprintf(stderr, "jpeg_entropy_check: %s at (%d, %d): status 0x%x, the host routine returns %d (%s)\n", name, st[0], st[1],
                   r.status, rc, rc ? st_last_error() : "ok");
      return 1;
    }
    if (rc == ST_OK) {
      if (!r.all_written) {
        std::fprintf(stderr, "jpeg_entropy_check: %s at (%d, %d): accepted, but not every element was written once\n", name, st[0], st[1]);
        return 1;
      }
      if (coef != want || std::memcmp(desc.quant, quant.data(), 384) != 0) {
        std::fprintf(stderr, "jpeg_entropy_check: %s at (%d, %d): coefficients or tables differ from the host routine's\n", name, st[0], st[1]);
        return 1;
      }
    }
  }
  ++counts[rc == ST_OK ? 0 : 1];
  return 0;
}

bool read_file(const char* path, std::vector<uint8_t>& d) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + n);
  std::fclose(f);
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 5 && !std::strcmp(argv[1], "--probe")) {
    std::vector<uint8_t> d;
    if (!read_file(argv[2], d)) return 2;
    StJpegInfo info;
    std::memset(&info, 0, sizeof(info));
    info.struct_size = (int)sizeof(info);
    StJpegEntropyDesc desc;
    desc.struct_size = (int)sizeof(desc);
    if (st_jpeg_info(d.data(), d.size(), &info) || st_jpeg_entropy_prepare(d.data(), d.size(), &desc)) return 1;
    std::vector<int16_t> coef(info.coef_count);
    const Result r = emulate(desc, d.data(), info, std::atoi(argv[3]), std::atoi(argv[4]), coef);
    std::printf("status %u scan_bytes %u tiles %d subsequences %d max_passes %d sum_passes %d\n", r.status, desc.scan_bytes,
                r.stats.tiles, r.stats.subsequences, r.stats.max_passes, r.stats.sum_passes);
    return 0;
  }
  std::vector<std::vector<uint8_t>> files;
  for (int i = 1; i < argc; ++i) {
    std::vector<uint8_t> d;
    if (!read_file(argv[i], d)) {
      std::fprintf(stderr, "jpeg_entropy_check: cannot open %s\n", argv[i]);
      return 2;
    }
    files.push_back(d);
    if (run(d, argv[i])) return 1;
  }
  if (files.empty()) {
    std::fprintf(stderr, "usage: jpeg_entropy_check file.jpg ...\n");
    return 2;
  }
  const int intact[3] = {counts[0], counts[1], counts[2]};
  for (int k = 0; k < 200; ++k) {
    std::vector<uint8_t> d = files[lcg() % files.size()];
    const int kind = k % 3;
    if (kind != 1) {                                         // 1 .. 4 byte flips
      const int flips = 1 + (int)(lcg() % 4);
      for (int j = 0; j < flips; ++j) d[lcg() % d.size()] ^= (uint8_t)(1u << (lcg() % 8));
    }
    if (kind != 0) d.resize(1 + lcg() % d.size());           // truncation
    char name[32];
    std::snprintf(name, sizeof(name), "corruption %d", k);
    if (run(d, name)) return 1;
  }
  std::printf("jpeg_entropy_check: %d files (%d accepted, %d refused), 200 corruptions: %d accepted, %d refused by the entropy "
              "decode, %d by the header parse; %d settings each, verdicts and coefficients equal\n",
              (int)files.size(), intact[0], intact[1] + intact[2], counts[0] - intact[0], counts[1] - intact[1],
              counts[2] - intact[2], (int)(sizeof(kSettings) / sizeof(kSettings[0])));
  return 0;
}
