// Stand-alone host check of the JPEG reader's host routines (stereotracking_amd/csrc/jpeg_io.cpp on jpeg_core.h), built
// as plain host code with -fsanitize=address,undefined and run by hand (no pytest wrapper, no GPU):
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__
//       -I<rocm>/include tests/native/jpeg_check.cpp stereotracking_amd/csrc/jpeg_io.cpp
//       stereotracking_amd/csrc/st_common.cpp -o jpeg_check
//   ./jpeg_check tests/golden/jpeg/*.jpg
//
// Every file named on the command line, then 200 seeded corruptions of them (byte flips, truncations, both), goes
// through st_jpeg_info / st_jpeg_entropy_decode / st_jpeg_reconstruct_host with buffers of exactly the sizes
// st_jpeg_info states.  Each call must return ST_OK, ST_ERR_INVALID or ST_ERR_UNSUPPORTED (a flipped byte can turn the
// frame header into a progressive one) - and the sanitizers must have nothing to report.  Two crafted inputs go first:
// DHT segments with more codes of one length than fit (consistent segment length), and StJpegInfo structs whose grids
// are not what st_jpeg_info returns; both must be refused as ST_ERR_INVALID.  Exit status 0 and a summary line on success.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/stereotrack_jpeg.h"

namespace {

uint32_t lcg_state = 20241021u;
uint32_t lcg() {
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return lcg_state >> 8;
}

int counts[3] = {0, 0, 0};   // ok, invalid, unsupported

bool allowed(int rc, const char* what, const char* name) {
  if (rc == ST_OK || rc == ST_ERR_INVALID || rc == ST_ERR_UNSUPPORTED) return true;
  std::fprintf(stderr, "jpeg_check: %s on %s returned %d: %s\n", what, name, rc, st_last_error());
  return false;
}

// 0 = handled (decoded or refused), 1 = a status outside the contract
int run(const std::vector<uint8_t>& d, const char* name, bool must_decode) {
  StJpegInfo info;
  std::memset(&info, 0, sizeof(info));
  info.struct_size = (int)sizeof(info);
  int rc = st_jpeg_info(d.data(), d.size(), &info);
  if (!allowed(rc, "st_jpeg_info", name)) return 1;
  if (rc != ST_OK) {
    ++counts[rc == ST_ERR_INVALID ? 1 : 2];
    return must_decode ? 1 : 0;
  }
  if (info.coef_count > (size_t)1 << 26) {   // a flipped size byte: up to 65535 x 65535, not worth the memory here
    ++counts[0];
    return 0;
  }
  std::vector<int16_t> coef(info.coef_count);
  std::vector<uint16_t> quant(3 * 64);
  rc = st_jpeg_entropy_decode(d.data(), d.size(), coef.data(), quant.data());
  if (!allowed(rc, "st_jpeg_entropy_decode", name)) return 1;
  if (rc != ST_OK) {
    ++counts[rc == ST_ERR_INVALID ? 1 : 2];
    return must_decode ? 1 : 0;
  }
  std::vector<uint8_t> out((size_t)3 * info.height * info.width);
  rc = st_jpeg_reconstruct_host(coef.data(), quant.data(), &info, out.data(), (ptrdiff_t)info.height * info.width,
                                info.width, 1, 0);
  if (rc != ST_OK) {
    std::fprintf(stderr, "jpeg_check: st_jpeg_reconstruct_host on %s returned %d: %s\n", name, rc, st_last_error());
    return 1;
  }
  ++counts[0];
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  std::vector<std::vector<uint8_t>> files;
  for (int i = 1; i < argc; ++i) {
    FILE* f = std::fopen(argv[i], "rb");
    if (!f) {
      std::fprintf(stderr, "jpeg_check: cannot open %s\n", argv[i]);
      return 2;
    }
    std::vector<uint8_t> d;
    uint8_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + n);
    std::fclose(f);
    files.push_back(d);
    const bool refusal = std::strstr(argv[i], "refuse_") != nullptr;
    if (run(d, argv[i], !refusal)) {
      std::fprintf(stderr, "jpeg_check: %s did not decode\n", argv[i]);
      return 1;
    }
  }
  if (files.empty()) {
    std::fprintf(stderr, "usage: jpeg_check file.jpg ...\n");
    return 2;
  }
  // DHT segments whose counts are inconsistent while the segment length is consistent (what a flipped count byte never
  // gives: it changes the symbol total, and the length check refuses that first): more codes of one length than fit.
  // Stand-alone after SOI, and spliced in front of a real file's scan.
  {
    const int over[3][2] = {{1, 3}, {1, 200}, {3, 9}};        // (length, count)
    for (int v = 0; v < 3; ++v)
      for (int cls = 0; cls < 2; ++cls) {
        std::vector<uint8_t> seg = {0xFF, 0xC4, 0, 0, (uint8_t)(cls << 4 | 3)};
        for (int len = 1; len <= 16; ++len) seg.push_back(len == over[v][0] ? (uint8_t)over[v][1] : 0);
        for (int k = 0; k < over[v][1]; ++k) seg.push_back((uint8_t)(k % 12));
        seg[2] = (uint8_t)((seg.size() - 2) >> 8);
        seg[3] = (uint8_t)((seg.size() - 2) & 255);
        std::vector<uint8_t> alone = {0xFF, 0xD8};
        alone.insert(alone.end(), seg.begin(), seg.end());
        alone.push_back(0xFF);
        alone.push_back(0xD9);
        std::vector<uint8_t> spliced(files[0].begin(), files[0].begin() + 2);
        spliced.insert(spliced.end(), seg.begin(), seg.end());
        spliced.insert(spliced.end(), files[0].begin() + 2, files[0].end());
        const int before = counts[1];
        if (run(alone, "overfull DHT", false) || run(spliced, "overfull DHT in a file", false)) return 1;
        if (counts[1] != before + 2) {
          std::fprintf(stderr, "jpeg_check: an overfull DHT (%d codes of length %d) was not refused as invalid\n", over[v][1],
                       over[v][0]);
          return 1;
        }
      }
    counts[1] -= 12;
  }
  // an StJpegInfo that is not what st_jpeg_info returns (a grid shrunk, a negative grid) must be refused, not indexed with
  {
    StJpegInfo info;
    std::memset(&info, 0, sizeof(info));
    info.struct_size = (int)sizeof(info);
    if (st_jpeg_info(files[0].data(), files[0].size(), &info) != ST_OK) return 1;
    std::vector<int16_t> coef(info.coef_count);
    std::vector<uint16_t> quant(3 * 64, 1);
    std::vector<uint8_t> out((size_t)3 * info.height * info.width);
    if (st_jpeg_entropy_decode(files[0].data(), files[0].size(), coef.data(), quant.data()) != ST_OK) return 1;
    for (int v = 0; v < 3; ++v) {
      StJpegInfo bad = info;
      if (v == 0) bad.blocks_w[0] = -5;
      if (v == 1) bad.width += 64;
      if (v == 2) bad.coef_offset[0] = 1u << 20;
      if (st_jpeg_reconstruct_host(coef.data(), quant.data(), &bad, out.data(), (ptrdiff_t)info.height * info.width,
                                   info.width, 1, 0) != ST_ERR_INVALID) {
        std::fprintf(stderr, "jpeg_check: an inconsistent StJpegInfo (%d) was not refused\n", v);
        return 1;
      }
    }
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
    if (run(d, name, false)) return 1;
  }
  std::printf("jpeg_check: %d files (%d decoded, %d refused), 12 overfull DHT segments and 3 inconsistent StJpegInfo refused, "
              "200 corruptions: %d decoded, %d invalid, %d unsupported\n",
              (int)files.size(), intact[0], intact[1] + intact[2], counts[0] - intact[0], counts[1] - intact[1],
              counts[2] - intact[2]);
  return 0;
}
