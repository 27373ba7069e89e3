// Stand-alone CPU checks of the packed read input (tests/test_packed_reads.py builds and runs this):
//   1. lancet2_amd/csrc/unpack_core.h -- the per-lane step of k_unpack_reads, with v_perm_b32 / v_alignbit_b32 restated in
//      plain C++ -- against a nibble-by-nibble decode: every start nibble 0 .. 7, every code in every position, two tables;
//   2. with a file argument: pipeline_host.hpp's packer (FlatBatch::PackReads) on the reads of that file -- `read_off` (u64
//      count, then the offsets), bases, qualities -- written back as bases4 / quals / qual_bits / qual_dict for the test to
//      compare with capi.pack_reads.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../lancet2_amd/csrc/unpack_core.h"
#include "../../lancet2_amd/host/pipeline_host.hpp"

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

static void core_units() {
  const char* kBases = "=ACMGRSVTWYHKDBN";
  uint8_t tables[2][16];
  for (int i = 0; i < 16; ++i) {
    tables[0][i] = static_cast<uint8_t>(kBases[i]);
    tables[1][i] = static_cast<uint8_t>(i == 0 ? 0 : (i == 15 ? 93 : 2 + 6 * i));  // a quality dictionary with 0 and 93
  }
  uint32_t seed = 12345u;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
  for (int tb = 0; tb < 2; ++tb) {
    uint32_t t[4];
    std::memcpy(t, tables[tb], 16);
    for (int trial = 0; trial < 4000; ++trial) {
      uint8_t bytes[8];
      for (auto& b : bytes) b = static_cast<uint8_t>(rnd());
      if (trial < 16) std::memset(bytes, trial * 0x11, 8);  // every code in every position
      uint32_t w0, w1;
      std::memcpy(&w0, bytes, 4);
      std::memcpy(&w1, bytes + 4, 4);
      for (uint32_t k = 0; k < 8; ++k) {
        uint32_t out[2];
        ma::expand8(w0, k ? w1 : 0xDEADBEEFu, k, t, out);
        uint8_t got[8];
        std::memcpy(got, out, 8);
        for (uint32_t j = 0; j < 8; ++j) {
          uint32_t const nib = k + j;
          uint8_t const byte = bytes[nib >> 1];
          uint8_t const code = (nib & 1u) ? (byte & 15u) : (byte >> 4);
          CHECK(got[j] == tables[tb][code]);
        }
      }
    }
  }
}

static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> v;
  if (FILE* f = std::fopen(path, "rb")) {
    uint8_t buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
  }
  return v;
}

static int packer(const char* in_path, const char* out_path) {
  std::vector<uint8_t> const in = slurp(in_path);
  if (in.size() < 8) return 2;
  uint64_t n_off = 0;
  std::memcpy(&n_off, in.data(), 8);
  lancet2_amd::host::FlatBatch fb;
  fb.read_off.resize(n_off);
  std::memcpy(fb.read_off.data(), in.data() + 8, 8 * n_off);
  uint64_t const total = n_off ? fb.read_off.back() : 0;
  if (in.size() != 8 + 8 * n_off + 2 * total) return 2;
  fb.read_bases.assign(in.begin() + 8 + 8 * n_off, in.begin() + 8 + 8 * n_off + total);
  fb.read_quals.assign(in.begin() + 8 + 8 * n_off + total, in.end());
  fb.PackReads();
  FILE* f = std::fopen(out_path, "wb");
  if (!f) return 2;
  uint64_t const head[3] = {fb.bases4.size(), fb.quals_packed.size(), static_cast<uint64_t>(fb.packed.qual_bits)};
  std::fwrite(head, 8, 3, f);
  std::fwrite(fb.packed.qual_dict, 1, 16, f);
  std::fwrite(fb.bases4.data(), 1, fb.bases4.size(), f);
  std::fwrite(fb.quals_packed.data(), 1, fb.quals_packed.size(), f);
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3) return packer(argv[1], argv[2]);
  core_units();
  if (fails) return 1;
  std::printf("packed units ok\n");
  return 0;
}
