// The decode core of ma_inflate_blocks_batch (lancet2_amd/csrc/inflate_core.h) on the host, one lane: every member of the case
// table tests/inflate_cases.py dumps -- u32 count, then per case u32 member bytes, the member, u32 expected state, u32 payload
// bytes, the payload -- through parse_member, inflate_member and the CRC-32, the way k_inf_decode strings them together; then
// the CRC combine as the kernel's 64 lanes use it.  Built with -fsanitize=address,undefined by tests/test_inflate_cases.py: the
// member sits in an exactly sized heap block and so does the output, so a read or write one byte outside either is reported.
// usage: inflate_units <case file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../lancet2_amd/csrc/inflate_core.h"

namespace z = ma::zcore;

struct HostCx {
  static constexpr uint32_t kLanes = 1;
  const uint8_t* data;
  uint32_t data_len;
  uint8_t* out;
  uint32_t lane() const { return 0; }
  void sync() {}
  uint32_t byte(uint32_t ip) const { return ip < data_len ? data[ip] : 0u; }
  uint32_t next32(uint32_t ip) const { return byte(ip) | (byte(ip + 1) << 8) | (byte(ip + 2) << 16) | (byte(ip + 3) << 24); }
  void literal(uint32_t pos, uint32_t b) { out[pos] = static_cast<uint8_t>(b); }
  void copy(uint32_t pos, uint32_t len, uint32_t dist) {
    for (uint32_t i = 0; i < len; ++i) out[pos + i] = out[pos - dist + i % dist];
  }
  void stored(uint32_t pos, uint32_t ip, uint32_t len) {
    if (len) std::memcpy(out + pos, data + ip, len);
  }
};

// what the kernel does with the 64 slices of a payload
static uint32_t crc_by_slices(const uint8_t* p, uint32_t n) {
  uint32_t const per = (n + 63u) / 64u;
  uint32_t crc = 0;
  for (uint32_t lane = 0; lane < 64u; ++lane) {
    uint32_t const from = lane * per < n ? lane * per : n, upto = from + per < n ? from + per : n;
    uint32_t const reg = z::crc_bytes(lane == 0u ? 0xFFFFFFFFu : 0u, p + from, upto - from);
    crc ^= z::crc_mul(reg, z::crc_x8n(n - upto));
  }
  return crc ^ 0xFFFFFFFFu;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  auto rd = [&]() {
    uint32_t v = 0;
    if (std::fread(&v, 4, 1, f) != 1) std::exit(2);
    return v;
  };
  uint32_t const n_cases = rd();
  int failed = 0;
  static z::Tables T;
  for (uint32_t c = 0; c < n_cases; ++c) {
    uint32_t const mlen = rd();
    uint8_t* member = static_cast<uint8_t*>(std::malloc(mlen ? mlen : 1));
    if (mlen && std::fread(member, 1, mlen, f) != mlen) return 2;
    uint32_t const want_state = rd(), plen = rd();
    std::vector<uint8_t> payload(plen);
    if (plen && std::fread(payload.data(), 1, plen, f) != plen) return 2;
    z::Member const m = z::parse_member(member, mlen);
    uint32_t state = m.state;
    uint8_t* out = nullptr;
    if (state == 0u) {
      out = static_cast<uint8_t*>(std::malloc(m.isize ? m.isize : 1));
      HostCx cx{member + m.data_at, m.data_len, out};
      state = z::inflate_member(cx, T, m.data_len, m.isize);
      if (state == 0u && crc_by_slices(out, m.isize) != m.crc) state = MA_Z_CRC;
      if (state == 0u && z::crc_bytes(0xFFFFFFFFu, out, m.isize) != (m.crc ^ 0xFFFFFFFFu)) state = 0x100u;  // (the two CRC routes differ)
    }
    bool ok = state == want_state;
    if (ok && state == 0u) ok = m.isize == plen && (plen == 0 || std::memcmp(out, payload.data(), plen) == 0);
    if (!ok) {
      std::fprintf(stderr, "case %u: state %u, wanted %u%s\n", c, state, want_state, state == want_state ? " (payload differs)" : "");
      ++failed;
    }
    std::free(out);
    std::free(member);
  }
  std::fclose(f);
  if (failed) return 1;
  std::printf("inflate units ok: %u cases\n", n_cases);
  return 0;
}
