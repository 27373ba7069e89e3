// The decode core of ma_inflate_blocks_batch (inflate.hip): the BGZF member header (SAM specification 4.1, RFC 1952), the
// canonical-code tables and the symbol / length / distance decode of RFC 1951, and CRC-32 with its x^(8n) mod P combine.  Host
// and device: plain C++ over byte pointers, so that every rule can be checked without a GPU (tests/host/inflate_units.cpp).
//
// inflate_member<Cx> is written for `Cx::kLanes` cooperating lanes that all run it with the same values -- one wavefront on the
// device, one thread (kLanes 1) on the host.  Everything that differs between the two is in the context Cx:
//   lane()                          this lane, 0 .. kLanes - 1
//   sync()                          the lanes meet; what each wrote to the tables or to the output is visible to all
//   next32(ip)                      the four input bytes at offset ip (a multiple of 4) of the DEFLATE data, zeros past its end
//   byte(ip)                        one input byte, zero past the end
//   literal(pos, b)                 output byte pos is b
//   copy(pos, len, dist)            output bytes [pos, pos + len) repeat the dist bytes in front of pos
//   stored(pos, ip, len)            output bytes [pos, pos + len) are the input bytes from offset ip
// The core checks every pos + len against the member's ISIZE and every dist against pos before it calls, and never asks for a
// refill once the bit position has passed the end of the data: each loop consumes at least one bit or ends the block, so a
// corrupt member ends in MA_Z_DATA after a bounded number of steps.
#pragma once
#include <cstdint>

#include "../../include/microasm.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MA_ZHD __host__ __device__ __forceinline__
#else
#define MA_ZHD inline
#endif

namespace ma {
namespace zcore {

constexpr uint32_t kLitBits = 10, kDistBits = 8;  // widths of the primary lookup tables; longer codes take the walk
constexpr uint32_t kMaxIsize = 65536;

// one wave's tables: 3.6 KB
struct Tables {
  uint16_t lit_fast[1u << kLitBits];    // (symbol << 4) | code length; 0: not here (a longer code, or none)
  uint16_t dist_fast[1u << kDistBits];  // likewise; while the code lengths are read, the code-length code's table
  uint16_t lit_sym[288], dist_sym[32];  // symbols in code order
  uint16_t lit_cnt[16], dist_cnt[16];   // codes of each length
  uint16_t first[16], offs[16];         // of the table being built: first code and first place in *_sym of each length
  uint8_t lens[352];                    // the code-length code's 19 from 0, a dynamic block's up to 316 from 32; 320 of a fixed one
  int32_t verdict;                      // what lane 0 found while counting
};

MA_ZHD uint32_t rd16(const uint8_t* p) { return static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8); }
MA_ZHD uint32_t rd32(const uint8_t* p) { return rd16(p) | (rd16(p + 2) << 16); }

// ---- the member header -------------------------------------------------------------------------------------------------------
struct Member {
  uint32_t state;     // 0, MA_Z_HEADER or MA_Z_ISIZE
  uint32_t data_at;   // offset of the DEFLATE data from the member's first byte
  uint32_t data_len;  // its bytes: up to the trailer
  uint32_t crc, isize;
};

// `m` points at `avail` readable bytes.  BgzfFile::Load's rules: magic 1f 8b, CM 8, FLG bit 2, a BC subfield of length 2 in
// the extra field, 12 + XLEN + 8 <= BSIZE + 1 <= avail.
MA_ZHD Member parse_member(const uint8_t* m, uint32_t avail) {
  Member r{MA_Z_HEADER, 0, 0, 0, 0};
  if (avail < 12u + 8u) return r;
  if (m[0] != 0x1fu || m[1] != 0x8bu || m[2] != 8u || !(m[3] & 4u)) return r;
  uint32_t const xlen = rd16(m + 10);
  if (12u + xlen + 8u > avail) return r;
  uint32_t at = 12u, total = 0;  // (no BC subfield: 0, which is under every 12 + XLEN + 8)
  while (at + 4u <= 12u + xlen) {  // (every turn moves `at` on by 4 or more)
    uint32_t const slen = rd16(m + at + 2);
    if (at + 4u + slen > 12u + xlen) return r;  // a subfield beyond the extra field
    if (m[at] == 'B' && m[at + 1] == 'C' && slen == 2u) total = rd16(m + at + 4) + 1u;  // the last one counts
    at += 4u + slen;
  }
  if (total < 12u + xlen + 8u || total > avail) return r;
  r.data_at = 12u + xlen;
  r.data_len = total - r.data_at - 8u;
  r.crc = rd32(m + total - 8u);
  r.isize = rd32(m + total - 4u);
  r.state = r.isize > kMaxIsize ? MA_Z_ISIZE : 0u;
  return r;
}

// ---- CRC-32 (RFC 1952 section 8), reflected polynomial ----------------------------------------------------------------------------
constexpr uint32_t kCrcPoly = 0xEDB88320u;

// the register after `n` more bytes (no pre- or post-conditioning: the caller's)
MA_ZHD uint32_t crc_bytes(uint32_t reg, const uint8_t* p, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    reg ^= p[i];
    for (int k = 0; k < 8; ++k) reg = (reg >> 1) ^ (kCrcPoly & (0u - (reg & 1u)));
  }
  return reg;
}

// a(x) b(x) mod P(x); bit 31 is x^0
MA_ZHD uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 0x80000000u; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
  }
  return p;
}

// x^(8 n) mod P: a register followed by n zero bytes is the register times this
MA_ZHD uint32_t crc_x8n(uint32_t n) {
  uint32_t r = 0x80000000u, p = 0x00800000u;  // 1, x^8
  for (; n; n >>= 1) {
    if (n & 1u) r = crc_mul(r, p);
    p = crc_mul(p, p);
  }
  return r;
}

// ---- canonical codes ---------------------------------------------------------------------------------------------------------------
MA_ZHD uint32_t rev_bits(uint32_t v, uint32_t n) {  // the low n bits of v, reversed
  uint32_t r = 0;
  for (uint32_t i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1u - i);
  return r;
}

// The code of lens[0 .. n) into cnt / sym / fast.  -> 0 a complete code, or one zlib takes all the same (no code at all; a
// single code of length 1 -- `lone_ok`: not for the code-length code); -1 over-subscribed or incomplete.
template <class Cx>
MA_ZHD int build_code(Cx& cx, Tables& T, uint32_t n, const uint8_t* lens, uint16_t* cnt, uint16_t* sym, uint16_t* fast, uint32_t fbits,
                      bool lone_ok) {
  uint32_t const lane = cx.lane();
  cx.sync();  // (lens is written; the table to be replaced is no longer read)
  if (lane == 0) {
    for (uint32_t l = 0; l < 16u; ++l) cnt[l] = 0;
    for (uint32_t s = 0; s < n; ++s) cnt[lens[s]] = static_cast<uint16_t>(cnt[lens[s]] + 1u);
    int32_t left = 1, verdict = 0;
    uint32_t code = 0, at = 0, longest = 0;
    for (uint32_t l = 1; l < 16u; ++l) {
      left = left * 2 - static_cast<int32_t>(cnt[l]);
      if (left < 0) {
        verdict = -1;
        break;
      }
      if (cnt[l]) longest = l;
      T.first[l] = static_cast<uint16_t>(code);
      T.offs[l] = static_cast<uint16_t>(at);
      code = (code + cnt[l]) << 1;
      at += cnt[l];
    }
    if (verdict == 0 && left > 0 && longest != 0u && !(lone_ok && longest == 1u)) verdict = -1;
    if (verdict == 0) {
      T.offs[0] = static_cast<uint16_t>(at);  // the coded symbols
      for (uint32_t s = 0; s < n; ++s) {
        uint32_t const l = lens[s];
        if (l) sym[T.offs[l]++] = static_cast<uint16_t>(s);
      }
      for (uint32_t l = 15u; l >= 1u; --l) T.offs[l] = static_cast<uint16_t>(T.offs[l] - cnt[l]);  // back to the first places
    }
    T.verdict = verdict;
  }
  for (uint32_t k = lane; k < (1u << fbits); k += Cx::kLanes) fast[k] = 0;
  cx.sync();
  if (T.verdict != 0) return -1;
  uint32_t const coded = T.offs[0];
  for (uint32_t i = lane; i < coded; i += Cx::kLanes) {
    uint32_t const s = sym[i], l = lens[s];
    if (l > fbits) continue;
    uint32_t const code = T.first[l] + (i - T.offs[l]);
    uint16_t const e = static_cast<uint16_t>((s << 4) | l);
    for (uint32_t k = rev_bits(code, l); k < (1u << fbits); k += 1u << l) fast[k] = e;
  }
  cx.sync();
  return 0;
}

// the bit reader: `bc` valid bits in `bb`, the next refill reads at `ip`
struct Bits {
  uint64_t bb;
  uint32_t bc, ip;
};
MA_ZHD uint32_t bits_used(Bits const& b) { return 8u * b.ip - b.bc; }
MA_ZHD uint32_t peek(Bits const& b, uint32_t n) { return static_cast<uint32_t>(b.bb) & ((1u << n) - 1u); }
MA_ZHD void drop(Bits& b, uint32_t n) {
  b.bb >>= n;
  b.bc -= n;
}
MA_ZHD uint32_t take(Bits& b, uint32_t n) {
  uint32_t const v = peek(b, n);
  drop(b, n);
  return v;
}
// at least 32 bits in the buffer; false once the bit position has passed the end of the data
template <class Cx>
MA_ZHD bool refill(Cx& cx, Bits& b, uint32_t data_bits) {
  if (b.bc < 32u) {
    if (bits_used(b) > data_bits) return false;
    b.bb |= static_cast<uint64_t>(cx.next32(b.ip)) << b.bc;
    b.bc += 32u;
    b.ip += 4u;
  }
  return true;
}

// one symbol of a code; -1: no such code.  Wants 15 bits in the buffer.
MA_ZHD int decode_sym(Bits& b, const uint16_t* fast, uint32_t fbits, const uint16_t* cnt, const uint16_t* sym) {
  uint32_t const e = fast[peek(b, fbits)];
  if (e & 15u) {
    drop(b, e & 15u);
    return static_cast<int>(e >> 4);
  }
  uint32_t code = 0, first = 0, index = 0, v = static_cast<uint32_t>(b.bb);
  for (uint32_t l = 1; l < 16u; ++l) {
    code |= v & 1u;
    v >>= 1;
    uint32_t const c = cnt[l];
    if (code < first + c) {
      drop(b, l);
      return sym[index + (code - first)];
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return -1;
}

// base values and extra bits of the length symbols 257 .. 285 and the distance symbols 0 .. 29 (RFC 1951 section 3.2.5), in closed form
MA_ZHD void length_of(uint32_t s, uint32_t& base, uint32_t& extra) {  // s = symbol - 257, 0 .. 28
  if (s < 8u) {
    base = 3u + s;
    extra = 0;
  } else if (s == 28u) {
    base = 258u;
    extra = 0;
  } else {
    extra = (s >> 2) - 1u;
    base = 3u + ((4u + (s & 3u)) << extra);
  }
}
MA_ZHD void distance_of(uint32_t s, uint32_t& base, uint32_t& extra) {  // 0 .. 29
  if (s < 4u) {
    base = 1u + s;
    extra = 0;
  } else {
    extra = (s >> 1) - 1u;
    base = 1u + ((2u + (s & 1u)) << extra);
  }
}

MA_ZHD uint32_t clen_order(uint32_t i) {  // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
  return i < 3u ? 16u + i : (i == 3u ? 0u : ((i & 1u) ? 8u - ((i - 3u) >> 1) : 8u + ((i - 4u) >> 1)));
}

// The DEFLATE stream of one member -> MA_Z_DATA, MA_Z_SHORT or 0 with exactly `isize` bytes written.  The CRC is the caller's.
template <class Cx>
MA_ZHD uint32_t inflate_member(Cx& cx, Tables& T, uint32_t data_len, uint32_t isize) {
  uint32_t const lane = cx.lane(), data_bits = 8u * data_len;
  Bits b{0, 0, 0};
  uint32_t pos = 0;
  for (;;) {  // a DEFLATE block per turn
    if (!refill(cx, b, data_bits)) return MA_Z_DATA;
    uint32_t const last = take(b, 1), type = take(b, 2);
    if (type == 3u) return MA_Z_DATA;
    if (type == 0u) {
      drop(b, b.bc & 7u);
      if (!refill(cx, b, data_bits)) return MA_Z_DATA;
      uint32_t const len = take(b, 16), nlen = take(b, 16);
      if (len != (nlen ^ 0xFFFFu)) return MA_Z_DATA;
      uint32_t const at = bits_used(b) >> 3;
      if (bits_used(b) > data_bits || len > data_len - at || len > isize - pos) return MA_Z_DATA;
      cx.stored(pos, at, len);
      pos += len;
      // the reader starts again behind the bytes, a byte at a time up to the next aligned dword
      b.bb = 0;
      b.bc = 0;
      b.ip = at + len;
      while (b.ip & 3u) {
        b.bb |= static_cast<uint64_t>(cx.byte(b.ip)) << b.bc;
        b.bc += 8u;
        b.ip += 1u;
      }
    } else {
      if (type == 1u) {
        cx.sync();
        for (uint32_t s = lane; s < 320u; s += Cx::kLanes)
          T.lens[s] = static_cast<uint8_t>(s < 144u ? 8u : (s < 256u ? 9u : (s < 280u ? 7u : (s < 288u ? 8u : 5u))));
        (void)build_code(cx, T, 288u, T.lens, T.lit_cnt, T.lit_sym, T.lit_fast, kLitBits, true);
        (void)build_code(cx, T, 32u, T.lens + 288, T.dist_cnt, T.dist_sym, T.dist_fast, kDistBits, true);
      } else {
        uint32_t const nlen = take(b, 5) + 257u, ndist = take(b, 5) + 1u, ncode = take(b, 4) + 4u;
        if (nlen > 286u || ndist > 30u) return MA_Z_DATA;
        cx.sync();
        for (uint32_t s = lane; s < 19u; s += Cx::kLanes) T.lens[s] = 0;
        cx.sync();
        for (uint32_t i = 0; i < ncode; ++i) {
          if (!refill(cx, b, data_bits)) return MA_Z_DATA;
          uint32_t const l = take(b, 3);
          if (lane == 0) T.lens[clen_order(i)] = static_cast<uint8_t>(l);
        }
        // (the code-length code borrows the distance tables)
        if (build_code(cx, T, 19u, T.lens, T.dist_cnt, T.dist_sym, T.dist_fast, 7u, false) != 0) return MA_Z_DATA;
        // its 19 lengths are used up; the nlen + ndist lengths follow in the same array from 32 on
        uint8_t* const lens = T.lens + 32;
        uint32_t have = 0, prev = 0;
        while (have < nlen + ndist) {
          if (!refill(cx, b, data_bits)) return MA_Z_DATA;
          int const s = decode_sym(b, T.dist_fast, 7u, T.dist_cnt, T.dist_sym);
          if (s < 0) return MA_Z_DATA;
          uint32_t rep = 1, val = static_cast<uint32_t>(s);
          if (s == 16) {
            if (have == 0u) return MA_Z_DATA;
            val = prev;
            rep = 3u + take(b, 2);
          } else if (s == 17) {
            val = 0;
            rep = 3u + take(b, 3);
          } else if (s == 18) {
            val = 0;
            rep = 11u + take(b, 7);
          }
          if (have + rep > nlen + ndist) return MA_Z_DATA;
          for (uint32_t k = lane; k < rep; k += Cx::kLanes) lens[have + k] = static_cast<uint8_t>(val);
          have += rep;
          prev = val;
        }
        cx.sync();
        if (T.lens[32u + 256u] == 0u) return MA_Z_DATA;  // no code for the end of the block
        if (build_code(cx, T, nlen, lens, T.lit_cnt, T.lit_sym, T.lit_fast, kLitBits, true) != 0) return MA_Z_DATA;
        if (build_code(cx, T, ndist, lens + nlen, T.dist_cnt, T.dist_sym, T.dist_fast, kDistBits, true) != 0) return MA_Z_DATA;
      }
      for (;;) {  // a symbol per turn
        if (!refill(cx, b, data_bits)) return MA_Z_DATA;
        int const s = decode_sym(b, T.lit_fast, kLitBits, T.lit_cnt, T.lit_sym);
        if (s < 0 || s >= 286) return MA_Z_DATA;
        if (s < 256) {
          if (pos >= isize) return MA_Z_DATA;
          cx.literal(pos, static_cast<uint32_t>(s));
          pos += 1u;
          continue;
        }
        if (s == 256) break;
        uint32_t base, extra;
        length_of(static_cast<uint32_t>(s) - 257u, base, extra);
        uint32_t const len = base + take(b, extra);
        if (!refill(cx, b, data_bits)) return MA_Z_DATA;
        int const d = decode_sym(b, T.dist_fast, kDistBits, T.dist_cnt, T.dist_sym);
        if (d < 0 || d >= 30) return MA_Z_DATA;
        distance_of(static_cast<uint32_t>(d), base, extra);
        uint32_t const dist = base + take(b, extra);
        if (dist > pos || len > isize - pos) return MA_Z_DATA;
        cx.copy(pos, len, dist);
        pos += len;
      }
    }
    if (bits_used(b) > data_bits) return MA_Z_DATA;
    if (last) break;
  }
  return pos == isize ? 0u : MA_Z_SHORT;
}

}  // namespace zcore
}  // namespace ma
