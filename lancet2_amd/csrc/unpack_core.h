// The per-lane step of k_unpack_reads (unpack.hip): eight 4-bit codes of a nibble array -> eight table bytes.  Host and
// device: the host build stands in for v_perm_b32 / v_alignbit_b32 with plain C++, so that the byte shuffles can be checked
// without a GPU (tests/host/packed_units.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MA_HD __host__ __device__ __forceinline__
#else
#define MA_HD inline
#endif

namespace ma {

// v_perm_b32: byte i of the result is byte sel[i] of {s0 (bytes 4..7), s1 (bytes 0..3)}; selectors used here are 0 .. 7
MA_HD uint32_t perm_b32(uint32_t s0, uint32_t s1, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(s0, s1, sel);
#else
  uint64_t const both = (static_cast<uint64_t>(s0) << 32) | s1;
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) r |= static_cast<uint32_t>((both >> (8 * ((sel >> (8 * i)) & 7u))) & 0xFFu) << (8 * i);
  return r;
#endif
}

// v_alignbit_b32: the low dword of {hi, lo} >> sh, sh in 0 .. 31
MA_HD uint32_t alignbit_b32(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, sh);
#else
  return static_cast<uint32_t>(((static_cast<uint64_t>(hi) << 32) | lo) >> (sh & 31u));
#endif
}

MA_HD uint32_t bswap_b32(uint32_t w) { return perm_b32(0u, w, 0x00010203u); }

// four codes 0 .. 15, one per byte, through a 16-entry byte table held in four dwords: entries 0 .. 7 and 8 .. 15 by one
// v_perm each, bit 3 of the code picks between them
MA_HD uint32_t lut16x4(uint32_t codes, const uint32_t (&t)[4]) {
  uint32_t const low3 = codes & 0x07070707u;
  uint32_t const a = perm_b32(t[1], t[0], low3);
  uint32_t const b = perm_b32(t[3], t[2], low3);
  uint32_t const pick = ((codes >> 3) & 0x01010101u) * 0xFFu;
  return (a & ~pick) | (b & pick);
}

// w0, w1: the two consecutive aligned dwords of the nibble array, as loaded (little endian), that hold the eight codes
// starting at nibble k (0 .. 7) of w0 -- "high nibble first": nibble 0 is the high half of the lowest byte.  w1 is not looked
// at when k == 0.  out[0] = table bytes of codes 0 .. 3 (code 0 in the lowest byte), out[1] = of codes 4 .. 7.
MA_HD void expand8(uint32_t w0, uint32_t w1, uint32_t k, const uint32_t (&t)[4], uint32_t (&out)[2]) {
  uint32_t const h = bswap_b32(w0), l = bswap_b32(w1);          // nibble 0 now in bits 31:28
  uint32_t const q = k ? alignbit_b32(h, l, 32u - 4u * k) : h;  // ({h, l} << 4 k) >> 32
  uint32_t const even = (q >> 4) & 0x0F0F0F0Fu;                 // codes 0 2 4 6 in bytes 3 2 1 0
  uint32_t const odd = q & 0x0F0F0F0Fu;                         // codes 1 3 5 7
  out[0] = lut16x4(perm_b32(odd, even, 0x06020703u), t);
  out[1] = lut16x4(perm_b32(odd, even, 0x04000501u), t);
}

}  // namespace ma
