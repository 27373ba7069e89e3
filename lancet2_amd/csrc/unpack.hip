// Packed read input (ma_process_packed_batch): the 4-bit base codes -- and 4-bit quality codes -- of a lane's slice expanded
// into the ASCII and Phred arrays that stage_lane_inputs / stage_batch fill by copy in a plain call.  Pure bandwidth: half a
// byte read and one written per base and array.  32 lanes share a read; a lane takes 8 codes per step (two aligned dwords of
// the nibble array, funnel-shifted to the chunk's first nibble), looks them up in the 16-entry table -- four scalar dwords,
// v_perm_b32 -- and stores 8 bytes at an 8-byte aligned destination.  Only a read's head (up to the first aligned
// destination byte: read_off[r] is arbitrary) and its tail of fewer than 8 bases are stored byte by byte.
#include <cstring>

#include "ma_internal.h"
#include "unpack_core.h"

namespace ma {

namespace {

constexpr u32 kLanesPerRead = 32, kReadsPerBlock = 8;

struct Lut {
  u32 t[4];
};

// src: byte 0 of the read in the nibble array; dst: its first output byte
__device__ __forceinline__ void expand_read(const u8* src, u8* dst, u32 len, const u32 (&t)[4], u32 sub) {
  u32 const head = min(len, static_cast<u32>(-reinterpret_cast<uintptr_t>(dst)) & 7u);
  u32 const chunks = 1u + (len - head + 7u) / 8u;  // chunk 0: the head; chunk c: bases [head + 8 (c - 1), + 8)
  for (u32 c = sub; c < chunks; c += kLanesPerRead) {
    u32 const s = c ? head + 8u * (c - 1u) : 0u;
    u32 const cnt = c ? min(8u, len - s) : head;
    if (cnt == 0) continue;
    const u8* bp = src + (s >> 1);  // the byte of the chunk's first code, and the aligned dword around it
    u32 const mis = static_cast<u32>(reinterpret_cast<uintptr_t>(bp)) & 3u;
    const u32* wp = reinterpret_cast<const u32*>(bp - mis);
    u32 const k = 2u * mis + (s & 1u);  // the code's nibble index in that dword
    u32 const w0 = wp[0];
    u32 const w1 = k + cnt > 8u ? wp[1] : 0u;  // (never a word that holds no code of this read)
    u32 out[2];
    expand8(w0, w1, k, t, out);
    if (cnt == 8u) {
      *reinterpret_cast<uint2*>(dst + s) = make_uint2(out[0], out[1]);
    } else {
      u64 const both = (static_cast<u64>(out[1]) << 32) | out[0];
      for (u32 j = 0; j < cnt; ++j) dst[s + j] = static_cast<u8>(both >> (8u * j));
    }
  }
}

__global__ __launch_bounds__(256) void k_unpack_reads(const u8* bases4, const u8* quals4, u8* out_bases, u8* out_quals,
                                                       Lut base_lut, Lut qual_lut, const u64* read_off, u64 first, u64 n) {
  u32 const sub = threadIdx.x & (kLanesPerRead - 1u);
  u64 const i = static_cast<u64>(blockIdx.x) * kReadsPerBlock + threadIdx.x / kLanesPerRead;
  if (i >= n) return;
  u64 const o0 = read_off[i], o1 = read_off[i + 1];
  if (o1 <= o0) return;
  u32 const len = static_cast<u32>(o1 - o0);
  u64 const at = (o0 + first + i) >> 1;  // the read's first byte in a nibble array
  expand_read(bases4 + at, out_bases + o0, len, base_lut.t, sub);
  if (quals4) expand_read(quals4 + at, out_quals + o0, len, qual_lut.t, sub);
}

}  // namespace

void set_unpack_luts(DPacked* d, const ma_packed_reads_t* pk) {
  static const char kBases[17] = "=ACMGRSVTWYHKDBN";  // BAM's 4-bit codes (hts/alignment.cpp:123-143 decodes with the same table)
  for (int w = 0; w < 4; ++w) {
    d->base_lut[w] = d->qual_lut[w] = 0;
    for (int j = 0; j < 4; ++j) {
      d->base_lut[w] |= static_cast<u32>(static_cast<u8>(kBases[4 * w + j])) << (8 * j);
      d->qual_lut[w] |= static_cast<u32>(pk->qual_dict[4 * w + j]) << (8 * j);
    }
  }
}

int launch_unpack(ma_ctx* ctx, const DPacked& d, const u64* read_off, u64 first, u64 n) {
  if (n == 0) return MA_OK;
  Lut bl, ql;
  std::memcpy(bl.t, d.base_lut, sizeof(bl.t));
  std::memcpy(ql.t, d.qual_lut, sizeof(ql.t));
  u64 const blocks = (n + kReadsPerBlock - 1) / kReadsPerBlock;
  if (blocks > 0x7FFFFFFFull) {
    ma_set_err(ctx, "k_unpack_reads: too many reads in one slice");
    return MA_ERR_PARAM;
  }
  ctx->tic("k_unpack_reads");
  hipLaunchKernelGGL(k_unpack_reads, dim3(static_cast<u32>(blocks)), dim3(kLanesPerRead * kReadsPerBlock), 0, ctx->stream,
                     d.bases4, d.quals4, d.out_bases, d.out_quals, bl, ql, read_off, first, n);
  ctx->toc();
  MA_HIP(ctx, hipGetLastError());
  return MA_OK;
}

}  // namespace ma
