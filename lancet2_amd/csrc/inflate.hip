// ma_inflate_blocks_batch and ma_index_records_batch (include/microasm.h): compressed BGZF blocks in, their payloads out as
// one byte array on the device, and the alignment records of byte ranges of such an array -- what the host shell's
// BgzfFile::Load and record walk do a block at a time, so that the inflated bytes never cross the link.
//
// ma_inflate_blocks_batch, three kernels:
//   k_inf_header   a lane per block: blk_off + blk_len against the blob, the member header (inflate_core.h: parse_member) -- one
//                  16-byte row per block, the position of the first block outside the blob
//   k_inf_scan     one block: the exclusive sum of the payload sizes -> blk_raw_off, *n_raw, the header pass's states and count
//   k_inf_decode   a wavefront per block: the DEFLATE stream (inflate_core.h: inflate_member), then the CRC-32 of what it wrote
// ma_index_records_batch, four:
//   k_idx_count    a lane per stream: the stream's bounds, then the block_size chain -- count and state
//   k_idx_scan     one block: the exclusive sum of the counts -> str_rec_off, *n_found, str_state
//   k_idx_fill     a lane per stream: the chain again, rec_off / rec_len to their places
//   k_idx_fields   a lane per record: refID, pos, the CIGAR's reference span
//
// Nothing of the caller's is written before the whole input is known to be good and to fit: the first kernel of either call
// writes workspace only, the scan writes the need alone when it passes the capacity, the others look at the status block first.
//
// THE DECODE KERNEL.  DEFLATE is serial inside a block, so the speed is blocks in flight: a workgroup is one wavefront, its LDS
// is the 3.6 KB of code tables, a 256-byte slice of the input and 256 bytes of CRC parts -- 4.1 KB, so the 32 waves a CU can hold
// are all resident (a 32 KB window in LDS would leave 4).  All 64 lanes run the decode loop with the same values (table reads
// are LDS broadcasts, no lane waits for another, no divergence); what they share out is the work with bytes:
//   input    the wave fetches 256 bytes at a time, four byte loads per lane checked against the end of the data, into LDS; the
//            bit reader takes dwords from there
//   tables   cleared and filled by all lanes (a lane per coded symbol), counted by lane 0
//   literals up to 64 wait in a register, lane k holding the k-th; one store instruction writes them
//   matches  lane i copies bytes i, i + 64, ...; a copy with distance < length is a periodic fill: byte i comes from
//            i mod distance of the distance bytes in front.  The source bytes were written by other lanes of this wave to
//            global memory: a workgroup-scope fence stands between the stores and the loads
//   CRC      lane i takes the i-th 64th of the payload bit by bit; the 64 registers are combined with x^(8 n) mod P
// No scratch, no loop without a bound: see inflate_core.h.
#include "inflate_core.h"
#include "ma_internal.h"

namespace ma {

namespace {

constexpr u64 kNone = ~0ull;
enum : u32 { kStBad = 0, kStFlags = 1, kStTotal = 2, kStFlagged = 3, kStWords = 4 };
enum : u64 { kFlagCap = 1 };

__device__ __forceinline__ bool good(const u64* st) { return st[kStFlags] == 0 && st[kStBad] == kNone; }

// one block: the exclusive sums of val(i), i < n, to put(i, sum); -> the total (every thread's)
template <class Val, class Put>
__device__ __forceinline__ u64 block_scan(u32 n, u64* wsum, Val val, Put put) {
  u32 const tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  u64 carry = 0;
  for (u32 base = 0; base < n; base += 256u) {
    u32 const at = base + tid;
    u64 const v = at < n ? val(at) : 0ull;
    u64 incl = v;
    for (u32 d = 1; d < 64u; d <<= 1) {
      u64 const up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63u) wsum[wave] = incl;
    __syncthreads();
    u64 before = 0, all = 0;
    for (u32 k = 0; k < 4u; ++k) {
      u64 const c = wsum[k];
      before += k < wave ? c : 0ull;
      all += c;
    }
    if (at < n) put(at, carry + before + incl - v);
    carry += all;
    __syncthreads();
  }
  return carry;
}

// ---- inflate ---------------------------------------------------------------------------------------------------------------------
struct alignas(16) InfRow {  // what k_inf_header keeps of a block
  u32 state, data_at, data_len, isize;
};

struct InfWs {
  u64* st;       // [kStWords]
  InfRow* rows;  // [n_blocks]
  u64* off;      // [n_blocks] place of the block's payload in raw
};

__global__ __launch_bounds__(256) void k_inf_header(ma_bgzf_t in, InfWs ws) {
  u64 const b = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (b >= static_cast<u64>(in.n_blocks)) return;
  u64 const off = in.blk_off[b];
  u32 const len = in.blk_len[b];
  InfRow row{MA_Z_HEADER, 0, 0, 0};
  if (off > in.cblob_bytes || len > in.cblob_bytes - off) {
    atomicMin(reinterpret_cast<unsigned long long*>(ws.st + kStBad), static_cast<unsigned long long>(b));
  } else {
    zcore::Member const m = zcore::parse_member(in.cblob + off, len);
    row.state = m.state;
    if (m.state == 0u) {
      row.data_at = m.data_at;
      row.data_len = m.data_len;
      row.isize = m.isize;
    }
  }
  ws.rows[b] = row;
}

__global__ __launch_bounds__(256) void k_inf_scan(u32 n_blocks, InfWs ws, ma_inflate_out_t o) {
  if (ws.st[kStBad] != kNone) return;
  __shared__ u64 wsum[4];
  __shared__ u32 flagged;
  if (threadIdx.x == 0) flagged = 0;
  __syncthreads();
  u64 const total = block_scan(n_blocks, wsum, [&](u32 i) { return static_cast<u64>(ws.rows[i].isize); }, [&](u32 i, u64 s) { ws.off[i] = s; });
  if (total > o.raw_cap) {  // the need, and nothing else
    if (threadIdx.x == 0) {
      *o.n_raw = total;
      ws.st[kStTotal] = total;
      ws.st[kStFlags] = kFlagCap;
    }
    return;
  }
  u32 mine = 0;
  for (u32 i = threadIdx.x; i < n_blocks; i += 256u) {
    u32 const state = ws.rows[i].state;
    o.blk_raw_off[i] = ws.off[i];
    o.blk_state[i] = static_cast<u8>(state);  // (k_inf_decode writes a good header's again)
    mine += state != 0u;
  }
  if (mine) atomicAdd(&flagged, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    o.blk_raw_off[n_blocks] = total;
    *o.n_raw = total;
    *o.n_flagged = flagged;
    ws.st[kStTotal] = total;
    ws.st[kStFlagged] = flagged;
  }
}

struct DecodeLds {
  zcore::Tables T;
  u32 in[64];  // 256 bytes of the DEFLATE data from offset `in_at`
};

// the wave's side of inflate_core.h's contract
struct WaveCx {
  static constexpr u32 kLanes = 64;
  DecodeLds& L;
  const u8* data;   // the DEFLATE data, data_len bytes
  u32 data_len;
  u8* out;          // the block's range of raw
  u32 in_at;        // offset of L.in; far away: nothing fetched yet
  u32 pend_at, pend;  // literals that wait: `pend` of them from output byte pend_at, lane k holds the k-th
  u32 lit;
  u32 ln;
  __device__ __forceinline__ u32 lane() const { return ln; }
  __device__ __forceinline__ void sync() { __syncthreads(); }  // (one wave: the fences of it are what counts)
  __device__ __forceinline__ u32 byte(u32 ip) const { return ip < data_len ? data[ip] : 0u; }
  __device__ __forceinline__ u32 next32(u32 ip) {
    if (ip - in_at >= 256u) {
      __syncthreads();
      u32 const at = ip + 4u * ln;
      L.in[ln] = byte(at) | (byte(at + 1u) << 8) | (byte(at + 2u) << 16) | (byte(at + 3u) << 24);
      in_at = ip;
      __syncthreads();
    }
    return L.in[(ip - in_at) >> 2];
  }
  __device__ __forceinline__ void flush() {
    if (ln < pend) out[pend_at + ln] = static_cast<u8>(lit);
    pend = 0;
  }
  __device__ __forceinline__ void literal(u32 pos, u32 b) {
    if (pend == 0u) pend_at = pos;
    if (ln == pend) lit = b;
    if (++pend == kLanes) flush();
  }
  __device__ __forceinline__ void copy(u32 pos, u32 len, u32 dist) {
    flush();
    __threadfence_block();  // the bytes in front of pos are other lanes' stores
    const u8* src = out + (pos - dist);
    if (dist >= len) {
      for (u32 i = ln; i < len; i += kLanes) out[pos + i] = src[i];
    } else {  // periodic: byte i repeats byte i mod dist
      u32 const step = kLanes % dist;
      u32 k = ln % dist;
      for (u32 i = ln; i < len; i += kLanes) {
        out[pos + i] = src[k];
        k += step;
        k -= k >= dist ? dist : 0u;
      }
    }
  }
  __device__ __forceinline__ void stored(u32 pos, u32 ip, u32 len) {
    flush();
    for (u32 i = ln; i < len; i += kLanes) out[pos + i] = data[ip + i];
  }
};

__global__ __launch_bounds__(64) void k_inf_decode(ma_bgzf_t in, InfWs ws, ma_inflate_out_t o) {
  if (!good(ws.st)) return;
  __shared__ DecodeLds L;
  __shared__ u32 part[64];
  u32 const b = blockIdx.x, lane = threadIdx.x;
  InfRow const row = ws.rows[b];
  if (row.state != 0u) return;  // (k_inf_scan wrote the state and counted it)
  const u8* member = in.cblob + in.blk_off[b];
  u8* out = o.raw + ws.off[b];
  WaveCx cx{L, member + row.data_at, row.data_len, out, 0x80000000u, 0, 0, 0, lane};
  u32 state = zcore::inflate_member(cx, L.T, row.data_len, row.isize);
  if (state == 0u) {
    cx.flush();
    __threadfence_block();
    __syncthreads();
    // lane k: the k-th slice of `per` bytes; the register of the whole is the sum of the slices' registers times x^(8 bytes behind)
    u32 const n = row.isize, per = (n + 63u) / 64u;
    u32 const from = min(lane * per, n), upto = min(from + per, n);
    u32 reg = zcore::crc_bytes(lane == 0u ? 0xFFFFFFFFu : 0u, out + from, upto - from);
    part[lane] = zcore::crc_mul(reg, zcore::crc_x8n(n - upto));
    __syncthreads();
    u32 crc = 0;
    for (u32 k = 0; k < 64u; ++k) crc ^= part[k];
    u32 const want = zcore::rd32(member + row.data_at + row.data_len);
    if ((crc ^ 0xFFFFFFFFu) != want) state = MA_Z_CRC;
  }
  if (state != 0u && lane == 0u) {
    o.blk_state[b] = static_cast<u8>(state);
    atomicAdd(reinterpret_cast<unsigned long long*>(o.n_flagged), 1ull);
    atomicAdd(reinterpret_cast<unsigned long long*>(ws.st + kStFlagged), 1ull);
  }
}

// ---- the record index ------------------------------------------------------------------------------------------------------------
struct IdxWs {
  u64* st;     // [kStWords]
  u64* cnt;    // [n_streams] records of the stream
  u64* off;    // [n_streams] its first place in the rec_ arrays
  u8* state;   // [n_streams]
};

// The chain of one stream; put(k, p + 4, block_size) for its k-th record.  -> the count; *bad: the walk ended at a bad record.
// Every load is a byte load inside [raw, raw + raw_bytes); p rises by 36 or more per turn.
template <class Put>
__device__ __forceinline__ u64 walk_stream(const u8* raw, u64 raw_bytes, u64 begin, u64 end, bool* bad, Put put) {
  u64 p = begin, k = 0;
  *bad = false;
  while (p < end) {
    *bad = true;
    if (raw_bytes - p < 4u) break;
    u64 const bs = zcore::rd32(raw + p);
    if (bs > raw_bytes - p - 4u || bs < 32u) break;
    const u8* r = raw + p + 4u;
    u64 const l_name = r[8], n_cigar = zcore::rd16(r + 12), l_seq = zcore::rd32(r + 16);
    if (32u + l_name + 4u * n_cigar + (l_seq + 1u) / 2u + l_seq > bs) break;
    *bad = false;
    put(k, p + 4u, static_cast<u32>(bs));
    ++k;
    p += 4u + bs;
  }
  return k;
}

__global__ __launch_bounds__(256) void k_idx_count(ma_record_streams_t in, IdxWs ws) {
  u64 const s = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (s >= static_cast<u64>(in.n_streams)) return;
  u64 const begin = in.str_begin[s], end = in.str_end[s];
  u64 cnt = 0;
  bool bad = false;
  if (begin > end || end > in.raw_bytes) {
    atomicMin(reinterpret_cast<unsigned long long*>(ws.st + kStBad), static_cast<unsigned long long>(s));
  } else {
    cnt = walk_stream(in.raw, in.raw_bytes, begin, end, &bad, [](u64, u64, u32) {});
  }
  ws.cnt[s] = cnt;
  ws.state[s] = bad ? MA_X_BAD_RECORD : 0;
}

__global__ __launch_bounds__(256) void k_idx_scan(u32 n_streams, IdxWs ws, ma_index_out_t o) {
  if (ws.st[kStBad] != kNone) return;
  __shared__ u64 wsum[4];
  __shared__ u32 flagged;
  if (threadIdx.x == 0) flagged = 0;
  __syncthreads();
  u64 const total = block_scan(n_streams, wsum, [&](u32 i) { return ws.cnt[i]; }, [&](u32 i, u64 v) { ws.off[i] = v; });
  if (total > o.rec_cap) {  // the need, and nothing else
    if (threadIdx.x == 0) {
      *o.n_found = total;
      ws.st[kStTotal] = total;
      ws.st[kStFlags] = kFlagCap;
    }
    return;
  }
  u32 mine = 0;
  for (u32 i = threadIdx.x; i < n_streams; i += 256u) {
    o.str_rec_off[i] = ws.off[i];
    o.str_state[i] = ws.state[i];
    mine += ws.state[i] != 0;
  }
  if (mine) atomicAdd(&flagged, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    o.str_rec_off[n_streams] = total;
    *o.n_found = total;
    ws.st[kStTotal] = total;
    ws.st[kStFlagged] = flagged;
  }
}

__global__ __launch_bounds__(256) void k_idx_fill(ma_record_streams_t in, IdxWs ws, ma_index_out_t o) {
  if (!good(ws.st)) return;
  u64 const s = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (s >= static_cast<u64>(in.n_streams)) return;
  u64 const at = ws.off[s], cnt = ws.cnt[s];
  bool bad;
  (void)walk_stream(in.raw, in.raw_bytes, in.str_begin[s], in.str_end[s], &bad, [&](u64 k, u64 off, u32 len) {
    if (k < cnt) {  // (what the count pass found: the bytes have not changed)
      o.rec_off[at + k] = off;
      o.rec_len[at + k] = len;
    }
  });
}

__global__ __launch_bounds__(256) void k_idx_fields(ma_record_streams_t in, IdxWs ws, ma_index_out_t o) {
  if (!good(ws.st)) return;
  u64 const i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= ws.st[kStTotal]) return;
  const u8* r = in.raw + o.rec_off[i];  // (k_idx_fill's: the core fits rec_len, rec_len fits raw)
  u32 const l_name = r[8], n_cigar = zcore::rd16(r + 12);
  const u8* cg = r + 32u + l_name;
  u32 span = 0;
  for (u32 c = 0; c < n_cigar; ++c) {
    u32 const v = zcore::rd32(cg + 4u * c), op = v & 15u;
    if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) span += v >> 4;
  }
  o.rec_ref[i] = static_cast<i32>(zcore::rd32(r));
  o.rec_pos[i] = static_cast<i32>(zcore::rd32(r + 4));
  o.rec_span[i] = span;
}

template <class Ws>
int status_block(ma_ctx* ctx, Ws& ws, u64* status) {
  MA_HIP(ctx, hipGetLastError());
  MA_HIP(ctx, hipMemcpyAsync(status, ws.st, 8 * kStWords, hipMemcpyDeviceToHost, ctx->stream));
  MA_HIP(ctx, ma_stream_sync(ctx));  // (`status` is the caller's frame: the copy has landed before it can return)
  return MA_OK;
}

size_t up16(size_t b) { return (b + 15) & ~static_cast<size_t>(15); }

}  // namespace

int launch_inflate(ma_ctx* ctx, const ma_bgzf_t& in, const ma_inflate_out_t& out, u64* status) {
  u32 const n = static_cast<u32>(in.n_blocks);
  size_t const o_rows = up16(8 * kStWords), o_off = o_rows + up16(sizeof(InfRow) * n), bytes = o_off + up16(8 * static_cast<size_t>(n));
  MA_HIP(ctx, ctx->inf_ws.reserve(bytes));
  char* base = ctx->inf_ws.as<char>();
  InfWs ws{reinterpret_cast<u64*>(base), reinterpret_cast<InfRow*>(base + o_rows), reinterpret_cast<u64*>(base + o_off)};
  // the status block: no block outside the blob, no flag, no byte, no flagged block
  MA_HIP(ctx, hipMemsetAsync(ws.st, 0xFF, 8, ctx->stream));
  MA_HIP(ctx, hipMemsetAsync(ws.st + kStFlags, 0, 24, ctx->stream));
  if (n) {
    ctx->tic("k_inf_header");
    hipLaunchKernelGGL(k_inf_header, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, in, ws);
    ctx->toc();
  }
  ctx->tic("k_inf_scan");
  hipLaunchKernelGGL(k_inf_scan, dim3(1), dim3(256), 0, ctx->stream, n, ws, out);
  ctx->toc();
  if (n) {
    ctx->tic("k_inf_decode");
    hipLaunchKernelGGL(k_inf_decode, dim3(n), dim3(64), 0, ctx->stream, in, ws, out);
    ctx->toc();
  }
  return status_block(ctx, ws, status);
}

int launch_index(ma_ctx* ctx, const ma_record_streams_t& in, const ma_index_out_t& out, u64* status) {
  u32 const n = static_cast<u32>(in.n_streams);
  size_t const o_cnt = up16(8 * kStWords), o_off = o_cnt + up16(8 * static_cast<size_t>(n)), o_state = o_off + up16(8 * static_cast<size_t>(n)),
               bytes = o_state + up16(n);
  MA_HIP(ctx, ctx->idx_ws.reserve(bytes));
  char* base = ctx->idx_ws.as<char>();
  IdxWs ws{reinterpret_cast<u64*>(base), reinterpret_cast<u64*>(base + o_cnt), reinterpret_cast<u64*>(base + o_off),
           reinterpret_cast<u8*>(base + o_state)};
  MA_HIP(ctx, hipMemsetAsync(ws.st, 0xFF, 8, ctx->stream));
  MA_HIP(ctx, hipMemsetAsync(ws.st + kStFlags, 0, 24, ctx->stream));
  if (n) {
    ctx->tic("k_idx_count");
    hipLaunchKernelGGL(k_idx_count, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, in, ws);
    ctx->toc();
  }
  ctx->tic("k_idx_scan");
  hipLaunchKernelGGL(k_idx_scan, dim3(1), dim3(256), 0, ctx->stream, n, ws, out);
  ctx->toc();
  if (n) {
    ctx->tic("k_idx_fill");
    hipLaunchKernelGGL(k_idx_fill, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, in, ws, out);
    ctx->toc();
  }
  MA_TRY_RC(status_block(ctx, ws, status));
  u64 const found = status[kStTotal];
  if (found && status[kStBad] == kNone && status[kStFlags] == 0) {  // (the grid is the count's: known only now)
    ctx->tic("k_idx_fields");
    hipLaunchKernelGGL(k_idx_fields, dim3(static_cast<u32>((found + 255u) / 256u)), dim3(256), 0, ctx->stream, in, ws, out);
    ctx->toc();
    MA_HIP(ctx, hipGetLastError());
  }
  return MA_OK;
}

}  // namespace ma
