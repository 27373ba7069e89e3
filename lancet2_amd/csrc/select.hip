// ma_select_records_batch: the candidates of every window in, which of them go on and what becomes of the window out
// (include/microasm.h) -- what the host shell's IsActiveRegion, ReadCollector::Filtered, the sums of SelectKept and the
// anchor-coverage gate do per window, as five kernels on the record bytes the device gets anyway:
//
//   k_sel_check    a lane per window: rec_win_off rises from 0 to n_records
//   k_sel_fields   a lane per candidate: the fixed header checked against rec_len and the blob, the two record bits, the walk
//                  over the auxiliary fields to the last MD:Z -- one 32-byte row per candidate, the position of the first bad one
//   k_sel_window   a workgroup per window: rec_keep, the per-sample sums (LDS atomics), the stable rank of every collected
//                  record (wave ballots), then sample after sample the events of the eligible records into an LDS table --
//                  a lane per record walks its MD string and its CIGAR -- and the window's state
//   k_sel_scan     one block: the exclusive sum of the listed windows' counts -> sel_win_off, *n_selected
//   k_sel_gather   a lane per candidate: the collected records of the listed windows to their places
//
// Nothing of the caller's is written before the whole input is known to be good: the first two kernels write workspace only,
// the others look at the status block first.  Every load from the blob is a byte load at an offset inside the record's
// [rec_off, rec_off + rec_len), which k_sel_fields checked against the blob; a bad record has a zero row (no bits, no MD, no
// CIGAR).
//
// THE EVENT TABLE.  Only "did a (multiset, position) come twice" matters, so the table is a set: kTableSlots position slots,
// open addressing, claimed with one atomicCAS; beside every slot four bits, one per multiset, set with one atomicOr whose
// return value tells whether the bit was set before -- a hit.  The position 0xFFFFFFFF is the empty slot's value and has four
// bits of its own behind the last slot.  A new bit counts one key; more than MA_SELECT_EVENT_KEYS is the overflow.  At most
// the key cap + one insertion in flight per thread slots are ever claimed, fewer than the table has: every probe ends.
// 48 KB of slots + 6 KB of bits + 3 KB of sample sums: under 64 KB, two workgroups per CU.
#include "ma_internal.h"

namespace ma {

namespace {

constexpr u32 kWinThreads = 256, kWaves = kWinThreads / 64;
constexpr u32 kTableSlots = 12288, kMaskWords = kTableSlots / 8 + 1;
constexpr u32 kEmpty = 0xFFFFFFFFu;
constexpr u64 kNoBad = ~0ull;
static_assert(kTableSlots > MA_SELECT_EVENT_KEYS + kWinThreads + 1, "a probe must always find a free slot");
enum : u32 { kEvMismatch = 0, kEvInsertion = 1, kEvDeletion = 2, kEvSoftclip = 3 };

// status block (device, read back once per call)
enum : u32 { kStBadRec = 0, kStFlags = 1, kStSelected = 2, kStHostWins = 3, kStWords = 4 };
enum : u64 { kFlagWinList = 1 };

struct alignas(8) SelRow {  // what k_sel_fields keeps of a candidate
  u64 off;                  // rec_off
  u32 l_seq;                // 0: a bad record
  u32 md_at, md_len;        // the MD string without its NUL, from `off`; md_at 0: none
  u32 cg_at;                // the CIGAR words, from `off`
  i32 pos;
  u16 n_cigar;
  u8 keep, sample;
};
static_assert(sizeof(SelRow) == 32, "SelRow layout");

struct SelWs {
  u64* st;       // [kStWords]
  SelRow* rows;  // [n_records]
  u32* rank;     // [n_records] of a collected record: the collected records of its window in front of it
  u32* cnt;      // [n_windows] records the window lists
};

__device__ __forceinline__ u32 ld16(const u8* p) { return static_cast<u32>(p[0]) | (static_cast<u32>(p[1]) << 8); }
__device__ __forceinline__ u32 ld32(const u8* p) { return ld16(p) | (ld16(p + 2) << 16); }
__device__ __forceinline__ bool good(const u64* st) { return st[kStFlags] == 0 && st[kStBadRec] == kNoBad; }

__global__ __launch_bounds__(256) void k_sel_check(ma_records_t in, SelWs ws) {
  u32 const g = blockIdx.x * blockDim.x + threadIdx.x;
  u32 const n = static_cast<u32>(in.n_windows);
  bool bad = false;
  if (g == 0) bad = in.rec_win_off[0] != 0u || static_cast<i64>(in.rec_win_off[n]) != in.n_records;
  if (g < n) bad = bad || in.rec_win_off[g + 1] < in.rec_win_off[g];
  if (bad) atomicOr(reinterpret_cast<unsigned long long*>(ws.st + kStFlags), kFlagWinList);
}

__global__ __launch_bounds__(256) void k_sel_fields(ma_records_t in, SelWs ws) {
  if (ws.st[kStFlags] != 0) return;
  u64 const i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= static_cast<u64>(in.n_records)) return;
  SelRow row{};
  u64 const off = in.rec_off[i];
  u32 const len = in.rec_len[i];
  u32 const smp = in.rec_sample[i];
  bool bad = off > in.blob_bytes || len > in.blob_bytes - off || len < 32u || smp >= static_cast<u32>(in.n_samples_in);
  if (!bad) {
    const u8* b = in.blob + off;
    i32 const pos = static_cast<i32>(ld32(b + 4));
    u32 const l_name = b[8], mapq = b[9], n_cigar = ld16(b + 12), flag = ld16(b + 14);
    i32 const l_seq = static_cast<i32>(ld32(b + 16));
    bad = l_seq <= 0 || l_name == 0u;
    u64 const ls = bad ? 0ull : static_cast<u64>(l_seq);
    u64 const core = 32ull + l_name + 4ull * n_cigar + (ls + 1) / 2 + ls;
    if (!bad) bad = core > len;
    if (!bad) {
      bool const usable = (flag & (0x200u | 0x400u | 0x4u)) == 0u;
      row.off = off;
      row.l_seq = static_cast<u32>(l_seq);
      row.cg_at = 32u + l_name;
      row.pos = pos;
      row.n_cigar = static_cast<u16>(n_cigar);
      row.keep = static_cast<u8>((usable && mapq >= 20u ? MA_SK_COLLECT : 0) | (usable && mapq != 0u ? MA_SK_ELIGIBLE : 0));
      row.sample = static_cast<u8>(smp);
      // the auxiliary fields, for the last MD:Z (only an eligible record's is ever read)
      u32 p = static_cast<u32>(core);
      while ((row.keep & MA_SK_ELIGIBLE) && len - p >= 3u) {
        u32 const t0 = b[p], t1 = b[p + 1], ty = b[p + 2];
        p += 3u;
        u64 fl = 0;
        if (ty == 'Z' || ty == 'H') {
          u32 q = p;
          while (q < len && b[q] != 0u) ++q;
          if (q == len) break;  // no NUL: nothing further can be trusted
          if (ty == 'Z' && t0 == 'M' && t1 == 'D') {
            row.md_at = p;
            row.md_len = q - p;
          }
          fl = static_cast<u64>(q - p) + 1u;
        } else if (ty == 'A' || ty == 'c' || ty == 'C') {
          fl = 1;
        } else if (ty == 's' || ty == 'S') {
          fl = 2;
        } else if (ty == 'i' || ty == 'I' || ty == 'f') {
          fl = 4;
        } else if (ty == 'B') {
          if (len - p < 5u) break;
          u32 const sub = b[p];
          i32 const cnt = static_cast<i32>(ld32(b + p + 1));
          if (cnt < 0) break;
          u64 const es = (sub == 'c' || sub == 'C') ? 1u : ((sub == 's' || sub == 'S') ? 2u : 4u);
          fl = 5u + es * static_cast<u64>(cnt);
        } else {
          break;
        }
        if (fl > len - p) break;
        p += static_cast<u32>(fl);
      }
    }
  }
  if (bad) atomicMin(reinterpret_cast<unsigned long long*>(ws.st + kStBadRec), static_cast<unsigned long long>(i));
  ws.rows[i] = row;
}

// ---- one window ---------------------------------------------------------------------------------------------------------------
struct WinLds {
  u32 tab[kTableSlots];
  u32 mask[kMaskWords];
  u64 bases[256];
  u32 reads[256];
  u32 elig[8];        // samples with an eligible record
  u32 wsum[kWaves];
  u64 total_bases;
  u32 hit, full, full_any, md_range, nkeys, capped;
};
static_assert(sizeof(WinLds) <= 65536, "two workgroups share a CU");

// one event; after a hit, or once this sample's table is full, nothing more is looked up
__device__ __forceinline__ void add_event(WinLds& L, u32 kind, u32 pos) {
  if (*const_cast<volatile u32*>(&L.hit) | *const_cast<volatile u32*>(&L.full)) return;
  u32 slot = kTableSlots;  // (the bits of position 0xFFFFFFFF)
  if (pos != kEmpty) {
    slot = static_cast<u32>((static_cast<u64>(pos * 0x9E3779B1u) * kTableSlots) >> 32);
    u32 steps = 0;
    for (;;) {
      u32 const old = atomicCAS(&L.tab[slot], kEmpty, pos);
      if (old == kEmpty || old == pos) break;
      slot = slot + 1u == kTableSlots ? 0u : slot + 1u;
      if (++steps == kTableSlots) {  // (cannot happen, see the top; a full table is an overflow all the same)
        L.full = L.full_any = 1u;
        return;
      }
    }
  }
  u32 const bit = (1u << kind) << ((slot & 7u) * 4u);
  if (atomicOr(&L.mask[slot >> 3], bit) & bit) {
    L.hit = 1u;
  } else if (atomicAdd(&L.nkeys, 1u) >= static_cast<u32>(MA_SELECT_EVENT_KEYS)) {
    L.full = L.full_any = 1u;
  }
}

__device__ void record_events(WinLds& L, const u8* blob, SelRow const& row) {
  const u8* b = blob + row.off;
  u32 const start = static_cast<u32>(row.pos);
  if (row.pos >= 0 && row.md_at != 0u) {
    const u8* md = b + row.md_at;
    const u8* qual = b + row.cg_at + 4u * row.n_cigar + (row.l_seq + 1u) / 2u;
    u32 gpos = start, num = 0, digits = 0;
    for (u32 k = 0; k < row.md_len; ++k) {
      u32 ch = md[k];
      if (ch >= '0' && ch <= '9') {
        if (digits < 9u) num = num * 10u + (ch - '0');
        ++digits;
        continue;
      }
      if (digits > 9u) {
        L.md_range = 1u;
        break;
      }
      gpos += num;
      num = digits = 0;
      u32 const idx = gpos - start;
      if (idx >= row.l_seq) {
        L.md_range = 1u;
        break;
      }
      if (qual[idx] < 20u) continue;
      if (ch >= 'a' && ch <= 'z') ch -= 32u;
      if (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T') add_event(L, kEvMismatch, gpos);
    }
  }
  const u8* cg = b + row.cg_at;
  u32 gpos = start;
  for (u32 c = 0; c < row.n_cigar; ++c) {
    u32 const v = ld32(cg + 4u * c), op = v & 15u, ln = v >> 4;
    if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) gpos += ln;
    if (op == 1u) add_event(L, kEvInsertion, gpos);
    else if (op == 2u) add_event(L, kEvDeletion, gpos);
    else if (op == 8u) add_event(L, kEvMismatch, gpos);
    else if (op == 4u) add_event(L, kEvSoftclip, gpos);
  }
}

__global__ __launch_bounds__(kWinThreads) void k_sel_window(ma_records_t in, ma_select_params_t sp, SelWs ws, ma_select_out_t o) {
  if (!good(ws.st)) return;
  __shared__ WinLds L;
  u32 const w = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  u32 const r0 = in.rec_win_off[w], n = in.rec_win_off[w + 1] - r0;
  u32 const S = static_cast<u32>(in.n_samples_in);
  if (tid < S) {
    L.bases[tid] = 0;
    L.reads[tid] = 0;
  }
  if (tid < 8u) L.elig[tid] = 0;
  if (tid == 0) {
    L.total_bases = 0;
    L.hit = L.full = L.full_any = L.md_range = L.nkeys = L.capped = 0;
  }
  __syncthreads();
  // the record bits, the sums, the stable ranks of the collected records: chunks of a block in arrival order
  u32 carry = 0;
  for (u32 base = 0; base < n; base += kWinThreads) {
    u32 const i = base + tid;
    bool collect = false;
    if (i < n) {
      SelRow const& row = ws.rows[r0 + i];
      u32 const keep = row.keep, smp = row.sample;
      o.rec_keep[r0 + i] = static_cast<u8>(keep);
      collect = (keep & MA_SK_COLLECT) != 0u;
      if (collect) {
        atomicAdd(&L.reads[smp], 1u);
        atomicAdd(reinterpret_cast<unsigned long long*>(&L.bases[smp]), static_cast<unsigned long long>(row.l_seq));
      }
      if (keep & MA_SK_ELIGIBLE) atomicOr(&L.elig[smp >> 5], 1u << (smp & 31u));
    }
    u64 const vote = __ballot(collect);
    if (lane == 0) L.wsum[wave] = static_cast<u32>(__popcll(vote));
    __syncthreads();
    u32 before = 0, all = 0;
    for (u32 k = 0; k < kWaves; ++k) {
      u32 const c = L.wsum[k];
      before += k < wave ? c : 0u;
      all += c;
    }
    if (collect) ws.rank[r0 + i] = carry + before + static_cast<u32>(__popcll(vote & ((1ull << lane) - 1ull)));
    carry += all;
    __syncthreads();
  }
  // the events, sample after sample: the table is one (window, sample)'s
  if (!sp.skip_active_region) {
    for (u32 s = 0; s < S; ++s) {
      if (!((L.elig[s >> 5] >> (s & 31u)) & 1u)) continue;
      if (!L.hit) {
        for (u32 k = tid; k < kTableSlots; k += kWinThreads) L.tab[k] = kEmpty;
        for (u32 k = tid; k < kMaskWords; k += kWinThreads) L.mask[k] = 0;
        if (tid == 0) L.full = L.nkeys = 0;
      }
      __syncthreads();
      for (u32 i = tid; i < n; i += kWinThreads) {
        SelRow const row = ws.rows[r0 + i];
        if (row.sample == s && (row.keep & MA_SK_ELIGIBLE)) record_events(L, in.blob, row);
      }
      __syncthreads();
    }
  }
  // the window
  if (tid < S) {
    u32 const reads = L.reads[tid];
    u64 const bases = L.bases[tid];
    o.win_sample_reads[static_cast<size_t>(w) * S + tid] = reads;
    o.win_sample_bases[static_cast<size_t>(w) * S + tid] = bases;
    if (reads) {
      f64 const per_read = static_cast<f64>(bases) / static_cast<f64>(reads);
      f64 const max_reads = ceil(sp.max_sample_cov * static_cast<f64>(sp.win_len[w]) / per_read);
      if (static_cast<f64>(reads) > max_reads) L.capped = 1u;
      atomicAdd(reinterpret_cast<unsigned long long*>(&L.total_bases), static_cast<unsigned long long>(bases));
    }
  }
  __syncthreads();
  if (tid == 0) {
    u32 state = 0;
    if (sp.skip_active_region) {
      state |= MA_S_ACTIVE;
    } else {
      if (L.hit) state |= MA_S_ACTIVE;
      else if (L.full_any) state |= MA_S_EVENTS;
      if (L.md_range) state |= MA_S_MD_RANGE;
    }
    if (L.capped) state |= MA_S_CAPPED;
    if (static_cast<f64>(L.total_bases) / static_cast<f64>(sp.win_len[w]) < static_cast<f64>(sp.min_anchor_cov)) state |= MA_S_LOW_COVERAGE;
    if ((state & MA_S_ACTIVE) && !(state & (MA_S_HOST_BITS | MA_S_LOW_COVERAGE))) state |= MA_S_LISTED;
    o.win_state[w] = static_cast<u8>(state);
    ws.cnt[w] = (state & MA_S_LISTED) ? carry : 0u;
    if (state & MA_S_HOST_BITS) atomicAdd(reinterpret_cast<unsigned long long*>(ws.st + kStHostWins), 1ull);
  }
}

// one block: cnt -> sel_win_off (exclusive sums), the total to *n_selected and the status block
__global__ __launch_bounds__(kWinThreads) void k_sel_scan(u32 n_windows, SelWs ws, ma_select_out_t o) {
  if (!good(ws.st)) return;
  __shared__ u32 wsum[kWaves];
  u32 const tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  u32 carry = 0;
  for (u32 base = 0; base < n_windows; base += kWinThreads) {
    u32 const at = base + tid;
    u32 const val = at < n_windows ? ws.cnt[at] : 0u;
    u32 incl = val;  // the wave's inclusive sums
    for (u32 d = 1; d < 64u; d <<= 1) {
      u32 const up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63u) wsum[wave] = incl;
    __syncthreads();
    u32 before = 0, all = 0;
    for (u32 k = 0; k < kWaves; ++k) {
      u32 const c = wsum[k];
      before += k < wave ? c : 0u;
      all += c;
    }
    if (at < n_windows) o.sel_win_off[at] = carry + before + incl - val;
    carry += all;
    __syncthreads();
  }
  if (tid == 0) {
    o.sel_win_off[n_windows] = carry;
    *o.n_selected = carry;
    ws.st[kStSelected] = carry;
  }
}

__global__ __launch_bounds__(256) void k_sel_gather(ma_records_t in, SelWs ws, ma_select_out_t o) {
  if (!good(ws.st)) return;
  u64 const i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= static_cast<u64>(in.n_records)) return;
  SelRow const& row = ws.rows[i];
  if (!(row.keep & MA_SK_COLLECT)) return;
  // the record's window: the last w with rec_win_off[w] <= i (k_sel_check: the list rises from 0 to n_records)
  u32 lo = 0, hi = static_cast<u32>(in.n_windows);
  while (hi - lo > 1u) {
    u32 const mid = lo + (hi - lo) / 2u;
    if (static_cast<u64>(in.rec_win_off[mid]) <= i) lo = mid; else hi = mid;
  }
  if (!(o.win_state[lo] & MA_S_LISTED)) return;
  u32 const at = o.sel_win_off[lo] + ws.rank[i];
  o.sel_off[at] = row.off;
  o.sel_len[at] = in.rec_len[i];
  o.sel_sample[at] = row.sample;
  o.sel_src[at] = static_cast<u32>(i);
}

}  // namespace

int launch_select(ma_ctx* ctx, const ma_records_t& in, const ma_select_params_t& sp, const ma_select_out_t& out, u64* status) {
  u64 const n = static_cast<u64>(in.n_records);
  u32 const nw = static_cast<u32>(in.n_windows);
  auto up16 = [](size_t b) { return (b + 15) & ~static_cast<size_t>(15); };
  size_t const o_st = 0, o_rows = o_st + up16(8 * kStWords), o_rank = o_rows + up16(sizeof(SelRow) * n), o_cnt = o_rank + up16(4 * n),
               bytes = o_cnt + up16(4 * static_cast<size_t>(nw));
  MA_HIP(ctx, ctx->sl_ws.reserve(bytes));
  char* base = ctx->sl_ws.as<char>();
  SelWs ws;
  ws.st = reinterpret_cast<u64*>(base + o_st);
  ws.rows = reinterpret_cast<SelRow*>(base + o_rows);
  ws.rank = reinterpret_cast<u32*>(base + o_rank);
  ws.cnt = reinterpret_cast<u32*>(base + o_cnt);
  // the status block: no bad record, no flag, nothing selected, no window for the host
  MA_HIP(ctx, hipMemsetAsync(ws.st, 0xFF, 8, ctx->stream));
  MA_HIP(ctx, hipMemsetAsync(ws.st + kStFlags, 0, 24, ctx->stream));

  ctx->tic("k_sel_check");
  hipLaunchKernelGGL(k_sel_check, dim3(nw / 256 + 1), dim3(256), 0, ctx->stream, in, ws);
  ctx->toc();
  if (n) {
    ctx->tic("k_sel_fields");
    hipLaunchKernelGGL(k_sel_fields, dim3(static_cast<u32>((n + 255) / 256)), dim3(256), 0, ctx->stream, in, ws);
    ctx->toc();
  }
  if (nw) {
    ctx->tic("k_sel_window");
    hipLaunchKernelGGL(k_sel_window, dim3(nw), dim3(kWinThreads), 0, ctx->stream, in, sp, ws, out);
    ctx->toc();
  }
  ctx->tic("k_sel_scan");
  hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(kWinThreads), 0, ctx->stream, nw, ws, out);
  ctx->toc();
  if (n) {
    ctx->tic("k_sel_gather");
    hipLaunchKernelGGL(k_sel_gather, dim3(static_cast<u32>((n + 255) / 256)), dim3(256), 0, ctx->stream, in, ws, out);
    ctx->toc();
  }
  MA_HIP(ctx, hipGetLastError());
  MA_HIP(ctx, hipMemcpyAsync(status, ws.st, 8 * kStWords, hipMemcpyDeviceToHost, ctx->stream));
  MA_HIP(ctx, ma_stream_sync(ctx));  // (`status` is the caller's frame: the copy has landed before it can return)
  return MA_OK;
}

}  // namespace ma
