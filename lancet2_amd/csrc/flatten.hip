// ma_flatten_records_batch: raw BAM alignment records in, the read arrays of a batch out (include/microasm.h) -- what the host
// shell's ReadCollector::CollectFlat does after the kept set is chosen, as six kernels on the bytes the device gets anyway:
//
//   k_rec_check    a lane per window: rec_win_off rises from 0 to n_records, no window beyond the sort's cap; block 0 also turns
//                  sample_rank into dense ranks (a byte per sample)
//   k_rec_fields   a lane per record: the fixed header, the CIGAR words, the name's hash, the lengths checked against rec_len
//                  and the blob -- one 40-byte row per record, and the position of the first bad record
//   k_rec_sort     a workgroup per window: a bitonic network in LDS over 8-byte (key, arrival) elements, then the names interned
//                  through an LDS table keyed by the name hash.  Two instances, up to 1024 records (8 KB of keys, 256 threads)
//                  and up to 16384 (128 KB, 1024 threads); each leaves the other's windows alone
//   k_rec_scan_*   the batch-wide exclusive sum of l_seq in output order (block sums, their scan, the offsets)
//   k_rec_gather   32 lanes per read: sequence and quality bytes into the batch layout (dword stores wherever the destination
//                  allows, byte loads: records sit at any alignment), the small per-read rows
//
// Nothing of the caller's is written before the whole input is known to be good: the kernels up to the scan write workspace
// only, k_rec_gather looks at the status block first.  Every load from the blob is a byte load at an offset k_rec_fields
// checked; a bad record has a zero row (no name, no bases), so that the kernels behind it stay inside the blob too.
//
// THE KEY.  notpass:1 | dense sample rank: rbits | name: nbits | arrival: ibits, with rbits and ibits as small as the call's
// sample count and the window's size allow (nbits >= 40).  Illumina names share their first 20+ bytes, so the window's common
// name prefix is measured first (an LDS atomicMin of every name's agreement with the window's first) and the key takes the
// nbits behind it, big-endian, zero-padded: its order is the names' order while it differs.  Elements that agree in all but the
// arrival bits are compared in memory: the rest of the names byte by byte, a proper prefix first, then chrom, pos, arrival.
#include "ma_internal.h"

namespace ma {

namespace {

constexpr u32 kSortSmall = 1024, kSortLarge = MA_FLATTEN_MAX_WINDOW;
constexpr u32 kSortSmallThreads = 256, kSortLargeThreads = 1024;
constexpr u32 kScanThreads = 256, kScanPerThread = 8, kScanBlock = kScanThreads * kScanPerThread;
constexpr u32 kLanesPerRead = 32, kReadsPerBlock = 8;
constexpr u32 kEmpty = 0xFFFFFFFFu;
constexpr u64 kNoBad = ~0ull;

// status block (device, read back once per call)
enum : u32 { kStBadRec = 0, kStFlags = 1, kStBases = 2, kStBigWin = 3, kStWords = 4 };
enum : u64 { kFlagWinList = 1, kFlagWinCap = 2 };

struct alignas(8) RecRow {   // what k_rec_fields keeps of a record
  u64 seq_off;               // offset in the blob of the sequence bytes; the qualities follow them
  u32 l_seq;                 // 0: a bad record
  u32 hash;                  // of the name
  i32 chrom, pos;
  i32 hint, isize;
  u32 name_len;              // without the NUL
  u8 flags, mapq, mflags, sample;  // the output bytes
};
static_assert(sizeof(RecRow) == 40, "RecRow layout");

struct FlatWs {
  u64* st;        // [kStWords]
  u8* drank;      // [256] dense rank of every input sample
  RecRow* rows;   // [n_records] by input position
  u32* src;       // [n_records] by output position: the input position
  u32* id;        // [n_records] by output position: read_qname_id
  u32* len;       // [n_records] by output position: l_seq
  u64* off;       // [n_records + 1] by output position
  u64* part;      // [blocks of the scan + 1]
};

__device__ __forceinline__ u32 ld16(const u8* p) { return static_cast<u32>(p[0]) | (static_cast<u32>(p[1]) << 8); }
__device__ __forceinline__ u32 ld32(const u8* p) { return ld16(p) | (ld16(p + 2) << 16); }

__device__ __forceinline__ bool go_on(const u64* st) { return st[kStFlags] == 0; }

__global__ __launch_bounds__(256) void k_rec_check(ma_records_t in, FlatWs ws) {
  u32 const g = blockIdx.x * blockDim.x + threadIdx.x;
  u32 const n = static_cast<u32>(in.n_windows);
  if (g == 0) {
    if (in.rec_win_off[0] != 0u || static_cast<i64>(in.rec_win_off[n]) != in.n_records) atomicOr(reinterpret_cast<unsigned long long*>(ws.st + kStFlags), kFlagWinList);
  }
  if (g < n) {
    u32 const a = in.rec_win_off[g], b = in.rec_win_off[g + 1];
    if (b < a) {
      atomicOr(reinterpret_cast<unsigned long long*>(ws.st + kStFlags), kFlagWinList);
    } else if (b - a > kSortLarge) {
      atomicOr(reinterpret_cast<unsigned long long*>(ws.st + kStFlags), kFlagWinCap);
      atomicMin(reinterpret_cast<unsigned long long*>(ws.st + kStBigWin), static_cast<unsigned long long>(g));
    }
  }
  if (blockIdx.x == 0) {  // dense ranks: samples that tie in sample_rank tie in the key, as in the comparator
    for (u32 s = threadIdx.x; s < static_cast<u32>(in.n_samples_in); s += blockDim.x) {
      u32 const mine = in.sample_rank[s];
      u32 below = 0;
      for (u32 t = 0; t < static_cast<u32>(in.n_samples_in); ++t) below += in.sample_rank[t] < mine ? 1u : 0u;
      ws.drank[s] = static_cast<u8>(below);
    }
  }
}

__global__ __launch_bounds__(256) void k_rec_fields(ma_records_t in, FlatWs ws) {
  if (!go_on(ws.st)) return;
  u64 const i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= static_cast<u64>(in.n_records)) return;
  RecRow row{};
  u64 const off = in.rec_off[i], len = in.rec_len[i];
  u32 const smp = in.rec_sample[i];
  bool bad = off > in.blob_bytes || len > in.blob_bytes - off || len < 32u || smp >= static_cast<u32>(in.n_samples_in);
  if (!bad) {
    const u8* b = in.blob + off;
    i32 const refid = static_cast<i32>(ld32(b)), pos = static_cast<i32>(ld32(b + 4));
    u32 const l_name = b[8], mapq = b[9], n_cigar = ld16(b + 12), flag = ld16(b + 14);
    i32 const l_seq = static_cast<i32>(ld32(b + 16)), tlen = static_cast<i32>(ld32(b + 28));
    bad = l_seq <= 0 || l_name == 0u;
    u64 const ls = bad ? 0ull : static_cast<u64>(l_seq);
    u64 const head = 32ull + l_name + 4ull * n_cigar;
    if (!bad) bad = head + (ls + 1) / 2 + ls > len;
    if (!bad) {
      // the name: FNV-1a over the bytes in front of the NUL
      u32 h = 0x811C9DC5u;
      for (u32 k = 0; k + 1 < l_name; ++k) h = (h ^ b[32 + k]) * 0x01000193u;
      // the CIGAR: the leading clip is the FIRST operation if it is S; IsSoftClipped sums every S
      const u8* cg = b + 32 + l_name;
      u32 lead = 0, clip = 0;
      for (u32 c = 0; c < n_cigar; ++c) {
        u32 const v = ld32(cg + 4u * c);
        if ((v & 15u) == 4u) {
          clip += v >> 4;
          if (c == 0) lead = v >> 4;
        }
      }
      i32 chrom = -1;
      if (refid >= 0 && refid < in.n_refs) chrom = in.ref_map ? in.ref_map[static_cast<size_t>(smp) * in.n_refs + refid] : refid;
      // the record's window: the last w with rec_win_off[w] <= i (k_rec_check: the list rises from 0 to n_records)
      u32 lo = 0, hi = static_cast<u32>(in.n_windows);
      while (hi - lo > 1u) {
        u32 const mid = lo + (hi - lo) / 2u;
        if (static_cast<u64>(in.rec_win_off[mid]) <= i) lo = mid; else hi = mid;
      }
      i64 const hint = static_cast<i64>(pos) - in.win_start0[lo] - static_cast<i64>(lead);
      bool const hinted = chrom == in.win_chrom[lo] && hint > INT32_MIN && hint < INT32_MAX;
      bool const clipped = static_cast<double>(clip) / static_cast<double>(l_seq) >= 0.06;
      row.seq_off = off + head;
      row.l_seq = static_cast<u32>(l_seq);
      row.hash = h;
      row.chrom = chrom;
      row.pos = pos;
      row.hint = hinted ? static_cast<i32>(hint) : MA_NO_HINT;
      row.isize = tlen;
      row.name_len = l_name - 1u;
      row.flags = static_cast<u8>((mapq >= 20u ? MA_RF_PASS : 0u) | (in.sample_case[smp] == 1 ? MA_RF_CASE : 0u) | ((flag & 0x10u) ? MA_RF_REV : 0u));
      row.mapq = static_cast<u8>(mapq);
      row.mflags = static_cast<u8>((clipped ? MA_RM_SOFTCLIP : 0u) | ((flag & 0x2u) ? MA_RM_PROPER : 0u));
      row.sample = in.sample_index[smp];
    }
  }
  if (bad) atomicMin(reinterpret_cast<unsigned long long*>(ws.st + kStBadRec), static_cast<unsigned long long>(i));
  ws.rows[i] = row;
}

// ---- the sort and the interning of one window -----------------------------------------------------------------------------------
struct WinView {
  const u8* blob;
  const u64* rec_off;   // of the window's first record on
  const RecRow* rows;   // likewise
  u32 cpl;              // the names' common prefix
  u32 skip;             // bytes of every name that elements with equal keys are known to share: cpl + the key's whole bytes
  u32 ibits;
};

__device__ __forceinline__ const u8* name_of(const WinView& v, u32 idx) { return v.blob + v.rec_off[idx] + 32; }

// a before b?  Elements that differ above the arrival bits are ordered by the key; the rest in memory.  ~0 is the padding.
__device__ bool elem_less(const WinView& v, u64 a, u64 b) {
  if (a == b || a == ~0ull) return false;
  if (b == ~0ull) return true;
  u64 const ka = a >> v.ibits, kb = b >> v.ibits;
  if (ka != kb) return ka < kb;
  u32 const ia = static_cast<u32>(a & ((1ull << v.ibits) - 1)), ib = static_cast<u32>(b & ((1ull << v.ibits) - 1));
  RecRow const& ra = v.rows[ia];
  RecRow const& rb = v.rows[ib];
  u32 const la = ra.name_len, lb = rb.name_len, lm = min(la, lb);
  if (v.skip < lm) {
    const u8* na = name_of(v, ia);
    const u8* nb = name_of(v, ib);
    for (u32 k = v.skip; k < lm; ++k) {
      u32 const ca = na[k], cb = nb[k];
      if (ca != cb) return ca < cb;
    }
  }
  if (la != lb) return la < lb;
  if (ra.chrom != rb.chrom) return ra.chrom < rb.chrom;
  if (ra.pos != rb.pos) return ra.pos < rb.pos;
  return ia < ib;
}

__device__ bool same_name(const WinView& v, u32 ia, u32 ib) {
  if (ia == ib) return true;
  RecRow const& ra = v.rows[ia];
  RecRow const& rb = v.rows[ib];
  if (ra.hash != rb.hash || ra.name_len != rb.name_len) return false;
  const u8* na = name_of(v, ia);
  const u8* nb = name_of(v, ib);
  for (u32 k = v.cpl; k < ra.name_len; ++k)
    if (na[k] != nb[k]) return false;
  return true;
}

extern __shared__ __attribute__((aligned(16))) unsigned char rec_lds[];

// windows of (LOW, CAP] records; NT threads.  LDS: CAP x 8 bytes (the elements, then the name table of 2 x CAP slots, then the
// head counts), NT x 4 (the block scan), 16 (the common prefix)
template <u32 CAP, u32 LOW, u32 NT>
__global__ __launch_bounds__(NT) void k_rec_sort(ma_records_t in, FlatWs ws) {
  if (!go_on(ws.st)) return;
  u32 const w = blockIdx.x, tid = threadIdx.x;
  u32 const r0 = in.rec_win_off[w], n = in.rec_win_off[w + 1] - r0;
  if (n <= LOW || n > CAP) return;
  u64* elem = reinterpret_cast<u64*>(rec_lds);
  u32* part = reinterpret_cast<u32*>(rec_lds + static_cast<size_t>(CAP) * 8);
  u32* scal = part + NT;
  WinView v;
  v.blob = in.blob;
  v.rec_off = in.rec_off + r0;
  v.rows = ws.rows + r0;
  // the names' common prefix
  u32 const len0 = v.rows[0].name_len;
  if (tid == 0) scal[0] = len0;
  __syncthreads();
  {
    const u8* n0 = name_of(v, 0);
    for (u32 i = tid; i < n; i += NT) {
      u32 const li = min(v.rows[i].name_len, len0);
      const u8* ni = name_of(v, i);
      u32 k = 0;
      while (k < li && ni[k] == n0[k]) ++k;
      if (k < len0) atomicMin(&scal[0], k);
    }
  }
  __syncthreads();
  u32 N = 1;
  while (N < n) N <<= 1;
  u32 const ibits = 32u - static_cast<u32>(__clz(static_cast<int>(n)));  // n itself fits: no element is all ones
  u32 const rbits = in.n_samples_in > 1 ? 32u - static_cast<u32>(__clz(in.n_samples_in - 1)) : 0u;
  u32 const nbits = 63u - rbits - ibits;
  v.cpl = scal[0];
  v.skip = v.cpl + (nbits >> 3);
  v.ibits = ibits;
  for (u32 i = tid; i < N; i += NT) {
    u64 e = ~0ull;
    if (i < n) {
      RecRow const& r = v.rows[i];
      const u8* nm = name_of(v, i);
      u64 pre = 0;
      for (u32 k = 0; k < 8u; ++k) pre = (pre << 8) | (v.cpl + k < r.name_len ? static_cast<u64>(nm[v.cpl + k]) : 0ull);
      u64 const notpass = r.mapq >= 20 ? 0ull : 1ull;
      // (masked: a record with no such sample -- the batch is rejected for it -- reads a rank nobody wrote)
      u64 const dr = static_cast<u64>(ws.drank[in.rec_sample[r0 + i]]) & ((1ull << rbits) - 1);
      e = (notpass << 63) | (dr << (63u - rbits)) | ((pre >> (64u - nbits)) << ibits) | i;
    }
    elem[i] = e;
  }
  __syncthreads();
  for (u32 k = 2; k <= N; k <<= 1) {
    for (u32 j = k >> 1; j > 0; j >>= 1) {
      for (u32 t = tid; t < N / 2; t += NT) {
        u32 const lo = 2u * t - (t & (j - 1u)), hi = lo + j;
        bool const up = (lo & k) == 0u;
        u64 const a = elem[lo], b = elem[hi];
        if (elem_less(v, b, a) == up) {
          elem[lo] = b;
          elem[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  // the order: output position p of the window holds arrival `mine`.  The elements are dead after this
  constexpr u32 kPer = CAP / NT;
  u32 mine[kPer], slot[kPer];
#pragma unroll
  for (u32 q = 0; q < kPer; ++q) {
    u32 const p = tid + q * NT;
    mine[q] = p < n ? static_cast<u32>(elem[p] & ((1ull << ibits) - 1)) : 0u;
    slot[q] = 0;
  }
  __syncthreads();
  // interning: open addressing on the name hash.  A slot holds (output position << 16 | arrival) of one read of its name and
  // only ever sinks to an earlier read of the SAME name, so whatever it holds can stand for the name in the byte comparison
  u32* table = reinterpret_cast<u32*>(rec_lds);
  u32 const T = 2u * N;
  for (u32 s = tid; s < T; s += NT) table[s] = kEmpty;
  __syncthreads();
#pragma unroll
  for (u32 q = 0; q < kPer; ++q) {
    u32 const p = tid + q * NT;
    if (p >= n) continue;
    u32 const idx = mine[q];
    ws.src[r0 + p] = r0 + idx;
    ws.len[r0 + p] = v.rows[idx].l_seq;
    u32 const val = (p << 16) | idx;
    u32 s = ((v.rows[idx].hash * 0x9E3779B1u) >> 7) & (T - 1u);
    for (;;) {
      u32 const old = atomicCAS(&table[s], kEmpty, val);
      if (old == kEmpty) break;
      if (same_name(v, old & 0xFFFFu, idx)) {
        atomicMin(&table[s], val);
        break;
      }
      s = (s + 1u) & (T - 1u);  // (at most n of the 2 N >= 2 n slots are ever taken: the walk ends)
    }
    slot[q] = s;
  }
  __syncthreads();
  u32 first[kPer];
#pragma unroll
  for (u32 q = 0; q < kPer; ++q) first[q] = tid + q * NT < n ? table[slot[q]] >> 16 : 0u;
  __syncthreads();
  // dense ranks of the first appearances: heads[p] = 1 where a name appears first, then the exclusive sum over the positions
  u32* heads = reinterpret_cast<u32*>(rec_lds);
#pragma unroll
  for (u32 q = 0; q < kPer; ++q) {
    u32 const p = tid + q * NT;
    if (p < n) heads[p] = first[q] == p ? 1u : 0u;
  }
  __syncthreads();
  u32 const chunk = (n + NT - 1u) / NT, c0 = min(n, tid * chunk), c1 = min(n, c0 + chunk);
  u32 sum = 0;
  for (u32 p = c0; p < c1; ++p) sum += heads[p];
  part[tid] = sum;
  __syncthreads();
  for (u32 d = 1; d < NT; d <<= 1) {
    u32 const add = tid >= d ? part[tid - d] : 0u;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  u32 run = part[tid] - sum;
  for (u32 p = c0; p < c1; ++p) {
    u32 const h = heads[p];
    heads[p] = run;
    run += h;
  }
  __syncthreads();
#pragma unroll
  for (u32 q = 0; q < kPer; ++q) {
    u32 const p = tid + q * NT;
    if (p < n) ws.id[r0 + p] = heads[first[q]];
  }
}

// ---- the batch-wide exclusive sum of l_seq in output order -----------------------------------------------------------------
// exclusive scan of one u64 per thread over a block of kScanThreads; *total = the block's sum.  lds: [kScanThreads]
__device__ __forceinline__ u64 block_excl_scan(u64 val, u64* lds, u32 tid, u64* total) {
  lds[tid] = val;
  __syncthreads();
  for (u32 d = 1; d < kScanThreads; d <<= 1) {
    u64 const add = tid >= d ? lds[tid - d] : 0ull;
    __syncthreads();
    lds[tid] += add;
    __syncthreads();
  }
  u64 const incl = lds[tid];
  *total = lds[kScanThreads - 1u];
  __syncthreads();
  return incl - val;
}

__global__ __launch_bounds__(kScanThreads) void k_rec_scan_part(u64 n, FlatWs ws) {
  if (!go_on(ws.st)) return;
  u64* lds = reinterpret_cast<u64*>(rec_lds);
  u64 const base = static_cast<u64>(blockIdx.x) * kScanBlock + static_cast<u64>(threadIdx.x) * kScanPerThread;
  u64 sum = 0;
  for (u32 k = 0; k < kScanPerThread; ++k) sum += base + k < n ? ws.len[base + k] : 0u;
  u64 total;
  (void)block_excl_scan(sum, lds, threadIdx.x, &total);
  if (threadIdx.x == 0) ws.part[blockIdx.x] = total;
}

// one block: the block sums become their exclusive sums; the batch's total goes to the status block and to *n_bases
__global__ __launch_bounds__(kScanThreads) void k_rec_scan_top(u64 n, u64 blocks, FlatWs ws, u64* n_bases) {
  if (!go_on(ws.st)) return;
  u64* lds = reinterpret_cast<u64*>(rec_lds);
  u64 carry = 0;
  for (u64 base = 0; base < blocks; base += kScanThreads) {
    u64 const at = base + threadIdx.x;
    u64 const val = at < blocks ? ws.part[at] : 0ull;
    u64 total;
    u64 const ex = block_excl_scan(val, lds, threadIdx.x, &total);
    if (at < blocks) ws.part[at] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    ws.off[n] = carry;
    ws.st[kStBases] = carry;
    *n_bases = carry;
  }
}

__global__ __launch_bounds__(kScanThreads) void k_rec_scan_fin(u64 n, FlatWs ws) {
  if (!go_on(ws.st)) return;
  u64* lds = reinterpret_cast<u64*>(rec_lds);
  u64 const base = static_cast<u64>(blockIdx.x) * kScanBlock + static_cast<u64>(threadIdx.x) * kScanPerThread;
  u32 l[kScanPerThread];
  u64 sum = 0;
#pragma unroll
  for (u32 k = 0; k < kScanPerThread; ++k) {
    l[k] = base + k < n ? ws.len[base + k] : 0u;
    sum += l[k];
  }
  u64 total;
  u64 run = ws.part[blockIdx.x] + block_excl_scan(sum, lds, threadIdx.x, &total);
#pragma unroll
  for (u32 k = 0; k < kScanPerThread; ++k) {
    if (base + k < n) ws.off[base + k] = run;
    run += l[k];
  }
}

// ---- the copy into the batch layout -----------------------------------------------------------------------------------------
// n bytes from src (any alignment, byte loads) to dst (any alignment: bytes up to the first dword boundary and behind the last,
// dword stores between); ZQ: 0xFF -> 0, the qualities' "absent"
template <bool ZQ>
__device__ __forceinline__ void copy_bytes(u8* dst, const u8* src, u32 n, u32 sub) {
  u32 const head = min(n, static_cast<u32>(-reinterpret_cast<uintptr_t>(dst)) & 3u);
  u32 const chunks = 1u + (n - head + 3u) / 4u;  // chunk 0: the head; chunk c: bytes [head + 4 (c - 1), + 4)
  for (u32 c = sub; c < chunks; c += kLanesPerRead) {
    u32 const s = c ? head + 4u * (c - 1u) : 0u;
    u32 const cnt = c ? min(4u, n - s) : head;
    u32 wd = 0;
    for (u32 j = 0; j < cnt; ++j) {
      u32 b = src[s + j];
      if (ZQ && b == 0xFFu) b = 0u;
      wd |= b << (8u * j);
    }
    if (cnt == 4u) {
      *reinterpret_cast<u32*>(dst + s) = wd;
    } else {
      for (u32 j = 0; j < cnt; ++j) dst[s + j] = static_cast<u8>(wd >> (8u * j));
    }
  }
}

__global__ __launch_bounds__(kLanesPerRead * kReadsPerBlock) void k_rec_gather(ma_records_t in, FlatWs ws, ma_flat_out_t o) {
  // nothing of the caller's is written unless the whole input was good and the bases fit
  if (!go_on(ws.st) || ws.st[kStBadRec] != kNoBad || ws.st[kStBases] > o.bases_cap) return;
  u64 const n = static_cast<u64>(in.n_records);
  if (blockIdx.x == 0 && threadIdx.x == 0) o.read_off[n] = ws.off[n];
  u32 const sub = threadIdx.x & (kLanesPerRead - 1u);
  u64 const r = static_cast<u64>(blockIdx.x) * kReadsPerBlock + threadIdx.x / kLanesPerRead;
  if (r >= n) return;
  u32 const i = ws.src[r];
  RecRow const row = ws.rows[i];
  u64 const at = ws.off[r];
  u64 const b4 = (at + r) >> 1;
  u32 const nb = (row.l_seq + 1u) / 2u;
  if (sub == 0) {
    o.read_off[r] = at;
    o.read_src[r] = i;
    o.read_qname_id[r] = ws.id[r];
    o.read_sample[r] = row.sample;
    o.read_flags[r] = row.flags;
    o.read_hint[r] = row.hint;
    o.read_mapq[r] = row.mapq;
    o.read_mflags[r] = row.mflags;
    o.read_isize[r] = row.isize;
    o.read_start[r] = max(0, row.pos);
    // the byte between this read and the next (an even-length read at an odd nibble), the array's last byte behind the last read
    u64 const next = r + 1 < n ? (ws.off[r + 1] + r + 1) >> 1 : (ws.off[n] + n + 1) / 2;
    for (u64 g = b4 + nb; g < next; ++g) o.bases4[g] = 0;
  }
  const u8* seq = in.blob + row.seq_off;
  copy_bytes<false>(o.bases4 + b4, seq, nb, sub);
  copy_bytes<true>(o.read_quals + at, seq + nb, row.l_seq, sub);
}

}  // namespace

int launch_flatten(ma_ctx* ctx, const ma_records_t& in, const ma_flat_out_t& out, u64* status) {
  u64 const n = static_cast<u64>(in.n_records);
  u32 const nw = static_cast<u32>(in.n_windows);
  u64 const scan_blocks = (n + kScanBlock - 1) / kScanBlock;
  // workspace: every array on a 16-byte boundary
  auto up16 = [](size_t b) { return (b + 15) & ~static_cast<size_t>(15); };
  size_t const o_st = 0, o_dr = o_st + up16(8 * kStWords), o_rows = o_dr + 256, o_src = o_rows + up16(sizeof(RecRow) * n),
               o_id = o_src + up16(4 * n), o_len = o_id + up16(4 * n), o_off = o_len + up16(4 * n),
               o_part = o_off + up16(8 * (n + 1)), bytes = o_part + up16(8 * (scan_blocks + 1));
  MA_HIP(ctx, ctx->fl_ws.reserve(bytes));
  char* base = ctx->fl_ws.as<char>();
  FlatWs ws;
  ws.st = reinterpret_cast<u64*>(base + o_st);
  ws.drank = reinterpret_cast<u8*>(base + o_dr);
  ws.rows = reinterpret_cast<RecRow*>(base + o_rows);
  ws.src = reinterpret_cast<u32*>(base + o_src);
  ws.id = reinterpret_cast<u32*>(base + o_id);
  ws.len = reinterpret_cast<u32*>(base + o_len);
  ws.off = reinterpret_cast<u64*>(base + o_off);
  ws.part = reinterpret_cast<u64*>(base + o_part);
  // the status block: no bad record, no flag, no bases, no oversized window
  MA_HIP(ctx, hipMemsetAsync(ws.st, 0xFF, 8 * kStWords, ctx->stream));
  MA_HIP(ctx, hipMemsetAsync(ws.st + kStFlags, 0, 16, ctx->stream));
  static_assert(kStFlags + 1 == kStBases, "the two words cleared together");

  ctx->tic("k_rec_check");
  hipLaunchKernelGGL(k_rec_check, dim3(nw / 256 + 1), dim3(256), 0, ctx->stream, in, ws);
  ctx->toc();
  if (n) {
    ctx->tic("k_rec_fields");
    hipLaunchKernelGGL(k_rec_fields, dim3(static_cast<u32>((n + 255) / 256)), dim3(256), 0, ctx->stream, in, ws);
    ctx->toc();
  }
  if (nw && n) {
    constexpr size_t lds_small = static_cast<size_t>(kSortSmall) * 8 + 4 * kSortSmallThreads + 16;
    constexpr size_t lds_large = static_cast<size_t>(kSortLarge) * 8 + 4 * kSortLargeThreads + 16;
    auto* small = k_rec_sort<kSortSmall, 0u, kSortSmallThreads>;
    auto* large = k_rec_sort<kSortLarge, kSortSmall, kSortLargeThreads>;
    if (!ctx->fl_lds_set) {  // (the attribute belongs to the function on the context's device: once per context)
      MA_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(large), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      static_cast<int>(lds_large)));
      ctx->fl_lds_set = true;
    }
    ctx->tic("k_rec_sort");
    hipLaunchKernelGGL(small, dim3(nw), dim3(kSortSmallThreads), lds_small, ctx->stream, in, ws);
    ctx->toc();
    // the windows of more than kSortSmall records; the others end at their first branch.  Not launched where no window can be
    // that large
    if (n > kSortSmall) {
      ctx->tic("k_rec_sort_large");
      hipLaunchKernelGGL(large, dim3(nw), dim3(kSortLargeThreads), lds_large, ctx->stream, in, ws);
      ctx->toc();
    }
  }
  size_t const lds_scan = 8 * kScanThreads;
  ctx->tic("k_rec_scan");
  if (scan_blocks) hipLaunchKernelGGL(k_rec_scan_part, dim3(static_cast<u32>(scan_blocks)), dim3(kScanThreads), lds_scan, ctx->stream, n, ws);
  hipLaunchKernelGGL(k_rec_scan_top, dim3(1), dim3(kScanThreads), lds_scan, ctx->stream, n, scan_blocks, ws, out.n_bases);
  if (scan_blocks) hipLaunchKernelGGL(k_rec_scan_fin, dim3(static_cast<u32>(scan_blocks)), dim3(kScanThreads), lds_scan, ctx->stream, n, ws);
  ctx->toc();
  ctx->tic("k_rec_gather");
  hipLaunchKernelGGL(k_rec_gather, dim3(static_cast<u32>(n / kReadsPerBlock + 1)), dim3(kLanesPerRead * kReadsPerBlock), 0,
                     ctx->stream, in, ws, out);
  ctx->toc();
  MA_HIP(ctx, hipGetLastError());
  MA_HIP(ctx, hipMemcpyAsync(status, ws.st, 8 * kStWords, hipMemcpyDeviceToHost, ctx->stream));
  MA_HIP(ctx, ma_stream_sync(ctx));  // (`status` is the caller's frame: the copy has landed before it can return)
  return MA_OK;
}

}  // namespace ma
