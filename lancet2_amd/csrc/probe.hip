// Probe variants (ma_assemble_probe_batch): where in a window's assembly a known allele was lost -- the reference's
// --probe-variants diagnostic (cbdg/probe_tracker.cpp) for a batch.  include/microasm.h states the contract: contexts, equality
// of k-mers, ALT-unique k-mers and their numbering, profiles.
//
// Three kernels share one device routine, pb_build, which lays a CHUNK of a window's probes out in LDS: the spliced ALT
// contexts, and one entry per ALT-unique k-mer -- where it starts in its context, whose it is, and a 64-bit hash of the
// k-mer that is the same for both strands -- chained from a bucket table.  A hash only proposes: every match is decided on the
// letters, the k-mer as it stands or reverse complemented.  A chunk is at most kPbChunk probes, kPbCtx context bytes and
// kPbEnt context k-mers (one probe always fits: 764 bytes, 760 k-mers), so that every kernel stays below 80 KB of LDS.
//
//   k_probe_raw    between the build and the clean pass of every attempt: the raw nodes the build pass leaves -- the survivors
//                  of RemoveLowCovNodes(0), each an original k-mer (build.hip: k_rank 2b, k_graph 3) -- against the table; a
//                  bit per entry, reduced to the profile of every probe (pb_lowcov1)
//   k_probe_nodes  where k_graph_export runs, from the same marks and arrays: every node of a reported component is spelled
//                  (graph_ws.h: gx_spell_node) under a rolling hash; a bitmap per component row (pb_final)
//   k_probe_reads  once at the end: every read of the window under a rolling hash, a lane per read (pb_in_reads), and every
//                  haplotype searched for every ALT context (pb_hap_mask); also what checks the probes themselves
#include "graph_ws.h"

namespace ma {

namespace {

constexpr u32 kPbMaxProbes = 256;   // per window
constexpr u32 kPbMaxAllele = 256;   // bases of REF and of ALT
constexpr u32 kPbChunk = 64;        // probes per chunk: a lane's "this read holds one" flags are one u64
constexpr u32 kPbCtx = 8192;        // bytes of ALT contexts per chunk
constexpr u32 kPbEnt = 2048;        // k-mers of ALT contexts per chunk
constexpr u32 kPbBuckets = 2048;
constexpr u32 kPbCtxMax = 768;      // the longest context: 254 + 256 + 254 bases
constexpr u32 kPbNone = 0xFFFFu;
constexpr u32 kPbBmWords = kPbEnt / 32 + 1;  // (pb_profile reads one word beyond the last bit's)
static_assert(2 * (255 - 1) + kPbMaxAllele <= kPbCtxMax && kPbCtxMax <= kPbCtx && kPbCtxMax <= kPbEnt, "one probe fits a chunk");

constexpr u64 pb_inverse(u64 a) {  // a odd: Newton iteration mod 2^64
  u64 x = a;
  for (int i = 0; i < 6; ++i) x *= 2 - a * x;
  return x;
}
constexpr u64 kPbPinv = pb_inverse(kHashP);
static_assert(kPbPinv * kHashP == 1ull, "inverse of the hash base");

struct PbTable {
  u64 ent_hash[kPbEnt];     // per entry (ALT-unique k-mer): strand-symmetric hash, never 0
  u64 tmp_ref[kPbCtxMax];   // build only: the REF-context k-mers of the probe being built (0: holds a non-ACGT byte)
  u64 tmp_alt[kPbCtxMax];   // build only: its ALT-context k-mers
  u32 head[kPbBuckets];     // bucket -> first entry of its chain, kPbNone: empty
  u16 ent_pos[kPbEnt];      // where the k-mer starts in ctx
  u16 ent_next[kPbEnt];
  u8 ent_probe[kPbEnt];     // the probe of the chunk it belongs to
  u8 ctx[kPbCtx];           // the chunk's ALT contexts, one after the other
  u8 uflag[kPbCtxMax];      // build only: ALT-context k-mer j is ALT-unique
  u16 ctx_off[kPbChunk + 1];
  u16 ent0[kPbChunk + 1];   // entries of probe q: [ent0[q], ent0[q + 1]), offset j = entry - ent0[q]
  u32 np;                   // probes of the chunk
  u32 nent;
};

__device__ __forceinline__ u32 pb_code(u8 c) {  // upper-case A C G T only; 4: anything else
  return c == 'A' ? 0u : (c == 'C' ? 1u : (c == 'G' ? 2u : (c == 'T' ? 3u : 4u)));
}
// forward hash sum c_i P^(K-1-i), reverse-complement hash sum (3 - c_i) P^i: a k-mer's pair is its reverse complement's swapped
__device__ __forceinline__ u64 pb_key(u64 hf, u64 hr) {
  u64 const h = dev_fmix64(hf < hr ? hf : hr);
  return h ? h : 1ull;
}
template <class Get>
__device__ __forceinline__ u64 pb_hash_of(u32 K, Get&& get) {  // 0: the k-mer holds a byte that is none of A C G T
  u64 hf = 0, hr = 0, pw = 1;
  bool ok = true;
  for (u32 i = 0; i < K; ++i) {
    u32 c = pb_code(get(i));
    ok &= c < 4u;
    c &= 3u;
    hf = hf * kHashP + c;
    hr += (3u - c) * pw;
    pw *= kHashP;
  }
  return ok ? pb_key(hf, hr) : 0ull;
}
// the letters decide: the query equals the entry's k-mer or its reverse complement (both hold A C G T only)
template <class Get>
__device__ __forceinline__ bool pb_equal(u32 K, Get&& getq, const u8* ek) {
  bool f = true, r = true;
  for (u32 i = 0; i < K && (f || r); ++i) {
    u8 const q = getq(i);
    f &= q == ek[i];
    r &= q == dev_complement(ek[K - 1u - i]);
  }
  return f || r;
}

// a k-mer's hash under a window of K letters that moves one letter at a time; letters that are none of A C G T count as A in
// the sums and make the K k-mers that hold them invalid
struct PbRoll {
  u64 hf = 0, hr = 0, pw = 1;
  u32 run = 0;
  // `pos`: index of the letter that enters, `out`: the letter at pos - K (read only when pos >= K)
  template <class Out>
  __device__ __forceinline__ u64 push(u32 pos, u8 in, u32 K, u64 pk1, Out&& out) {  // 0: no valid k-mer ends here
    u32 c = pb_code(in);
    run = c < 4u ? run + 1u : 0u;
    c &= 3u;
    if (pos >= K) {
      u32 const co = pb_code(out()) & 3u;
      hf = (hf - co * pk1) * kHashP + c;
      hr = (hr - (3u - co)) * kPbPinv + (3u - c) * pk1;
    } else {
      hf = hf * kHashP + c;
      hr += (3u - c) * pw;
      pw *= kHashP;
    }
    return run >= K ? pb_key(hf, hr) : 0ull;
  }
};
__device__ __forceinline__ u64 pb_pow(u32 e) {
  u64 p = 1;
  for (u32 i = 0; i < e; ++i) p *= kHashP;
  return p;
}

struct PbGeom {
  u32 bad;  // bit 0: outside the window, bit 1: an allele beyond kPbMaxAllele
  u32 pos, ref_len, alt_off, alt_len;
  u32 a, e, left, clen;  // REF context ref[a:e]; the ALT context is `clen` bytes, the first `left` of them ref[a:pos]
};
__device__ __forceinline__ PbGeom pb_geom(ma_probes_t const& in, u32 p, u32 len, u32 K) {
  PbGeom g;
  g.pos = in.probe_pos[p];
  g.ref_len = in.probe_ref_len[p];
  g.alt_off = in.probe_alt_off[p];
  g.alt_len = in.probe_alt_len[p];
  g.bad = ((g.pos < len && g.ref_len <= len - g.pos) ? 0u : 1u) | ((g.alt_len <= kPbMaxAllele && g.ref_len <= kPbMaxAllele) ? 0u : 2u);
  g.a = g.e = g.left = g.clen = 0;
  if (g.bad == 0u && K > 0u) {
    u32 const f = K - 1u;
    g.a = g.pos > f ? g.pos - f : 0u;
    g.e = min(len, g.pos + g.ref_len + f);
    g.left = g.pos - g.a;
    g.clen = g.left + g.alt_len + (g.e - g.pos - g.ref_len);
  }
  return g;
}

// The chunk of window probes that starts at p0 (p0 < p_end), for the whole workgroup (at least one wavefront; wavefront 0
// numbers the entries).  A bad probe has an empty context and no entries.  Ends synchronised; T.np >= 1 probes were taken.
__device__ __forceinline__ void pb_build(PbTable& T, ma_probes_t const& in, const u8* refb, u32 len, u32 K, u32 p0, u32 p_end) {
  u32 const tid = threadIdx.x, nt = blockDim.x;
  if (tid == 0) {
    u32 np = 0, cb = 0, ne = 0;
    T.ctx_off[0] = 0;
    for (u32 p = p0; p < p_end && np < kPbChunk; ++p) {
      PbGeom const g = pb_geom(in, p, len, K);
      u32 const nk = g.clen >= K ? g.clen - K + 1u : 0u;
      if (np > 0 && (cb + g.clen > kPbCtx || ne + nk > kPbEnt)) break;
      cb += g.clen;
      ne += nk;
      T.ctx_off[++np] = static_cast<u16>(cb);
    }
    T.np = np;
    T.nent = 0;
  }
  for (u32 i = tid; i < kPbBuckets; i += nt) T.head[i] = kPbNone;
  __syncthreads();
  u32 const np = T.np;
  unsigned long long const below = (1ull << (tid & 63u)) - 1ull;
  for (u32 q = 0; q < np; ++q) {
    PbGeom const g = pb_geom(in, p0 + q, len, K);
    u32 const off = T.ctx_off[q], nent = T.nent;
    // the ALT context: ref[a:pos] + ALT + ref[pos + ref_len:e]
    for (u32 i = tid; i < g.clen; i += nt)
      T.ctx[off + i] = i < g.left ? refb[g.a + i]
                                  : (i < g.left + g.alt_len ? in.alt_pool[g.alt_off + (i - g.left)] : refb[g.pos + g.ref_len + (i - g.left - g.alt_len)]);
    // the k-mers of the REF context ref[a:e]
    u32 const rl = g.e - g.a, nref = rl >= K ? rl - K + 1u : 0u;
    for (u32 x = tid; x < nref; x += nt) T.tmp_ref[x] = pb_hash_of(K, [&](u32 i) { return refb[g.a + x + i]; });
    __syncthreads();
    // ALT-unique: a k-mer of A C G T only that equals no k-mer of the REF context
    u32 const nk = g.clen >= K ? g.clen - K + 1u : 0u;
    for (u32 j = tid; j < nk; j += nt) {
      const u8* km = T.ctx + off + j;
      u64 const h = pb_hash_of(K, [&](u32 i) { return km[i]; });
      bool uniq = h != 0ull;
      for (u32 x = 0; x < nref && uniq; ++x)
        if (T.tmp_ref[x] == h && pb_equal(K, [&](u32 i) { return refb[g.a + x + i]; }, km)) uniq = false;
      T.tmp_alt[j] = h;
      T.uflag[j] = uniq ? 1 : 0;
    }
    __syncthreads();
    // offsets 0, 1, ... in context order
    if (tid < 64u) {
      u32 at = nent;
      for (u32 j0 = 0; j0 < nk; j0 += 64) {
        u32 const j = j0 + tid;
        bool const f = j < nk && T.uflag[j] != 0;
        unsigned long long const m = __ballot(f);
        if (f) {
          u32 const e = at + static_cast<u32>(__popcll(m & below));
          T.ent_hash[e] = T.tmp_alt[j];
          T.ent_pos[e] = static_cast<u16>(off + j);
          T.ent_probe[e] = static_cast<u8>(q);
        }
        at += static_cast<u32>(__popcll(m));
      }
      if (tid == 0) {
        T.ent0[q] = static_cast<u16>(nent);
        T.ent0[q + 1] = static_cast<u16>(at);
        T.nent = at;
      }
    }
    __syncthreads();
  }
  u32 const nent = T.nent;
  for (u32 e = tid; e < nent; e += nt)
    T.ent_next[e] = static_cast<u16>(atomicExch(&T.head[static_cast<u32>(T.ent_hash[e]) & (kPbBuckets - 1u)], e));
  __syncthreads();
}

// every entry whose k-mer equals the query: eq(entry's letters) decides, hit(entry) takes it
template <class Eq, class Hit>
__device__ __forceinline__ void pb_lookup(PbTable const& T, u64 h, Eq&& eq, Hit&& hit) {
  for (u32 e = T.head[static_cast<u32>(h) & (kPbBuckets - 1u)]; e != kPbNone; e = T.ent_next[e])
    if (T.ent_hash[e] == h && eq(T.ctx + T.ent_pos[e])) hit(e);
}

// CountSurvivingKmers (probe_tracker.cpp:602-654) over the bits [e0, e0 + n) of a bitmap of surviving entries: count, the two
// edge bits, the rest, and the gaps -- adjacent survivors more than one offset apart, i.e. the runs of survivors but one
__device__ __forceinline__ void pb_profile(const u32* bm, u32 e0, u32 n, u32* out) {
  u32 cnt = 0, runs = 0, prev = 0;
  for (u32 x = 0; x < n; x += 32) {
    u32 const at = e0 + x, wi = at >> 5, sh = at & 31u;
    u32 v = sh ? (bm[wi] >> sh) | (bm[wi + 1] << (32u - sh)) : bm[wi];
    if (n - x < 32u) v &= (1u << (n - x)) - 1u;
    cnt += static_cast<u32>(__popc(v));
    runs += static_cast<u32>(__popc(v & ~((v << 1) | prev)));
    prev = v >> 31;
  }
  u32 edge = 0;
  if (n > 0) {
    u32 const last = e0 + n - 1u;
    edge = (bm[e0 >> 5] >> (e0 & 31u)) & 1u;
    if (n > 1) edge += (bm[last >> 5] >> (last & 31u)) & 1u;
  }
  out[0] = cnt;
  out[1] = edge;
  out[2] = cnt - edge;
  out[3] = runs ? runs - 1u : 0u;
}

// ---- rows to zero: every window at the start of the call, the windows a capacity retry pass takes again before it ----
__global__ __launch_bounds__(64) void k_probe_clear(ProbeDev pd, const u32* win_status, int only_overflowed) {
  int const w = blockIdx.x;
  if (only_overflowed && !(win_status[w] & MA_W_TABLE_OVERFLOW)) return;
  u32 const MC = pd.max_comps;
  for (u32 p = pd.in.probe_win_off[w] + threadIdx.x; p < pd.in.probe_win_off[w + 1]; p += 64) {
    pd.o.pb_k[p] = 0;
    pd.o.pb_alt_kmers[p] = 0;
    pd.o.pb_in_reads[2 * static_cast<size_t>(p)] = 0;
    pd.o.pb_in_reads[2 * static_cast<size_t>(p) + 1] = 0;
    for (u32 x = 0; x < 4; ++x) pd.o.pb_lowcov1[4 * static_cast<size_t>(p) + x] = 0;
    for (u32 x = 0; x < 4 * MC; ++x) pd.o.pb_final[4 * static_cast<size_t>(p) * MC + x] = 0;
    for (u32 x = 0; x < MC; ++x) pd.o.pb_hap_mask[static_cast<size_t>(p) * MC + x] = 0;
  }
}

// ---- pb_lowcov1: the raw graph the build pass hands to the clean pass ----
__global__ __launch_bounds__(256) void k_probe_raw(DBatch b, GraphWs ws, ProbeDev pd) {
  __shared__ PbTable T;
  __shared__ u32 bm[kPbBmWords];
  int const a = blockIdx.x;
  int const w = static_cast<int>(ws.active[a]);
  u32 const p0 = pd.in.probe_win_off[w], p1 = pd.in.probe_win_off[w + 1];
  if (p1 <= p0 || p1 - p0 > kPbMaxProbes) return;  // (too many: k_probe_reads says so; the rows stay zero)
  u32 const K = static_cast<u32>(win_kmer(ws, w));
  const u8* refb = b.ref_bases + b.ref_off[w];
  u32 const len = b.ref_off[w + 1] - b.ref_off[w];
  const u8* readb = b.read_bases + b.read_off[b.read_win_off[w]];
  // nodes [0, n_nodes) are the survivors of the first low-coverage pass, all alive; a window the build pass flagged for a
  // capacity has no complete set (the retry pass assembles it again)
  u32 const n = (ws.win_flags[w] & 4u) ? 0u : min(ws.n_nodes[a], ws.nc);
  const u32* src = ws.nd_src + static_cast<size_t>(a) * ws.nc;
  for (u32 c0 = p0; c0 < p1;) {
    pb_build(T, pd.in, refb, len, K, c0, p1);
    for (u32 i = threadIdx.x; i < kPbBmWords; i += 256) bm[i] = 0;
    __syncthreads();
    if (T.nent > 0)
      for (u32 i = threadIdx.x; i < n; i += 256) {
        u32 const sv = src[i];
        const u8* p = (sv & 0x80000000u) ? readb + (sv & 0x3FFFFFFFu) : refb + sv;
        u64 const h = pb_hash_of(K, [&](u32 x) { return p[x]; });
        if (h == 0ull) continue;
        pb_lookup(T, h, [&](const u8* ek) { return pb_equal(K, [&](u32 x) { return p[x]; }, ek); },
                  [&](u32 e) { atomicOr(&bm[e >> 5], 1u << (e & 31u)); });
      }
    __syncthreads();
    u32 const np = T.np;
    for (u32 q = threadIdx.x; q < np; q += 256)
      pb_profile(bm, T.ent0[q], static_cast<u32>(T.ent0[q + 1]) - T.ent0[q], pd.o.pb_lowcov1 + 4 * static_cast<size_t>(c0 + q));
    __syncthreads();
    c0 += np;
  }
}

// ---- pb_final: the alive nodes of every component that got a row of comp_*, as k_graph_export sees them ----
__global__ __launch_bounds__(64) void k_probe_nodes(DBatch b, GraphWs ws, const u32* marks, ProbeDev pd) {
  __shared__ PbTable T;
  __shared__ u32 bm[16][kPbBmWords];
  __shared__ u8 ring[256 * 64];  // the last 256 letters of every lane's node, letter-major: lanes side by side
  __shared__ u32 s_comp[16];
  int const a = blockIdx.x;
  u32 const lane = threadIdx.x;
  const u32* mark = marks + static_cast<size_t>(a) * kGxMark;
  u32 const m0 = mark[0];
  if (m0 == 0u) return;  // not reported by this pass
  u32 const MC = pd.max_comps;
  u32 const rows = min(min(m0 & 0xFFu, 16u), MC), route = (m0 >> 8) - 1u;
  int const w = static_cast<int>(ws.active[a]);
  u32 const p0 = pd.in.probe_win_off[w], p1 = pd.in.probe_win_off[w + 1];
  if (p1 <= p0 || p1 - p0 > kPbMaxProbes) return;
  u32 const K = static_cast<u32>(win_kmer(ws, w));
  if (lane < rows) s_comp[lane] = mark[1 + 3 * lane];
  __syncthreads();
  GxNodes const g = gx_nodes(b, ws, a, w, route);
  u32 const len = b.ref_off[w + 1] - b.ref_off[w];
  u64 const pk1 = pb_pow(K - 1u);
  auto row_of = [&](u32 i) -> u32 {  // the row of comp_* node i belongs to, kNoNode: none (graph_export.hip)
    if (!g.alive[i]) return kNoNode;
    u32 const cc = g.comp[i];
    u32 r = kNoNode;
    for (u32 x = 0; x < rows; ++x)
      if (s_comp[x] == cc) r = x;
    return r;
  };
  for (u32 c0 = p0; c0 < p1;) {
    pb_build(T, pd.in, g.refb, len, K, c0, p1);
    for (u32 i = lane; i < 16u * kPbBmWords; i += 64) (&bm[0][0])[i] = 0;
    __syncthreads();
    if (T.nent > 0)
      for (u32 base = 0; base < g.n; base += 64) {
        u32 const i = base + lane;
        u32 const r = i < g.n ? row_of(i) : kNoNode;
        if (r == kNoNode) continue;
        PbRoll roll;
        gx_spell_node(g, i, g.len[i], K, [&](u32 pos, u8 ch) {
          u64 const h = roll.push(pos, ch, K, pk1, [&]() { return ring[((pos - K) & 255u) * 64u + lane]; });
          ring[(pos & 255u) * 64u + lane] = ch;
          if (h == 0ull) return;
          u32 const first = pos + 1u - K;
          pb_lookup(T, h, [&](const u8* ek) { return pb_equal(K, [&](u32 x) { return ring[((first + x) & 255u) * 64u + lane]; }, ek); },
                    [&](u32 e) { atomicOr(&bm[r][e >> 5], 1u << (e & 31u)); });
        });
      }
    __syncthreads();
    u32 const np = T.np;
    for (u32 x = lane; x < np * rows; x += 64) {
      u32 const q = x / rows, r = x % rows;
      pb_profile(bm[r], T.ent0[q], static_cast<u32>(T.ent0[q + 1]) - T.ent0[q], pd.o.pb_final + 4 * (static_cast<size_t>(c0 + q) * MC + r));
    }
    __syncthreads();
    c0 += np;
  }
}

// ---- pb_in_reads, pb_hap_mask, pb_k, pb_alt_kmers; the checks of the probes themselves ----
__global__ __launch_bounds__(256) void k_probe_reads(DBatch b, ma_asm_out_t o, ProbeDev pd, u32 MH, u32 ML) {
  __shared__ PbTable T;
  __shared__ u32 s_occ[kPbChunk], s_nrd[kPbChunk], s_mask[kPbChunk * 16];
  int const w = blockIdx.x;
  u32 const tid = threadIdx.x, lane = tid & 63u;
  u32 const p0 = pd.in.probe_win_off[w], p1 = pd.in.probe_win_off[w + 1];
  if (p1 <= p0) return;  // a window without probes
  if (p1 - p0 > kPbMaxProbes) {
    if (tid == 0) atomicOr(pd.err, 2u);
    return;
  }
  u32 const len = b.ref_off[w + 1] - b.ref_off[w];
  u32 bad = 0;
  for (u32 p = p0 + tid; p < p1; p += 256) bad |= pb_geom(pd.in, p, len, 0u).bad;
  if (bad) atomicOr(pd.err, bad);
  u32 const K = o.win_k[w];
  if (K == 0u) return;  // never attempted: the rows are zero
  u32 const MC = pd.max_comps;
  const u8* refb = b.ref_bases + b.ref_off[w];
  u32 const r0 = b.read_win_off[w], r1 = b.read_win_off[w + 1];
  u32 const ncomp = min(o.win_ncomp[w], min(MC, 16u));
  u64 const pk1 = pb_pow(K - 1u);
  for (u32 c0 = p0; c0 < p1;) {
    pb_build(T, pd.in, refb, len, K, c0, p1);
    for (u32 i = tid; i < kPbChunk; i += 256) s_occ[i] = s_nrd[i] = 0;
    for (u32 i = tid; i < kPbChunk * 16u; i += 256) s_mask[i] = 0;
    __syncthreads();
    u32 const np = T.np;
    // the reads, a lane each
    if (T.nent > 0)
      for (u32 rb = r0; rb < r1; rb += 256) {
        u32 const r = rb + tid;
        unsigned long long held = 0;
        if (r < r1) {
          u64 const at = b.read_off[r];
          u32 const L = static_cast<u32>(b.read_off[r + 1] - at);
          const u8* s = b.read_bases + at;
          if (L >= K) {
            PbRoll roll;
            for (u32 pos = 0; pos < L; ++pos) {
              u64 const h = roll.push(pos, s[pos], K, pk1, [&]() { return s[pos - K]; });
              if (h == 0ull) continue;
              const u8* km = s + (pos + 1u - K);
              pb_lookup(T, h, [&](const u8* ek) { return pb_equal(K, [&](u32 x) { return km[x]; }, ek); },
                        [&](u32 e) {
                          u32 const q = T.ent_probe[e];
                          atomicAdd(&s_occ[q], 1u);
                          held |= 1ull << q;
                        });
            }
          }
        }
        for (u32 q = 0; q < np; ++q) {  // reads that hold at least one, a ballot per probe
          unsigned long long const m = __ballot((held >> q) & 1ull);
          if (lane == 0 && m) atomicAdd(&s_nrd[q], static_cast<u32>(__popcll(m)));
        }
      }
    // CheckPaths: the ALT context as a substring of every haplotype, forward only
    for (u32 q = 0; q < np; ++q) {
      if (pb_geom(pd.in, c0 + q, len, K).bad) continue;
      const u8* cx = T.ctx + T.ctx_off[q];
      u32 const m = static_cast<u32>(T.ctx_off[q + 1]) - T.ctx_off[q];
      for (u32 c = 0; c < ncomp; ++c) {
        u32 const h0 = o.comp_hap0[static_cast<size_t>(w) * MC + c], nh = min(o.comp_nhaps[static_cast<size_t>(w) * MC + c], 32u);
        for (u32 h = 0; h < nh && h0 + h < MH; ++h) {
          size_t const slot = static_cast<size_t>(w) * MH + h0 + h;
          u32 const hl = min(o.hap_len[slot], ML);
          if (m > hl) continue;
          const u8* hb = o.hap_bases + slot * ML;
          bool found = false;
          for (u32 s = tid; s + m <= hl && !found; s += 256) {
            u32 i = 0;
            while (i < m && hb[s + i] == cx[i]) ++i;
            found = i == m;
          }
          if (found) atomicOr(&s_mask[q * 16u + c], 1u << h);
        }
      }
    }
    __syncthreads();
    for (u32 q = tid; q < np; q += 256) {
      u32 const p = c0 + q;
      if (pb_geom(pd.in, p, len, K).bad) continue;  // a bad probe's row stays zero
      pd.o.pb_k[p] = K;
      pd.o.pb_alt_kmers[p] = static_cast<u32>(T.ent0[q + 1]) - T.ent0[q];
      pd.o.pb_in_reads[2 * static_cast<size_t>(p)] = s_occ[q];
      pd.o.pb_in_reads[2 * static_cast<size_t>(p) + 1] = s_nrd[q];
      for (u32 c = 0; c < ncomp; ++c) pd.o.pb_hap_mask[static_cast<size_t>(p) * MC + c] = s_mask[q * 16u + c];
    }
    __syncthreads();
    c0 += np;
  }
}

}  // namespace

int run_probe_clear(ma_ctx* ctx, const ProbeDev& pd, const u32* win_status, int n, bool only_overflowed) {
  if (n == 0) return MA_OK;
  hipLaunchKernelGGL(k_probe_clear, dim3(n), dim3(64), 0, ctx->stream, pd, win_status, only_overflowed ? 1 : 0);
  MA_HIP(ctx, hipGetLastError());
  return MA_OK;
}

int run_probe_raw(ma_ctx* ctx, const DBatch& b, const GraphWs& ws, const ProbeDev& pd) {
  if (ws.n_active == 0) return MA_OK;
  ctx->tic("k_probe_raw");
  hipLaunchKernelGGL(k_probe_raw, dim3(ws.n_active), dim3(256), 0, ctx->stream, b, ws, pd);
  ctx->toc();
  MA_HIP(ctx, hipGetLastError());
  return MA_OK;
}

int run_probe_nodes(ma_ctx* ctx, const DBatch& b, const GraphWs& ws, const u32* mark, const ProbeDev& pd) {
  if (ws.n_active == 0) return MA_OK;
  ctx->tic("k_probe_nodes");
  hipLaunchKernelGGL(k_probe_nodes, dim3(ws.n_active), dim3(64), 0, ctx->stream, b, ws, mark, pd);
  ctx->toc();
  MA_HIP(ctx, hipGetLastError());
  return MA_OK;
}

int run_probe_reads(ma_ctx* ctx, const DBatch& b, const ma_asm_out_t& a, const ProbeDev& pd) {
  if (b.n_windows == 0) return MA_OK;
  ctx->tic("k_probe_reads");
  hipLaunchKernelGGL(k_probe_reads, dim3(b.n_windows), dim3(256), 0, ctx->stream, b, a, pd, static_cast<u32>(ctx->prm.max_haps),
                     static_cast<u32>(ctx->prm.max_hap_len));
  ctx->toc();
  MA_HIP(ctx, hipGetLastError());
  return MA_OK;
}

}  // namespace ma
