// Read-level FORMAT statistics of the genotype stage (evidence.hip): what it shares with align.hip -- the evidence table's
// key and sizing, the per-read record k_assign<true> leaves for k_evid_stats, and the launch.
#pragma once
#include "ma_internal.h"

namespace ma {

__device__ __forceinline__ u64 ev_key_of(u32 var, u32 sample, u32 allele, u32 qname) {
  return ((static_cast<u64>(var) << 44) | (static_cast<u64>(sample) << 40) | (static_cast<u64>(allele) << 33) |
          (static_cast<u64>(qname) << 1)) + 1ull;
}

// The evidence table of a window: ev_slots() slots of its own -- a power of two, at least 64, that holds 1.5 x (its reads x
// its variants) keys; every read files at most one key per variant, so the table never fills and a probe always ends at a
// free slot.  The tables lie one behind the other: window w's begins at slot win_off[w].y, an exclusive scan of ev_slots() over
// the genotyped windows (k_plan, k_scan_pairs; align.hip), and k_assign, k_evidence, k_ev_clear and k_evid_stats all size
// and place it through this one function.  1-4 k slots per window on the whole-genome workload, where a fixed 8192 per
// window used to be reserved -- and a window of 160 reads x 60 variants lost the depths that did not fit them.
// (the reads of a window are bounded by k_vote's LDS, a few ten thousand: times max_vars <= 128 the count is far below 2^31)
__device__ __forceinline__ u32 ev_slots(u32 nrw, u32 nv) {
  u64 const need = static_cast<u64>(nrw) * nv * 3u / 2u + 16u;
  if (need > (1ull << 31)) return 1u << 31;
  u32 const c = 1u << (32 - __builtin_clz(static_cast<u32>(need) - 1u));
  return max(c, 64u);
}

// The winning assignment of a read at a variant, beside its allele (asg_allele): 8 bytes per (read, variant slot), written by
// k_assign<true> for the assigned pairs only and read by k_evid_stats for the evidence reads only.
//   x: hap_id (haplotype within its component, 0 = REF) | base_qual << 8 | qpos << 16      y: own_nm | ref_nm << 16
// (a read has at most 608 bases: every edit distance, and every position in the read, fits 16 bits)
// qpos: the query position of the variant's start in the winning CIGAR (combined_scorer.cpp:96-105); 0 unless the call asked
// for the statistics over the read metadata
__device__ __forceinline__ uint2 ev_rec_pack(u32 hap_id, u32 base_qual, u32 own_nm, u32 ref_nm, u32 qpos = 0) {
  return make_uint2(hap_id | (base_qual << 8) | (min(qpos, 0xFFFFu) << 16), min(own_nm, 0xFFFFu) | (min(ref_nm, 0xFFFFu) << 16));
}

inline bool fmt_wanted(const ma_fmt_out_t& f) { return f.ev_sums || f.fmt_npbq || f.fmt_cmlod || f.fmt_stat; }
inline bool fmeta_wanted(const ma_fmt_meta_out_t& f) { return f.ev_meta || f.ev_rpcd || f.fmt_rmq || f.fmt_mstat; }

// k_evid_stats sorts the keys of a cell -- one per evidence read and one more per ALT read -- in LDS while they fit
// kEvSortCap keys (two buffers of 16 KB: with the tallies 40 KB per workgroup, four workgroups per CU); a cell with more
// sorts in its (window, variant)'s slice of a workspace buffer.  Both places hold a power of two of keys, at least 256.
constexpr u32 kEvSortCap = 2048;
__host__ __device__ inline u32 ev_sort_pad(u32 nkeys) {
  u32 p = 256;
  while (p < nkeys) p <<= 1;
  return p;
}

struct EvStatArgs {
  int n_windows;
  ma_params_t prm;
  // the batch and the stages before
  const u32* read_win_off;
  const u32* read_qname_id;
  const u8* read_sample;
  const u32* comp_nhaps;
  const u32* win_nvars;
  const u32* var_comp;
  const u32* var_nalts;
  const i32* alt_length;
  // the genotype stage's own
  const u32* win_slotmask;
  const ulonglong2* win_off;  // [n + 1] .y: first slot of every window's table
  const u64* ev_key;
  const u32* ev_min;
  const u8* asg_allele;     // [n_reads * max_vars]
  const uint2* ev_rec;      // [n_reads * max_vars]
  const u32* allele_counts;
  ma_fmt_out_t o;
  // the statistics over the read metadata (all of m null: off)
  const u64* read_off;
  const u8* read_mapq;
  const u8* read_mflags;
  const i32* read_isize;
  const i32* read_start;
  const u64* sort_off;  // [n] first key of the window's sort slices, ~0: none -- 2 ev_sort_pad(2 reads) keys per variant (null:
  u64* sort_ws;         //     no window of the batch holds more than kEvSortCap / 2 reads)
  ma_fmt_meta_out_t m;
};

// clears the requested arrays (0; fmt_stat, fmt_mstat: NaN) and launches k_evid_stats on the context's stream
// max_win_reads: the most reads of a window of the batch (sizes the sort slices)
int launch_evid_stats(ma_ctx* ctx, EvStatArgs A, u32 max_win_reads);

}  // namespace ma
