// Read-level FORMAT statistics of a call (ma_genotype_stats_batch / ma_process_stats_batch): NPBQ, BQCD, CMLOD, ASMD, AHDD and
// HSE of every (window, variant, sample), from the de-duplicated evidence reads that the allele depths count.
//
// Every one of them is a function of small integer tallies over the evidence reads of a (variant, sample): a 256-bin
// base-quality histogram per allele, three integer sums per allele (base_qual, ref_nm, own_nm) and the ALT reads per
// haplotype.  k_assign<true> (align.hip) leaves an 8-byte record per (read, variant) -- evidence.h -- and k_evid_stats
// below tallies the evidence reads' records in LDS and finishes over the BINS, never over the reads:
//   NPBQ   (caller/posterior_base_qual.cpp:14-40, variant_call.cpp:368-373)  two log sums over an allele's bins
//   BQCD   (base/mann_whitney.h:127-225)  the rank sum and the tie term are exact 64-bit integers of the bins:
//            2 R_alt = sum_q alt[q] (2 below[q] + t[q] + 1),   tie = sum_q t[q]^3 - t[q]
//   CMLOD  (caller/genotype_likelihood.cpp:141-196, :307-345)  one log sum per hypothesis over (allele, bin)
//   ASMD / AHDD (caller/variant_support.h:361-387, variant_call.cpp:177-184)  means of the integer sums
//   HSE    (caller/variant_support.h:389-411)  entropy of the ALT reads' haplotype counts
// The f64 operations after the sums follow the reference's order; the sums themselves run over bins (count x term) where the
// reference adds read by read, and through the device's log10 / log2 / pow / sqrt: compared at 1e-9 relative, like QUAL.
//
// k_evid_stats<true> (ma_genotype_meta_batch / ma_process_meta_batch) adds the six statistics over the read metadata of
// ma_read_meta_t, of the same evidence reads:
//   RMQ    (caller/variant_support.cpp:184-194)  sqrt of an allele's integer sum of mapq^2 over its depth
//   MQCD   (base/mann_whitney.h:127-225)  BQCD's integer form over a 256-bin MAPQ histogram of REF and of the pooled ALTs
//   SCA    (variant_support.cpp:261-279)  two fractions of integer counts
//   FLD    (variant_support.cpp:49-51, variant_support.h:361-387)  means of the signed insert sizes of the proper pairs
//   RPCD   (mann_whitney.h over caller/combined_scorer.cpp:96-105)  the rank test over the folded positions min(x, 1.0 - x),
//            x = f64(qpos) / f64(read length): the reference ranks the DOUBLES, and 1 - fl(100/150) is not fl(50/150), so the
//            kernel computes the same two f64 operations and sorts their bit patterns (non-negative: unsigned order is value
//            order); 2 R_alt and the tie term are then exact integers of the sorted sequence
//   FSSE   (variant_support.h:391-411, .cpp:358-363)  entropy of the ALT reads' start / 3 bins: runs of the sorted sequence
// One sort per cell serves RPCD and FSSE: every evidence read files bits(folded) << 1 | is_alt, every ALT read also
// 1 << 63 | start / 3; a merge sort (one binary search per thread and segment, then a sequential merge: O(n log n)) between
// two buffers, in LDS up to kEvSortCap keys and in the (window, variant)'s slice of ctx->ws_sort beyond.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "evidence.h"

namespace ma {
namespace {

__constant__ u64 c_phred_bits_e[256] = {
#include "../../include/ma_phred_lut.inc"
};

constexpr int kEvThreads = 256;  // one thread per quality bin in the finish
constexpr int kEvMaxHaps = 32;   // check_params: max_haps <= 32

// Sum over the workgroup; every thread gets it.  T is f64 or u64 (8 bytes: red[] serves both).
template <class T>
__device__ __forceinline__ T block_sum(T v, u64* red) {
  static_assert(sizeof(T) == 8, "block_sum: 8-byte values");
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    if constexpr (std::is_same<T, f64>::value) v += __shfl_xor(v, d, 64);
    else v += static_cast<T>(__shfl_xor(static_cast<unsigned long long>(v), d, 64));
  }
  __syncthreads();  // (red[] of the sum before has been read)
  T* r = reinterpret_cast<T*>(red);
  if ((threadIdx.x & 63u) == 0) r[threadIdx.x >> 6] = v;
  __syncthreads();
  return r[0] + r[1] + r[2] + r[3];
}

// the statistics of a rank test from its integers (mann_whitney.h:194-225; the order of BQCD's tail below)
__device__ __forceinline__ f64 mw_effect(u64 m, u64 na, u64 rank2, u64 tie) {
  f64 const n_ref = static_cast<f64>(m), n_alt = static_cast<f64>(na), n_total = static_cast<f64>(m + na);
  f64 const alt_rank_sum = static_cast<f64>(rank2) / 2.0;
  f64 const u_stat = alt_rank_sum - ((n_alt * (n_alt + 1.0)) / 2.0);
  f64 const mean_u = (n_ref * n_alt) / 2.0;
  f64 const var_u = (n_ref * n_alt / 12.0) * ((n_total + 1.0) - (static_cast<f64>(tie) / (n_total * (n_total - 1.0))));
  if (!(var_u > 0.0)) return 0.0;
  f64 const z = (u_stat - mean_u) / sqrt(var_u);
  return z / sqrt(n_total);
}

// what two keys must share to be one tie group (RPCD: the value without the ALT bit) or one bin (FSSE: the whole key)
__device__ __forceinline__ u64 ev_group_of(u64 key) { return (key >> 63) ? key : (key >> 1); }

// One pass of the merge sort: runs of `run` keys of src, pairwise, into dst.  npad (a power of two, >= 256) keys in all; a
// thread writes npad / 256 consecutive keys, in segments that lie in one pair of runs: a binary search along the segment's
// first diagonal of the merge (keys of the first run before equal keys of the second), then a sequential merge.
__device__ void ev_merge_pass(const u64* src, u64* dst, u32 npad, u32 run) {
  u32 const per = npad / kEvThreads, seg = min(per, 2u * run);
  for (u32 o0 = threadIdx.x * per; o0 < (threadIdx.x + 1u) * per; o0 += seg) {
    u32 const base = o0 & ~(2u * run - 1u), d = o0 - base;
    const u64* a = src + base;
    const u64* b = a + run;
    u32 lo = d > run ? d - run : 0u, hi = min(d, run);
    while (lo < hi) {
      u32 const mid = (lo + hi) >> 1;
      if (a[mid] <= b[d - 1u - mid]) lo = mid + 1u;
      else hi = mid;
    }
    u32 i = lo, j = d - lo;
    for (u32 x = 0; x < seg; ++x) {
      bool const take_a = j >= run || (i < run && a[i] <= b[j]);
      dst[o0 + x] = take_a ? a[i] : b[j];
      i += take_a ? 1u : 0u;
      j += take_a ? 0u : 1u;
    }
  }
}

// One workgroup per (window, variant slot), variant-major like k_qual: the slots no window uses leave at once.
// kMeta: also the statistics over the read metadata (A.m, A.read_mapq ...); k_evid_stats<false> is the kernel without them
// (k_evid_stats<false> keeps the 128 registers and four wavefronts per SIMD the kernel had before it became a template)
template <bool kMeta>
__global__ __launch_bounds__(kEvThreads) __attribute__((amdgpu_waves_per_eu(kMeta ? 3 : 4, kMeta ? 3 : 4))) void k_evid_stats(EvStatArgs A) {
  extern __shared__ u32 ev_lds[];
  __shared__ u64 red[4];
  __shared__ u32 wave_tot[4];
  ma_params_t const& P = A.prm;
  int const MV = P.max_vars, MA = P.max_alts, NA = MA + 1, S = P.num_samples;
  int const w = static_cast<int>(blockIdx.x % static_cast<u32>(A.n_windows)), v = static_cast<int>(blockIdx.x / static_cast<u32>(A.n_windows));
  u32 const nv = A.win_nvars[w];
  if (static_cast<u32>(v) >= nv || A.win_slotmask[w] == 0) return;  // (k_assign / k_evidence leave at the same test: no evidence)
  u32 const tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  u32* hist = ev_lds;               // [NA][256] evidence reads per allele and base quality
  u32* sums = hist + NA * 256;      // [NA][3]   sum of base_qual, ref_nm, own_nm
  u32* hapc = sums + NA * 3;        // [32]      ALT evidence reads per haplotype of the component
  u32 const lds_words = static_cast<u32>(NA) * 259u + kEvMaxHaps;
  // kMeta, behind them (8-byte aligned): [NA] u64 sum of mapq^2, [NA] u64 sum of isize (two's complement), two sort buffers of
  // kEvSortCap keys; then u32: [2][256] MAPQ histogram of REF and of the pooled ALTs, [NA] soft-clipped reads, [NA] proper-pair
  // reads with an insert size, [1] keys filed
  u64* msq = reinterpret_cast<u64*>(ev_lds + ((lds_words + 1u) & ~1u));
  u64* isum = msq + NA;
  u64* key_a = isum + NA;
  u64* key_b = key_a + kEvSortCap;
  u32* mqh = reinterpret_cast<u32*>(key_b + kEvSortCap);
  u32* scn = mqh + 512;
  u32* ppn = scn + NA;
  u32* nkeys = ppn + NA;
  u32 const meta_words = 512u + 2u * static_cast<u32>(NA) + 1u;
  size_t const vi = static_cast<size_t>(w) * MV + v;
  int const K = min(static_cast<int>(A.var_nalts[vi]) + 1, NA);
  u32 const nhaps = A.comp_nhaps[static_cast<size_t>(w) * P.max_comps + A.var_comp[vi]];
  u32 const r0 = A.read_win_off[w], nrw = A.read_win_off[w + 1] - r0;
  const u64* evk = A.ev_key + A.win_off[w].y;
  const u32* evm = A.ev_min + A.win_off[w].y;
  u32 const evmask = ev_slots(nrw, nv) - 1;
  f64 max_var_len = 0.0;  // variant_call.cpp:179-182: the longest |AltAllele::mLength| of the variant
  for (int a = 0; a + 1 < K; ++a) max_var_len = fmax(max_var_len, fabs(static_cast<f64>(A.alt_length[vi * MA + a])));
  // this thread's bin: the error probability of its quality and the two logs NPBQ adds up
  f64 const eps = reinterpret_cast<const f64*>(c_phred_bits_e)[tid];
  f64 const l_err = log10(fmax(eps, 1e-300)), l_ok = log10(fmax(1.0 - eps, 1e-300));

  for (int s = 0; s < S; ++s) {
    const u32* cnt = A.allele_counts + (vi * S + s) * NA * 2;
    auto depth = [&](int a) { return cnt[2 * a] + cnt[2 * a + 1]; };  // AD: what k_evidence counted
    u32 total = 0;
    for (int a = 0; a < NA; ++a) total += depth(a);
    if (total == 0) continue;  // no evidence of this sample: the launcher's zeros / NaNs stand
    __syncthreads();           // (the sample before is done with the tallies)
    for (u32 x = tid; x < lds_words; x += kEvThreads) ev_lds[x] = 0;
    // where this cell's keys are sorted: in LDS, or -- more than kEvSortCap of them -- in the slice of (w, v); npad keys per buffer
    u64* srt_a = nullptr;
    u64* srt_b = nullptr;
    u32 nk_want = 0, npad = 0;
    if constexpr (kMeta) {
      for (u32 x = tid; x < meta_words; x += kEvThreads) mqh[x] = 0;
      if (tid < 2u * static_cast<u32>(NA)) msq[tid] = 0;
      nk_want = total + (total - depth(0));  // one key per evidence read, one more per ALT read
      npad = ev_sort_pad(nk_want);
      if (nk_want <= kEvSortCap) {
        srt_a = key_a;
        srt_b = key_b;
      } else if (A.sort_off && A.sort_off[w] != ~0ull) {
        u64 const slice = 2ull * ev_sort_pad(2u * nrw);  // (nk_want <= 2 nrw: evidence reads are reads of the window)
        srt_a = A.sort_ws + A.sort_off[w] + static_cast<u64>(v) * slice;
        srt_b = srt_a + slice / 2;
      }
    }
    __syncthreads();
    for (u32 rl = tid; rl < nrw; rl += kEvThreads) {
      size_t const r = static_cast<size_t>(r0) + rl;
      if (A.read_sample[r] != static_cast<u32>(s)) continue;
      u32 const al = A.asg_allele[r * MV + v];
      if (al >= static_cast<u32>(NA)) continue;  // 255: not assigned
      // the evidence read of its (variant, sample, allele, qname): the lowest read index, as k_evidence finds it
      u64 const key = ev_key_of(static_cast<u32>(v), static_cast<u32>(s), al, A.read_qname_id[r]);
      u32 slot = static_cast<u32>(key * 0x9E3779B97F4A7C15ULL >> 40) & evmask;
      bool win = false;
      for (u32 probe = 0; probe <= evmask; ++probe) {
        u64 const cur = evk[slot];
        if (cur == key) {
          win = evm[slot] == rl;
          break;
        }
        if (cur == 0) break;
        slot = (slot + 1) & evmask;
      }
      if (!win) continue;
      uint2 const rec = A.ev_rec[r * MV + v];
      u32 const bq = (rec.x >> 8) & 0xFFu;
      atomicAdd(&hist[al * 256 + bq], 1u);
      atomicAdd(&sums[al * 3 + 0], bq);
      atomicAdd(&sums[al * 3 + 1], rec.y >> 16);
      atomicAdd(&sums[al * 3 + 2], rec.y & 0xFFFFu);
      if (al > 0) atomicAdd(&hapc[rec.x & (kEvMaxHaps - 1)], 1u);
      if constexpr (kMeta) {
        u32 const mq = A.read_mapq[r], fl = A.read_mflags[r];
        i32 const isz = A.read_isize[r];
        atomicAdd(&mqh[(al > 0 ? 256u : 0u) + mq], 1u);
        atomicAdd(reinterpret_cast<unsigned long long*>(&msq[al]), static_cast<unsigned long long>(mq * mq));
        if (fl & MA_RM_SOFTCLIP) atomicAdd(&scn[al], 1u);
        if ((fl & MA_RM_PROPER) && isz != 0) {
          atomicAdd(&ppn[al], 1u);
          atomicAdd(reinterpret_cast<unsigned long long*>(&isum[al]), static_cast<unsigned long long>(static_cast<i64>(isz)));
        }
        if (srt_a) {
          // the folded read position: the reference's two f64 operations, then its bits (not negative: integer order is value order)
          u32 const rlen = static_cast<u32>(A.read_off[r + 1] - A.read_off[r]);
          f64 const rel = rlen > 0 ? static_cast<f64>(rec.x >> 16) / static_cast<f64>(rlen) : 0.5;
          f64 const mirror = 1.0 - rel;
          f64 const fold = mirror < rel ? mirror : rel;  // std::min(rel, 1.0 - rel)
          u32 const at = atomicAdd(nkeys, al > 0 ? 2u : 1u);
          if (at + (al > 0 ? 2u : 1u) <= nk_want) {  // (always: the depths counted these reads)
            srt_a[at] = (static_cast<u64>(__double_as_longlong(fold)) << 1) | (al > 0 ? 1ull : 0ull);
            if (al > 0) srt_a[at + 1] = (1ull << 63) | static_cast<u64>(static_cast<u32>(max(A.read_start[r], 0)) / 3u);
          }
        }
      }
    }
    __syncthreads();

    size_t const cell = vi * S + s;
    if (A.o.ev_sums && tid < static_cast<u32>(NA) * 3u) A.o.ev_sums[cell * NA * 3 + tid] = sums[tid];

    if (A.o.fmt_npbq) {
      for (int a = 0; a < K; ++a) {
        f64 const c = static_cast<f64>(hist[a * 256 + tid]);
        f64 const log_err = block_sum(c * l_err, red), log_ok = block_sum(c * l_ok, red);
        if (tid == 0) {
          u32 const d = depth(a);
          f64 npbq = 0.0;
          if (d > 0) {
            f64 const max_log = fmax(log_err, log_ok);
            f64 const log_sum = max_log + log10(1.0 + pow(10.0, fmin(log_err, log_ok) - max_log));
            f64 const log_posterior_err = log_err - log_sum;
            npbq = (-10.0 * log_posterior_err) / static_cast<f64>(d);
          }
          A.o.fmt_npbq[cell * NA + a] = npbq;
        }
      }
    }

    if (A.o.fmt_cmlod && K >= 2) {
      f64 const total_f = static_cast<f64>(total);
      int const km1 = max(1, K - 1);
      f64 const mismatch = eps / km1, bonus = (1.0 - eps) - mismatch;
      // the pileup's log10 likelihood under fractions f: target < 0 is the MLE, else the null hypothesis of ALT `target`
      auto pileup = [&](int target) {
        f64 const null_mass = target < 0 ? 0.0 : static_cast<f64>(depth(target)) / total_f;
        f64 const remaining = 1.0 - null_mass;
        f64 part = 0.0;
        for (int a = 0; a < K; ++a) {
          f64 f = static_cast<f64>(depth(a)) / total_f;
          if (target >= 0) {
            if (a == target) f = 0.0;
            if (remaining <= 0.0) f = a == 0 ? 1.0 : f;
            else f /= remaining;
          }
          u32 const c = hist[a * 256 + tid];
          if (c) part += static_cast<f64>(c) * log10(fmax(1e-15, mismatch + f * bonus));
        }
        return block_sum(part, red);
      };
      f64 const ll_mle = pileup(-1);
      for (int t = 1; t < K; ++t) {
        if (depth(t) == 0) continue;  // (uniform: the launcher's zero stands)
        f64 const ll_null = pileup(t);
        if (tid == 0) A.o.fmt_cmlod[cell * MA + (t - 1)] = fmax(0.0, ll_mle - ll_null);
      }
    }

    if (A.o.fmt_stat) {
      u32 const t_ref = hist[tid];
      u32 t_alt = 0;
      for (int a = 1; a < NA; ++a) t_alt += hist[a * 256 + tid];
      u32 const t = t_ref + t_alt;
      // below[q]: pooled observations of a smaller quality -- an exclusive scan over the 256 bins
      u32 incl = t;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        u32 const up = __shfl_up(incl, d, 64);
        if (lane >= static_cast<u32>(d)) incl += up;
      }
      __syncthreads();
      if (lane == 63) wave_tot[wave] = incl;
      __syncthreads();
      u32 below = incl - t;
      for (u32 x = 0; x < wave; ++x) below += wave_tot[x];
      u64 const m = block_sum(static_cast<u64>(t_ref), red), na = block_sum(static_cast<u64>(t_alt), red);
      u64 const rank2 = block_sum(static_cast<u64>(t_alt) * (2ull * below + t + 1ull), red);  // 2 x the ALT mid-rank sum
      u64 const tie = block_sum(static_cast<u64>(t) * t * t - t, red);
      if (tid == 0) {
        f64* st = A.o.fmt_stat + cell * 4;
        if (m > 0 && na > 0) {
          f64 const n_ref = static_cast<f64>(m), n_alt = static_cast<f64>(na), n_total = static_cast<f64>(m + na);
          f64 const alt_rank_sum = static_cast<f64>(rank2) / 2.0;
          f64 const u_stat = alt_rank_sum - ((n_alt * (n_alt + 1.0)) / 2.0);
          f64 const mean_u = (n_ref * n_alt) / 2.0;
          f64 const var_u = (n_ref * n_alt / 12.0) * ((n_total + 1.0) - (static_cast<f64>(tie) / (n_total * (n_total - 1.0))));
          f64 bqcd = 0.0;
          if (var_u > 0.0) {
            f64 const z = (u_stat - mean_u) / sqrt(var_u);
            bqcd = z / sqrt(n_total);
          }
          st[0] = bqcd;
          u64 alt_ref_nm = 0, alt_own_nm = 0;
          for (int a = 1; a < NA; ++a) {
            alt_ref_nm += sums[a * 3 + 1];
            alt_own_nm += sums[a * 3 + 2];
          }
          st[1] = (static_cast<f64>(alt_ref_nm) / n_alt - max_var_len) - static_cast<f64>(sums[1]) / n_ref;
          st[2] = (static_cast<f64>(alt_own_nm) / n_alt - 0.0) - static_cast<f64>(sums[2]) / n_ref;
        }
        if (na >= 3 && nhaps >= 2) {
          f64 const tot = static_cast<f64>(na);
          f64 entropy = 0.0;
          for (int h = 0; h < kEvMaxHaps; ++h) {
            if (!hapc[h]) continue;
            f64 const prob = static_cast<f64>(hapc[h]) / tot;
            entropy -= prob * log2(prob);
          }
          f64 const max_entropy = log2(fmin(tot, static_cast<f64>(nhaps)));
          st[3] = max_entropy > 0.0 ? entropy / max_entropy : 0.0;
        }
      }
    }

    if constexpr (kMeta) {
      u64 const m = depth(0), na = total - depth(0);
      if (A.m.ev_meta && tid < static_cast<u32>(NA)) {
        i64* em = A.m.ev_meta + (cell * NA + tid) * 4;
        em[0] = static_cast<i64>(msq[tid]);
        em[1] = scn[tid];
        em[2] = ppn[tid];
        em[3] = static_cast<i64>(isum[tid]);
      }
      if (A.m.fmt_rmq && tid < static_cast<u32>(K)) {
        u32 const d = depth(static_cast<int>(tid));
        A.m.fmt_rmq[cell * NA + tid] = d > 0 ? sqrt(static_cast<f64>(msq[tid]) / static_cast<f64>(d)) : 0.0;
      }
      f64* ms = A.m.fmt_mstat ? A.m.fmt_mstat + cell * 5 : nullptr;
      if (ms && tid == 0) {
        u64 alt_sc = 0, alt_pp = 0;
        i64 alt_isum = 0;
        for (int a = 1; a < NA; ++a) {
          alt_sc += scn[a];
          alt_pp += ppn[a];
          alt_isum += static_cast<i64>(isum[a]);
        }
        f64 const alt_frac = na > 0 ? static_cast<f64>(alt_sc) / static_cast<f64>(na) : 0.0;
        f64 const ref_frac = m > 0 ? static_cast<f64>(scn[0]) / static_cast<f64>(m) : 0.0;
        ms[0] = alt_frac - ref_frac;
        if (ppn[0] > 0 && alt_pp > 0) {
          f64 const ref_mean = static_cast<f64>(static_cast<i64>(isum[0])) / static_cast<f64>(ppn[0]);
          f64 const alt_mean = static_cast<f64>(alt_isum) / static_cast<f64>(alt_pp);
          ms[1] = (alt_mean - 0.0) - ref_mean;
        }
      }
      if (ms) {  // MQCD: BQCD's integer form over the MAPQ histogram
        u32 const t_ref = mqh[tid], t_alt = mqh[256 + tid], t = t_ref + t_alt;
        u32 incl = t;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          u32 const up = __shfl_up(incl, d, 64);
          if (lane >= static_cast<u32>(d)) incl += up;
        }
        __syncthreads();
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        u32 below = incl - t;
        for (u32 x = 0; x < wave; ++x) below += wave_tot[x];
        u64 const rank2 = block_sum(static_cast<u64>(t_alt) * (2ull * below + t + 1ull), red);
        u64 const tie = block_sum(static_cast<u64>(t) * t * t - t, red);
        if (tid == 0 && m > 0 && na > 0) ms[3] = mw_effect(m, na, rank2, tie);
      }
      if ((ms || A.m.ev_rpcd) && srt_a) {
        // the keys filed above (the filing loop ended at a barrier), padded with the largest key and sorted: the positions
        // first, then the bins.  Padded from the count that WAS filed: the depths say nk_want, and if the table walk ever found
        // fewer winners the slots behind them hold another cell's keys -- those are never ranked (and the cell keeps NaN / zero).
        u32 const nk_filed = min(*nkeys, nk_want);
        for (u32 x = nk_filed + tid; x < npad; x += kEvThreads) srt_a[x] = ~0ull;
        bool const filed_all = nk_filed == nk_want;
        __syncthreads();
        u64* src = srt_a;
        u64* dst = srt_b;
        for (u32 run = 1; run < npad; run <<= 1) {
          ev_merge_pass(src, dst, npad, run);
          __syncthreads();
          u64* const tmp = src;
          src = dst;
          dst = tmp;
        }
        // every run of equal values, from its first key: 2 x mid-rank = first + 1 + end (mann_whitney.h:170-192)
        u64 rank2 = 0, tie = 0;
        f64 entropy = 0.0;
        for (u32 i = tid; i < nk_want; i += kEvThreads) {
          u64 const g = ev_group_of(src[i]);
          if (i > 0 && ev_group_of(src[i - 1]) == g) continue;
          u32 j = i, alts = 0;
          for (; j < nk_want && ev_group_of(src[j]) == g; ++j) alts += static_cast<u32>(src[j] & 1ull);
          u64 const t = j - i;
          if (i < total) {
            tie += t * t * t - t;
            rank2 += static_cast<u64>(alts) * (static_cast<u64>(i) + 1ull + j);
          } else {
            f64 const prob = static_cast<f64>(t) / static_cast<f64>(na);
            entropy -= prob * log2(prob);
          }
        }
        rank2 = block_sum(rank2, red);
        tie = block_sum(tie, red);
        entropy = block_sum(entropy, red);
        if (tid == 0 && filed_all) {
          if (A.m.ev_rpcd) {
            u64* er = A.m.ev_rpcd + cell * 4;
            er[0] = m;
            er[1] = na;
            er[2] = rank2;
            er[3] = tie;
          }
          if (ms && m > 0 && na > 0) ms[2] = mw_effect(m, na, rank2, tie);
          if (ms && na >= 3) {
            f64 const max_entropy = log2(fmin(static_cast<f64>(na), 20.0));
            ms[4] = max_entropy > 0.0 ? entropy / max_entropy : 0.0;
          }
        }
      }
    }
  }
}

}  // namespace

int launch_evid_stats(ma_ctx* ctx, EvStatArgs A, u32 max_win_reads) {
  ma_params_t const& P = A.prm;
  size_t const cells = static_cast<size_t>(A.n_windows) * P.max_vars * P.num_samples, NA = P.max_alts + 1;
  if (A.n_windows <= 0) return MA_OK;
  if (P.max_haps > kEvMaxHaps || static_cast<size_t>(A.n_windows) * P.max_vars > 0x7FFFFFFFull) {
    ma_set_err(ctx, "FORMAT statistics: max_haps above 32 or more than 2^31 variant slots in a batch");
    return MA_ERR_PARAM;
  }
  bool const meta = fmeta_wanted(A.m);
  A.sort_off = nullptr;
  A.sort_ws = nullptr;
  if (meta && 2ull * max_win_reads > kEvSortCap) {
    // some cell may file more keys than the LDS buffers hold: every such window gets two buffers per variant in ws_sort.
    // Offsets from the host (rare: a window of more than kEvSortCap / 2 reads), [n] u64 in front of the slices.
    size_t const n = static_cast<size_t>(A.n_windows);
    std::vector<u32> rwo(n + 1), nvars(n);
    MA_HIP(ctx, hipMemcpyAsync(rwo.data(), A.read_win_off, 4 * (n + 1), hipMemcpyDeviceToHost, ctx->stream));
    MA_HIP(ctx, hipMemcpyAsync(nvars.data(), A.win_nvars, 4 * n, hipMemcpyDeviceToHost, ctx->stream));
    MA_HIP(ctx, ma_stream_sync(ctx));
    std::vector<u64> off(n, ~0ull);
    u64 keys = 0;
    for (size_t w = 0; w < n; ++w) {
      u32 const nrw = rwo[w + 1] - rwo[w], nv = std::min(nvars[w], static_cast<u32>(P.max_vars));
      if (2ull * nrw <= kEvSortCap || nv == 0) continue;
      off[w] = keys;
      keys += 2ull * ev_sort_pad(2u * nrw) * nv;
    }
    size_t const head = (8 * n + 255) & ~size_t(255);
    MA_HIP(ctx, ctx->ws_sort.reserve(head + 8 * keys + 256));
    MA_HIP(ctx, hipMemcpyAsync(ctx->ws_sort.p, off.data(), 8 * n, hipMemcpyHostToDevice, ctx->stream));
    MA_HIP(ctx, ma_stream_sync(ctx));  // (off is a local)
    A.sort_off = ctx->ws_sort.as<u64>();
    A.sort_ws = reinterpret_cast<u64*>(static_cast<char*>(ctx->ws_sort.p) + head);
  }
  ctx->tic("k_evid_stats");
  if (A.o.ev_sums) MA_HIP(ctx, hipMemsetAsync(A.o.ev_sums, 0, 4 * cells * NA * 3, ctx->stream));
  if (A.o.fmt_npbq) MA_HIP(ctx, hipMemsetAsync(A.o.fmt_npbq, 0, 8 * cells * NA, ctx->stream));
  if (A.o.fmt_cmlod) MA_HIP(ctx, hipMemsetAsync(A.o.fmt_cmlod, 0, 8 * cells * P.max_alts, ctx->stream));
  if (A.o.fmt_stat) MA_HIP(ctx, hipMemsetAsync(A.o.fmt_stat, 0xFF, 8 * cells * 4, ctx->stream));  // (all ones: a quiet NaN)
  if (A.m.ev_meta) MA_HIP(ctx, hipMemsetAsync(A.m.ev_meta, 0, 8 * cells * NA * 4, ctx->stream));
  if (A.m.ev_rpcd) MA_HIP(ctx, hipMemsetAsync(A.m.ev_rpcd, 0, 8 * cells * 4, ctx->stream));
  if (A.m.fmt_rmq) MA_HIP(ctx, hipMemsetAsync(A.m.fmt_rmq, 0, 8 * cells * NA, ctx->stream));
  if (A.m.fmt_mstat) MA_HIP(ctx, hipMemsetAsync(A.m.fmt_mstat, 0xFF, 8 * cells * 5, ctx->stream));
  size_t const lds = 4 * (NA * 259 + kEvMaxHaps);
  dim3 const grid(static_cast<u32>(A.n_windows) * static_cast<u32>(P.max_vars));
  if (meta) {
    // (the tallies, 8-byte aligned; 2 NA sums and two sort buffers of u64; the histogram, 2 NA counts and the key counter)
    size_t const lds_meta = ((lds + 7) & ~size_t(7)) + 8 * (2 * NA + 2 * kEvSortCap) + 4 * (512 + 2 * NA + 1);
    hipLaunchKernelGGL(k_evid_stats<true>, grid, dim3(kEvThreads), lds_meta, ctx->stream, A);
  } else {
    hipLaunchKernelGGL(k_evid_stats<false>, grid, dim3(kEvThreads), lds, ctx->stream, A);
  }
  ctx->toc();
  MA_HIP(ctx, hipGetLastError());
  return MA_OK;
}

}  // namespace ma
