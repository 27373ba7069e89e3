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
#include <type_traits>

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

// One workgroup per (window, variant slot), variant-major like k_qual: the slots no window uses leave at once.
__global__ __launch_bounds__(kEvThreads) void k_evid_stats(EvStatArgs A) {
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
  }
}

}  // namespace

int launch_evid_stats(ma_ctx* ctx, const EvStatArgs& A) {
  ma_params_t const& P = A.prm;
  size_t const cells = static_cast<size_t>(A.n_windows) * P.max_vars * P.num_samples, NA = P.max_alts + 1;
  if (A.n_windows <= 0) return MA_OK;
  if (P.max_haps > kEvMaxHaps || static_cast<size_t>(A.n_windows) * P.max_vars > 0x7FFFFFFFull) {
    ma_set_err(ctx, "FORMAT statistics: max_haps above 32 or more than 2^31 variant slots in a batch");
    return MA_ERR_PARAM;
  }
  ctx->tic("k_evid_stats");
  if (A.o.ev_sums) MA_HIP(ctx, hipMemsetAsync(A.o.ev_sums, 0, 4 * cells * NA * 3, ctx->stream));
  if (A.o.fmt_npbq) MA_HIP(ctx, hipMemsetAsync(A.o.fmt_npbq, 0, 8 * cells * NA, ctx->stream));
  if (A.o.fmt_cmlod) MA_HIP(ctx, hipMemsetAsync(A.o.fmt_cmlod, 0, 8 * cells * P.max_alts, ctx->stream));
  if (A.o.fmt_stat) MA_HIP(ctx, hipMemsetAsync(A.o.fmt_stat, 0xFF, 8 * cells * 4, ctx->stream));  // (all ones: a quiet NaN)
  size_t const lds = 4 * (NA * 259 + kEvMaxHaps);
  hipLaunchKernelGGL(k_evid_stats, dim3(static_cast<u32>(A.n_windows) * static_cast<u32>(P.max_vars)), dim3(kEvThreads), lds,
                     ctx->stream, A);
  ctx->toc();
  MA_HIP(ctx, hipGetLastError());
  return MA_OK;
}

}  // namespace ma
