/* microasm.h -- C-ABI of the MI355X-native per-window microassembly engine.
 *
 * Drop-in boundary for Lancet2's per-window worker (core/variant_builder.cpp:201-276).  The
 * reference has no FFI layer; each entry point below replaces one C++ seam inside
 * VariantBuilder::ProcessWindow and is batched over windows (the unit of data parallelism):
 *
 *   ma_repeat_gate_batch   <- base::HasRepeat / HasExactRepeat            (base/repeat.h:22-27;
 *                             callers cbdg/graph.h:127-131, core/variant_builder.cpp:116-117)
 *   ma_assemble_batch      <- cbdg::Graph::BuildComponentResults          (cbdg/graph.h:53)
 *   ma_msa_batch           <- caller::MsaBuilder::UpdateSpoaState + caller::VariantSet ctor
 *                             (caller/msa_builder.h:81-92, caller/variant_set.h:25)
 *   ma_genotype_batch      <- caller::Genotyper::Genotype                 (caller/genotyper.h:219)
 *   ma_annotate_batch      <- core::VariantAnnotator::Annotate{Sequence,Graph}Complexity (core/variant_annotator.h)
 *   ma_process_batch       <- the chained body of ProcessWindow           (core/variant_builder.cpp:229-262)
 *   ma_genotype_stats_batch / ma_process_stats_batch: the same two calls + seven of the read-level FORMAT statistics
 *                             (caller/variant_support.h:361-411, caller/variant_call.cpp:141-196, :347-381)
 *   ma_process_packed_batch / ma_prefetch_packed_batch: ma_process_stats_batch / ma_prefetch_batch with the read bases, and
 *                             optionally the qualities, as 4-bit codes (ma_packed_reads_t): half the bytes over the link
 *   ma_genotype_meta_batch / ma_process_meta_batch / ma_prefetch_meta_batch: the calls above + four facts of every read's BAM
 *                             record (ma_read_meta_t) and the six FORMAT statistics over them: RMQ, MQCD, SCA, FLD, RPCD, FSSE
 *                             (caller/variant_support.cpp:184-194, :261-305, :358-363, base/mann_whitney.h:127-225)
 *   ma_process_cx_batch    <- ma_process_meta_batch + the annotation of ma_annotate_batch as a stage of the chain, where
 *                             VariantBuilder::ExtractVariants has it (core/variant_builder.cpp:157-160): the whole per-window
 *                             body in one call
 *   ma_assemble_probe_batch <- ma_assemble_batch + the --probe-variants diagnostic: each truth allele followed through the
 *                             window's reads, raw graph, pruned graph and haplotypes (cbdg/probe_tracker.cpp)
 *   ma_flatten_records_batch <- core::ReadCollector's sort, name interning and per-read copies (core/read_collector.cpp:42-53,
 *                             :218-234) from raw BAM alignment records: the read arrays of a batch, made on the device
 *   ma_select_records_batch <- the record filters and per-sample sums of core::ReadCollector (core/read_collector.cpp:147-216),
 *                             core::ActiveRegionDetector (core/active_region_detector.cpp:85-232) and the anchor-coverage gate
 *                             (core/variant_builder.cpp:214-224) on every candidate record of a window: which records go on,
 *                             as the lists ma_flatten_records_batch takes
 *   ma_inflate_blocks_batch <- htslib's BGZF reader under hts::Extractor (hts/extractor.cpp): compressed BGZF blocks to their
 *                             payloads, CRC checked, on the device; ma_index_records_batch <- its record iteration: where the
 *                             alignment records of the inflated bytes are, with refID, pos and reference span of each
 *
 * Conventions: plain pointers and sizes only; all buffers are caller owned, struct-of-arrays;
 * every function returns 0 on success and a negative ma_error otherwise and never throws.
 * Pointers are HOST pointers when the context was created with MA_MEM_HOST (the library stages
 * them through HBM itself) and DEVICE pointers with MA_MEM_DEVICE (zero-copy; the bench path).
 * Reads of a window must arrive in the collector's sorted order (core/read_collector.cpp:42-53).
 */
#ifndef MICROASM_H_
#define MICROASM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MA_VERSION 3

enum ma_error {
  MA_OK = 0,
  MA_ERR_ARG = -1,      /* bad argument / inconsistent sizes */
  MA_ERR_NO_DEVICE = -2,/* no HIP device: the engine has NO CPU fallback */
  MA_ERR_HIP = -3,      /* HIP runtime error (see ma_last_error) */
  MA_ERR_NOMEM = -4,    /* workspace allocation failed */
  MA_ERR_PARAM = -5     /* parameter out of the supported range */
};

enum ma_memspace { MA_MEM_HOST = 0, MA_MEM_DEVICE = 1 };

/* Per-window status bits (0 == assembled cleanly). Mirrors the skip reasons of
 * VariantBuilder::StatusCode (core/variant_builder.h:73-83) plus engine capacity flags. */
enum ma_wstatus {
  MA_W_NO_HAPLOTYPE = 1u << 0,   /* SKIPPED_NOASM_HAPLOTYPE: no ALT haplotype at any k */
  MA_W_HAP_OVERFLOW = 1u << 1,   /* more haplotypes / components than max_haps / max_comps */
  MA_W_LEN_OVERFLOW = 1u << 2,   /* haplotype longer than max_hap_len, or than the POA stage takes (poa.hip: poa_max_hap_len, printed under MA_VERBOSE), or more runs than max_runs */
  MA_W_BFS_LIMIT = 1u << 3,      /* MaxFlow::HitTraversalLimit (max_flow.h:69) in some component */
  MA_W_TABLE_OVERFLOW = 1u << 4, /* k-mer table / edge list / search arena capacity exceeded, or the traversal cap fell where
                                    the folded walk search cannot place it: the window's result is not the reference's */
  MA_W_VAR_OVERFLOW = 1u << 5,   /* more variants / alleles / allele bytes than the caps */
  MA_W_CIGAR_OVERFLOW = 1u << 6, /* a read<->haplotype CIGAR had more than max_cigar operations and was cut before the scoring
                                    epilogue (local_scorer.cpp:166-279 scores the whole CIGAR): re-submit the window with a
                                    larger max_cigar -- 2 * ((read length - 80) / 15) + 3 operations always suffice */
  MA_W_READ_OVERFLOW = 1u << 7   /* the window holds a read longer than the stage supports (assembly: 1024 bases, genotyping:
                                    608): the stage skips the window (no haplotypes / no allele counts) instead of failing
                                    the batch */
};

/* GraphParams (cbdg/graph_params.h:29-53) + the constants the reference hard-codes + engine caps. */
typedef struct ma_params {
  int32_t min_k, max_k, k_step;          /* 13, 127, 6 */
  int32_t min_node_cov, min_anchor_cov;  /* 2, 5 */
  int32_t num_samples;                   /* GraphParams::mNumSamples */
  int32_t min_anchor_len;                /* 150  (graph.cpp:88) */
  int32_t max_mismatch;                  /* 2    (graph.h:129) */
  int32_t bfs_limit;                     /* 1<<20 (max_flow.h:69) */
  /* read<->haplotype aligner (genotyper.cpp:89-191 as restated in DESIGN.md).  There is no band parameter: like the
   * reference (bw = 10000, genotyper.cpp:140) the search region never excludes an alignment its seeds support; it is
   * derived per pair from the seed diagonals, the read length and min_aln_score. */
  int32_t aln_tier;                      /* testing knob, results NEVER depend on it.  0 (default): every pair takes the
                                            cheapest exact route.  bit 0: all DP pairs through the generic any-width kernel;
                                            bit 1: the gapless certificates are off (every seeded pair runs the DP) */
  int32_t min_aln_score;                 /* 80 (minimap2 min_dp_max default) */
  /* engine caps (outputs are fixed-stride; overflow sets a status bit) */
  int32_t max_comps;                     /* components kept per window (default 4) */
  int32_t max_haps;                      /* haplotype slots per window, REF included (default 16, at most 32: a component of
                                            17 .. 32 haplotypes takes the POA's 32-bit-label kernels; the reference has no cap,
                                            cbdg/graph.cpp:846-924 -- beyond 32 the window is flagged MA_W_HAP_OVERFLOW) */
  int32_t max_hap_len;                   /* bytes per haplotype slot (default 2048) */
  int32_t max_runs;                      /* (weight,nbases) runs per haplotype (default 256) */
  int32_t max_vars;                      /* variants per window (default 64) */
  int32_t max_alts;                      /* ALT alleles per variant (default 4) */
  int32_t max_allele_bytes;              /* allele-string pool per window (default 4096) */
  int32_t max_cigar;                     /* CIGAR ops kept per read x haplotype alignment (default 16) */
  int32_t case_ctrl_mode;                /* 1: QUAL = SOLOR (variant_call.cpp:316-345) */
} ma_params_t;

void ma_default_params(ma_params_t* p);

/* One batch of windows.  Window w owns reference bytes [ref_off[w], ref_off[w+1]) and reads
 * [read_win_off[w], read_win_off[w+1]); read r owns bases/quals [read_off[r], read_off[r+1]).
 * Limits: windows up to 8192 bases (repeat gate), reads up to 608 bases (ma_genotype_batch answers MA_ERR_PARAM
 * beyond: short-read data only, like the reference's 150 bp workloads). */
typedef struct ma_batch {
  int32_t n_windows;
  int64_t n_reads;
  const uint8_t* ref_bases;       /* ASCII, already normalised to ACGTN (hts/reference.cpp:176-194) */
  const uint32_t* ref_off;        /* [n_windows + 1] */
  const uint32_t* read_win_off;   /* [n_windows + 1] */
  const uint64_t* read_off;       /* [n_reads + 1] */
  const uint8_t* read_bases;      /* ASCII (hts/alignment.cpp:123-143 decode) */
  const uint8_t* read_quals;      /* Phred */
  const uint32_t* read_qname_id;  /* host-interned QNAME, unique per distinct name within a window */
  const uint8_t* read_sample;     /* cbdg::Read::SampleIndex() */
  const uint8_t* read_flags;      /* MA_RF_* */
  /* OPTIONAL (may be NULL) performance hint: window-relative 0-based reference offset at which base 0 of
   * the read is expected to align (cbdg::Read::StartPos0() - window start - leading soft clip), or
   * MA_NO_HINT.  Results never depend on it: k-mers that equal the reference k-mer at the hinted offset
   * skip the hash table, everything else takes the general path. */
  const int32_t* read_hint;
} ma_batch_t;

#define MA_NO_HINT INT32_MIN

enum ma_read_flags {
  MA_RF_PASS = 1u << 0,  /* cbdg::Read::PassesAlnFilters(): mapq >= 20 (cbdg/read.h:35-38) */
  MA_RF_CASE = 1u << 1,  /* Label::CASE (tumor) if set, Label::CTRL (normal) otherwise */
  MA_RF_REV = 1u << 2    /* SAM flag 0x10: reverse strand (genotyper.cpp:427) */
};

/* ---- repeat gate ------------------------------------------------------------------------ */
/* max_approx[w] = length of the longest pair of equal-length substrings at different offsets of
 * window w that differ in <= max_mismatch positions; max_exact[w] likewise with 0 mismatches.
 * HasRepeat(SlidingView(ref,k), mm) (base/repeat.cpp:348-371) == (max_approx[w] >= k);
 * HasExactRepeat(SlidingView(ref,max_k)) (variant_builder.cpp:116-117) == (max_exact[w] >= max_k). */
typedef struct ma_gate_out {
  uint32_t* max_approx; /* [n_windows] */
  uint32_t* max_exact;  /* [n_windows] */
} ma_gate_out_t;

/* ---- assembly output (ComponentResult, cbdg/component_result.h:32-81) -------------------- */
typedef struct ma_asm_out {
  uint32_t* win_status;   /* [n]            ma_wstatus bits */
  uint32_t* win_k;        /* [n]            Graph::CurrentK() */
  uint32_t* win_ncomp;    /* [n]            components with >= 1 walk */
  /* per component, stride max_comps */
  uint32_t* comp_anchor;  /* AnchorStartOffset() */
  uint32_t* comp_hap0;    /* first haplotype slot of this component (REF) */
  uint32_t* comp_nhaps;   /* NumPaths() */
  uint32_t* comp_cx;      /* [.. * 3] cyclomatic, branch points, max single-direction degree */
  double* comp_cxf;       /* [.. * 4] unitig ratio, coverage CV, tip/path cov ratio, MaxAltPathCv (-1: none) */
  /* per haplotype slot, stride max_haps */
  uint32_t* hap_len;      /* Path::Sequence().size() */
  uint32_t* hap_nruns;    /* number of (weight, nbases) runs (Path::mNodeWeights) */
  double* hap_stats;      /* [.. * 6] mean, median, sd, cv, qcv, total coverage (path.cpp:39-70) */
  uint8_t* hap_bases;     /* [.. * max_hap_len] */
  uint32_t* hap_runs;     /* [.. * max_runs * 2] weight, nbases */
} ma_asm_out_t;

/* ---- MSA + variant extraction (RawVariant, caller/raw_variant.h) ------------------------- */
typedef struct ma_var_out {
  uint32_t* win_nvars;    /* [n] */
  /* per variant, stride max_vars */
  uint32_t* var_comp;     /* component index within the window */
  uint32_t* var_pos;      /* 0-based offset in the window of mGenomeChromPos1 (pos1 = StartPos1 + var_pos) */
  uint32_t* var_ref_start;/* mLocalRefStart0Idx */
  uint32_t* var_ref_off;  /* REF allele: offset/len into this window's allele pool */
  uint32_t* var_ref_len;
  uint32_t* var_nalts;
  /* per (variant, alt), stride max_alts */
  uint32_t* alt_off;
  uint32_t* alt_len;
  int32_t* alt_type;      /* AlleleType: 0 SNV 1 INS 2 DEL 3 MNP 4 CPX (caller/alt_allele.h:14) */
  int32_t* alt_length;    /* AltAllele::mLength */
  /* per (variant, haplotype-of-its-component), stride max_haps: which allele the haplotype carries
   * (0 = REF, a+1 = ALT a) and where the bubble starts on it (AltAllele::mLocalHapStart0Idxs) */
  uint8_t* var_hap_allele;
  uint32_t* var_hap_start;
  uint8_t* allele_pool;   /* [n * max_allele_bytes] */
} ma_var_out_t;

/* ---- genotyping (VariantSupport, caller/variant_support.cpp:24-66) ----------------------- */
typedef struct ma_geno_out {
  /* [n * max_vars * num_samples * (max_alts+1) * 2]: fwd, rev read counts per allele (AD = fwd+rev) */
  uint32_t* allele_counts;
  double* var_qual;       /* [n * max_vars] site QUAL: SOLOR in case/ctrl mode (variant_call.cpp:316-345), else the largest
                           * PL[0/0] over the samples with evidence (variant_call.cpp:289-303) */
  /* optional debug taps (may be NULL): per read x haplotype slot of the read's window */
  int32_t* aln_rec;       /* [n_reads * max_haps * 6] hit, score, rs, re, qs, qe */
  uint32_t* aln_cigar;    /* [n_reads * max_haps * (1 + max_cigar)] n_ops, then len<<4|op (op: 0 M 1 I 2 D 4 S) */
  /* optional: per read x variant: allele (255 = none) and CombinedScore */
  uint8_t* asg_allele;    /* [n_reads * max_vars] */
  double* asg_score;      /* [n_reads * max_vars] */
  /* optional (may be NULL): FORMAT PL and GQ of every sample with evidence -- Dirichlet-multinomial genotype
   * likelihoods over the sample's allele depths (caller/genotype_likelihood.cpp:93-272), VCF genotype order
   * (0/0, 0/1, 1/1, 0/2, ...), G = (max_alts + 1)(max_alts + 2) / 2 slots of which the first K(K+1)/2 are used for a
   * variant with K alleles; zero for samples without evidence */
  uint32_t* var_pl;       /* [n * max_vars * num_samples * G] */
  uint32_t* var_gq;       /* [n * max_vars * num_samples] */
} ma_geno_out_t;

/* ---- variant annotation (core/variant_annotator.cpp:43-101; VCF INFO SEQ_CX / GRAPH_CX) ------ */
typedef struct ma_cx_out {
  /* per variant, stride max_vars.  SequenceComplexity (base/sequence_complexity.h:106-158), merged over the
   * variant's (ALT, haplotype) sites with MergeMax exactly as AnnotateSequenceComplexity does */
  int32_t* seq_cx_i;  /* [.. * 4] ContextHRun, DeltaHRun, TrPeriod, IsStutterIndel */
  float* seq_cx_f;    /* [.. * 4] ContextEntropy, DeltaEntropy, TrAffinity, TrPurity */
  double* seq_cx_d;   /* [.. * 3] ContextFlankLQ, ContextHaplotypeLQ, DeltaFlankLQ */
  double* graph_cx;   /* [.. * 3] GraphEntanglementIndex, TipToPathCovRatio, MaxSingleDirDegree
                       * (caller::GraphMetrics, variant_annotator.cpp:87-99) */
} ma_cx_out_t;

/* ---- read-level FORMAT statistics (since MA_VERSION 3) ------------------------------------------------------------ */
/* One set per (window, variant slot, sample), over the de-duplicated evidence reads that allele_counts counts.  Per evidence
 * read, from the alignment that won AssignReadToAlleles (genotyper.cpp:269-321): base_qual = the representative base quality
 * of ComputeLocalScore (local_scorer.cpp:166-279), ref_nm = edit distance to the component's REF haplotype (the read length
 * without such an alignment, combined_scorer.cpp:24-38), own_nm = edit distance to the winning haplotype, hap_id = that
 * haplotype's index in its component.  Every member is optional (may be NULL); arrays that are asked for are zero -- fmt_stat
 * NaN -- in unused variant slots and for samples without evidence. */
typedef struct ma_fmt_out {
  uint32_t* ev_sums;   /* [n * max_vars * S * (max_alts+1) * 3] per allele: sum of base_qual, of ref_nm, of own_nm */
  double* fmt_npbq;    /* [n * max_vars * S * (max_alts+1)] NPBQ: posterior base quality / allele depth
                        * (caller/posterior_base_qual.cpp:14-40, variant_call.cpp:368-373) */
  double* fmt_cmlod;   /* [n * max_vars * S * max_alts] CMLOD per ALT (caller/genotype_likelihood.cpp:141-196, :307-345) */
  double* fmt_stat;    /* [n * max_vars * S * 4] BQCD (base/mann_whitney.h:127-225), ASMD, AHDD (variant_support.h:361-387),
                        * HSE (variant_support.h:389-411); NaN = missing (the reference's nullopt, "." in the VCF) */
} ma_fmt_out_t;

/* ---- packed read input: 4-bit bases, 4- or 8-bit qualities -------------------------------------------------------- */
/* The read bases -- and, when the batch holds at most 16 distinct Phred values, the qualities -- of a batch as 4-bit codes:
 * what BAM stores and binned instruments emit, and half of what ma_batch_t::read_bases / read_quals put on the link.  The
 * library expands them on the device (one kernel, k_unpack_reads) into the very ASCII and Phred arrays the stages read from a
 * plain call, so results are those of the plain call on the decoded arrays, byte for byte.
 *
 * A nibble array holds read after read, high nibble first.  Read r starts on a BYTE boundary, at byte (read_off[r] + r) >> 1,
 * and occupies (len + 1) / 2 bytes; the low nibble of the last byte of an odd-length read is ignored.  The whole array is
 * (read_off[n_reads] + n_reads + 1) / 2 bytes long.  The rule needs no offsets of its own and reads never overlap
 * (floor((x + len + 1) / 2) - floor(x / 2) >= ceil(len / 2)); bytes between two reads are ignored.  A host can memcpy the
 * sequence bytes of a BAM record straight to the read's offset: the base codes are BAM's.  (The kernel reads the aligned
 * 4-byte words that hold a byte of the array, nothing beyond them.) */
typedef struct ma_packed_reads {
  const uint8_t* bases4;   /* 4-bit base codes, BAM's own: index into "=ACMGRSVTWYHKDBN", high nibble first */
  const uint8_t* quals;    /* qual_bits == 4: 4-bit codes into qual_dict, laid out like bases4;
                              qual_bits == 8: Phred bytes at read_off[], as ma_batch_t::read_quals */
  int32_t qual_bits;       /* 4 or 8 */
  uint8_t qual_dict[16];   /* Phred value of each 4-bit code (qual_bits == 4) */
} ma_packed_reads_t;

/* ---- read metadata and the six FORMAT statistics over it ----------------------------------------------------------- */
/* RMQ, MQCD, SCA, FLD, RPCD and FSSE of every (window, variant slot, sample), over the same de-duplicated evidence reads as
 * ma_fmt_out_t (of mates that share a name, support one allele and belong to one sample only the first counts, with ITS
 * metadata).  Four facts per read come from the caller's BAM record; the fifth input, the position of the variant in the
 * read, is taken from the alignment that won AssignReadToAlleles (caller/combined_scorer.cpp:96-105). */
enum ma_read_mflags { MA_RM_SOFTCLIP = 1u << 0,   /* cbdg::Read::IsSoftClipped(): soft-clipped bases >= 6 % of the read (cbdg/read.h:39-50) */
                      MA_RM_PROPER = 1u << 1 };   /* SAM flag 0x2 (cbdg/read.h:72) */
typedef struct ma_read_meta {      /* every member [n_reads], all four required */
  const uint8_t* read_mapq;        /* cbdg::Read::MapQual() */
  const uint8_t* read_mflags;      /* MA_RM_* */
  const int32_t* read_isize;       /* InsertSize(): BAM tlen, signed */
  const int32_t* read_start;       /* StartPos0(): BAM pos, >= 0 */
} ma_read_meta_t;
/* Every member optional (may be NULL); a cell is a (window, variant slot, sample), laid out like ma_fmt_out_t.  Unused variant
 * slots and samples without evidence hold zeros (fmt_mstat: NaN).  ALT = the ALT alleles pooled.
 *   ev_meta  per allele: sum of mapq^2, soft-clipped reads, proper-pair reads with isize != 0, sum of their isize
 *   ev_rpcd  n_ref, n_alt, 2 x the ALT mid-rank sum, sum of t^3 - t over the tie groups -- of the folded positions
 *            min(x, 1.0 - x), x = (double)qpos / (double)read length, ranked as the doubles they are (bit patterns)
 *   fmt_rmq  RMQ per allele (caller/variant_support.cpp:184-194); 0.0 for an allele without reads
 *   fmt_mstat SCA (variant_support.cpp:261-279), FLD (:49-51, variant_support.h:361-387), RPCD, MQCD (base/mann_whitney.h:
 *            127-225), FSSE (variant_support.h:391-411, .cpp:358-363); NaN = missing (the reference's nullopt): FLD when REF
 *            or ALT has no insert size, RPCD / MQCD when REF or ALT has no read, FSSE below three ALT reads */
typedef struct ma_fmt_meta_out {
  int64_t* ev_meta;    /* [n * max_vars * S * (max_alts+1) * 4] */
  uint64_t* ev_rpcd;   /* [n * max_vars * S * 4] */
  double* fmt_rmq;     /* [n * max_vars * S * (max_alts+1)] */
  double* fmt_mstat;   /* [n * max_vars * S * 5] */
} ma_fmt_meta_out_t;

typedef struct ma_ctx ma_ctx_t;

int ma_create(const ma_params_t* prm, int device, int memspace, ma_ctx_t** out);
void ma_destroy(ma_ctx_t* ctx);
const char* ma_last_error(const ma_ctx_t* ctx);
/* HIP stream all launches and copies go to (void* == hipStream_t).  A context starts on a non-blocking stream of its
 * own, so that several contexts on one device overlap; NULL selects the legacy null stream. */
int ma_set_stream(ma_ctx_t* ctx, void* hip_stream);
int ma_synchronize(ma_ctx_t* ctx);

int ma_repeat_gate_batch(ma_ctx_t* ctx, const ma_batch_t* b, const ma_gate_out_t* out);
int ma_assemble_batch(ma_ctx_t* ctx, const ma_batch_t* b, const ma_asm_out_t* out);
int ma_msa_batch(ma_ctx_t* ctx, const ma_batch_t* b, const ma_asm_out_t* asmb, const ma_var_out_t* out);
int ma_genotype_batch(ma_ctx_t* ctx, const ma_batch_t* b, const ma_asm_out_t* asmb,
                      const ma_var_out_t* vars, const ma_geno_out_t* out);
/* VariantAnnotator::AnnotateSequenceComplexity + AnnotateGraphComplexity (core/variant_annotator.cpp:43-101,
 * called from VariantBuilder::ExtractVariants, core/variant_builder.cpp:159-160) for every variant of the batch.
 * gc_frac = the --genome-gc-bias background GC fraction of the LongdustQ null model (default 0.41).
 * Integer features are exact; the f32/f64 features go through device log2f/log1p/log10. */
int ma_annotate_batch(ma_ctx_t* ctx, const ma_batch_t* b, const ma_asm_out_t* asmb, const ma_var_out_t* vars,
                      double gc_frac, const ma_cx_out_t* out);
/* gate -> assemble -> msa -> genotype on one batch; any output struct may be NULL-filled only in
 * its optional members. */
int ma_process_batch(ma_ctx_t* ctx, const ma_batch_t* b, const ma_gate_out_t* gate,
                     const ma_asm_out_t* asmb, const ma_var_out_t* vars, const ma_geno_out_t* geno);

/* ma_genotype_batch / ma_process_batch + the read-level FORMAT statistics.  fmt == NULL, or all four members NULL, IS the
 * plain call: the same kernels, nothing allocated.  Otherwise the genotype stage keeps one 8-byte record per read and
 * variant slot and one more kernel (k_evid_stats) reduces the evidence reads' records to the statistics. */
int ma_genotype_stats_batch(ma_ctx_t* ctx, const ma_batch_t* b, const ma_asm_out_t* asmb, const ma_var_out_t* vars,
                            const ma_geno_out_t* geno, const ma_fmt_out_t* fmt);
int ma_process_stats_batch(ma_ctx_t* ctx, const ma_batch_t* b, const ma_gate_out_t* gate, const ma_asm_out_t* asmb,
                           const ma_var_out_t* vars, const ma_geno_out_t* geno, const ma_fmt_out_t* fmt);

/* MA_MEM_HOST only (a no-op otherwise): hand over the batch the caller will pass to ma_process_batch NEXT and return at
 * once -- the staged pipeline of the reference's AsyncWorker (core/async_worker.cpp:47-110: extract window j + 1 while window
 * j is assembled) at batch granularity:
 *     ma_prefetch_batch(ctx, &batch[j + 1]);  ma_process_batch(ctx, &batch[j], ...);
 * The context uploads the batch in the background (an uploader thread, 16 MB pieces) and queues its COMPUTE behind whatever
 * its lanes are doing: a lane goes from the last kernel of batch j straight to the first of batch j + 1, and
 * ma_process_batch(j + 1) only waits for the packed records and scatters them into the caller's arrays.  Work that was
 * queued ahead assumes that the call will ask for the same optional output arrays (statistics included) as the previous one did, with
 * the same parameters and timing mode; if it does not (or asks for the per-read debug taps), the queued results are dropped
 * and the batch is computed in the call -- results never depend on whether, or how, a batch was prefetched.
 * `next` and the arrays it points to must stay unchanged until the ma_process_batch call that consumes it (recognised by
 * the struct's address, window and read counts) has returned; the arrays should be page-locked (hipHostMalloc /
 * hipHostRegister), a copy from pageable memory is slow.  At most two batches wait at a time; further calls do nothing. */
int ma_prefetch_batch(ma_ctx_t* ctx, const ma_batch_t* next);

/* ma_process_stats_batch / ma_prefetch_batch on packed reads.  b->read_bases and b->read_quals must be NULL (MA_ERR_ARG
 * otherwise: a batch is either ASCII or packed); pk == NULL, a NULL member of it or a qual_bits other than 4 and 8 are
 * MA_ERR_ARG too.  Everything else is ma_process_stats_batch's: fmt is optional, the same lanes, caps and status flags.  Both
 * memory spaces: with MA_MEM_DEVICE pk's two pointers are device pointers (the struct itself is always in host memory) and
 * the expansion goes into workspace of the context.  A prefetched batch is recognised by the batch struct's address, its
 * counts AND pk's address: a batch queued as ASCII and brought packed, or the other way round, is dropped and computed in
 * the call, like one queued for other optional outputs.  pk and its arrays stay unchanged as long as `next` must.
 * The single-stage calls (ma_repeat_gate_batch, ma_assemble_batch, ma_msa_batch, ma_genotype_batch, ma_genotype_stats_batch,
 * ma_annotate_batch) do not take the packed form. */
int ma_process_packed_batch(ma_ctx_t* ctx, const ma_batch_t* b, const ma_packed_reads_t* pk, const ma_gate_out_t* gate,
                            const ma_asm_out_t* asmb, const ma_var_out_t* vars, const ma_geno_out_t* geno,
                            const ma_fmt_out_t* fmt);
int ma_prefetch_packed_batch(ma_ctx_t* ctx, const ma_batch_t* next, const ma_packed_reads_t* next_pk);

/* ma_genotype_stats_batch / ma_process_stats_batch / ma_process_packed_batch (pk != NULL) / the two prefetch calls + the
 * read metadata and the statistics over it.  fmeta == NULL, or all four members NULL, IS the call without them -- the same
 * kernels, nothing allocated, and `meta` is not read.  Any member of fmeta set with meta NULL, or with a NULL member of meta,
 * is MA_ERR_ARG.  Both memory spaces: with MA_MEM_DEVICE meta's four arrays are device pointers (the structs themselves are
 * always in host memory).  The genotype stage then notes the variant's position in the winning alignment in the record it
 * keeps per read and variant slot, and k_evid_stats tallies the metadata of the evidence reads and ranks their positions (one
 * sort per cell).  A prefetched batch is recognised by the batch's address, its counts, pk's address AND
 * meta's: one queued by ma_prefetch_batch / ma_prefetch_packed_batch and brought here with statistics wanted, or queued with
 * another meta, is dropped and computed in the call; a call that does not ask for the statistics takes a queued batch whatever
 * metadata came with it.  meta and its arrays stay unchanged as long as `next` must.
 * Workspace: a cell's keys are sorted in LDS up to 2048 of them (evidence reads + ALT reads); only windows of more than 1024
 * reads get a sort slice in device memory, 16 bytes x the next power of two of twice the window's reads per variant of the
 * window (a deep-panel window of 7000 reads: 256 KB per variant; 2048 such windows of three variants: 1.6 GB). */
int ma_genotype_meta_batch(ma_ctx_t* ctx, const ma_batch_t* b, const ma_read_meta_t* meta, const ma_asm_out_t* asmb,
                           const ma_var_out_t* vars, const ma_geno_out_t* geno, const ma_fmt_out_t* fmt,
                           const ma_fmt_meta_out_t* fmeta);
int ma_process_meta_batch(ma_ctx_t* ctx, const ma_batch_t* b, const ma_packed_reads_t* pk /* NULL: an ASCII batch */,
                          const ma_read_meta_t* meta, const ma_gate_out_t* gate, const ma_asm_out_t* asmb,
                          const ma_var_out_t* vars, const ma_geno_out_t* geno, const ma_fmt_out_t* fmt,
                          const ma_fmt_meta_out_t* fmeta);
int ma_prefetch_meta_batch(ma_ctx_t* ctx, const ma_batch_t* next, const ma_packed_reads_t* next_pk /* or NULL */,
                           const ma_read_meta_t* next_meta);

/* ma_process_meta_batch + the annotation of ma_annotate_batch as a stage of the chain (after the MSA, before genotyping, as
 * in VariantBuilder::ExtractVariants).  cx == NULL, or all four members NULL, IS ma_process_meta_batch: the same kernels,
 * nothing allocated, gc_frac not read.  Some but not all four members set is MA_ERR_ARG, and so is a NaN gc_frac with cx
 * wanted; a gc_frac outside [0, 1] is clamped, as in ma_annotate_batch.  The stage reads the engine's own device-side assembly
 * and variant arrays -- nothing is uploaded for it, and with MA_MEM_HOST a caller may leave hap_bases, hap_runs and any other
 * optional array out and still get the annotation; only the used variant slots come back (80 bytes each).  In every variant
 * slot a window uses (slot < win_nvars[w]) the result is byte for byte what ma_annotate_batch returns for the same assembly
 * and variant arrays and the same gc_frac; what unused slots hold is unspecified.  There is no prefetch call of its own: a
 * batch queued by ma_prefetch_batch / ma_prefetch_packed_batch / ma_prefetch_meta_batch is computed for what the previous
 * call asked for -- the four annotation arrays and that call's gc_frac included -- and dropped and computed in the call if
 * this call asks for other arrays or another gc_frac. */
int ma_process_cx_batch(ma_ctx_t* ctx, const ma_batch_t* b, const ma_packed_reads_t* pk /* NULL: ASCII */,
                        const ma_read_meta_t* meta /* or NULL */, const ma_gate_out_t* gate, const ma_asm_out_t* asmb,
                        const ma_var_out_t* vars, const ma_geno_out_t* geno, const ma_fmt_out_t* fmt,
                        const ma_fmt_meta_out_t* fmeta, double gc_frac, const ma_cx_out_t* cx);

/* Kernel timing mode: 0 = off, 1 = reset at every API call (default), 2 = accumulate across calls
 * until ma_timing_control is called again (used by bench.py to time kernels over the timed region), 3 = as 2 and
 * one extra small kernel per k attempt gathers the workload statistics ma_last_stats reports in out[8..13]
 * (bench.py runs one untimed step in this mode). */
int ma_timing_control(ma_ctx_t* ctx, int mode);

/* Per-kernel timing of the last call, measured with HIP events on the launch stream.
 * names[i] points to a static string; returns the number of entries written (<= cap). */
int ma_last_kernel_times(ma_ctx_t* ctx, const char** names, float* ms, int cap);

/* ma_process_batch runs a batch as `n` contiguous window ranges concurrently, each on its own HIP stream and
 * workspace (the stages have complementary bottlenecks, so two ranges in flight fill each other's gaps).
 * n = 0 (default): automatic -- 3 for batches of >= 6144 windows, 2 for >= 2048, else 1.  Results do not depend on n.
 * The caller's stream (ma_set_stream) still orders the call as a whole. */
int ma_set_streams(ma_ctx_t* ctx, int n);

/* 0 (default): the POA stage as it is.  1: windows whose POA graph ran out of nodes or of per-node edge / aligned-node
 * slots are re-run inside the call -- from their first component -- by a second pass with a larger graph; only what that
 * pass cannot hold either stays MA_W_VAR_OVERFLOW.  Applies to ma_msa_batch and every chained call, on every lane and route.
 * Results of windows that were not flagged never depend on it.  Any other value of `on`: MA_ERR_ARG.
 * (MA_W_VAR_OVERFLOW from an output cap -- max_vars, max_alts, max_allele_bytes -- is cured by larger caps, not by this.) */
int ma_set_poa_retry(ma_ctx_t* ctx, int on);
/* Of the last call that ran the POA stage, summed over its lanes:
 *   out[0] windows marked for the edge width   out[1] marked for the node capacity only
 *   out[2] windows the retry passes called     out[3] windows left MA_W_VAR_OVERFLOW by them
 * All zero while the setting is off.  Returns the number of entries written. */
int ma_last_poa_retry(ma_ctx_t* ctx, unsigned long long* out, int cap);

/* ---- graph export: the pruned graph every reported component came from ------------------------------------------------ */
/* What the reference draws per component of the reported k attempt with --out-graphs-tgz (cbdg/graph.cpp:216-223,
 * BufferFinalSnapshot): for every window, the components that have a row in comp_* at the reported attempt win_k -- every
 * alive node of the component and every edge stored on those nodes, in the state ComputeComponentComplexity and
 * BuildHaplotypes see (graph.cpp:186-216): after PruneComponent, before and unchanged by the walk search.  comp_cx, comp_cxf,
 * hap_runs and hap_stats are functions of exactly these nodes and edges.
 * NOT exported: components that yielded no walk (the reference draws those as `fully_pruned`; they have no row in comp_*),
 * and attempts that were retried at a larger k -- only the rung that produced the window's result leaves anything.  Windows
 * without a result (win_ncomp == 0) have all four counts 0.  For a window whose win_status carries MA_W_TABLE_OVERFLOW,
 * MA_W_HAP_OVERFLOW or MA_W_LEN_OVERFLOW the export is unspecified beyond staying inside the caps.
 * Node order within a window is deterministic (a component's nodes keep the order of the engine's node arrays, the
 * components of a window interleave) but otherwise unspecified: key nodes by sequence -- the node sequences of a component
 * are distinct.  node_label: bit 0 = REFERENCE, bit 1 = read of a normal (CTRL) sample, bit 2 = read of a tumour (CASE) sample
 * -- the engine's own bits.  A node's sequence is stored in its default orientation; a walk spells a node as stored when it
 * arrives over an edge whose sign on the node's side is PLUS, and reverse complemented otherwise (max_flow.cpp:64-113).
 * The counts always hold the NEED.  If a need exceeds its cap the window gets the matching ma_gstatus bit and none of its
 * rows is defined; a write never passes a cap; re-submit with the reported need.  win_status is never touched by the export.
 * With the export asked for, the call climbs the k ladder rung by rung (what MA_NO_SPEC selects) instead of attempting the
 * last rungs six at a time; the two ladders give the same results.  Single lane, like every stage call. */
enum ma_gstatus { MA_G_NODE_OVERFLOW = 1u << 0, MA_G_EDGE_OVERFLOW = 1u << 1, MA_G_SEQ_OVERFLOW = 1u << 2 };
typedef struct ma_graph_out {
  int32_t max_nodes, max_edges, max_seq_bytes;   /* caller's caps, per window */
  uint32_t* win_gstatus;  /* [n] ma_gstatus */
  uint32_t* win_nnodes;   /* [n] the NEED, also when it exceeds the cap */
  uint32_t* win_nedges;   /* [n] likewise */
  uint32_t* win_nseq;     /* [n] likewise: bytes of node sequence */
  /* per node, stride max_nodes */
  uint32_t* node_comp;    /* component slot c < win_ncomp[w]: the row of comp_* it belongs to */
  uint32_t* node_seq_off; /* into the window's seq_pool */
  uint32_t* node_len;
  uint32_t* node_cnt;     /* [.. * num_samples] per-sample read support (Node::mCounts after merges) */
  uint8_t*  node_sign;    /* 1 = PLUS: sign of the stored (default) sequence */
  uint8_t*  node_label;   /* Label bits as the engine keeps them: bit 0 = REFERENCE */
  uint8_t*  node_flags;   /* bit 0 source anchor, bit 1 sink anchor of its component */
  /* per stored directed edge, stride max_edges (mirror edges both present, as on the nodes); the edges of a node are
   * contiguous, in the node's list order, nodes in slot order */
  uint32_t* edge_src; uint32_t* edge_dst;   /* node slots of this window */
  uint8_t*  edge_kind;    /* 0 ++, 1 +-, 2 -+, 3 --  (source sign, destination sign) */
  uint8_t*  seq_pool;     /* [n * max_seq_bytes] default-orientation sequences, ASCII */
} ma_graph_out_t;
/* ma_assemble_batch + the export.  gx == NULL IS ma_assemble_batch: the same kernels, nothing allocated.  Otherwise every
 * array of gx is required (MA_ERR_ARG) and every cap must be >= 1 (MA_ERR_PARAM).  Both memory spaces: with MA_MEM_DEVICE the
 * arrays of gx are device pointers (the struct itself is always in host memory).  The assembly outputs are byte for byte
 * those of ma_assemble_batch on the same batch.  One more kernel per pass (k_graph_export) writes the rows of the windows
 * that pass reported, from the arrays the clean kernels leave behind. */
int ma_assemble_graph_batch(ma_ctx_t* ctx, const ma_batch_t* b, const ma_asm_out_t* out, const ma_graph_out_t* gx);
/* Windows whose rows the last ma_assemble_graph_batch wrote, by the clean route that reported them:
 *   out[0] small LDS tail image   out[1] large LDS tail image   out[2] HBM tail   out[3] k_clean
 * A window flagged MA_G_* is not counted (only its needs were written).  A window that a capacity retry pass assembles again
 * after an earlier pass had reported it with components counts once per pass that wrote its rows.
 * Returns the number of entries written. */
int ma_last_graph_export(ma_ctx_t* ctx, unsigned long long* out, int cap);

/* ---- probe variants: where in a window's assembly a known allele was lost ---------------------------------------------- */
/* The reference's --probe-variants diagnostic (cbdg/probe_index.{h,cpp}, cbdg/probe_tracker.{h,cpp}, cbdg/
 * probe_results_writer.cpp, core/probe_diagnostics.h) for a batch: every truth allele is followed through four checkpoints --
 * its ALT k-mers in the window's reads, after the first low-coverage pass, in the pruned graph, and in the haplotypes.
 *
 * A PROBE belongs to one window: pos = window-relative 0-based offset of the first REF base (pos < window length), ref_len
 * (pos + ref_len <= window length) and an ALT string; the REF bases are the window's own.  A truth variant that lies in two
 * overlapping windows is two probes.  At most 256 probes per window, ref_len and the ALT at most 256 bases (MA_ERR_PARAM
 * beyond); a probe outside its window is MA_ERR_ARG -- checked on the host with MA_MEM_HOST and by the kernel for device
 * pointers, where the bad probe's row is zeroed, never read out of bounds.  (alt_pool itself cannot be checked on the device:
 * probe_alt_off + probe_alt_len must lie inside it.)
 * k is win_k[w] as the call returns it: the last rung the window attempted.  A window with win_k == 0 has all-zero rows.
 * CONTEXTS (probe_tracker.cpp:62-96, ComputeFlankRange / BuildAltContext): with f = k - 1, a = max(0, pos - f),
 * e = min(len, pos + ref_len + f), the REF context is ref[a:e] and the ALT context ref[a:pos] + ALT + ref[pos + ref_len:e].
 * EQUALITY of k-mers: two k-mers are equal if one equals the other or its reverse complement (the canonical form of
 * DESIGN.md section 2).  A k-mer that holds any byte other than A C G T equals nothing, is never ALT-unique and never
 * counted -- a stated deviation: the reference hashes such k-mers (kmer.cpp:17-28).  Equality is decided on the letters.
 * ALT-UNIQUE k-mers: the k-mers of the ALT context, in order, that equal no k-mer of the REF context (probe_tracker.cpp:
 * 99-121, :273-285); offset j = 0, 1, ... numbers them in context order, and n_alt is their number.  A k-mer that occurs at two
 * offsets counts at both, as the reference's two tags on one node do.  Stated deviation in the numbering: the reference
 * numbers only the ALT-unique k-mers that are in the graph at build time (GenerateAndTag, :279-283); this call numbers all of
 * them, so that "edge" means the true first and last ALT-unique k-mer.
 * A PROFILE of a set of surviving offsets (CountSurvivingKmers, probe_tracker.cpp:602-654) is four numbers: count; edge =
 * survivors at offset 0 or n_alt - 1; interior = the rest; gaps = adjacent survivors whose offsets differ by more than 1. */
typedef struct ma_probes {
  const uint32_t* probe_win_off;  /* [n_windows + 1]: window w owns probes [probe_win_off[w], probe_win_off[w + 1]) */
  const uint32_t* probe_pos;      /* per probe */
  const uint32_t* probe_ref_len;
  const uint32_t* probe_alt_off;  /* into alt_pool */
  const uint32_t* probe_alt_len;
  const uint8_t* alt_pool;        /* ASCII */
} ma_probes_t;
/* All arrays are indexed by probe and all are required.  Rows of windows with win_k == 0 are zero.
 *   pb_k         the k the row was computed at
 *   pb_alt_kmers n_alt
 *   pb_in_reads  [0] occurrences of ALT-unique k-mers over ALL reads of the window, whatever their flags, per occurrence and
 *                per offset (CountInReads, probe_tracker.cpp:299-330); [1] the reads that hold at least one
 *   pb_lowcov1   the profile over the raw graph after BuildGraph and RemoveLowCovNodes(0), window-wide: the reference's
 *                pruned_at_lowcov1 with its component-0 sentinel -- what the build pass hands to the clean pass
 *   pb_final     per component that has a row in comp_*: the profile over the alive nodes of the component in the state
 *                ma_graph_out_t shows -- the reference's pruned_at_tips.  A k-mer survives iff it occurs in the sequence of an
 *                alive node of that component: merges lose nothing, removals lose whole nodes
 *   pb_hap_mask  per component row: bit h is set iff haplotype h of the component (0 = REF) contains the ALT context as a
 *                substring, forward only, byte for byte (CheckPaths, probe_tracker.cpp:472-496)
 * Rows are those of the last pass that attempted the window: a window that a capacity retry pass assembles again has its rows
 * cleared first, as the graph export does.  For a window the call leaves MA_W_TABLE_OVERFLOW pb_lowcov1 and pb_final are
 * unspecified, as the graph export is: the capacity may have run out in the build pass (no complete raw graph: zeros) or in
 * the walk search, after some components were reported and others not.
 * NOT produced: counts inside the fused clean kernels (the second low-coverage pass, the compression
 * stages) and before the first low-coverage pass, one record per rung, the anchor / cycle / complexity flags, the MSA and
 * genotyper attribution, the chained and multi-lane calls. */
typedef struct ma_probe_out {
  uint32_t* pb_k;          /* [n_probes] */
  uint32_t* pb_alt_kmers;  /* [n_probes] */
  uint32_t* pb_in_reads;   /* [n_probes * 2] */
  uint32_t* pb_lowcov1;    /* [n_probes * 4] count, edge, interior, gaps */
  uint32_t* pb_final;      /* [n_probes * max_comps * 4] */
  uint32_t* pb_hap_mask;   /* [n_probes * max_comps] */
} ma_probe_out_t;
/* ma_assemble_batch + one row per probe.  probes == NULL or probe_out == NULL IS ma_assemble_batch: the same kernels, nothing
 * allocated.  Otherwise every array of both structs is required, and so are win_k, win_ncomp, comp_hap0, comp_nhaps, hap_len
 * and hap_bases of `out` (MA_ERR_ARG).  Both memory spaces: with MA_MEM_DEVICE the arrays of both structs are device pointers
 * (the structs themselves are always in host memory).  The assembly outputs are byte for byte those of ma_assemble_batch on
 * the same batch.  Like ma_assemble_graph_batch the call climbs the k ladder rung by rung and takes the clean kernels that
 * leave marks; three kernels of its own do the matching (probe.hip): k_probe_raw between the build and the clean pass of
 * every attempt, k_probe_nodes where k_graph_export runs, k_probe_reads once at the end.  Single lane, like every stage call.
 * After an error return the probe rows are unspecified (bad probes' rows are zero). */
int ma_assemble_probe_batch(ma_ctx_t* ctx, const ma_batch_t* b, const ma_asm_out_t* out, const ma_probes_t* probes,
                            const ma_probe_out_t* probe_out);

/* ---- POA export: the SPOA graph and the MSA rows of every component --------------------------------------------------- */
/* What the reference writes per component with --out-graphs-tgz beside the DOT file (core/variant_builder.cpp:47-70,
 * caller/msa_builder.cpp:44-102): msa__<region>__c<i>.gfa -- one segment per POA node, one link per edge, one path per
 * haplotype -- and msa__<region>__c<i>.fasta, the rows of spoa::Graph::GenerateMultipleSequenceAlignment.  Exported is the
 * graph the variants of ma_var_out_t were read from: after the component's last haplotype, in the state the bubble walk sees.
 * The counts always hold the NEED.  If a need exceeds its cap the window gets the matching ma_pstatus bit and none of its
 * rows is defined; a write never passes a cap; re-submit with the reported need.  All counts and win_pstatus are 0 for the
 * windows the stage skips (win_ncomp == 0, MA_W_NO_HAPLOTYPE, MA_W_LEN_OVERFLOW).  For a window this call leaves
 * MA_W_VAR_OVERFLOW the export only promises to stay inside the caps.  With ma_set_poa_retry a retried window's rows are
 * those of the retry pass that called it (its first pass's counts are cleared first).  A component that holds an empty
 * haplotype is undefined (SPOA gives an empty sequence no label).  NOT exported: edge weights (the engine does not keep
 * them, the GFA does not print them) and SPOA's consensus.  win_status is never touched by the export. */
enum ma_pstatus { MA_P_NODE_OVERFLOW = 1u << 0, MA_P_EDGE_OVERFLOW = 1u << 1, MA_P_COL_OVERFLOW = 1u << 2 };
typedef struct ma_poa_out {
  int32_t max_pnodes, max_pedges;  /* caller's caps per window, summed over the window's components */
  int32_t max_cols;                /* cap per component: MSA columns; also the stride of one haplotype's row */
  uint32_t* win_pstatus;           /* [n] ma_pstatus */
  uint32_t* win_npnodes;           /* [n] the NEED, also beyond the cap */
  uint32_t* win_npedges;           /* [n] likewise */
  uint32_t* win_ncols;             /* [n] likewise: the most columns of any component */
  /* per component, [n * max_comps] */
  uint32_t *comp_pnode0, *comp_npnodes, *comp_pedge0, *comp_npedges, *comp_ncols;
  /* per POA node, stride max_pnodes.  A component's nodes are contiguous from comp_pnode0, in spoa's id order:
     Node::id = slot - comp_pnode0 */
  uint8_t*  pnode_base;            /* decoder(code): the ASCII letter */
  uint32_t* pnode_rank;            /* index in Graph::rank_to_node() */
  uint32_t* pnode_col;             /* MSA column */
  uint32_t* pnode_haps;            /* bit h: the path of the component's h-th haplotype (0 = REF) holds the node */
  /* per out-edge, stride max_pedges.  A node's out-edges are contiguous in Node::outedges order, nodes in id order,
     components in order from comp_pedge0 */
  uint32_t *pedge_tail, *pedge_head;  /* component-local ids */
  uint32_t* pedge_haps;               /* Edge::labels as a mask */
  /* per haplotype slot, [n * max_haps] */
  uint32_t* hap_first;             /* Graph::sequences()[h]: component-local id of the path's first node */
  uint8_t*  msa;                   /* [n * max_haps * max_cols]: row of slot comp_hap0 + h, comp_ncols bytes, '-' = gap */
} ma_poa_out_t;
/* ma_msa_batch + the export.  px == NULL IS ma_msa_batch: the same kernels, nothing allocated.  Otherwise every array of px
 * is required (MA_ERR_ARG) and every cap must be >= 1 (MA_ERR_PARAM).  Both memory spaces: with MA_MEM_DEVICE the arrays of
 * px are device pointers (the struct itself is always in host memory).  The ma_var_out_t arrays and win_status are byte for
 * byte those of ma_msa_batch on the same input.  An exporting call runs every pass as host-counted rounds (what
 * MA_POA_SCHED=0 selects) with kernels of its own; single lane, like every stage call. */
int ma_msa_graph_batch(ma_ctx_t* ctx, const ma_batch_t* b, const ma_asm_out_t* asmb, const ma_var_out_t* out, const ma_poa_out_t* px);
/* Windows the last ma_msa_graph_batch ran to their end with the export, per kind of pass:
 *   out[0] first pass (16-bit labels)   out[1] LAB32 pass   out[2] width retry   out[3] capacity retry
 * A retried window counts in its first pass and in its retry pass.  All zero after a call with px == NULL.
 * Returns the number of entries written. */
int ma_last_poa_export(ma_ctx_t* ctx, unsigned long long* out, int cap);

/* ---- raw BAM records in, a batch's read arrays out ------------------------------------------------------------------------ */
/* What the host shell's ReadCollector::CollectFlat does after the kept set of a window is chosen -- the collector's sort
 * (core/read_collector.cpp:42-53), name interning, the CIGAR-derived flags and hints, the copy of every read's sequence and
 * quality bytes into the batch layout -- on the device, from the bytes of the BAM alignment records as they sit in an inflated
 * BGZF block.  The caller picks which records belong to which window (filters, coverage cap: its business) and lists them in
 * arrival order; a record that falls into two windows is uploaded once and listed twice.  Nothing is dropped: read_win_off of
 * the resulting batch IS rec_win_off, and n_reads is n_records.
 * A RECORD is addressed by the offset of its refID field (the byte behind block_size, SAM specification 4.2) and the number of
 * bytes available from there; these must hold the record's core -- 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq --
 * the tags may be cut off.  Records sit at any alignment, in any order, with anything between them.  A read's name is the
 * l_read_name - 1 bytes in front of the terminating NUL.
 * ORDER within a window, ascending by, in turn: mapq >= 20 first; sample_rank of the record's sample; the name's bytes as
 * unsigned chars (a proper prefix sorts first); the mapped chrom index (ref_map[rec_sample * n_refs + refID], the refID itself
 * with ref_map == NULL, -1 for a refID outside [0, n_refs)); pos; arrival.
 * OUTPUTS, per read in that order:
 *   read_src       the position in rec_off of the record the read is
 *   read_qname_id  the number of distinct names in front of the name's first appearance in the window's order; two reads share
 *                  an id iff their names are equal byte for byte (a hash proposes, the bytes decide)
 *   read_sample    sample_index of the record's sample
 *   read_flags     MA_RF_PASS (mapq >= 20) | MA_RF_CASE (sample_case) | MA_RF_REV (flag 0x10)
 *   read_hint      pos - win_start0[w] - (length of the FIRST CIGAR operation if it is S, else 0); MA_NO_HINT when the mapped
 *                  chrom is not win_chrom[w] or the value is not inside (INT32_MIN, INT32_MAX)
 *   read_mapq      mapq          read_isize  tlen          read_start  max(0, pos)
 *   read_mflags    MA_RM_SOFTCLIP iff (double)(bases of all S operations) / (double)l_seq >= 0.06, | MA_RM_PROPER (flag 0x2)
 *   read_off       the running sum of l_seq; *n_bases = read_off[n_records]
 *   bases4         the record's (l_seq + 1) / 2 sequence bytes as they are, at byte (read_off[r] + r) >> 1: ma_packed_reads_t's
 *                  layout with BAM's own codes; the bytes between two reads and behind the last one are zero
 *   read_quals     the record's quality bytes at read_off[r], 0xFF (absent) as 0
 * so that ma_batch_t {read_bases = read_quals = NULL}, ma_packed_reads_t {bases4, read_quals, 8} and ma_read_meta_t built from
 * the same pointers go to ma_process_cx_batch / ma_process_packed_batch unchanged.
 * ERRORS, never silent; after any of them no output but *n_bases (where stated) is defined, and none is written:
 *   MA_ERR_ARG    a record whose core does not fit rec_len, whose rec_off + rec_len passes blob_bytes, with l_seq <= 0 or
 *                 l_read_name == 0, or with rec_sample >= n_samples_in: ma_last_error names the first such position in rec_off.
 *                 No kernel reads outside [blob, blob + blob_bytes), whatever a record claims
 *   MA_ERR_ARG    *n_bases > bases_cap: *n_bases holds the need, re-submit with that capacity
 *   MA_ERR_ARG    rec_win_off does not rise from 0 to n_records
 *   MA_ERR_PARAM  a window of more than MA_FLATTEN_MAX_WINDOW records
 * One 32-byte status block is read back per call; with MA_MEM_DEVICE nothing else crosses the link. */
#define MA_FLATTEN_MAX_WINDOW 16384
typedef struct ma_records {
  int32_t n_windows; int64_t n_records;
  const uint8_t*  blob;         uint64_t blob_bytes;   /* raw BAM alignment records, any alignment, any order, gaps allowed */
  const uint64_t* rec_off;      /* [n_records] offset in blob of the record's refID field (the byte behind block_size) */
  const uint32_t* rec_len;      /* [n_records] bytes of the record available from there (>= its core part; tags may be cut) */
  const uint32_t* rec_win_off;  /* [n_windows + 1]; position in this list = arrival order */
  const uint8_t*  rec_sample;   /* [n_records] index into the three sample tables below */
  int32_t n_samples_in;         /* 1 .. 256 */
  const uint8_t*  sample_index; /* -> read_sample */
  const uint8_t*  sample_case;  /* 1 -> MA_RF_CASE */
  const uint32_t* sample_rank;  /* comparator keys 2+3: order of (tag, sample name), host computed */
  int32_t n_refs; const int32_t* ref_map; /* [n_samples_in * n_refs] BAM refID -> chrom index, NULL = identity; out of range -> -1 */
  const int32_t*  win_chrom;    /* [n_windows] */
  const int64_t*  win_start0;   /* [n_windows] 0-based start of the window on its contig */
} ma_records_t;
typedef struct ma_flat_out {    /* every member required; the ma_batch_t / ma_packed_reads_t (qual_bits 8) / ma_read_meta_t arrays */
  uint64_t bases_cap;           /* caller's capacity of read_quals in bytes; bases4 holds (bases_cap + n_records + 1) / 2 */
  uint64_t* n_bases;            /* [1] the NEED: sum of l_seq */
  uint64_t* read_off;           /* [n_records + 1] */
  uint8_t* bases4; uint8_t* read_quals;
  uint32_t* read_qname_id; uint8_t* read_sample; uint8_t* read_flags; int32_t* read_hint;
  uint8_t* read_mapq; uint8_t* read_mflags; int32_t* read_isize; int32_t* read_start;
  uint32_t* read_src;           /* [n_records] which input record each output read is */
} ma_flat_out_t;
/* Both memory spaces: with MA_MEM_DEVICE every array of both structs is a device pointer (the structs themselves are always in
 * host memory); with MA_MEM_HOST the inputs are uploaded and the outputs downloaded (read_quals and bases4 as far as they were
 * written).  Single lane, like every stage call.  Eight kernels of its own (flatten.hip), which ma_last_kernel_times reports
 * under six names: k_rec_check, k_rec_fields, k_rec_sort and k_rec_sort_large (the two instances of the sort: windows of up
 * to 1024 records and of more), k_rec_scan (three kernels, one name), k_rec_gather; no other call runs them and this call
 * runs no other kernel.  win_start0 must lie inside (-2^62, 2^62): the hint is computed in 64 bits. */
int ma_flatten_records_batch(ma_ctx_t* ctx, const ma_records_t* in, const ma_flat_out_t* out);

/* ---- which records of a window go on: filters, active-region detection, coverage gates ------------------------------------- */
/* What the host shell does per window BEFORE the kept set is known -- MutationAccumulator::CheckAlignment over every record
 * (core/active_region_detector.cpp:85-232), ReadCollector::Filtered and the per-sample sums of SelectKept
 * (core/read_collector.cpp:147-216), the anchor-coverage gate (core/variant_builder.cpp:214-224) -- on the device, from the
 * same record bytes.  `in` is ma_records_t read differently: per window it lists the CANDIDATES, every record the host's
 * ForRegion would visit for that window, for every sample, in arrival order and unfiltered; rec_len covers the auxiliary
 * fields (as far as the caller has them: tags cut off anywhere end the walk there).  sample_index, sample_case, sample_rank,
 * ref_map, win_chrom and win_start0 are not read and may be NULL.
 * RECORD BITS (rec_keep, one byte per candidate):
 *   MA_SK_COLLECT   none of flag 0x200, 0x400, 0x4 is set and mapq >= 20: what ReadCollector::Filtered lets through
 *   MA_SK_ELIGIBLE  none of those three flags is set and mapq != 0: what CheckAlignment looks at
 * EVENTS.  An eligible record adds events to four multisets of 32-bit positions -- mismatches, insertions, deletions,
 * softclips -- kept per (window, sample).  All position arithmetic is modulo 2^32 and starts from (uint32_t)pos.
 *   MD     if pos >= 0 and the auxiliary fields hold an MD field of type Z.  The fields are walked from the end of the core:
 *          two tag bytes, a type byte, then A c C: 1 byte; s S: 2; i I f: 4; Z H: up to and with the NUL; B: a subtype byte, an
 *          int32 count, count elements of 1 (c C), 2 (s S) or 4 (any other subtype) bytes.  The walk ends at an unknown type, a
 *          negative count, a string without NUL, a field that passes rec_len, or with fewer than 3 bytes left.  The LAST MD:Z
 *          found wins.  Its bytes are read in turn: a digit extends the pending number; any other byte first advances the
 *          position by the pending number (none: 0), then looks at qual[position - (uint32_t)pos]: an index >= l_seq, or a
 *          pending number of more than 9 digits, sets MA_S_MD_RANGE on the window and ends this record's MD walk (the host
 *          throws there -- and whether it gets that far depends on the record order); a quality under 20 skips the byte;
 *          otherwise the byte, upper-cased, adds a MISMATCH event at the position if it is A, C, G or T.  So the letters
 *          behind '^' land on one position, the quality index ignores clips and insertions, and absent (0xFF) qualities pass.
 *   CIGAR  a running position advances by the length of every M, D, N, = and X.  AFTER the advance an I adds an INSERTION
 *          event, a D a DELETION event, an X a MISMATCH event (the multiset of the MD mismatches) at the position; an S adds
 *          a SOFTCLIP event at the position reached so far.
 * WINDOW STATE (win_state, one byte per window):
 *   MA_S_ACTIVE        some sample has, in one multiset, a position with two or more events -- the host's early returns only
 *                      skip work once that is known to be so, whatever the record order.  With skip_active_region every window
 *                      is active and no event is looked at: MA_S_MD_RANGE and MA_S_EVENTS are never set then
 *   MA_S_CAPPED        for some sample with reads: reads > ceil(max_sample_cov * win_len / (bases / reads)), in f64 -- the host
 *                      would downsample (a seeded std::shuffle: host business)
 *   MA_S_LOW_COVERAGE  (double)(sum of bases over the samples) / (double)win_len < (double)min_anchor_cov; meaningless when
 *                      the window is capped (the host's sum is taken after the downsampling)
 *   MA_S_MD_RANGE      see MD
 *   MA_S_EVENTS        no position reached two and a (window, sample) held more than MA_SELECT_EVENT_KEYS distinct (multiset,
 *                      position) keys: the kernel's table was full.  (With more keys than that AND a position that reaches
 *                      two, the window is reported MA_S_ACTIVE or MA_S_EVENTS, whichever the kernel met first; either is true
 *                      to the host's answer, since the caller settles an MA_S_EVENTS window itself)
 *   MA_S_LISTED        active, none of CAPPED, MD_RANGE, EVENTS, and not LOW_COVERAGE: the window's MA_SK_COLLECT records are
 *                      in the selected lists.  Every other window has an empty sel_win_off range; for one with any of
 *                      MA_S_HOST_BITS the caller does the selection itself, the others are skipped windows (inactive: not
 *                      MA_S_ACTIVE; else low coverage)
 * reads and bases above are win_sample_reads / win_sample_bases: the count and the sum of l_seq of the window's MA_SK_COLLECT
 * records per sample -- SampleInfo::sampled_reads / sampled_bases of an uncapped window.
 * SELECTED LISTS.  n_selected, sel_win_off and, per selected record in window order and arrival order within the window,
 * sel_off / sel_len / sel_sample (rec_off, rec_len, rec_sample of the candidate) and sel_src (its position in rec_off), so that
 * ma_records_t{n_windows, *n_selected, blob, blob_bytes, sel_off, sel_len, sel_win_off, sel_sample, ... the rest of `in`} goes to
 * ma_flatten_records_batch unchanged.  The four sel_ arrays are sized n_records by the caller.
 * ERRORS, never silent; after any of them no output is defined, and none is written:
 *   MA_ERR_ARG    a record whose core does not fit rec_len, whose rec_off + rec_len passes blob_bytes, with l_seq <= 0 or
 *                 l_read_name == 0, or with rec_sample >= n_samples_in: ma_last_error names the first such position in rec_off.
 *                 No kernel reads outside [blob, blob + blob_bytes), whatever a record claims
 *   MA_ERR_ARG    rec_win_off does not rise from 0 to n_records; a NULL member of `sp` or `out`
 * Both memory spaces like ma_flatten_records_batch; one 32-byte status block is read back per call, with MA_MEM_DEVICE nothing
 * else crosses the link.  Five kernels of its own (select.hip), reported by ma_last_kernel_times as k_sel_check, k_sel_fields,
 * k_sel_window, k_sel_scan, k_sel_gather; no other call runs them and this call runs no other kernel. */
#define MA_SK_COLLECT 1
#define MA_SK_ELIGIBLE 2
#define MA_S_ACTIVE 1
#define MA_S_LOW_COVERAGE 2
#define MA_S_CAPPED 4
#define MA_S_MD_RANGE 8
#define MA_S_EVENTS 16
#define MA_S_LISTED 32
#define MA_S_HOST_BITS (MA_S_CAPPED | MA_S_MD_RANGE | MA_S_EVENTS)
#define MA_SELECT_EVENT_KEYS 8192 /* distinct (multiset, position) keys a (window, sample) may hold */
typedef struct ma_select_params {
  double max_sample_cov;        /* ReadCollector::Params::max_sample_cov */
  uint32_t min_anchor_cov;
  int32_t skip_active_region;   /* != 0: every window is active */
  const uint32_t* win_len;      /* [n_windows] Window::Length() */
} ma_select_params_t;
typedef struct ma_select_out {  /* every member required */
  uint8_t* rec_keep;            /* [n_records] MA_SK_* */
  uint8_t* win_state;           /* [n_windows] MA_S_* */
  uint32_t* win_sample_reads;   /* [n_windows * n_samples_in] */
  uint64_t* win_sample_bases;   /* [n_windows * n_samples_in] */
  uint64_t* n_selected;         /* [1] */
  uint32_t* sel_win_off;        /* [n_windows + 1] */
  uint64_t* sel_off; uint32_t* sel_len; uint8_t* sel_sample; uint32_t* sel_src;  /* [n_records] each, *n_selected written */
} ma_select_out_t;
int ma_select_records_batch(ma_ctx_t* ctx, const ma_records_t* in, const ma_select_params_t* sp, const ma_select_out_t* out);

/* ---- BGZF blocks inflated on the device ------------------------------------------------------------------------------------------ */
/* What the host shell's BgzfFile::Load does a block at a time with zlib, for a list of blocks at once and with the CRC-32 that
 * Load leaves out: the compressed members of a BAM file go up, their payloads stay on the device as one byte array, which is the
 * `blob` of ma_records_t.  A BGZF block is a gzip member (RFC 1952) with an extra subfield that tells its size (SAM specification
 * 4.1); its data is one DEFLATE stream (RFC 1951).
 * INPUT.  Block b is the blk_len[b] bytes of cblob from blk_off[b], which must lie inside cblob: the bytes AVAILABLE for the
 * member, the member itself may be shorter.  Any alignment, any order, gaps, overlaps and repeats are allowed.
 * HEADER RULES (BgzfFile::Load's).  Bytes 0 .. 3 are 1f 8b 08 and a FLG with bit 2 set; XLEN is the 16-bit value at byte 10; the
 * extra field, bytes [12, 12 + XLEN), is a chain of subfields SI1 SI2 SLEN(16 bits) data[SLEN], walked while 4 bytes are left; a
 * subfield that passes the end of the extra field breaks the rule; the last subfield 'B' 'C' with SLEN 2 holds BSIZE, the
 * member's size less one (none: the rule is broken); 12 + XLEN + 8 <= BSIZE + 1 <= blk_len.  blk_len < 20 breaks the rule too.
 * The DEFLATE data are bytes [12 + XLEN, BSIZE + 1 - 8), the trailer is CRC32 then ISIZE, 32 bits each, little endian.
 * BLOCK STATE (blk_state, one byte per block; 0: good, otherwise exactly one of)
 *   MA_Z_HEADER  a header rule is broken                     } the block contributes 0 bytes: blk_raw_off[b + 1] == blk_raw_off[b]
 *   MA_Z_ISIZE   ISIZE > 65536                               }
 *   MA_Z_DATA    the DEFLATE stream is invalid, needs a bit from behind its data bytes, or would write more than ISIZE bytes.
 *                Invalid is what zlib's inflate rejects: block type 3; a stored block with LEN != ~NLEN; more than 286
 *                literal/length or more than 30 distance code lengths; an over-subscribed code-length, literal/length or
 *                distance code; an incomplete one, except a code with no lengths at all (using it is invalid) and, for
 *                literal/length and distance codes, a single code of length 1 (the other bit pattern is invalid); repeat code 16
 *                as the first code length, a repeat that passes the count of lengths; no code for symbol 256; a bit pattern
 *                without a code; literal/length symbols 286, 287 and distance symbols 30, 31 of the fixed code; a distance
 *                greater than the bytes this block has written so far (there is no dictionary and no window across blocks)
 *   MA_Z_SHORT   the last DEFLATE block (BFINAL) ended with fewer than ISIZE bytes written
 *   MA_Z_CRC     ISIZE bytes were written and their CRC-32 is not the trailer's
 * A member with ISIZE 0 is decoded and checked like any other (the 28-byte end-of-file member is good).  Data bytes left over
 * between the end of the last DEFLATE block and the trailer are not an error (zlib's Z_FINISH accepts them, and so does Load).
 * OUTPUT.  blk_raw_off[0] = 0, blk_raw_off[b + 1] = blk_raw_off[b] + (ISIZE of block b, 0 for MA_Z_HEADER and MA_Z_ISIZE);
 * *n_raw = blk_raw_off[n_blocks]; raw[blk_raw_off[b] .. blk_raw_off[b + 1]) is the payload of a good block -- list order, no
 * gaps, so a record that straddles two blocks of the file is contiguous in raw.  A flagged block never fails the call; the
 * bytes of its own range are undefined, nothing outside of it is written.  *n_flagged counts the blocks with a state != 0.
 * ERRORS, never silent; after any of them no output is defined, and none but *n_raw in the second case is written:
 *   MA_ERR_ARG   blk_off[b] + blk_len[b] > cblob_bytes: ma_last_error names the first such block
 *   MA_ERR_ARG   *n_raw > raw_cap: *n_raw holds the need, re-submit with that capacity
 *   MA_ERR_ARG   n_blocks < 0, a NULL member of `in` or `out` (cblob, blk_off, blk_len and raw too, even where empty)
 * Both memory spaces like ma_flatten_records_batch; one 32-byte status block is read back per call, with MA_MEM_DEVICE nothing
 * else crosses the link.  No kernel reads outside [cblob, cblob + cblob_bytes) -- the bit reader's loads are byte loads in front
 * of the member's trailer -- or writes outside the output arrays, whatever a block claims.  Three kernels of its own
 * (inflate.hip), reported by ma_last_kernel_times as k_inf_header, k_inf_scan, k_inf_decode (the last one only with
 * n_blocks > 0); no other call runs them and this call runs no other kernel. */
#define MA_Z_HEADER 1
#define MA_Z_ISIZE 2
#define MA_Z_DATA 4
#define MA_Z_SHORT 8
#define MA_Z_CRC 16
typedef struct ma_bgzf {
  int64_t n_blocks;
  const uint8_t* cblob;         /* BGZF members as they are in the file */
  uint64_t cblob_bytes;
  const uint64_t* blk_off;      /* [n_blocks] offset in cblob of the member's first byte (0x1f) */
  const uint32_t* blk_len;      /* [n_blocks] bytes available from there (>= BSIZE + 1 for a good block) */
} ma_bgzf_t;
typedef struct ma_inflate_out { /* every member required */
  uint64_t raw_cap;             /* caller's capacity of raw in bytes */
  uint8_t* raw;
  uint64_t* blk_raw_off;        /* [n_blocks + 1] */
  uint8_t* blk_state;           /* [n_blocks] MA_Z_* */
  uint64_t* n_raw;              /* [1] */
  uint64_t* n_flagged;          /* [1] */
} ma_inflate_out_t;
int ma_inflate_blocks_batch(ma_ctx_t* ctx, const ma_bgzf_t* in, const ma_inflate_out_t* out);

/* ---- the alignment records in inflated bytes ---------------------------------------------------------------------------------------- */
/* Finds the BAM alignment records (SAM specification 4.2) of byte ranges of `raw` -- the output of ma_inflate_blocks_batch, or
 * any inflated BAM bytes -- so that a host can assign records to windows from 12 bytes per record without seeing the bytes.
 * A STREAM s is walked from str_begin[s], the offset of a record's block_size field: with p the place of that field, the
 * walk goes on while p < str_end[s] (a record that STARTS before str_end belongs to the stream, as with a BAI chunk's end);
 * the record is the block_size bytes from p + 4, the next one's field is at p + 4 + block_size.  The walk ends, with
 * MA_X_BAD_RECORD in str_state[s], at a record
 *   - whose block_size field or whose block_size bytes pass raw_bytes (p + 4 + block_size > raw_bytes),
 *   - with block_size < 32,
 *   - whose core 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq, l_seq read as unsigned, exceeds block_size;
 * the records in front of it are kept, it is not listed itself.  Streams may overlap; a record in two streams is listed twice.
 * OUTPUT.  str_rec_off (exclusive sums of the streams' record counts, n_streams + 1 values), *n_found = the last of them,
 * str_state (0 or MA_X_BAD_RECORD), and per record in stream order, then file order: rec_off (the offset in raw of refID, that
 * is p + 4) and rec_len (block_size) -- exactly what ma_records_t takes with blob = raw -- and rec_ref (refID), rec_pos (pos,
 * 0-based, as stored) and rec_span: the sum of the lengths of the CIGAR operations M, D, N, = and X (codes 0, 2, 3, 7, 8)
 * modulo 2^32.  A CIGAR carried in a CG tag is not looked at (as in ma_flatten_records_batch).
 * ERRORS, never silent; after any of them no output is defined, and none but *n_found in the second case is written:
 *   MA_ERR_ARG   str_begin[s] > str_end[s] or str_end[s] > raw_bytes: ma_last_error names the first such stream
 *   MA_ERR_ARG   *n_found > rec_cap: *n_found holds the need, re-submit with that capacity
 *   MA_ERR_ARG   n_streams < 0, a NULL member of `in` or `out`
 * Both memory spaces; one 32-byte status block is read back per call.  No kernel reads outside [raw, raw + raw_bytes).  Four
 * kernels of its own (inflate.hip): k_idx_count, k_idx_scan, k_idx_fill, k_idx_fields (the first and third only with
 * n_streams > 0, the last only with records found); no other call runs them and this call runs no other kernel. */
#define MA_X_BAD_RECORD 1
typedef struct ma_record_streams {
  const uint8_t* raw;
  uint64_t raw_bytes;
  int64_t n_streams;
  const uint64_t* str_begin;    /* [n_streams] offset in raw of the first record's block_size field */
  const uint64_t* str_end;      /* [n_streams] */
} ma_record_streams_t;
typedef struct ma_index_out {   /* every member required */
  uint64_t rec_cap;             /* caller's capacity of the five rec_ arrays in records */
  uint64_t* n_found;            /* [1] */
  uint64_t* str_rec_off;        /* [n_streams + 1] */
  uint8_t* str_state;           /* [n_streams] MA_X_* */
  uint64_t* rec_off;            /* [rec_cap], *n_found written: as ma_records_t takes it */
  uint32_t* rec_len;
  int32_t* rec_ref;
  int32_t* rec_pos;
  uint32_t* rec_span;
} ma_index_out_t;
int ma_index_records_batch(ma_ctx_t* ctx, const ma_record_streams_t* in, const ma_index_out_t* out);

/* Work counters accumulated over the same region as ma_last_kernel_times (reset by ma_timing_control):
 *   out[0] read x haplotype pairs seen by ma_genotype_batch      out[1] pairs that needed the DP
 *   out[2] windows passed to ma_assemble_batch                   out[3] k attempts x windows assembled
 *   out[4..7] DP pairs by region width: <= 41, <= 65, <= 129 diagonals, wider (any-width kernel)
 *   out[8..13] (timing mode 3 only) distinct k-mers, nodes after the first low-coverage pass, k-mer instances on the
 *              hash-table path, k-mer instances, (k+1)-mers of reads queued for the edge builder, read-support counts
 *              queued -- each summed over the window attempts
 *   out[14..19] (timing mode 3 only) DP cells: [14] cells of the read aligner's DP regions (rows x region width, summed over
 *              the pairs that ran the DP), [15] cells of the POA's banded fills (rows x band columns), [16] banded fills,
 *              [17] cells of the POA's full fills (rows x haplotype length), [18] haplotype <-> graph alignments,
 *              [19] alignments written down in closed form (no fill) -- what bench.py's `gcups` block divides the kernel times by
 * Used by bench.py to price the kernels' algorithmic HBM bytes.  Returns the number of entries written. */
int ma_last_stats(ma_ctx_t* ctx, unsigned long long* out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* MICROASM_H_ */
