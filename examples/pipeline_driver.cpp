// pipeline_driver.cpp -- the `pipeline` host around the engine: reference + alignment files in,
// coordinate-sorted de-duplicated variant records out.  Three stages run side by side, as the reference's AsyncWorker /
// PipelineExecutor do at window granularity (core/async_worker.cpp:47-110, core/pipeline_executor.cpp:174-252):
//   extract   WindowBuilder tiles the regions; per window the skip gates (N-only, max-k repeat, inactive region), the read
//             collector (filters, coverage-capped paired downsampling, comparator) and the coverage gate; the windows that
//             are left are flattened into batches
//   engine    ma_prefetch_batch(next) + ma_process_batch(this): the next batch uploads under this batch's kernels
//             (--out-vcf: ONE call, ma_process_cx_batch -- the chain, the FORMAT statistics and the SEQ_CX / GRAPH_CX annotation)
//             (--packed-reads: the ma_*_packed_batch pair on 4-bit read bases and qualities, half the bytes over the link)
//             (--read-meta with --out-vcf: ma_prefetch_meta_batch, and that call with the reads' MAPQ, clip and pair flags,
//              insert size and start -- RMQ, SCA, FLD, RPCD, MQCD, FSSE are printed too: 24 of 24 FORMAT values)
//             (--out-graphs-dir DIR: debugging -- the batch once more through ma_assemble_graph_batch, one DOT file per component)
//             (--out-msa-dir DIR: debugging -- the batch once more through ma_assemble_batch + ma_msa_graph_batch, a GFA and a
//              FASTA file per component)
//             (--probe-variants FILE --probe-results FILE: debugging -- the batch once more through ma_assemble_probe_batch, the
//              reference's probe_results.tsv with the columns the engine produces)
//   flush    results -> records -> VariantStore (same CHROM+POS+REF from overlapping windows: the better covered call wins)
//             -> everything before the next batch's first window is written, in coordinate order
// Build (no HIP headers needed; zlib only for BAM input):
//   g++ -std=c++17 -O2 examples/pipeline_driver.cpp -Iinclude -Llancet2_amd -lmicroasm -Wl,-rpath,$PWD/lancet2_amd
//       -Wl,--allow-shlib-undefined -DLANCET2_AMD_WITH_ZLIB -lz -lpthread -o pipeline_driver
//   ./pipeline_driver --reference ref.fa --normal n.sam --tumor t.sam --region chr1:1-20000 --out calls.tsv
// Flags follow the reference CLI (cli/cli_interface.cpp:203-303) where the engine has the knob.
#include <malloc.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

#include "../lancet2_amd/host/pipeline_host.hpp"

using namespace lancet2_amd::host;

namespace {

struct Outputs {  // caller-owned fixed-stride result buffers of one batch
  std::vector<uint32_t> u32;
  std::vector<double> f64;
  std::vector<uint8_t> u8;
  std::vector<int32_t> i32;
  ma_gate_out_t gate{};
  ma_asm_out_t asmb{};
  ma_var_out_t vars{};
  ma_geno_out_t geno{};
  ma_cx_out_t cx{};
  std::vector<int32_t> cx_i;
  std::vector<float> cx_f;
  std::vector<double> cx_d;
  ma_fmt_out_t fmt{};  // read-level FORMAT statistics: asked for with --out-vcf only
  std::vector<double> fmt_d;
  ma_fmt_meta_out_t fmeta{};  // RMQ and SCA / FLD / RPCD / MQCD / FSSE: asked for with --out-vcf --read-meta only
  std::vector<double> fmeta_d;
  void Allocate(const ma_params_t& p, int n, bool with_stats, bool with_meta = false) {
    size_t const N = n, MC = p.max_comps, MH = p.max_haps, ML = p.max_hap_len, MR = p.max_runs, MV = p.max_vars, MA = p.max_alts,
                 MP = p.max_allele_bytes, S = p.num_samples;
    size_t const G = (MA + 1) * (MA + 2) / 2;
    u32.assign(2 * N + 3 * N + 6 * N * MC + 2 * N * MH + 2 * N * MH * MR + N + 6 * N * MV + 2 * N * MV * MA + N * MV * MH +
                   N * MV * S * (MA + 1) * 2 + N * MV * S * G + N * MV * S + 64, 0);
    cx_i.assign(4 * N * MV, 0);
    cx_f.assign(4 * N * MV, 0.f);
    cx_d.assign(6 * N * MV, 0.0);
    cx.seq_cx_i = cx_i.data(); cx.seq_cx_f = cx_f.data(); cx.seq_cx_d = cx_d.data(); cx.graph_cx = cx_d.data() + 3 * N * MV;
    f64.assign(4 * N * MC + 6 * N * MH + N * MV, 0.0);
    u8.assign(N * MH * ML + N * MV * MH + N * MP, 0);
    i32.assign(2 * N * MV * MA, 0);
    uint32_t* u = u32.data();
    double* d = f64.data();
    uint8_t* b = u8.data();
    int32_t* s = i32.data();
    auto tu = [&](size_t c) { uint32_t* r = u; u += c; return r; };
    auto td = [&](size_t c) { double* r = d; d += c; return r; };
    auto tb = [&](size_t c) { uint8_t* r = b; b += c; return r; };
    auto ti = [&](size_t c) { int32_t* r = s; s += c; return r; };
    gate.max_approx = tu(N); gate.max_exact = tu(N);
    asmb.win_status = tu(N); asmb.win_k = tu(N); asmb.win_ncomp = tu(N);
    asmb.comp_anchor = tu(N * MC); asmb.comp_hap0 = tu(N * MC); asmb.comp_nhaps = tu(N * MC);
    asmb.comp_cx = tu(3 * N * MC); asmb.comp_cxf = td(4 * N * MC);
    asmb.hap_len = tu(N * MH); asmb.hap_nruns = tu(N * MH); asmb.hap_stats = td(6 * N * MH);
    asmb.hap_bases = tb(N * MH * ML); asmb.hap_runs = tu(2 * N * MH * MR);
    vars.win_nvars = tu(N); vars.var_comp = tu(N * MV); vars.var_pos = tu(N * MV); vars.var_ref_start = tu(N * MV);
    vars.var_ref_off = tu(N * MV); vars.var_ref_len = tu(N * MV); vars.var_nalts = tu(N * MV);
    vars.alt_off = tu(N * MV * MA); vars.alt_len = tu(N * MV * MA); vars.alt_type = ti(N * MV * MA);
    vars.alt_length = ti(N * MV * MA); vars.var_hap_allele = tb(N * MV * MH); vars.var_hap_start = tu(N * MV * MH);
    vars.allele_pool = tb(N * MP);
    geno.allele_counts = tu(N * MV * S * (MA + 1) * 2); geno.var_qual = td(N * MV);
    geno.var_pl = tu(N * MV * S * G); geno.var_gq = tu(N * MV * S);  // FORMAT PL / GQ (and GT = the smallest PL)
    if (with_stats) {  // FORMAT NPBQ, CMLOD and BQCD / ASMD / AHDD / HSE (ev_sums is not needed for the VCF)
      fmt_d.assign(N * MV * S * ((MA + 1) + MA + 4), 0.0);
      fmt.fmt_npbq = fmt_d.data();
      fmt.fmt_cmlod = fmt.fmt_npbq + N * MV * S * (MA + 1);
      fmt.fmt_stat = fmt.fmt_cmlod + N * MV * S * MA;
    }
    if (with_meta) {  // (the integer tallies ev_meta / ev_rpcd are not needed for the VCF)
      fmeta_d.assign(N * MV * S * ((MA + 1) + 5), 0.0);
      fmeta.fmt_rmq = fmeta_d.data();
      fmeta.fmt_mstat = fmeta.fmt_rmq + N * MV * S * (MA + 1);
    }
  }
};

template <class T>
class Channel {  // bounded hand-over between two stages
 public:
  explicit Channel(size_t cap) : cap_(cap) {}
  void Push(T v) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return q_.size() < cap_; });
    q_.push_back(std::move(v));
    cv_.notify_all();
  }
  void Close() {
    std::lock_guard<std::mutex> lk(mu_);
    closed_ = true;
    cv_.notify_all();
  }
  bool Pop(T* out) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return !q_.empty() || closed_; });
    if (q_.empty()) return false;
    *out = std::move(q_.front());
    q_.pop_front();
    cv_.notify_all();
    return true;
  }
  bool Peek(T** out) {  // the element a later Pop will return, once there is one (or the channel is closed and empty)
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return !q_.empty() || closed_; });
    if (q_.empty()) return false;
    *out = &q_.front();
    return true;
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<T> q_;
  size_t cap_;
  bool closed_ = false;
};

constexpr int kHostRouteFailed = -1000;  // Job::rc of a batch whose handed-back window could not be collected (no ma_error)
struct Job {
  std::unique_ptr<FlatBatch> batch;
  std::unique_ptr<Outputs> out;
  // --device-select: the windows ma_select_records_batch handed back (MA_S_HOST_BITS), collected by the host route and run as
  // one-window batches of their own
  std::vector<std::pair<std::unique_ptr<FlatBatch>, std::unique_ptr<Outputs>>> host_windows;
  int rc = MA_OK;
  std::string err;
};

void DumpBatch(const std::string& dir, FlatBatch const& fb) {
  auto put = [&](const char* name, const void* p, size_t bytes) {
    FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
    if (!f) { std::perror(name); std::exit(4); }
    std::fwrite(p, 1, bytes, f);
    std::fclose(f);
  };
  put("ref_bases.u8", fb.ref_bases.data(), fb.ref_bases.size());
  put("ref_off.u32", fb.ref_off.data(), 4 * fb.ref_off.size());
  if (fb.raw_mode) {  // --raw-records: the arrays of ma_records_t (include/microasm.h) beside the window list; no read arrays yet
    ma_records_t const& r = fb.records;
    size_t const n = static_cast<size_t>(r.n_records), nw = static_cast<size_t>(r.n_windows), ns = static_cast<size_t>(r.n_samples_in);
    int32_t const counts[2] = {r.n_samples_in, r.n_refs};
    put("blob.u8", r.blob, static_cast<size_t>(r.blob_bytes));
    put("rec_off.u64", r.rec_off, 8 * n);
    put("rec_len.u32", r.rec_len, 4 * n);
    put("rec_win_off.u32", r.rec_win_off, 4 * (nw + 1));
    put("rec_sample.u8", r.rec_sample, n);
    put("sample_index.u8", r.sample_index, ns);
    put("sample_case.u8", r.sample_case, ns);
    put("sample_rank.u32", r.sample_rank, 4 * ns);
    put("ref_map.i32", r.ref_map, 4 * ns * static_cast<size_t>(r.n_refs));
    put("counts.i32", counts, sizeof counts);  // n_samples_in, n_refs
    put("win_chrom.i32", r.win_chrom, 4 * nw);
    put("win_start0.i64", r.win_start0, 8 * nw);
  } else {
    put("read_win_off.u32", fb.read_win_off.data(), 4 * fb.read_win_off.size());
    put("read_off.u64", fb.read_off.data(), 8 * fb.read_off.size());
    put("read_bases.u8", fb.read_bases.data(), fb.read_bases.size());
    put("read_quals.u8", fb.read_quals.data(), fb.read_quals.size());
    if (fb.packed_mode) put("bases4.u8", fb.bases4.data(), fb.bases4.size());  // (--packed-reads: read_bases.u8 is the pad alone)
    put("read_qname_id.u32", fb.read_qname_id.data(), 4 * fb.read_qname_id.size());
    put("read_sample.u8", fb.read_sample.data(), fb.read_sample.size());
    put("read_flags.u8", fb.read_flags.data(), fb.read_flags.size());
    put("read_hint.i32", fb.read_hint.data(), 4 * fb.read_hint.size());
    put("read_mapq.u8", fb.read_mapq.data(), fb.read_mapq.size());  // the read metadata of ma_read_meta_t
    put("read_mflags.u8", fb.read_mflags.data(), fb.read_mflags.size());
    put("read_isize.i32", fb.read_isize.data(), 4 * fb.read_isize.size());
    put("read_start.i32", fb.read_start.data(), 4 * fb.read_start.size());
  }
  std::vector<uint64_t> wins;
  for (auto const& w : fb.windows) {
    wins.push_back(static_cast<uint64_t>(w.chrom));
    wins.push_back(w.start1);
    wins.push_back(w.end1);
    wins.push_back(w.genome_index);
  }
  put("windows.u64", wins.data(), 8 * wins.size());
}

// --out-graphs-dir: the batch once more through ma_assemble_graph_batch, one DOT file per exported component.  The caps start
// at the binding's defaults; windows that come back flagged (MA_G_*) are re-submitted once -- the batch again, with the
// largest reported needs as caps; a component that still has no graph then is named on stderr.  The arrays are sized
// batch windows x caps on the host and again in the engine's staging: 62 KB per window at the first caps (1 GB at
// --batch-windows 16384), more on a re-submission -- a debugging mode, run it on the regions in question with batches of a few
// hundred windows.  Returns the number of files written, -1 when a call failed.
struct GraphArrays {
  std::vector<uint32_t> u32;
  std::vector<uint8_t> u8;
  ma_graph_out_t g{};
  void Allocate(const ma_params_t& p, int n, int32_t mn, int32_t me, int32_t ms) {
    size_t const N = n, S = p.num_samples, MN = mn, ME = me, MS = ms;
    u32.assign(4 * N + 3 * N * MN + N * MN * S + 2 * N * ME, 0);
    u8.assign(3 * N * MN + N * ME + N * MS, 0);
    uint32_t* u = u32.data();
    uint8_t* b = u8.data();
    auto tu = [&](size_t c) { uint32_t* r = u; u += c; return r; };
    auto tb = [&](size_t c) { uint8_t* r = b; b += c; return r; };
    g.max_nodes = mn; g.max_edges = me; g.max_seq_bytes = ms;
    g.win_gstatus = tu(N); g.win_nnodes = tu(N); g.win_nedges = tu(N); g.win_nseq = tu(N);
    g.node_comp = tu(N * MN); g.node_seq_off = tu(N * MN); g.node_len = tu(N * MN); g.node_cnt = tu(N * MN * S);
    g.node_sign = tb(N * MN); g.node_label = tb(N * MN); g.node_flags = tb(N * MN);
    g.edge_src = tu(N * ME); g.edge_dst = tu(N * ME); g.edge_kind = tb(N * ME);
    g.seq_pool = tb(N * MS);
  }
};

long WriteGraphs(ma_ctx_t* ctx, const ma_params_t& prm, Reference const& ref, FlatBatch const& fb, std::string const& dir) {
  int const n = fb.view.n_windows;
  Outputs o;
  o.Allocate(prm, n, false);
  GraphArrays ga;
  int32_t caps[3] = {512, 2048, 32768};
  for (int attempt = 0; attempt < 2; ++attempt) {
    ga.Allocate(prm, n, caps[0], caps[1], caps[2]);
    if (ma_assemble_graph_batch(ctx, &fb.view, &o.asmb, &ga.g) != MA_OK) return -1;
    bool flagged = false;
    for (int w = 0; w < n; ++w) {
      flagged = flagged || ga.g.win_gstatus[w] != 0;
      caps[0] = std::max<int32_t>(caps[0], static_cast<int32_t>(ga.g.win_nnodes[w]));
      caps[1] = std::max<int32_t>(caps[1], static_cast<int32_t>(ga.g.win_nedges[w]));
      caps[2] = std::max<int32_t>(caps[2], static_cast<int32_t>(ga.g.win_nseq[w]));
    }
    if (!flagged) break;
  }
  long written = 0;
  for (int w = 0; w < n; ++w) {
    auto const& win = fb.windows[static_cast<size_t>(w)];
    for (uint32_t c = 0; c < o.asmb.win_ncomp[w]; ++c) {
      std::string const name = ref.chroms[static_cast<size_t>(win.chrom)].name + "_" + std::to_string(win.start1) + "_" + std::to_string(win.end1) +
                               "__c" + std::to_string(c) + "__k" + std::to_string(o.asmb.win_k[w]);
      std::string const dot = RenderComponentDot(prm, o.asmb, ga.g, w, c, o.asmb.win_k[w], name);
      if (dot.empty()) {  // still flagged after the re-submission (the needs are the batch's largest: not expected), or no node
        std::fprintf(stderr, "pipeline_driver: --out-graphs-dir: no graph for %s (export status %u: needs %u nodes, %u edges, %u bases)\n",
                     name.c_str(), ga.g.win_gstatus[w], ga.g.win_nnodes[w], ga.g.win_nedges[w], ga.g.win_nseq[w]);
        continue;
      }
      FILE* f = std::fopen((dir + "/" + name + ".dot").c_str(), "w");
      if (!f) { std::perror("--out-graphs-dir"); return -1; }
      std::fputs(dot.c_str(), f);
      std::fclose(f);
      ++written;
    }
  }
  return written;
}

// --out-msa-dir: the batch once more through ma_assemble_batch + ma_msa_graph_batch; per component of every assembled window
// msa__<chrom>_<start>_<end>__c<comp>.gfa (the SPOA graph) and .fasta (the MSA rows), as the reference names and prints them
// with --out-graphs-tgz.  Windows that come back flagged (MA_P_*) are re-submitted once -- the batch again, with the largest
// reported needs as caps.  Returns the number of files written, -1 when a call failed.
struct PoaArrays {
  std::vector<uint32_t> u32;
  std::vector<uint8_t> u8;
  ma_poa_out_t x{};
  void Allocate(const ma_params_t& p, int n, int32_t mn, int32_t me, int32_t mx) {
    size_t const N = n, MC = p.max_comps, MH = p.max_haps, MN = mn, ME = me, MX = mx;
    u32.assign(4 * N + 5 * N * MC + 3 * N * MN + 3 * N * ME + N * MH, 0);
    u8.assign(N * MN + N * MH * MX, 0);
    uint32_t* u = u32.data();
    uint8_t* b = u8.data();
    auto tu = [&](size_t c) { uint32_t* r = u; u += c; return r; };
    auto tb = [&](size_t c) { uint8_t* r = b; b += c; return r; };
    x.max_pnodes = mn; x.max_pedges = me; x.max_cols = mx;
    x.win_pstatus = tu(N); x.win_npnodes = tu(N); x.win_npedges = tu(N); x.win_ncols = tu(N);
    x.comp_pnode0 = tu(N * MC); x.comp_npnodes = tu(N * MC); x.comp_pedge0 = tu(N * MC); x.comp_npedges = tu(N * MC);
    x.comp_ncols = tu(N * MC);
    x.pnode_base = tb(N * MN); x.pnode_rank = tu(N * MN); x.pnode_col = tu(N * MN); x.pnode_haps = tu(N * MN);
    x.pedge_tail = tu(N * ME); x.pedge_head = tu(N * ME); x.pedge_haps = tu(N * ME);
    x.hap_first = tu(N * MH); x.msa = tb(N * MH * MX);
  }
};

long WriteMsaFiles(ma_ctx_t* ctx, const ma_params_t& prm, Reference const& ref, FlatBatch const& fb, std::string const& dir) {
  int const n = fb.view.n_windows;
  Outputs o;
  PoaArrays pa;
  int32_t caps[3] = {2048, 4096, 2048};
  for (int attempt = 0; attempt < 2; ++attempt) {
    o.Allocate(prm, n, false);
    pa.Allocate(prm, n, caps[0], caps[1], caps[2]);
    if (ma_assemble_batch(ctx, &fb.view, &o.asmb) != MA_OK) return -1;
    if (ma_msa_graph_batch(ctx, &fb.view, &o.asmb, &o.vars, &pa.x) != MA_OK) return -1;
    bool flagged = false;
    for (int w = 0; w < n; ++w) {
      flagged = flagged || pa.x.win_pstatus[w] != 0;
      caps[0] = std::max<int32_t>(caps[0], static_cast<int32_t>(pa.x.win_npnodes[w]));
      caps[1] = std::max<int32_t>(caps[1], static_cast<int32_t>(pa.x.win_npedges[w]));
      caps[2] = std::max<int32_t>(caps[2], static_cast<int32_t>(pa.x.win_ncols[w]));
    }
    if (!flagged) break;
  }
  long written = 0;
  for (int w = 0; w < n; ++w) {
    auto const& win = fb.windows[static_cast<size_t>(w)];
    for (uint32_t c = 0; c < o.asmb.win_ncomp[w]; ++c) {
      std::string const name = "msa__" + ref.chroms[static_cast<size_t>(win.chrom)].name + "_" + std::to_string(win.start1) + "_" +
                               std::to_string(win.end1) + "__c" + std::to_string(c);
      std::string const texts[2] = {RenderComponentGfa(prm, o.asmb, pa.x, w, c), RenderComponentFasta(prm, o.asmb, pa.x, w, c)};
      if (texts[0].empty()) {  // a window the POA stage left out or capped, or one still flagged after the re-submission
        std::fprintf(stderr, "pipeline_driver: --out-msa-dir: no MSA for %s (window status %u, export status %u: needs %u nodes, %u edges, %u columns)\n",
                     name.c_str(), o.asmb.win_status[w], pa.x.win_pstatus[w], pa.x.win_npnodes[w], pa.x.win_npedges[w], pa.x.win_ncols[w]);
        continue;
      }
      for (int k = 0; k < 2; ++k) {
        FILE* f = std::fopen((dir + "/" + name + (k ? ".fasta" : ".gfa")).c_str(), "w");
        if (!f) { std::perror("--out-msa-dir"); return -1; }
        std::fputs(texts[k].c_str(), f);
        std::fclose(f);
        ++written;
      }
    }
  }
  return written;
}

// --probe-variants / --probe-results: the batch once more through ma_assemble_probe_batch with the truth variants whose start
// lies in one of its windows; the lines of lancet2_amd::host::RenderProbeLines go to `out`.  Returns the number of lines
// written, -1 when the call failed.
long WriteProbeResults(ma_ctx_t* ctx, const ma_params_t& prm, Reference const& ref, FlatBatch const& fb,
                       std::vector<ProbeVariant> const& variants, FILE* out, size_t* skipped) {
  int const n = fb.view.n_windows;
  ProbeBatch const pb = ActivateProbes(variants, fb.windows, [&](int chrom) -> std::string const& { return ref.chroms[static_cast<size_t>(chrom)].name; });
  *skipped += pb.skipped;
  size_t const np = pb.id.size(), MC = static_cast<size_t>(prm.max_comps);
  if (np == 0) return 0;
  Outputs o;
  o.Allocate(prm, n, false);
  std::vector<uint32_t> rows(np * (8 + 5 * MC), 0);
  ma_probe_out_t po{};
  po.pb_k = rows.data(); po.pb_alt_kmers = po.pb_k + np; po.pb_in_reads = po.pb_alt_kmers + np; po.pb_lowcov1 = po.pb_in_reads + 2 * np;
  po.pb_final = po.pb_lowcov1 + 4 * np; po.pb_hap_mask = po.pb_final + 4 * MC * np;
  ma_probes_t const pv = pb.View();
  if (ma_assemble_probe_batch(ctx, &fb.view, &o.asmb, &pv, &po) != MA_OK) return -1;
  long written = 0;
  for (int w = 0; w < n; ++w) {
    auto const& win = fb.windows[static_cast<size_t>(w)];
    std::string const region = ref.chroms[static_cast<size_t>(win.chrom)].name + ":" + std::to_string(win.start1) + "-" + std::to_string(win.end1);
    for (uint32_t i = pb.win_off[static_cast<size_t>(w)]; i < pb.win_off[static_cast<size_t>(w) + 1]; ++i) {
      std::string const lines = RenderProbeLines(prm, o.asmb, po, i, w, pb.id[i], variants[pb.id[i]], region);
      std::fputs(lines.c_str(), out);
      written += static_cast<long>(std::count(lines.begin(), lines.end(), '\n'));
    }
  }
  return written;
}

AlignmentSource LoadAlignments(const std::string& path, Reference const& ref, bool keep_packed, bool keep_raw, bool keep_tags = false) {
  bool const bam = path.size() > 4 && path.substr(path.size() - 4) == ".bam";
#ifdef LANCET2_AMD_WITH_ZLIB
  if (bam) {
    // a .bai next to the file: region-indexed access (only the blocks of the regions asked for are read and inflated);
    // without one the whole file is read once
    for (std::string const& bai : {path + ".bai", path.substr(0, path.size() - 4) + ".bai"}) {
      std::ifstream probe(bai, std::ios::binary);
      if (probe && !getenv("PIPELINE_NO_INDEX")) return AlignmentSource::OpenIndexedBam(path, bai, ref, keep_packed, keep_raw, keep_tags);
    }
    return AlignmentSource::LoadBam(path, ref, keep_packed, keep_raw, keep_tags);
  }
#else
  if (bam) throw std::runtime_error("built without zlib (-DLANCET2_AMD_WITH_ZLIB -lz): BAM input is not available");
#endif
  return AlignmentSource::LoadSam(path, ref);
}

}  // namespace

int main(int argc, char** argv) {
  // The extract stage allocates a window's flat arrays (100-200 KB each) on its collector threads and frees them on the batching
  // thread.  glibc serves blocks of that size with mmap / munmap -- a system call, fresh page faults and the process-wide
  // address-space lock per array, which is what kept eight collectors from being faster than one.  From the heap arenas
  // (one per thread) the same blocks are recycled without leaving user space.  (The reference links mimalloc for the same reason.)
  // (64-bit glibc caps M_MMAP_THRESHOLD at HEAP_MAX_SIZE / 2 = 32 MiB and REJECTS anything larger, leaving the 128 KiB default
  //  in force -- ADVICE r5; the flat arrays are far below 32 MiB)
  if (mallopt(M_MMAP_THRESHOLD, 32 << 20) != 1 || mallopt(M_TRIM_THRESHOLD, 1 << 30) != 1 || mallopt(M_TOP_PAD, 64 << 20) != 1)
    std::fprintf(stderr, "pipeline_driver: mallopt rejected a setting; large arrays fall back to mmap (slower, still correct)\n");
  std::string ref_path, out_path, dump_dir, vcf_path, command_line, graphs_dir, msa_dir, probe_variants_path, probe_results_path;
  for (int i = 0; i < argc; ++i) command_line += std::string(i ? " " : "") + argv[i];
  double gc_frac = 0.41;  // --genome-gc-bias of the reference CLI: background GC of the LongdustQ null model
  std::vector<std::string> normals, tumors, regions;
  std::string bed_path;
  WindowBuilder::Params wp;
  ReadCollector::Params rp;
  ma_params_t prm;
  ma_default_params(&prm);
  bool no_active_region = false, extract_only = false, collect_reads = false, packed_reads = false, read_meta = false, poa_retry = false, raw_records = false, device_select = false;
  int batch_windows = 512;
  int extract_threads = static_cast<int>(std::min(8u, std::max(1u, std::thread::hardware_concurrency())));
  for (int i = 1; i < argc; ++i) {
    std::string const a = argv[i];
    auto next = [&]() -> const char* { return i + 1 < argc ? argv[++i] : ""; };
    if (a == "--reference" || a == "-r") ref_path = next();
    else if (a == "--normal" || a == "-n") normals.emplace_back(next());
    else if (a == "--tumor" || a == "-t") tumors.emplace_back(next());
    else if (a == "--region" || a == "-R") regions.emplace_back(next());
    else if (a == "--bed-file" || a == "-b") bed_path = next();  // cli_interface.cpp: regions from a BED file (core/bed_parser.cpp)
    else if (a == "--out" || a == "-o") out_path = next();
    else if (a == "--out-vcf") vcf_path = next();  // VCF text instead of the TSV lines (adds the SEQ_CX / GRAPH_CX annotation)
    else if (a == "--genome-gc-bias") gc_frac = std::atof(next());
    else if (a == "--window-size" || a == "-w") wp.window_length = static_cast<uint32_t>(std::atoi(next()));
    else if (a == "--pct-overlap" || a == "-p") wp.percent_overlap = static_cast<uint32_t>(std::atoi(next()));
    else if (a == "--padding" || a == "-P") wp.region_padding = static_cast<uint32_t>(std::atoi(next()));
    else if (a == "--min-kmer" || a == "-k") prm.min_k = std::atoi(next());
    else if (a == "--max-kmer" || a == "-K") prm.max_k = std::atoi(next());
    else if (a == "--kmer-step") prm.k_step = std::atoi(next());
    else if (a == "--min-anchor-cov") prm.min_anchor_cov = std::atoi(next());
    else if (a == "--min-node-cov") prm.min_node_cov = std::atoi(next());
    else if (a == "--max-sample-cov") rp.max_sample_cov = std::atof(next());
    else if (a == "--extract-pairs") rp.extract_pairs = true;
    else if (a == "--no-active-region") no_active_region = true;
    else if (a == "--batch-windows") batch_windows = std::max(1, std::atoi(next()));
    else if (a == "--extract-threads") extract_threads = std::max(1, std::atoi(next()));  // (the reference: -T, one collector per worker)
    else if (a == "--dump") dump_dir = next();
    else if (a == "--out-graphs-dir") graphs_dir = next();  // debugging: one DOT file per assembled component (assembles twice)
    else if (a == "--out-msa-dir") msa_dir = next();  // debugging: a GFA and a FASTA file per component (assembles and aligns twice)
    else if (a == "--probe-variants") probe_variants_path = next();  // debugging: truth variants to follow (assembles twice)
    else if (a == "--probe-results") probe_results_path = next();    // ... and where their records go
    else if (a == "--collect-reads") collect_reads = true;  // the reference-shaped collector (a Read per alignment) instead of CollectFlat
    else if (a == "--packed-reads") packed_reads = true;  // 4-bit read bases (and qualities) to the engine: ma_process_packed_batch
    else if (a == "--raw-records") raw_records = true;  // BAM records as they are to the engine: ma_flatten_records_batch, then the chained call
    else if (a == "--device-select") device_select = true;  // with --raw-records: filters, active-region detection and coverage gates on the device
    else if (a == "--read-meta") read_meta = true;  // with --out-vcf: the six FORMAT statistics over the read metadata too
    else if (a == "--poa-retry") poa_retry = true;  // ma_set_poa_retry: a second POA pass over the windows whose graph overflowed
    else if (a == "--extract-only") extract_only = true;  // stage 1 alone (with --dump): no device needed
    else { std::fprintf(stderr, "pipeline_driver: unknown option %s\n", a.c_str()); return 2; }
  }
  if (ref_path.empty() || (normals.empty() && tumors.empty())) {
    std::fprintf(stderr, "usage: pipeline_driver --reference ref.fa [--normal n.sam|bam]... [--tumor t.sam|bam]... [--region chr:a-b]... [--out calls.tsv]\n"
                         "  --packed-reads  read bases (and <= 16 distinct qualities per batch) go to the engine as 4-bit codes: a BAM record's\n"
                         "                  sequence bytes are copied undecoded, SAM text is packed.  A base letter that is none of BAM's\n"
                         "                  =ACMGRSVTWYHKDBN (lower case included) becomes N, as in a BAM file; without the flag it is passed on\n"
                         "                  as it is.  Not with --collect-reads / --extract-pairs\n"
                         "  --out-graphs-dir DIR  a debugging mode that ASSEMBLES EVERY BATCH TWICE: after a batch's chained call the batch goes\n"
                         "                  through ma_assemble_graph_batch and DIR/<chrom>_<start>_<end>__c<comp>__k<k>.dot is written for every\n"
                         "                  component a window reported -- the pruned graph its haplotypes were walked on.  Not with --packed-reads.\n"
                         "                  Costs 62 KB of host memory per window of a batch (and as much on the device), more when windows\n"
                         "                  outgrow the first caps and the batch is re-submitted: keep --batch-windows at a few hundred\n"
                         "  --out-msa-dir DIR  a debugging mode that ASSEMBLES AND ALIGNS EVERY BATCH TWICE: after a batch's chained call the batch\n"
                         "                  goes through ma_assemble_batch + ma_msa_graph_batch and DIR/msa__<chrom>_<start>_<end>__c<comp>.gfa\n"
                         "                  (the SPOA graph: a segment per node, a link per edge, a path per haplotype) and .fasta (the MSA\n"
                         "                  rows) are written for every component.  Not with --packed-reads; keep --batch-windows at a few hundred\n"
                         "  --probe-variants FILE --probe-results FILE  a debugging mode that ASSEMBLES EVERY BATCH TWICE: FILE is the reference's\n"
                         "                  missed_variants.txt (a header line, then tab-separated chrom, 0-based start, end, ref, alt, type, length,\n"
                         "                  classification, raw_alt_count, ...).  A variant is followed in every window whose region holds its start\n"
                         "                  (ma_assemble_probe_batch) and the results file gets the reference's probe_results.tsv header and one line\n"
                         "                  per (probe, window, component) -- one with comp_id . for a window without a component: kmer_size,\n"
                         "                  n_expected_alt_kmers, n_alt_kmers_in_reads, n_surviving_lowcov1, n_surviving_tips, hap_indices and the\n"
                         "                  three n_last_* columns; every other result column is \".\".  Not with --packed-reads\n"
                         "  --raw-records   BAM inputs only: the kept records go to the engine as the file has them; ma_flatten_records_batch\n"
                         "                  sorts them, interns the names and lays out the bases, then the chained call runs as with\n"
                         "                  --packed-reads --read-meta.  With --extract-only --dump: the ma_records_t arrays\n"
                         "  --device-select with --raw-records: every candidate record of a window goes to the engine, whole block, tags included;\n"
                         "                  ma_select_records_batch applies the record filters, detects the active regions and gates on\n"
                         "                  coverage, ma_flatten_records_batch takes the selected lists.  The N-only and repeat gates stay on the\n"
                         "                  host; a window the call hands back (coverage cap, an MD string that leaves its read, a full event\n"
                         "                  table) is collected by the host route and run as a batch of its own -- on the engine thread, one\n"
                         "                  window at a time, while the device waits: meant for the few windows of ordinary depth, not for\n"
                         "                  data where most windows are capped (raise --max-sample-cov or run without the flag)\n"
                         "  --read-meta     with --out-vcf: MAPQ, soft-clip and proper-pair flags, insert size and start of every read go to the\n"
                         "                  engine beside the batch (ma_process_meta_batch) and RMQ, SCA, FLD, RPCD, MQCD and FSSE are printed:\n"
                         "                  all 24 FORMAT values.  Without it those six are \".\"\n"
                         "  --poa-retry     windows whose POA graph ran out of nodes or of per-node edge slots (MA_W_VAR_OVERFLOW that larger\n"
                         "                  caps do not cure) are re-run by the engine with a larger graph.  Default: off\n");
    return 2;
  }
  if (raw_records && (collect_reads || rp.extract_pairs || packed_reads)) {
    std::fprintf(stderr, "pipeline_driver: --raw-records is a collector of its own (not with --collect-reads / --extract-pairs / --packed-reads)\n");
    return 2;
  }
  for (auto const* paths : {&normals, &tumors})
    for (std::string const& path : *paths)
      if (raw_records && !(path.size() > 4 && path.substr(path.size() - 4) == ".bam")) {
        std::fprintf(stderr, "pipeline_driver: --raw-records hands BAM records to the engine; %s is not a BAM file\n", path.c_str());
        return 2;
      }
  if (device_select && !raw_records) {
    std::fprintf(stderr, "pipeline_driver: --device-select selects among raw records on the device (needs --raw-records)\n");
    return 2;
  }
  if (raw_records && (!graphs_dir.empty() || !probe_variants_path.empty() || !msa_dir.empty())) {  // (stage calls on ASCII reads)
    std::fprintf(stderr, "pipeline_driver: --out-graphs-dir / --probe-variants / --out-msa-dir need ASCII reads (not with --raw-records)\n");
    return 2;
  }
  if (packed_reads && (collect_reads || rp.extract_pairs)) {
    std::fprintf(stderr, "pipeline_driver: --packed-reads needs the flat collector (not with --collect-reads / --extract-pairs)\n");
    return 2;
  }
  if (packed_reads && !graphs_dir.empty()) {  // (the stage calls do not take the packed form: include/microasm.h)
    std::fprintf(stderr, "pipeline_driver: --out-graphs-dir needs ASCII reads (not with --packed-reads)\n");
    return 2;
  }
  if (probe_variants_path.empty() != probe_results_path.empty()) {
    std::fprintf(stderr, "pipeline_driver: --probe-variants and --probe-results go together\n");
    return 2;
  }
  if (packed_reads && !probe_variants_path.empty()) {  // (likewise)
    std::fprintf(stderr, "pipeline_driver: --probe-variants needs ASCII reads (not with --packed-reads)\n");
    return 2;
  }
  if (packed_reads && !msa_dir.empty()) {  // (likewise)
    std::fprintf(stderr, "pipeline_driver: --out-msa-dir needs ASCII reads (not with --packed-reads)\n");
    return 2;
  }
  rp.packed_reads = packed_reads;
  rp.raw_records = raw_records;
  Reference const ref = Reference::LoadFasta(ref_path);
  std::vector<AlignmentSource> sources;
  sources.reserve(normals.size() + tumors.size());
  std::vector<SampleInfo> samples;
  auto add_sample = [&](const std::string& path, Tag tag) {
    sources.push_back(LoadAlignments(path, ref, packed_reads, raw_records, device_select));  // (packed: BAM records keep their sequence bytes)
    std::string name = path.substr(path.find_last_of('/') == std::string::npos ? 0 : path.find_last_of('/') + 1);
    name = name.substr(0, name.find_last_of('.'));
    samples.push_back({name, tag, nullptr, 0, 0, 0});
  };
  try {  // (an eager source -- SAM text, an unindexed BAM -- is decoded here: a corrupt record ends the run as it does on a collector thread)
    for (auto const& p : normals) add_sample(p, Tag::CTRL);
    for (auto const& p : tumors) add_sample(p, Tag::CASE);
  } catch (std::exception const& e) {
    std::fprintf(stderr, "pipeline_driver: %s\n", e.what());
    return 5;
  }
  for (size_t i = 0; i < samples.size(); ++i) samples[i].source = &sources[i];
  FlatBatch::RawTables raw_tables;  // --raw-records: the sample tables and reference maps every batch's ma_records_t points to
  if (raw_records) raw_tables = MakeRawTables(ReadCollector(rp, samples).Samples());
  prm.num_samples = static_cast<int32_t>(samples.size());
  prm.case_ctrl_mode = (!normals.empty() && !tumors.empty()) ? 1 : 0;  // read_collector.cpp:88-94
  if (wp.window_length + 1 > static_cast<uint32_t>(prm.max_hap_len) - 16) prm.max_hap_len = 3072;  // -w 2500 (cli maximum)

  WindowBuilder wb(&ref, wp);
  std::vector<RegionSpec> bed_regions;
  if (!bed_path.empty()) {
    try {
      bed_regions = ParseBedFile(bed_path, [&](std::string const& c) { return ref.Find(c) >= 0; });
    } catch (std::exception const& e) {
      std::fprintf(stderr, "pipeline_driver: %s\n", e.what());
      return 2;
    }
  }
  if (regions.empty() && bed_regions.empty()) wb.AddAllReferenceRegions();
  for (auto const& r : regions) wb.AddRegion(r);
  for (auto const& r : bed_regions) wb.AddRegion(r);
  std::vector<Window> const windows = wb.BuildWindows();

  ma_ctx_t* ctx = nullptr;
  int const crc = extract_only ? MA_OK : ma_create(&prm, 0, MA_MEM_HOST, &ctx);
  if (crc != MA_OK) {
    std::fprintf(stderr, "pipeline_driver: ma_create failed with %d%s\n", crc,
                 crc == MA_ERR_NO_DEVICE ? " (no HIP device: the engine has no CPU fallback)" : "");
    return 3;
  }
  if (ctx && poa_retry) ma_set_poa_retry(ctx, 1);

  Channel<Job> to_engine(3), to_flush(3);
  // batches whose records are flushed go back to the extract stage with their arrays' memory (a fresh batch is 300 MB of
  // pages to fault in, on the copying threads: a quarter of the stage's time)
  std::mutex pool_mu;
  std::vector<std::unique_ptr<FlatBatch>> batch_pool;
  auto recycle = [&](std::unique_ptr<FlatBatch> b) {
    if (!b) return;
    b->Clear();
    std::lock_guard<std::mutex> g(pool_mu);
    if (batch_pool.size() < 6) batch_pool.push_back(std::move(b));
  };
  size_t n_skipped[5] = {0, 0, 0, 0, 0};
  // busy time of each stage (what it spends on its own work, not waiting for its neighbours): windows / busy second is the
  // rate the stage could sustain alone -- the slowest of the three bounds the pipeline
  using Clock = std::chrono::steady_clock;
  auto secs = [](Clock::duration d) { return std::chrono::duration<double>(d).count(); };
  double busy_extract = 0.0, busy_engine = 0.0, busy_flush = 0.0;
  size_t n_shipped = 0;
  auto const t_start = Clock::now();
  // ---- stage 1: extract ----
  // N worker threads take windows off a shared counter (gates + read collection, each with its own ReadCollector and its own
  // handle on an indexed BAM, as the reference's workers have: async_worker.h:45); one assembler thread appends their
  // results to the batches IN WINDOW ORDER, so the batches do not depend on N.
  struct Slot {
    std::atomic<int> ready{0};
    WindowStatus st = WindowStatus::RUN;
    std::unique_ptr<FlatBatch> flat;  // the window's reads as the batch holds them (flattened on the collector's thread)
  };
  std::vector<Slot> slots(windows.size());
  std::atomic<size_t> next_window{0}, consumed{0};
  constexpr size_t kRunAhead = 4096;  // windows collected but not yet batched (bounds the memory held in slots)
  std::vector<double> worker_busy(static_cast<size_t>(extract_threads), 0.0);
  std::atomic<bool> worker_failed{false};
  std::exception_ptr worker_error;
  std::mutex worker_mu;
  // Round 6: the ordered thread no longer copies the windows' arrays into the batch (43 us of ONE thread per window: the stage's
  // bound at 23-30 k windows/s whatever the number of collectors).  It appends a window's scalars (FlatBatch::PlaceHeader), and
  // when a batch is closed and sized its windows are copied into their places by whoever has a hand free -- the collectors
  // between two windows, the ordered thread while it waits.
  struct CopyTask {
    FlatBatch* dst = nullptr;
    std::unique_ptr<FlatBatch> src;
    FlatBatch::Place place{};
    std::atomic<size_t>* left = nullptr;
  };
  std::mutex copy_mu;
  std::deque<CopyTask> copy_q;
  std::atomic<size_t> copy_pending{0};
  std::atomic<bool> extract_done{false};
  auto serve_copy = [&]() -> bool {
    if (copy_pending.load(std::memory_order_acquire) == 0) return false;
    CopyTask t;
    {
      std::lock_guard<std::mutex> g(copy_mu);
      if (copy_q.empty()) return false;
      t = std::move(copy_q.front());
      copy_q.pop_front();
    }
    copy_pending.fetch_sub(1, std::memory_order_acq_rel);
    t.dst->CopyPlaced(*t.src, t.place);
    t.src.reset();
    t.left->fetch_sub(1, std::memory_order_acq_rel);
    return true;
  };
  std::vector<std::thread> workers;
  for (int t = 0; t < extract_threads; ++t)
    workers.emplace_back([&, t] {
      std::vector<SampleInfo> mine = samples;
      std::vector<AlignmentSource> clones;
#ifdef LANCET2_AMD_WITH_ZLIB
      clones.reserve(mine.size());
      for (auto& sm : mine)
        if (sm.source->indexed() && t > 0) {
          clones.push_back(sm.source->CloneIndexed());
          sm.source = &clones.back();
        }
#endif
      ReadCollector collector(rp, mine);
      while (true) {
        if (serve_copy()) continue;  // a closed batch waits for its windows' arrays: those first
        size_t const i = next_window.load() < windows.size() ? next_window.fetch_add(1) : windows.size();
        if (i >= windows.size()) {
          if (extract_done.load(std::memory_order_acquire)) break;
          std::this_thread::sleep_for(std::chrono::microseconds(50));
          continue;
        }
        if (worker_failed.load(std::memory_order_acquire)) {  // another collector hit a corrupt input: hand over empty slots, stop
          slots[i].st = WindowStatus::SKIPPED_NONLY_REF_BASES;
          slots[i].ready.store(1, std::memory_order_release);
          continue;
        }
        try {
        while (i > consumed.load(std::memory_order_acquire) + kRunAhead) std::this_thread::sleep_for(std::chrono::microseconds(200));
        auto const t0 = Clock::now();
        Window const& w = windows[i];
        std::string_view const seq(ref.chroms[static_cast<size_t>(w.chrom)].seq.data() + (w.start1 - 1), w.Length());
        Slot& sl = slots[i];
        // --device-select: the N-only and repeat gates here, the rest of the gate on the device
        sl.st = PreReadGate(seq, prm.max_k, no_active_region || device_select, collector.Samples(), w);
        if (sl.st == WindowStatus::RUN && device_select) {
          auto flat = std::make_unique<FlatBatch>();
          if (!collector.CollectCandidates(w, seq, flat.get())) throw std::runtime_error("--device-select: a source is not in raw mode");
          sl.flat = std::move(flat);
        } else if (sl.st == WindowStatus::RUN) {
          // the window's reads straight into its flat arrays (ReadCollector::CollectFlat); the reference-shaped path -- a Read
          // per alignment, then FlatBatch::Add -- when the options need it (--extract-pairs) or --collect-reads asks for it
          auto flat = std::make_unique<FlatBatch>();
          if (!collect_reads && (raw_records ? collector.CollectRaw(w, seq, flat.get()) : collector.CollectFlat(w, seq, flat.get()))) {
            if (CrossSampleMeanCoverage(collector.Samples(), w.Length()) < static_cast<double>(prm.min_anchor_cov)) sl.st = WindowStatus::SKIPPED_ANCHOR_COVERAGE;
            else sl.flat = std::move(flat);
          } else {
            ReadCollector::Result const rc = collector.CollectRegion(w);
            if (CrossSampleMeanCoverage(rc.samples, w.Length()) < static_cast<double>(prm.min_anchor_cov)) {
              sl.st = WindowStatus::SKIPPED_ANCHOR_COVERAGE;
            } else {
              sl.flat = std::move(flat);
              sl.flat->Add(w, seq, rc.reads, &rc.samples);
            }
          }
        }
        worker_busy[static_cast<size_t>(t)] += secs(Clock::now() - t0);
        sl.ready.store(1, std::memory_order_release);
        } catch (...) {  // (a BGZF / BAI / BAM decoding error surfaces lazily, on this thread: keep the first one for main())
          {
            std::lock_guard<std::mutex> g(worker_mu);
            if (!worker_error) worker_error = std::current_exception();
          }
          worker_failed.store(true, std::memory_order_release);
          slots[i].st = WindowStatus::SKIPPED_NONLY_REF_BASES;
          slots[i].flat.reset();
          slots[i].ready.store(1, std::memory_order_release);
        }
      }
    });
  std::thread extract([&] {
    size_t hint_bases = 0, hint_reads = 0, hint_ref = 0;  // the last batch's sizes: the next one's arrays are reserved whole
    auto fresh = [&] {
      Job j;
      {
        std::lock_guard<std::mutex> g(pool_mu);
        if (!batch_pool.empty()) {
          j.batch = std::move(batch_pool.back());
          batch_pool.pop_back();
        }
      }
      if (!j.batch) j.batch = std::make_unique<FlatBatch>();
      j.batch->packed_mode = packed_reads;
      j.batch->raw_mode = raw_records;
      if (hint_reads) j.batch->Reserve(static_cast<size_t>(batch_windows), hint_ref, hint_reads, hint_bases);
      return j;
    };
    Job cur = fresh();
    size_t n_dumped = 0;
    std::vector<CopyTask> staged;  // the current batch's windows, in order
    // A closed batch is NOT waited for: its copy tasks are queued and the thread goes on with the next batch's headers; the
    // batches whose copies are through are sealed and handed to the engine in order whenever this thread comes by (waiting
    // at every close put most of a batch's 512 copies on this one thread: the collectors only look between two windows).
    struct Pending {
      Job job;
      std::unique_ptr<std::atomic<size_t>> left;
    };
    std::deque<Pending> pending;
    auto flush_ready = [&](bool wait_all) {
      while (!pending.empty()) {
        if (pending.front().left->load(std::memory_order_acquire) != 0) {
          if (!wait_all) return;
          if (!serve_copy()) std::this_thread::yield();
          continue;
        }
        auto const ts = Clock::now();
        Job j = std::move(pending.front().job);
        pending.pop_front();
        if (device_select) {
          j.batch->SealCandidates(raw_tables, rp.max_sample_cov, static_cast<uint32_t>(std::max(0, prm.min_anchor_cov)), no_active_region);
        } else if (raw_records) {
          j.batch->SealRaw(raw_tables);
        } else {
          j.batch->Seal();
          if (packed_reads) j.batch->PackReads();
        }
        busy_extract += secs(Clock::now() - ts);  // (the Push below may wait for the engine: not this stage's time)
        if (!dump_dir.empty()) {
          char sub[64];
          std::snprintf(sub, sizeof sub, "/batch_%04zu", n_dumped++);
          std::string const d = dump_dir + sub;
          std::string const cmd = "mkdir -p '" + d + "'";
          if (std::system(cmd.c_str()) != 0) std::exit(4);
          DumpBatch(d, *j.batch);
        }
        to_engine.Push(std::move(j));
      }
    };
    auto ship = [&] {
      if (cur.batch->windows.empty()) return;
      auto const ts = Clock::now();
      cur.batch->SizeForPlaced();
      hint_bases = cur.batch->read_quals.size() + cur.batch->read_quals.size() / 16;
      hint_reads = cur.batch->read_qname_id.size() + cur.batch->read_qname_id.size() / 16;
      hint_ref = cur.batch->ref_bases.size() + 64;
      auto left = std::make_unique<std::atomic<size_t>>(staged.size());
      {
        std::lock_guard<std::mutex> g(copy_mu);
        for (auto& t : staged) {
          t.dst = cur.batch.get();
          t.left = left.get();
          copy_q.push_back(std::move(t));
        }
      }
      copy_pending.fetch_add(staged.size(), std::memory_order_acq_rel);
      staged.clear();
      pending.push_back(Pending{std::move(cur), std::move(left)});
      busy_extract += secs(Clock::now() - ts);
      cur = fresh();
      flush_ready(false);
    };
    for (size_t i = 0; i < windows.size(); ++i) {
      Slot& sl = slots[i];
      while (!sl.ready.load(std::memory_order_acquire)) {  // (no spinning: the collectors need the cores)
        flush_ready(false);
        auto const tc = Clock::now();
        bool const copied = serve_copy();
        if (copied) busy_extract += secs(Clock::now() - tc);
        else std::this_thread::sleep_for(std::chrono::microseconds(50));
      }
      auto const t0 = Clock::now();
      n_skipped[static_cast<int>(sl.st)]++;
      if (sl.st == WindowStatus::RUN) {
        CopyTask t;
        t.place = cur.batch->PlaceHeader(*sl.flat);
        t.src = std::move(sl.flat);
        staged.push_back(std::move(t));
        n_shipped++;
      }
      sl.flat.reset();
      consumed.store(i + 1, std::memory_order_release);
      busy_extract += secs(Clock::now() - t0);
      if (static_cast<int>(cur.batch->windows.size()) >= batch_windows) ship();
    }
    ship();
    flush_ready(true);
    extract_done.store(true, std::memory_order_release);
    to_engine.Close();
  });
  // ---- stage 2: engine ----
  // --raw-records: the flattened arrays go to the chained call as --packed-reads --read-meta would bring them
  bool const with_meta = (read_meta || raw_records) && !vcf_path.empty();
  bool const engine_packed = packed_reads || raw_records;
  size_t n_graph_files = 0, n_msa_files = 0, n_probe_lines = 0, n_probe_skipped = 0;
  std::vector<ProbeVariant> probe_variants;
  FILE* probe_out = nullptr;
  if (!probe_variants_path.empty()) {
    try {
      probe_variants = LoadProbeVariants(probe_variants_path);
    } catch (std::exception const& e) {
      std::fprintf(stderr, "pipeline_driver: %s\n", e.what());
      return 2;
    }
    probe_out = std::fopen(probe_results_path.c_str(), "w");
    if (!probe_out) { std::perror("--probe-results"); return 4; }
    std::fputs(kProbeResultsHeader, probe_out);
  }
  // --device-select: the host route of the windows the device hands back runs on the engine thread, with sources of its own
  std::vector<SampleInfo> engine_samples = samples;
  std::vector<AlignmentSource> engine_clones;
#ifdef LANCET2_AMD_WITH_ZLIB
  if (device_select) {
    engine_clones.reserve(engine_samples.size());
    for (auto& sm : engine_samples)
      if (sm.source->indexed()) {
        engine_clones.push_back(sm.source->CloneIndexed());
        sm.source = &engine_clones.back();
      }
  }
#endif
  size_t n_host_windows = 0;
  std::thread engine([&] {
    ReadCollector host_collector(rp, engine_samples);
    Job j;
    while (to_engine.Pop(&j)) {
      if (extract_only) {
        recycle(std::move(j.batch));
        continue;
      }
      Job* nxt = nullptr;
      if (!raw_records && to_engine.Peek(&nxt)) {  // uploads under this batch's kernels (a raw batch's arrays are made in its own turn)
        if (with_meta) ma_prefetch_meta_batch(ctx, engine_packed ? &nxt->batch->packed_view : &nxt->batch->view,
                                              engine_packed ? &nxt->batch->packed : nullptr, &nxt->batch->meta);
        else if (engine_packed) ma_prefetch_packed_batch(ctx, &nxt->batch->packed_view, &nxt->batch->packed);
        else ma_prefetch_batch(ctx, &nxt->batch->view);
      }
      auto const t0 = Clock::now();
      j.out = std::make_unique<Outputs>();
      j.out->Allocate(prm, j.batch->view.n_windows, !vcf_path.empty(), with_meta);
      // --raw-records: the batch's read arrays are made on the device first, brought back (the driver is a MA_MEM_HOST caller)
      // and taken by the chained call from where the batch keeps them
      auto chain = [&](FlatBatch& fb, Outputs& o) -> int {
        if (!vcf_path.empty())  // one call: the chain with the statistics and INFO SEQ_CX / GRAPH_CX (core/variant_builder.cpp:159-160)
          return ma_process_cx_batch(ctx, engine_packed ? &fb.packed_view : &fb.view, engine_packed ? &fb.packed : nullptr,
                                     with_meta ? &fb.meta : nullptr, &o.gate, &o.asmb, &o.vars, &o.geno,
                                     &o.fmt, with_meta ? &o.fmeta : nullptr, gc_frac, &o.cx);
        if (engine_packed)
          return ma_process_packed_batch(ctx, &fb.packed_view, &fb.packed, &o.gate, &o.asmb, &o.vars, &o.geno, nullptr);
        return ma_process_stats_batch(ctx, &fb.view, &o.gate, &o.asmb, &o.vars, &o.geno, nullptr);  // (null: ma_process_batch)
      };
      // --device-select: the candidates' record bits, the windows' states and the selected lists first; the flatten call and
      // the chain then see the selected records alone (a window that is not listed has none: nothing is made of it)
      if (device_select) {
        j.rc = ma_select_records_batch(ctx, &j.batch->records, &j.batch->sel_params, &j.batch->sel_out);
        if (j.rc == MA_OK) j.batch->UseSelected();
      }
      // (a batch of which nothing is listed has no read at all: there is nothing to flatten or to assemble, its outputs stay
      // as Allocate() made them -- no variant anywhere)
      bool const nothing_listed = device_select && j.rc == MA_OK && j.batch->n_selected == 0;
      if (nothing_listed)
        for (int w = 0; w < j.batch->view.n_windows; ++w) j.out->asmb.win_status[w] = MA_W_NO_HAPLOTYPE;
      if (j.rc == MA_OK && raw_records && !nothing_listed) j.rc = ma_flatten_records_batch(ctx, &j.batch->records, &j.batch->flat_out);
      if (j.rc == MA_OK && !nothing_listed) j.rc = chain(*j.batch, *j.out);
      if (j.rc != MA_OK) j.err = ma_last_error(ctx);
      for (size_t w = 0; device_select && j.rc == MA_OK && w < j.batch->windows.size(); ++w) {
        if (!(j.batch->win_state[w] & MA_S_HOST_BITS)) continue;
        // handed back: today's route for this window -- PreReadGate, CollectRaw with its downsampling, the coverage gate -- and
        // a batch of its own
        Window const& win = j.batch->windows[w];
        std::string_view const seq(ref.chroms[static_cast<size_t>(win.chrom)].seq.data() + (win.start1 - 1), win.Length());
        ++n_host_windows;
        try {
          if (PreReadGate(seq, prm.max_k, no_active_region, host_collector.Samples(), win) != WindowStatus::RUN) {
            j.batch->win_state[w] = static_cast<uint8_t>(j.batch->win_state[w] & ~MA_S_ACTIVE);  // (for the counts below)
            continue;
          }
          FlatBatch one;
          if (!host_collector.CollectRaw(win, seq, &one)) throw std::runtime_error("--device-select: a source is not in raw mode");
          if (CrossSampleMeanCoverage(host_collector.Samples(), win.Length()) < static_cast<double>(prm.min_anchor_cov)) {
            j.batch->win_state[w] = static_cast<uint8_t>(j.batch->win_state[w] | MA_S_ACTIVE | MA_S_LOW_COVERAGE);
            continue;
          }
          j.batch->win_state[w] = static_cast<uint8_t>((j.batch->win_state[w] | MA_S_ACTIVE) & ~MA_S_LOW_COVERAGE);
          auto hb = std::make_unique<FlatBatch>();
          hb->raw_mode = true;
          FlatBatch::Place const pl = hb->PlaceHeader(one);
          hb->SizeForPlaced();
          hb->CopyPlaced(one, pl);
          hb->SealRaw(raw_tables);
          auto ho = std::make_unique<Outputs>();
          ho->Allocate(prm, 1, !vcf_path.empty(), with_meta);
          j.rc = ma_flatten_records_batch(ctx, &hb->records, &hb->flat_out);
          if (j.rc == MA_OK) j.rc = chain(*hb, *ho);
          if (j.rc != MA_OK) j.err = ma_last_error(ctx);
          j.host_windows.emplace_back(std::move(hb), std::move(ho));
        } catch (std::exception const& e) {  // (reading the alignments failed: not an engine error, the batch fails all the same)
          j.rc = kHostRouteFailed;
          j.err = std::string("--device-select: the host route of window ") + std::to_string(win.start1) + "-" + std::to_string(win.end1) +
                  " failed: " + e.what();
        }
      }
      if (j.rc == MA_OK && !graphs_dir.empty()) {
        long const nf = WriteGraphs(ctx, prm, ref, *j.batch, graphs_dir);
        if (nf < 0) {
          j.rc = MA_ERR_HIP;
          j.err = std::string("--out-graphs-dir: ") + ma_last_error(ctx);
        } else {
          n_graph_files += static_cast<size_t>(nf);
        }
      }
      if (j.rc == MA_OK && probe_out) {
        long const nl = WriteProbeResults(ctx, prm, ref, *j.batch, probe_variants, probe_out, &n_probe_skipped);
        if (nl < 0) {
          j.rc = MA_ERR_HIP;
          j.err = std::string("--probe-variants: ") + ma_last_error(ctx);
        } else {
          n_probe_lines += static_cast<size_t>(nl);
        }
      }
      if (j.rc == MA_OK && !msa_dir.empty()) {
        long const nf = WriteMsaFiles(ctx, prm, ref, *j.batch, msa_dir);
        if (nf < 0) {
          j.rc = MA_ERR_HIP;
          j.err = std::string("--out-msa-dir: ") + ma_last_error(ctx);
        } else {
          n_msa_files += static_cast<size_t>(nf);
        }
      }
      busy_engine += secs(Clock::now() - t0);
      to_flush.Push(std::move(j));
    }
    to_flush.Close();
  });
  // ---- stage 3: store + ordered flush ----
  bool const as_vcf = !vcf_path.empty();
  FILE* out = as_vcf ? std::fopen(vcf_path.c_str(), "w") : (out_path.empty() ? stdout : std::fopen(out_path.c_str(), "w"));
  if (!out) { std::perror("--out"); return 4; }
  std::vector<SampleInfo> sorted_samples = samples;
  SortSamples(sorted_samples);
  std::vector<Tag> tags;
  for (auto const& s_ : sorted_samples) tags.push_back(s_.tag);
  if (as_vcf) std::fputs(VcfHeader(ref, sorted_samples, prm.case_ctrl_mode != 0, true, command_line, ref_path).c_str(), out);
  VariantStore store;
  size_t n_records = 0, n_assembled = 0, n_flagged = 0, idx_to_flush = 0;
  size_t n_dev_skipped[5] = {0, 0, 0, 0, 0};  // --device-select: windows the device call (or the host route behind it) skipped
  int rc_all = 0;
  auto write = [&](std::vector<VariantRecord> recs) {
    for (auto const& r : recs)
      std::fprintf(out, "%s\n", as_vcf ? AsVcfRecord(r, ref, tags, prm.case_ctrl_mode != 0).c_str() : r.AsLine(ref).c_str());
    n_records += recs.size();
  };
  {
    Job j;
    while (to_flush.Pop(&j)) {
      if (j.rc != MA_OK) {
        std::fprintf(stderr, "pipeline_driver: batch failed (%d): %s\n", j.rc, j.err.c_str());
        rc_all = 5;
        continue;
      }
      // pipeline_executor.cpp:215-252: the flush lags the last window done by NUM_BUFFER_WINDOWS = 100 windows, so that a
      // call can still be replaced by a better covered duplicate from a window that overlaps its own (batches finish in
      // window order here; windows the gates skipped count as done)
      auto const tf = Clock::now();
      auto records_of = [&](FlatBatch const& fb, Outputs const& o) {
        return RecordsOfBatch(prm, fb, o.vars, o.geno, as_vcf ? &o.cx : nullptr, true, as_vcf ? &o.fmt : nullptr, as_vcf ? &o.asmb : nullptr,
                              as_vcf && (read_meta || raw_records) ? &o.fmeta : nullptr);
      };
      std::vector<VariantRecord> recs = records_of(*j.batch, *j.out);
      if (!j.host_windows.empty()) {  // the handed-back windows' records where the batch would have had them: in window order
        for (auto const& hw : j.host_windows)
          for (auto& r : records_of(*hw.first, *hw.second)) recs.push_back(std::move(r));
        std::stable_sort(recs.begin(), recs.end(), [](VariantRecord const& a, VariantRecord const& b) { return a.window_index < b.window_index; });
      }
      store.AddVariants(std::move(recs));
      size_t const done_upto = j.batch->windows.back().genome_index + 1;
      constexpr size_t kBufferWindows = 100;
      if (done_upto > kBufferWindows && done_upto - kBufferWindows > idx_to_flush) {
        idx_to_flush = done_upto - kBufferWindows;
        write(store.ExtractBeforeWindow(windows[idx_to_flush]));
      }
      for (int w = 0; w < j.batch->view.n_windows; ++w) {
        if (device_select && !(j.batch->win_state[static_cast<size_t>(w)] & MA_S_LISTED)) {  // skipped on the device, or run by the host route
          uint8_t const ws = j.batch->win_state[static_cast<size_t>(w)];
          if (!(ws & MA_S_ACTIVE)) n_dev_skipped[3]++;
          else if (ws & MA_S_LOW_COVERAGE) n_dev_skipped[4]++;
          continue;
        }
        uint32_t const st = j.out->asmb.win_status[w];
        n_assembled += (st & MA_W_NO_HAPLOTYPE) ? 0 : 1;
        n_flagged += (st & ~static_cast<uint32_t>(MA_W_NO_HAPLOTYPE | MA_W_BFS_LIMIT)) ? 1 : 0;
      }
      for (auto const& hw : j.host_windows) {
        uint32_t const st = hw.second->asmb.win_status[0];
        n_assembled += (st & MA_W_NO_HAPLOTYPE) ? 0 : 1;
        n_flagged += (st & ~static_cast<uint32_t>(MA_W_NO_HAPLOTYPE | MA_W_BFS_LIMIT)) ? 1 : 0;
      }
      busy_flush += secs(Clock::now() - tf);
      recycle(std::move(j.batch));
    }
    auto const tf = Clock::now();
    write(store.ExtractAll());
    busy_flush += secs(Clock::now() - tf);
  }
  for (auto& t : workers) t.join();
  extract.join();
  engine.join();
  if (ctx) ma_destroy(ctx);
  if (out != stdout) std::fclose(out);
  if (worker_error) {  // a collector thread's decoding error: the driver's own message and exit code, not std::terminate
    try {
      std::rethrow_exception(worker_error);
    } catch (std::exception const& e) {
      std::fprintf(stderr, "pipeline_driver: reading the alignments failed: %s\n", e.what());
    } catch (...) {
      std::fprintf(stderr, "pipeline_driver: reading the alignments failed\n");
    }
    return 5;
  }
  std::fprintf(stderr,
               "pipeline_driver: %zu windows (%zu N-only, %zu max-k repeat, %zu inactive, %zu below anchor coverage), %zu assembled, "
               "%zu with a capacity flag, %zu records\n",
               windows.size(), n_skipped[1], n_skipped[2], n_skipped[3] + n_dev_skipped[3], n_skipped[4] + n_dev_skipped[4], n_assembled, n_flagged,
               n_records);
  if (device_select) std::fprintf(stderr, "pipeline_driver: --device-select handed %zu windows back to the host route\n", n_host_windows);
  if (probe_out) {
    std::fclose(probe_out);
    std::fprintf(stderr, "pipeline_driver: %zu probe records of %zu truth variants written to %s (%zu activations skipped: an allele past its window or the call's limits)\n",
                 n_probe_lines, probe_variants.size(), probe_results_path.c_str(), n_probe_skipped);
  }
  if (!graphs_dir.empty()) std::fprintf(stderr, "pipeline_driver: %zu component graphs written to %s\n", n_graph_files, graphs_dir.c_str());
  if (!msa_dir.empty()) std::fprintf(stderr, "pipeline_driver: %zu MSA files written to %s\n", n_msa_files, msa_dir.c_str());
  double const wall = secs(Clock::now() - t_start);
  size_t blocks = 0;
  bool any_indexed = false;
#ifdef LANCET2_AMD_WITH_ZLIB
  for (auto const& src : sources) {
    blocks += src.blocks_inflated();
    any_indexed = any_indexed || src.indexed();
  }
#endif
  auto rate = [](size_t nn, double t) { return t > 0.0 ? static_cast<double>(nn) / t : 0.0; };
  double collect_cpu = 0.0, collect_max = 0.0;
  for (double b : worker_busy) {
    collect_cpu += b;
    collect_max = std::max(collect_max, b);
  }
  double const busy_batching = busy_extract;
  busy_extract = std::max(busy_batching, collect_max);  // the stage's span: collectors and the ordered batching thread run side by side
  std::fprintf(stderr,
               "pipeline_driver: stages -- extract %.3f s busy (%.0f windows/s tiled, %.0f shipped/s) with %d collector thread(s), %.3f cpu-s of collection, %.3f s of ordered batching, engine %.3f s busy (%.0f windows/s), "
               "flush %.3f s busy (%.0f windows/s); wall %.3f s (%.0f shipped windows/s)%s\n",
               busy_extract, rate(windows.size(), busy_extract), rate(n_shipped, busy_extract), extract_threads, collect_cpu, busy_batching, busy_engine, rate(n_shipped, busy_engine),
               busy_flush, rate(n_shipped, busy_flush), wall, rate(n_shipped, wall),
               any_indexed ? (std::string("; indexed BAM: ") + std::to_string(blocks) + " BGZF blocks inflated").c_str() : "");
  return rc_all;
}
