// What tests/select_ref.py restates, from the host shell itself (argv: ref.fa normal.bam tumor.bam out_dir): the candidates of
// a few dozen windows as ReadCollector::CollectCandidates lists them (whole blocks, tags included), and per window the shell's
// own answers -- IsActiveRegion over the records as they come and in reverse, ReadCollector::Filtered and CheckAlignment's
// filter per record, the sums of SelectKept uncapped and whether a cap of 12x bites, CrossSampleMeanCoverage against two
// bounds.  Built and compared by tests/test_select_ref.py.
#include <cstdio>

#include "../../lancet2_amd/host/pipeline_host.hpp"

using namespace lancet2_amd::host;

static int failures = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

template <class T>
static void Put(std::string const& dir, const char* name, std::vector<T> const& v) {
  FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
  if (!f) std::exit(4);
  if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
  std::fclose(f);
}

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  std::string const dir = argv[4];
  Reference const ref = Reference::LoadFasta(argv[1]);
  AlignmentSource const plain[2] = {AlignmentSource::LoadBam(argv[2], ref), AlignmentSource::LoadBam(argv[3], ref)};
  AlignmentSource const whole[2] = {AlignmentSource::LoadBam(argv[2], ref, false, true, true), AlignmentSource::LoadBam(argv[3], ref, false, true, true)};
  for (int s = 0; s < 2; ++s) {  // a whole-block raw record: nothing decoded, the MD string found in its bytes on demand
    CHECK(whole[s].recs.size() == plain[s].recs.size() && !whole[s].recs.empty());
    for (size_t i = 0; i < whole[s].recs.size(); ++i) {
      SamRecord const &a = plain[s].recs[i], &r = whole[s].recs[i];
      std::string_view md;
      CHECK(r.is_raw && r.md.empty() && !r.has_md && r.raw.size() > r.raw_core && r.Md(&md) == a.has_md && md == a.md);
      CHECK(r.QualSize() == a.qual.size() && std::equal(a.qual.begin(), a.qual.end(), r.QualData()));
    }
  }
  ReadCollector::Params rp;
  rp.raw_records = true;
  std::vector<SampleInfo> const samples = {{"normal", Tag::CTRL, &whole[0], 0, 0, 0}, {"tumor", Tag::CASE, &whole[1], 0, 0, 0}};
  ReadCollector wide(rp, samples);
  rp.max_sample_cov = 12.0;
  ReadCollector tight(rp, samples);
  FlatBatch fb;
  std::vector<uint32_t> win_len;
  std::vector<uint8_t> keep;
  FILE* txt = std::fopen((dir + "/windows.txt").c_str(), "w");
  if (!txt) return 4;
  uint64_t const glen = ref.chroms[0].seq.size();
  for (uint64_t start1 = 1; start1 + 199 <= glen; start1 += 100) {
    Window const w{0, start1, start1 + 199};
    std::string_view const seq(ref.chroms[0].seq.data() + (w.start1 - 1), w.Length());
    CHECK(wide.CollectCandidates(w, seq, &fb));
    win_len.push_back(static_cast<uint32_t>(w.Length()));
    bool const active = IsActiveRegion(wide.Samples(), w);
    bool reversed = false;
    for (auto const& sm : wide.Samples()) {
      std::vector<SamRecord> recs;
      sm.source->ForRegion(w.chrom, static_cast<int64_t>(w.start1), static_cast<int64_t>(w.end1), [&](SamRecord const& a) {
        recs.push_back(a);
        keep.push_back(static_cast<uint8_t>((ReadCollector::Filtered(a) ? 0 : 1) |
                                            (a.IsQcFail() || a.IsDuplicate() || a.IsUnmapped() || a.mapq == 0 ? 0 : 2)));
      });
      MutationAccumulator acc;
      for (size_t i = recs.size(); i-- > 0;)
        if (acc.CheckAlignment(recs[i])) reversed = true;
    }
    std::vector<ReadCollector::Kept> sel;
    std::deque<SamRecord> arena;
    wide.SelectKept(w, &sel, &arena);
    double const cov = CrossSampleMeanCoverage(wide.Samples(), w.Length());
    std::vector<ReadCollector::Kept> sel12;
    tight.SelectKept(w, &sel12, &arena);
    std::fprintf(txt, "%d %d", active ? 1 : 0, reversed ? 1 : 0);
    for (size_t s = 0; s < 2; ++s)
      std::fprintf(txt, " %llu %llu", static_cast<unsigned long long>(wide.Samples()[s].sampled_reads),
                   static_cast<unsigned long long>(wide.Samples()[s].sampled_bases));
    std::fprintf(txt, " %d %d %d\n", sel12.size() < sel.size() ? 1 : 0, cov < 30.0 ? 1 : 0, cov < 60.0 ? 1 : 0);
  }
  std::fclose(txt);
  CHECK(fb.cand_mode && fb.raw_mode && fb.read_win_off.size() == win_len.size() + 1 && keep.size() == fb.rec_len.size());
  std::vector<uint8_t> const blob(fb.raw_blob.begin(), fb.raw_blob.end());
  Put(dir, "blob.u8", blob);
  Put(dir, "rec_off.u64", fb.rec_off);
  Put(dir, "rec_len.u32", fb.rec_len);
  Put(dir, "rec_win_off.u32", fb.read_win_off);
  Put(dir, "rec_sample.u8", fb.rec_sample);
  Put(dir, "win_len.u32", win_len);
  Put(dir, "keep.u8", keep);
  if (failures) return 1;
  std::printf("select units ok\n");
  return 0;
}
