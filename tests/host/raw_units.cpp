// ReadCollector::CollectRaw against CollectFlat on the same BAM files (argv: ref.fa normal.bam tumor.bam): the same filters
// and the same seeded downsampling -- the kept records of every window are the same, with and without the coverage cap -- and
// what CollectRaw hands over is each kept record's core bytes, in arrival order.  Built by tests/test_flatten_ref.py.
#include <cstdio>
#include <map>

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

// (name, flag, pos) of a raw record's bytes
static std::tuple<std::string, int, int32_t> KeyOfRaw(const uint8_t* b) {
  int32_t pos;
  std::memcpy(&pos, b + 4, 4);
  uint16_t flag;
  std::memcpy(&flag, b + 14, 2);
  return {std::string(reinterpret_cast<const char*>(b + 32), b[8] ? b[8] - 1u : 0u), flag, pos};
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  Reference const ref = Reference::LoadFasta(argv[1]);
  AlignmentSource const flat_src[2] = {AlignmentSource::LoadBam(argv[2], ref, true), AlignmentSource::LoadBam(argv[3], ref, true)};
  AlignmentSource const raw_src[2] = {AlignmentSource::LoadBam(argv[2], ref, false, true), AlignmentSource::LoadBam(argv[3], ref, false, true)};
  CHECK(raw_src[0].recs.size() == flat_src[0].recs.size() && !raw_src[0].recs.empty());
  for (size_t i = 0; i < raw_src[0].recs.size(); ++i) {  // a raw record: no name, no CIGAR vector, no sequence -- the scalars agree
    SamRecord const &a = flat_src[0].recs[i], &r = raw_src[0].recs[i];
    CHECK(r.is_raw && r.qname.empty() && r.cigar.empty() && r.seq.empty() && r.seq4.empty() && r.qual.empty());
    CHECK(r.NameHash() == a.NameHash() && r.RefSpan() == a.RefSpan() && r.SeqLen() == a.SeqLen() && r.NumCigar() == a.NumCigar());
    CHECK(r.flag == a.flag && r.mapq == a.mapq && r.pos0 == a.pos0 && r.chrom == a.chrom && r.md == a.md);
    CHECK(r.raw.size() == 32 + a.qname.size() + 1 + 4 * a.cigar.size() + (a.SeqLen() + 1) / 2 + a.SeqLen());
    CHECK(std::equal(a.qual.begin(), a.qual.end(), r.QualData()) && r.QualSize() == a.qual.size());
  }
  std::vector<Window> const windows = {{0, 1, 1000}, {0, 501, 1500}, {0, 2801, 3800}, {0, 5001, 6000}};
  size_t capped = 0, total = 0;
  for (double cov : {1000.0, 12.0}) {  // the default cap never bites on a 34x / 44x fixture; 12x does, for both samples
    ReadCollector::Params fp, rp;
    fp.max_sample_cov = rp.max_sample_cov = cov;
    fp.packed_reads = true;
    rp.raw_records = true;
    ReadCollector flat(fp, {{"normal", Tag::CTRL, &flat_src[0], 0, 0, 0}, {"tumor", Tag::CASE, &flat_src[1], 0, 0, 0}});
    ReadCollector raw(rp, {{"normal", Tag::CTRL, &raw_src[0], 0, 0, 0}, {"tumor", Tag::CASE, &raw_src[1], 0, 0, 0}});
    for (Window const& w : windows) {
      std::string_view const seq(ref.chroms[0].seq.data() + (w.start1 - 1), w.Length());
      // CollectFlat's kept set, through the selection the two share ... and through its own output
      std::vector<ReadCollector::Kept> sel;
      std::deque<SamRecord> arena;
      size_t const bases = flat.SelectKept(w, &sel, &arena);
      FlatBatch fb, rb;
      CHECK(flat.CollectFlat(w, seq, &fb) && raw.CollectRaw(w, seq, &rb));
      CHECK(rb.raw_mode && rb.rec_len.size() == sel.size() && fb.read_qname_id.size() == sel.size());
      CHECK(rb.read_off.back() == bases && fb.read_off.back() == bases && rb.read_win_off.back() == sel.size());
      CHECK(rb.sample_cov == fb.sample_cov && rb.ref_bases.size() == fb.ref_bases.size());
      std::map<std::tuple<std::string, int, int32_t>, int> want;
      for (size_t i = 0; i < sel.size(); ++i) {
        SamRecord const& a = *sel[i].rec;
        want[{a.qname, a.flag, static_cast<int32_t>(a.pos0)}]++;
        // arrival order: record i of the raw window IS the i-th kept record
        CHECK(KeyOfRaw(rb.raw_blob.data() + rb.rec_off[i]) == std::make_tuple(a.qname, static_cast<int>(a.flag), static_cast<int32_t>(a.pos0)));
        CHECK(rb.rec_sample[i] == sel[i].sample);
      }
      for (size_t i = 0; i < rb.rec_len.size(); ++i) want[KeyOfRaw(rb.raw_blob.data() + rb.rec_off[i])]--;
      for (auto const& kv : want) CHECK(kv.second == 0);
      uint64_t uncapped = 0;
      for (int s = 0; s < 2; ++s)
        flat_src[s].ForRegion(0, static_cast<int64_t>(w.start1), static_cast<int64_t>(w.end1), [&](SamRecord const& a) { uncapped += ReadCollector::Filtered(a) ? 0 : 1; });
      if (sel.size() < uncapped) ++capped;
      ++total;
    }
  }
  CHECK(capped >= 3 && capped < total);  // the cap bit in the 12x runs and only there
  if (failures) return 1;
  std::printf("raw units ok\n");
  return 0;
}
