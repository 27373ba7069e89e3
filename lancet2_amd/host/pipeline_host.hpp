// Host shell of the `pipeline` path around the microassembly engine: everything between the
// alignment files and the C-ABI batches, and between the engine's results and the ordered, de-duplicated variant stream.
// Plain C++17 (g++; zlib only for BAM) -- no htslib, no HIP.  What each piece restates:
//   Reference / AlignmentSource   hts::Reference, hts::Extractor (FASTA text; SAM text or BAM through zlib, whole file in memory:
//                                 a deployment keeps htslib's indexed iterators behind the same ForRegion interface)
//   WindowBuilder                 core/window_builder.cpp:76-284 (padding, step size, tiling, sort + genome index)
//   IsActiveRegion                core/active_region_detector.cpp:85-232 (MD mismatches, CIGAR indels, soft clips; >= 2 reads)
//   ReadCollector                 core/read_collector.cpp:42-309 (filters, coverage-capped paired downsampling with the fixed
//                                 seed, mate recapture, the 6-key comparator)
//   ShouldSkip / coverage gate    core/variant_builder.cpp:107-132, :214-224
//   Flatten                       cbdg::Read -> ma_batch_t (include/microasm.h): qname interning, flags, mapping hints
//   VariantStore                  core/variant_store.cpp:20-124 (same CHROM+POS+REF: keep the call with more coverage; flush
//                                 what lies before a window, coordinate-sorted; calls without ALT support are dropped)
// This header never includes anything under oracle/.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <optional>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <string_view>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <deque>
#include <vector>

#include "../../include/microasm.h"

#ifdef LANCET2_AMD_WITH_ZLIB
#include <zlib.h>
#endif

namespace lancet2_amd::host {

// ---- reference ---------------------------------------------------------------------------------------------------------
struct Chrom {
  std::string name;
  std::string seq;
};
struct Reference {
  std::vector<Chrom> chroms;
  int Find(std::string_view name) const {
    for (size_t i = 0; i < chroms.size(); ++i)
      if (chroms[i].name == name) return static_cast<int>(i);
    return -1;
  }
  static Reference LoadFasta(const std::string& path) {
    std::ifstream in(path);
    if (!in) throw std::runtime_error("cannot open reference " + path);
    Reference r;
    std::string line;
    while (std::getline(in, line)) {
      if (!line.empty() && line.back() == '\r') line.pop_back();
      if (line.empty()) continue;
      if (line[0] == '>') {
        size_t const e = line.find_first_of(" \t");
        r.chroms.push_back({line.substr(1, e == std::string::npos ? std::string::npos : e - 1), {}});
      } else if (!r.chroms.empty()) {
        r.chroms.back().seq += line;
      }
    }
    return r;
  }
};

// ---- alignment records -------------------------------------------------------------------------------------------------
struct CigarUnit {
  char op;
  uint32_t len;
  bool ConsumesReference() const { return op == 'M' || op == 'D' || op == 'N' || op == '=' || op == 'X'; }
};
inline uint64_t HashQname(std::string_view q) {  // (the reference hashes with absl; only equality of names matters)
  uint64_t h = 1469598103934665603ull;
  for (char c : q) h = (h ^ static_cast<uint8_t>(c)) * 1099511628211ull;
  return h;
}
// the auxiliary fields of a BAM record, `b + p` on: only MD (type Z or H; the last one) and the presence of SA matter here
inline void WalkAuxFields(const unsigned char* b, size_t block, size_t p, std::string_view* md, bool* has_md, bool* has_sa) {
  while (p + 3 <= block) {
    char const t0 = static_cast<char>(b[p]), t1 = static_cast<char>(b[p + 1]), ty = static_cast<char>(b[p + 2]);
    p += 3;
    size_t len = 0;
    if (ty == 'Z' || ty == 'H') {
      const void* const nul = std::memchr(b + p, 0, block - p);
      if (!nul) break;  // unterminated string: nothing further can be trusted
      len = static_cast<size_t>(static_cast<const unsigned char*>(nul) - (b + p)) + 1;
      if (t0 == 'M' && t1 == 'D') {
        *md = std::string_view(reinterpret_cast<const char*>(b + p), len - 1);
        *has_md = true;
      }
      if (t0 == 'S' && t1 == 'A') *has_sa = true;
    } else if (ty == 'A' || ty == 'c' || ty == 'C') len = 1;
    else if (ty == 's' || ty == 'S') len = 2;
    else if (ty == 'i' || ty == 'I' || ty == 'f') len = 4;
    else if (ty == 'B') {
      if (p + 5 > block) break;
      char const sub = static_cast<char>(b[p]);
      int32_t cnt;
      std::memcpy(&cnt, b + p + 1, 4);
      if (cnt < 0) break;
      size_t const es = (sub == 'c' || sub == 'C') ? 1 : ((sub == 's' || sub == 'S') ? 2 : 4);
      len = 5 + es * static_cast<size_t>(cnt);
    } else break;
    if (len > block - p) break;
    p += len;
  }
}
struct SamRecord {
  std::string qname;
  uint16_t flag = 0;
  int32_t chrom = -1;
  int64_t pos0 = -1;
  uint8_t mapq = 0;
  std::vector<CigarUnit> cigar;
  int32_t mate_chrom = -1;
  int64_t mate_pos0 = -1;
  int64_t tlen = 0;
  std::string seq;
  std::vector<uint8_t> seq4;  // a BAM source opened with keep_packed (--packed-reads): the record's (l_seq + 1) / 2 sequence bytes, `seq` stays empty
  uint32_t l_seq4 = 0;
  bool packed = false;
  size_t SeqLen() const { return packed ? l_seq4 : seq.size(); }
  // a BAM source opened in raw mode (--raw-records): the record's core bytes as the file has them -- the 32 fixed bytes, name,
  // CIGAR words, packed sequence, qualities (ma_records_t's unit, include/microasm.h) -- as ONE vector
  // per record, where the decoded record holds a name string, a CIGAR vector, a sequence and a quality vector (the bytes are
  // copied again on their way: an indexed source's records into the collector's arena, a kept record into its window's
  // raw_blob, the window into the batch's).  qname, cigar, seq, seq4
  // and qual stay empty; what the filters, the coverage cap and IsActiveRegion need beyond the fixed fields is kept as scalars
  // (the name's hash, the reference span) or read from the bytes (CIGAR words, qualities).  `packed` is set: SeqLen() is l_seq4
  // With keep_tags (--device-select) `raw` is the record's WHOLE block, auxiliary fields included; raw_core is where they begin
  // and nothing of them is decoded when the record is made: `md` stays empty, Md() finds the string in the bytes when asked
  // (CheckAlignment on the host route of a window the device handed back).
  std::vector<uint8_t> raw;
  uint32_t raw_core = 0;  // bytes of the core part
  bool is_raw = false;
  uint64_t raw_qh = 0;    // HashQname of the name
  int64_t raw_span = 1;   // RefSpan()
  uint64_t NameHash() const { return is_raw ? raw_qh : HashQname(qname); }
  size_t NumCigar() const { return is_raw ? static_cast<size_t>(raw[12] | (raw[13] << 8)) : cigar.size(); }
  CigarUnit Cigar(size_t i) const {
    if (!is_raw) return cigar[i];
    static const char* kOps = "MIDNSHP=X";
    uint32_t v;
    std::memcpy(&v, raw.data() + 32 + raw[8] + 4 * i, 4);
    return {(v & 15u) < 9 ? kOps[v & 15u] : '?', v >> 4};
  }
  const uint8_t* QualData() const { return is_raw ? raw.data() + raw_core - l_seq4 : qual.data(); }
  size_t QualSize() const { return is_raw ? l_seq4 : qual.size(); }
  std::vector<uint8_t> qual;
  std::string md;
  bool has_md = false, has_sa = false;
  // the MD string: decoded (`md`), or found in a whole-block raw record's auxiliary fields; false: the record has none.
  // On a keep_tags record `md`, `has_md` and `has_sa` are NOT filled (nothing was walked): read MD through Md() only -- it walks
  // the fields anew on every call, once per record on the host route.  has_sa has one reader, the mate collection of
  // --extract-pairs (ReadCollector::CollectRegion), which the driver refuses together with raw records
  inline bool Md(std::string_view* out) const;
  bool IsQcFail() const { return flag & 0x200; }
  bool IsDuplicate() const { return flag & 0x400; }
  bool IsUnmapped() const { return flag & 0x4; }
  bool IsMateMapped() const { return (flag & 0x1) && !(flag & 0x8); }
  bool IsMappedProperPair() const { return flag & 0x2; }
  bool IsReverse() const { return flag & 0x10; }
  int64_t RefSpan() const {
    if (is_raw) return raw_span;
    int64_t s = 0;
    for (auto const& c : cigar)
      if (c.ConsumesReference()) s += c.len;
    return s > 0 ? s : 1;
  }
  uint32_t LeadingSoftClip() const { return !cigar.empty() && cigar.front().op == 'S' ? cigar.front().len : 0u; }
  // cbdg::Read::IsSoftClipped (cbdg/read.h:39-50): the bases of ALL S operations of the record's CIGAR, at least 6 % of the read
  bool IsSoftClipped() const {
    uint32_t clip = 0;
    for (auto const& c : cigar)
      if (c.op == 'S') clip += c.len;
    size_t const len = SeqLen();
    double const frac = len > 0 ? static_cast<double>(clip) / static_cast<double>(len) : 0.0;
    return frac >= 0.06;
  }
  // the four facts of ma_read_meta_t (include/microasm.h): MAPQ is `mapq`; the MA_RM_* bits, the insert size, the start
  uint8_t MetaFlags() const { return static_cast<uint8_t>((IsSoftClipped() ? MA_RM_SOFTCLIP : 0) | (IsMappedProperPair() ? MA_RM_PROPER : 0)); }
  int32_t InsertSize32() const { return static_cast<int32_t>(std::max<int64_t>(INT32_MIN, std::min<int64_t>(INT32_MAX, tlen))); }
  int32_t Start32() const { return static_cast<int32_t>(std::max<int64_t>(0, std::min<int64_t>(INT32_MAX, pos0))); }
};

inline bool SamRecord::Md(std::string_view* out) const {
  if (is_raw && raw.size() > raw_core) {
    bool found = false, sa = false;
    WalkAuxFields(raw.data(), raw.size(), raw_core, out, &found, &sa);
    return found;
  }
  *out = md;
  return has_md;
}

inline std::vector<CigarUnit> ParseCigar(std::string_view s) {
  std::vector<CigarUnit> out;
  if (s == "*") return out;
  uint32_t n = 0;
  for (char c : s) {
    if (c >= '0' && c <= '9') {
      n = n * 10 + static_cast<uint32_t>(c - '0');
    } else {
      out.push_back({c, n});
      n = 0;
    }
  }
  return out;
}

#ifdef LANCET2_AMD_WITH_ZLIB
// ---- region-indexed BAM access without htslib: BGZF virtual offsets + the BAI index (SAM specification 4.1, 5.2) ---------
// What core/read_collector.cpp:106-204 gets from htslib's iterators: only the blocks that hold a region's records are read
// and inflated -- the whole file no longer has to fit in memory.
class BgzfFile {
 public:
  explicit BgzfFile(const std::string& path) : f_(std::fopen(path.c_str(), "rb")) {
    if (!f_) throw std::runtime_error("cannot open " + path);
  }
  ~BgzfFile() {
    if (f_) std::fclose(f_);
  }
  BgzfFile(BgzfFile const&) = delete;
  BgzfFile& operator=(BgzfFile const&) = delete;
  void Seek(uint64_t voff) {
    if (!have_ || (voff >> 16) != coff_) Load(voff >> 16);
    pos_ = static_cast<size_t>(voff & 0xFFFFu);
  }
  // virtual offset of the next byte Read() returns
  uint64_t Tell() {
    while (have_ && pos_ >= block_.size() && !eof_) Load(next_);
    return (coff_ << 16) | pos_;
  }
  bool Read(void* dst, size_t n) {
    auto* out = static_cast<unsigned char*>(dst);
    while (n > 0) {
      if (!have_) Load(0);
      while (pos_ >= block_.size()) {
        if (eof_) return false;
        Load(next_);
      }
      size_t const take = std::min(n, block_.size() - pos_);
      std::memcpy(out, block_.data() + pos_, take);
      out += take;
      pos_ += take;
      n -= take;
    }
    return true;
  }
  size_t blocks_inflated() const { return blocks_; }

 private:
  void Load(uint64_t coff) {
    have_ = true;
    coff_ = coff;
    pos_ = 0;
    block_.clear();
    unsigned char h[12];
    if (fseeko(f_, static_cast<off_t>(coff), SEEK_SET) != 0 || std::fread(h, 1, 12, f_) != 12) {
      eof_ = true;
      next_ = coff;
      return;
    }
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) throw std::runtime_error("not a BGZF block");
    size_t const xlen = h[10] | (static_cast<size_t>(h[11]) << 8);
    std::vector<unsigned char> extra(xlen);
    if (std::fread(extra.data(), 1, xlen, f_) != xlen) throw std::runtime_error("truncated BGZF block");
    size_t bsize = 0;
    for (size_t p = 0; p + 4 <= xlen;) {
      size_t const slen = extra[p + 2] | (static_cast<size_t>(extra[p + 3]) << 8);
      if (p + 4 + slen > xlen) throw std::runtime_error("corrupt BGZF block: extra subfield beyond the extra field");
      if (extra[p] == 'B' && extra[p + 1] == 'C' && slen == 2) bsize = (extra[p + 4] | (static_cast<size_t>(extra[p + 5]) << 8)) + 1;
      p += 4 + slen;
    }
    if (bsize < 12 + xlen + 8) throw std::runtime_error("BGZF block without a BC field");
    size_t const clen = bsize - 12 - xlen - 8;
    std::vector<unsigned char> cdata(clen + 8);
    if (std::fread(cdata.data(), 1, clen + 8, f_) != clen + 8) throw std::runtime_error("truncated BGZF block");
    uint32_t isize;
    std::memcpy(&isize, cdata.data() + clen + 4, 4);
    if (isize > 65536u) throw std::runtime_error("corrupt BGZF block: more than 64 KiB of payload");
    block_.resize(isize);
    if (isize > 0) {
      z_stream zs{};
      if (inflateInit2(&zs, -15) != Z_OK) throw std::runtime_error("zlib init failed");
      zs.next_in = cdata.data();
      zs.avail_in = static_cast<uInt>(clen);
      zs.next_out = block_.data();
      zs.avail_out = isize;
      int const rc = inflate(&zs, Z_FINISH);
      inflateEnd(&zs);
      if (rc != Z_STREAM_END) throw std::runtime_error("zlib inflate failed on a BGZF block");
    }
    next_ = coff + bsize;
    eof_ = false;
    ++blocks_;
  }
  FILE* f_ = nullptr;
  bool have_ = false, eof_ = false;
  uint64_t coff_ = 0, next_ = 0;
  std::vector<unsigned char> block_;
  size_t pos_ = 0, blocks_ = 0;
};

class BamIndex {  // .bai: per reference the binning index (bin -> chunks of virtual offsets) and the 16 kb linear index
 public:
  using Chunk = std::pair<uint64_t, uint64_t>;
  static BamIndex Load(const std::string& path) {
    std::ifstream in(path, std::ios::binary);
    if (!in) throw std::runtime_error("cannot open index " + path);
    std::vector<unsigned char> d((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    size_t at = 0;
    auto need = [&](size_t n) {
      if (at + n > d.size()) throw std::runtime_error("truncated BAI " + path);
    };
    auto rd32 = [&]() { need(4); int32_t v; std::memcpy(&v, d.data() + at, 4); at += 4; return v; };
    auto rdu32 = [&]() { need(4); uint32_t v; std::memcpy(&v, d.data() + at, 4); at += 4; return v; };
    auto rd64 = [&]() { need(8); uint64_t v; std::memcpy(&v, d.data() + at, 8); at += 8; return v; };
    need(4);
    if (std::memcmp(d.data(), "BAI\1", 4) != 0) throw std::runtime_error(path + " is not a BAI index");
    at = 4;
    BamIndex ix;
    int32_t const n_ref = rd32();
    ix.refs_.resize(static_cast<size_t>(n_ref));
    for (auto& r : ix.refs_) {
      int32_t const n_bin = rd32();
      for (int32_t b = 0; b < n_bin; ++b) {
        uint32_t const bin = rdu32();
        int32_t const n_chunk = rd32();
        auto& v = r.bins[bin];
        for (int32_t c = 0; c < n_chunk; ++c) {
          uint64_t const beg = rd64(), end = rd64();
          if (bin != 37450u) v.emplace_back(beg, end);  // (the pseudo-bin carries file statistics, not chunks)
        }
      }
      int32_t const n_intv = rd32();
      r.linear.resize(static_cast<size_t>(n_intv));
      for (auto& o : r.linear) o = rd64();
    }
    return ix;
  }
  // chunks that may hold records overlapping [beg0, end0) of reference rid, sorted, overlapping ones merged
  std::vector<Chunk> Query(int rid, int64_t beg0, int64_t end0) const {
    std::vector<Chunk> out;
    if (rid < 0 || static_cast<size_t>(rid) >= refs_.size() || end0 <= beg0) return out;
    Ref const& r = refs_[static_cast<size_t>(rid)];
    beg0 = std::max<int64_t>(beg0, 0);
    int64_t const e = end0 - 1;
    size_t const w = static_cast<size_t>(beg0 >> 14);
    uint64_t const min_off = r.linear.empty() ? 0 : r.linear[std::min(w, r.linear.size() - 1)];
    auto add = [&](uint32_t bin) {
      auto it = r.bins.find(bin);
      if (it == r.bins.end()) return;
      for (auto const& c : it->second)
        if (c.second > min_off) out.push_back(c);
    };
    add(0);
    for (int64_t k = 1 + (beg0 >> 26); k <= 1 + (e >> 26); ++k) add(static_cast<uint32_t>(k));
    for (int64_t k = 9 + (beg0 >> 23); k <= 9 + (e >> 23); ++k) add(static_cast<uint32_t>(k));
    for (int64_t k = 73 + (beg0 >> 20); k <= 73 + (e >> 20); ++k) add(static_cast<uint32_t>(k));
    for (int64_t k = 585 + (beg0 >> 17); k <= 585 + (e >> 17); ++k) add(static_cast<uint32_t>(k));
    for (int64_t k = 4681 + (beg0 >> 14); k <= 4681 + (e >> 14); ++k) add(static_cast<uint32_t>(k));
    std::sort(out.begin(), out.end());
    std::vector<Chunk> merged;
    for (auto const& c : out) {
      if (!merged.empty() && c.first <= merged.back().second) merged.back().second = std::max(merged.back().second, c.second);
      else merged.push_back(c);
    }
    return merged;
  }

 private:
  struct Ref {
    std::map<uint32_t, std::vector<Chunk>> bins;
    std::vector<uint64_t> linear;
  };
  std::vector<Ref> refs_;
};
#endif

// One sample's alignments, coordinate-sorted, in memory.  ForRegion visits the records that overlap chrom:start1-end1
// (1-based, closed -- the region syntax the reference hands to htslib), in file order.
class AlignmentSource {
 public:
  std::vector<SamRecord> recs;  // whole-file mode (SAM text, BAM without an index); empty in indexed mode

  void Finish(size_t n_chroms) {
    std::stable_sort(recs.begin(), recs.end(), [](SamRecord const& a, SamRecord const& b) {
      auto ka = a.chrom < 0 ? INT32_MAX : a.chrom, kb = b.chrom < 0 ? INT32_MAX : b.chrom;
      return ka != kb ? ka < kb : a.pos0 < b.pos0;
    });
    begin_.resize(n_chroms + 1);
    for (size_t c = 0; c <= n_chroms; ++c)
      begin_[c] = static_cast<size_t>(std::lower_bound(recs.begin(), recs.end(), static_cast<int32_t>(c),
                                                       [](SamRecord const& r, int32_t v) { return (r.chrom < 0 ? INT32_MAX : r.chrom) < v; }) -
                                      recs.begin());
    max_span_ = 1;
    for (auto const& r : recs) max_span_ = std::max(max_span_, r.RefSpan());
  }
  template <class F>
  void ForRegion(int chrom, int64_t start1, int64_t end1, F&& fn) const {
#ifdef LANCET2_AMD_WITH_ZLIB
    if (bgzf_) {  // indexed BAM: the index names the chunks, only their blocks are read; same records, same order
      if (chrom < 0 || static_cast<size_t>(chrom) >= chrom_rid_.size() || chrom_rid_[static_cast<size_t>(chrom)] < 0) return;
      int const rid = chrom_rid_[static_cast<size_t>(chrom)];
      int64_t const s0 = start1 - 1, e0 = end1;
      std::vector<unsigned char> buf;
      for (auto const& ck : index_->Query(rid, s0, e0)) {
        bgzf_->Seek(ck.first);
        bool done = false;
        while (!done && bgzf_->Tell() < ck.second) {
          int32_t block = 0;
          if (!bgzf_->Read(&block, 4) || block < 32) break;
          buf.resize(static_cast<size_t>(block));
          if (!bgzf_->Read(buf.data(), buf.size())) break;
          int32_t r_rid, r_pos;
          std::memcpy(&r_rid, buf.data(), 4);
          std::memcpy(&r_pos, buf.data() + 4, 4);
          if (r_rid != rid) {
            if (r_rid > rid || r_rid < 0) done = true;
            continue;
          }
          if (r_pos >= e0) {
            done = true;  // coordinate-sorted: nothing further in this chunk (or any later one) overlaps
            continue;
          }
          SamRecord rec = DecodeBamRecord(buf.data(), buf.size(), ref_map_, keep_packed_, keep_raw_, keep_tags_);
          if (rec.pos0 + rec.RefSpan() > s0) fn(rec);
        }
        if (done) break;
      }
      return;
    }
#endif
    if (chrom < 0 || static_cast<size_t>(chrom) + 1 >= begin_.size()) return;
    size_t const lo = begin_[static_cast<size_t>(chrom)], hi = begin_[static_cast<size_t>(chrom) + 1];
    int64_t const s0 = start1 - 1, e0 = end1;  // half-open [s0, e0)
    auto first = std::lower_bound(recs.begin() + static_cast<long>(lo), recs.begin() + static_cast<long>(hi), s0 - max_span_,
                                  [](SamRecord const& r, int64_t v) { return r.pos0 < v; });
    for (auto it = first; it != recs.begin() + static_cast<long>(hi) && it->pos0 < e0; ++it)
      if (it->pos0 + it->RefSpan() > s0) fn(*it);
  }

  static AlignmentSource LoadSam(const std::string& path, Reference const& ref) {
    std::ifstream in(path);
    if (!in) throw std::runtime_error("cannot open alignments " + path);
    AlignmentSource src;
    std::string line;
    while (std::getline(in, line)) {
      if (line.empty() || line[0] == '@') continue;
      std::vector<std::string_view> f;
      size_t p = 0;
      while (true) {
        size_t const t = line.find('\t', p);
        f.emplace_back(line.data() + p, (t == std::string::npos ? line.size() : t) - p);
        if (t == std::string::npos) break;
        p = t + 1;
      }
      if (f.size() < 11) continue;
      SamRecord r;
      r.qname = std::string(f[0]);
      r.flag = static_cast<uint16_t>(std::strtoul(std::string(f[1]).c_str(), nullptr, 10));
      r.chrom = f[2] == "*" ? -1 : ref.Find(f[2]);
      r.pos0 = std::strtoll(std::string(f[3]).c_str(), nullptr, 10) - 1;
      r.mapq = static_cast<uint8_t>(std::strtoul(std::string(f[4]).c_str(), nullptr, 10));
      r.cigar = ParseCigar(f[5]);
      r.mate_chrom = f[6] == "=" ? r.chrom : (f[6] == "*" ? -1 : ref.Find(f[6]));
      r.mate_pos0 = std::strtoll(std::string(f[7]).c_str(), nullptr, 10) - 1;
      r.tlen = std::strtoll(std::string(f[8]).c_str(), nullptr, 10);
      r.seq = f[9] == "*" ? std::string() : std::string(f[9]);
      if (f[10] != "*")
        for (char c : f[10]) r.qual.push_back(static_cast<uint8_t>(c - 33));
      else
        r.qual.assign(r.seq.size(), 0xFF);
      // (SAM spec: QUAL is '*' or as long as SEQ.  Everything downstream sizes the quality array by SEQ -- a longer QUAL would
      //  be written past it -- so a record that breaks the rule ends the run like a corrupt BAM record does)
      if (r.qual.size() != r.seq.size()) throw std::runtime_error("corrupt SAM record: QUAL and SEQ differ in length (" + r.qname + ")");
      for (size_t i = 11; i < f.size(); ++i) {
        if (f[i].substr(0, 5) == "MD:Z:") {
          r.md = std::string(f[i].substr(5));
          r.has_md = true;
        } else if (f[i].substr(0, 5) == "SA:Z:") {
          r.has_sa = true;
        }
      }
      src.recs.push_back(std::move(r));
    }
    src.Finish(ref.chroms.size());
    return src;
  }

  // one BAM alignment record (SAM specification 4.2; `b` points behind its block_size field)
  // keep_packed: the sequence stays as the file has it (SamRecord::seq4: 4-bit codes, high nibble first), `seq` stays empty
  // keep_raw: SamRecord's raw mode -- the core bytes in one vector, no name string, no CIGAR vector, no decoded sequence
  // keep_tags (with keep_raw): the whole block is kept and its auxiliary fields are not walked (SamRecord::Md does, on demand)
  static SamRecord DecodeBamRecord(const unsigned char* b, size_t block, std::vector<int> const& ref_map, bool keep_packed = false,
                                   bool keep_raw = false, bool keep_tags = false) {
    static const char* kSeq = "=ACMGRSVTWYHKDBN";
    static const char* kOps = "MIDNSHP=X";
    auto rd32 = [&](size_t at) { int32_t v; std::memcpy(&v, b + at, 4); return v; };
    int32_t const n_ref = static_cast<int32_t>(ref_map.size());
    SamRecord r;
    int32_t const rid = rd32(0), pos = rd32(4);
    uint8_t const l_read_name = b[8];
    r.mapq = b[9];
    uint16_t n_cigar, flag;
    std::memcpy(&n_cigar, b + 12, 2);
    std::memcpy(&flag, b + 14, 2);
    int32_t const l_seq = rd32(16), mrid = rd32(20), mpos = rd32(24), tlen = rd32(28);
    r.flag = flag;
    r.chrom = rid >= 0 && rid < n_ref ? ref_map[static_cast<size_t>(rid)] : -1;
    r.pos0 = pos;
    r.mate_chrom = mrid >= 0 && mrid < n_ref ? ref_map[static_cast<size_t>(mrid)] : -1;
    r.mate_pos0 = mpos;
    r.tlen = tlen;
    size_t p = 32;
    // every length comes from the file: a truncated or corrupt record must not send the decoder past its block
    if (block < 32 || l_seq < 0 ||
        32 + static_cast<size_t>(l_read_name) + 4u * static_cast<size_t>(n_cigar) + (static_cast<size_t>(l_seq) + 1) / 2 + static_cast<size_t>(l_seq) > block)
      throw std::runtime_error("corrupt BAM record: its fields do not fit its block");
    size_t const core = 32 + static_cast<size_t>(l_read_name) + 4u * static_cast<size_t>(n_cigar) + (static_cast<size_t>(l_seq) + 1) / 2 + static_cast<size_t>(l_seq);
    if (keep_raw) {  // the core bytes as they are, and the two scalars the collector needs of them
      r.raw.assign(b, b + (keep_tags ? block : core));
      r.raw_core = static_cast<uint32_t>(core);
      r.is_raw = r.packed = true;
      r.l_seq4 = static_cast<uint32_t>(l_seq);
      r.raw_qh = HashQname(std::string_view(reinterpret_cast<const char*>(b + p), l_read_name ? l_read_name - 1u : 0u));
      int64_t span = 0;
      for (size_t c = 0; c < n_cigar; ++c) {
        CigarUnit const u = r.Cigar(c);
        if (u.ConsumesReference()) span += u.len;
      }
      r.raw_span = span > 0 ? span : 1;
    } else {
      r.qname.assign(reinterpret_cast<const char*>(b + p), l_read_name ? l_read_name - 1u : 0u);
      p += l_read_name;
      for (uint16_t c = 0; c < n_cigar; ++c) {
        uint32_t v;
        std::memcpy(&v, b + p + 4u * c, 4);
        r.cigar.push_back({(v & 15u) < 9 ? kOps[v & 15u] : '?', v >> 4});
      }
      p += 4u * n_cigar;
      if (keep_packed) {  // copied, not decoded: the engine takes BAM's codes (ma_packed_reads_t)
        r.seq4.assign(b + p, b + p + (static_cast<size_t>(l_seq) + 1) / 2);
        r.l_seq4 = static_cast<uint32_t>(l_seq);
        r.packed = true;
      } else {
        r.seq.resize(static_cast<size_t>(l_seq));
        for (int32_t i = 0; i < l_seq; ++i) r.seq[static_cast<size_t>(i)] = kSeq[(b[p + static_cast<size_t>(i) / 2] >> (i % 2 ? 0 : 4)) & 15];
      }
      p += static_cast<size_t>(l_seq + 1) / 2;
      r.qual.assign(b + p, b + p + l_seq);
    }
    if (keep_raw && keep_tags) return r;
    std::string_view md_view;  // the auxiliary fields follow the core in either mode
    WalkAuxFields(b, block, core, &md_view, &r.has_md, &r.has_sa);
    if (r.has_md) r.md.assign(md_view);
    return r;
  }

#ifdef LANCET2_AMD_WITH_ZLIB
  // BAM: BGZF blocks are gzip members; the payload is the BAM record stream of the SAM specification, section 4.2
  static AlignmentSource LoadBam(const std::string& path, Reference const& ref, bool keep_packed = false, bool keep_raw = false,
                                 bool keep_tags = false) {
    std::ifstream in(path, std::ios::binary);
    if (!in) throw std::runtime_error("cannot open alignments " + path);
    std::vector<unsigned char> comp((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::vector<unsigned char> raw;
    z_stream zs{};
    if (inflateInit2(&zs, 31) != Z_OK) throw std::runtime_error("zlib init failed");
    zs.next_in = comp.data();
    zs.avail_in = static_cast<uInt>(comp.size());
    std::vector<unsigned char> chunk(1 << 16);
    while (zs.avail_in > 0) {
      zs.next_out = chunk.data();
      zs.avail_out = static_cast<uInt>(chunk.size());
      int const rc = inflate(&zs, Z_NO_FLUSH);
      raw.insert(raw.end(), chunk.data(), chunk.data() + (chunk.size() - zs.avail_out));
      if (rc == Z_STREAM_END) {
        if (zs.avail_in == 0) break;
        inflateReset(&zs);  // next BGZF block
      } else if (rc != Z_OK) {
        inflateEnd(&zs);
        throw std::runtime_error("zlib inflate failed on " + path);
      }
    }
    inflateEnd(&zs);
    auto rd32 = [&](size_t at) { int32_t v; std::memcpy(&v, raw.data() + at, 4); return v; };
    if (raw.size() < 12 || std::memcmp(raw.data(), "BAM\1", 4) != 0) throw std::runtime_error(path + " is not a BAM file");
    size_t at = 4;
    int32_t const l_text = rd32(at);
    at += 4 + static_cast<size_t>(l_text);
    int32_t const n_ref = rd32(at);
    at += 4;
    std::vector<int> ref_map(static_cast<size_t>(n_ref), -1);
    for (int32_t i = 0; i < n_ref; ++i) {
      int32_t const l_name = rd32(at);
      at += 4;
      ref_map[static_cast<size_t>(i)] = ref.Find(std::string_view(reinterpret_cast<const char*>(raw.data() + at), static_cast<size_t>(l_name - 1)));
      at += static_cast<size_t>(l_name) + 4;
    }
    AlignmentSource src;
    while (at + 4 <= raw.size()) {
      int32_t const block = rd32(at);
      size_t const b = at + 4;
      at = b + static_cast<size_t>(block);
      if (at > raw.size()) break;
      src.recs.push_back(DecodeBamRecord(raw.data() + b, static_cast<size_t>(block), ref_map, keep_packed, keep_raw, keep_tags));
    }
    src.ref_map_ = ref_map;
    src.Finish(ref.chroms.size());
    return src;
  }
  // BAM + .bai: header only; records are fetched per region (ForRegion)
  static AlignmentSource OpenIndexedBam(const std::string& path, const std::string& bai_path, Reference const& ref, bool keep_packed = false,
                                        bool keep_raw = false, bool keep_tags = false) {
    AlignmentSource src;
    src.keep_packed_ = keep_packed;
    src.keep_raw_ = keep_raw;
    src.keep_tags_ = keep_tags;
    src.index_ = std::make_shared<BamIndex>(BamIndex::Load(bai_path));
    src.path_ = path;
    src.bgzf_ = std::make_shared<BgzfFile>(path);
    BgzfFile& f = *src.bgzf_;
    char magic[4];
    int32_t l_text = 0, n_ref = 0;
    if (!f.Read(magic, 4) || std::memcmp(magic, "BAM\1", 4) != 0 || !f.Read(&l_text, 4)) throw std::runtime_error(path + " is not a BAM file");
    std::vector<char> text(static_cast<size_t>(l_text));
    if (l_text > 0 && !f.Read(text.data(), text.size())) throw std::runtime_error("truncated BAM header in " + path);
    if (!f.Read(&n_ref, 4)) throw std::runtime_error("truncated BAM header in " + path);
    src.ref_map_.assign(static_cast<size_t>(n_ref), -1);
    src.chrom_rid_.assign(ref.chroms.size(), -1);
    for (int32_t i = 0; i < n_ref; ++i) {
      int32_t l_name = 0, l_ref = 0;
      if (!f.Read(&l_name, 4)) throw std::runtime_error("truncated BAM header in " + path);
      std::string name(static_cast<size_t>(l_name), '\0');
      if (!f.Read(name.data(), name.size()) || !f.Read(&l_ref, 4)) throw std::runtime_error("truncated BAM header in " + path);
      if (!name.empty() && name.back() == '\0') name.pop_back();
      int const c = ref.Find(name);
      src.ref_map_[static_cast<size_t>(i)] = c;
      if (c >= 0) src.chrom_rid_[static_cast<size_t>(c)] = i;
    }
    return src;
  }
  // a second handle on the same indexed file for another extract thread (the BGZF reader is stateful; the index is shared)
  AlignmentSource CloneIndexed() const {
    AlignmentSource c;
    c.index_ = index_;
    c.path_ = path_;
    c.bgzf_ = std::make_shared<BgzfFile>(path_);
    c.ref_map_ = ref_map_;
    c.chrom_rid_ = chrom_rid_;
    c.keep_packed_ = keep_packed_;
    c.keep_raw_ = keep_raw_;
    c.keep_tags_ = keep_tags_;
    return c;
  }
  bool indexed() const { return bgzf_ != nullptr; }
  std::vector<int> const& RefMap() const { return ref_map_; }  // BAM reference id -> chromosome of the FASTA
  size_t blocks_inflated() const { return bgzf_ ? bgzf_->blocks_inflated() : 0; }
#endif

 private:
  std::vector<size_t> begin_;
  int64_t max_span_ = 1;
#ifdef LANCET2_AMD_WITH_ZLIB
  std::shared_ptr<BgzfFile> bgzf_;
  std::shared_ptr<BamIndex> index_;
  std::string path_;
  std::vector<int> ref_map_;    // BAM reference id -> chromosome of the FASTA (-1: not in it)
  std::vector<int> chrom_rid_;  // and back
  bool keep_raw_ = false;       // --raw-records: SamRecord's raw mode
  bool keep_tags_ = false;      // ... with the whole block kept (the candidates of ma_select_records_batch)
  bool keep_packed_ = false;    // --packed-reads: records keep their sequence bytes undecoded (for ReadCollector::Params::packed_reads)
#endif
};

// ---- windows -----------------------------------------------------------------------------------------------------------
struct RegionSpec {  // hts::Reference::ParseRegionResult: 1-based closed, either end optional
  std::string chrom;
  std::optional<uint64_t> start, end;
  uint64_t Length() const { return (start && end && *end >= *start) ? *end - *start + 1 : 0; }
  static RegionSpec Parse(const std::string& spec) {  // "chr", "chr:100-200", "chr:100"
    RegionSpec r;
    size_t const colon = spec.rfind(':');
    if (colon == std::string::npos) {
      r.chrom = spec;
      return r;
    }
    r.chrom = spec.substr(0, colon);
    std::string const rest = spec.substr(colon + 1);
    size_t const dash = rest.find('-');
    auto num = [](std::string s) {
      s.erase(std::remove(s.begin(), s.end(), ','), s.end());
      return static_cast<uint64_t>(std::strtoull(s.c_str(), nullptr, 10));
    };
    r.start = num(rest.substr(0, dash));
    if (dash != std::string::npos && dash + 1 < rest.size()) r.end = num(rest.substr(dash + 1));
    return r;
  }
};

struct Window {
  int chrom = -1;
  uint64_t start1 = 0, end1 = 0;  // 1-based closed: a 1000-base step yields 1001-base windows, as in the reference
  size_t genome_index = 0;
  uint64_t Length() const { return end1 - start1 + 1; }
};

// core/bed_parser.cpp:27-96: exactly three tab-separated columns per line, '#' lines and empty lines skipped, the chromosome must
// be in the reference; the two numbers go into the region span AS THEY ARE (the reference does not shift BED's 0-based start)
inline std::vector<RegionSpec> ParseBedFile(const std::string& path, std::function<bool(std::string const&)> const& chrom_known) {
  std::ifstream in(path);
  if (!in) throw std::runtime_error("Could not open bed file: " + path);
  std::vector<RegionSpec> out;
  std::string line;
  size_t line_num = 0;
  while (std::getline(in, line)) {
    line_num++;
    if (line.empty() || line[0] == '#') continue;
    std::vector<std::string> tok;
    size_t p = 0;
    while (true) {
      size_t const t = line.find('\t', p);
      tok.push_back(line.substr(p, t == std::string::npos ? std::string::npos : t - p));
      if (t == std::string::npos) break;
      p = t + 1;
    }
    if (tok.size() != 3) throw std::runtime_error("Invalid bed line with " + std::to_string(tok.size()) + " columns at line number " + std::to_string(line_num));
    char *e1 = nullptr, *e2 = nullptr;
    long long const a = std::strtoll(tok[1].c_str(), &e1, 10), b = std::strtoll(tok[2].c_str(), &e2, 10);
    if (tok[1].empty() || tok[2].empty() || *e1 != '\0' || *e2 != '\0') throw std::runtime_error("Could not parse line " + std::to_string(line_num) + " in bed: " + path);
    if (!chrom_known(tok[0])) throw std::runtime_error("Could not find chrom " + tok[0] + " from bed file line " + std::to_string(line_num) + " in reference");
    RegionSpec r;
    r.chrom = tok[0];
    r.start = static_cast<uint64_t>(a);
    r.end = static_cast<uint64_t>(b);
    out.push_back(r);
  }
  return out;
}

class WindowBuilder {
 public:
  struct Params {  // core/window_builder.h:19-38
    uint32_t window_length = 1000, region_padding = 500, percent_overlap = 20;
  };
  WindowBuilder(Reference const* ref, Params p) : ref_(ref), prm_(p) {}
  void AddRegion(const std::string& spec) { regions_.push_back(RegionSpec::Parse(spec)); }
  void AddRegion(RegionSpec const& r) { regions_.push_back(r); }  // (a BED line: core/window_builder.cpp:70-74)
  static bool ShouldExcludeChrom(std::string_view c) {  // window_builder.cpp:41-53
    auto starts = [&](std::string_view p) { return c.substr(0, p.size()) == p; };
    auto ends = [&](std::string_view s) { return c.size() >= s.size() && c.substr(c.size() - s.size()) == s; };
    return c == "MT" || c == "chrM" || starts("GL") || starts("chrUn") || starts("chrEBV") || starts("HLA-") ||
           ends("_random") || ends("_alt") || ends("_decoy");
  }
  void AddAllReferenceRegions() {
    for (auto const& c : ref_->chroms)
      if (!ShouldExcludeChrom(c.name)) regions_.push_back(RegionSpec{c.name, 1, c.seq.size()});
  }
  static int64_t StepSize(Params const& p) {  // window_builder.cpp:86-91: steps move in multiples of 100
    double const val = (static_cast<double>(100 - p.percent_overlap) / 100.0) * static_cast<double>(p.window_length);
    return static_cast<int64_t>(std::ceil(val / 100.0) * 100.0);
  }
  void PadInputRegion(RegionSpec& r) const {  // window_builder.cpp:287-323
    int const ci = ref_->Find(r.chrom);
    if (ci < 0) throw std::runtime_error("No chromosome named " + r.chrom + " found in reference");
    uint64_t const contig_max_len = ref_->chroms[static_cast<size_t>(ci)].seq.size();
    uint64_t const curr_start = r.start.value_or(1), curr_end = r.end.value_or(contig_max_len);
    bool const start_underflows = curr_start <= prm_.region_padding;
    bool const end_overflows = (curr_end > contig_max_len) || ((contig_max_len - curr_end) <= prm_.region_padding);
    r.start = start_underflows ? 1 : curr_start - prm_.region_padding;
    r.end = end_overflows ? contig_max_len : curr_end + prm_.region_padding;
    if (r.Length() < prm_.window_length) {
      uint64_t const diff = static_cast<uint64_t>(std::llabs(static_cast<int64_t>(r.Length()) - static_cast<int64_t>(prm_.window_length) - 1));
      uint64_t const curr_left = *r.start, curr_right = *r.end;
      uint64_t const left_new_val = (diff / 2) > curr_left ? curr_left - 1 : curr_left - (diff / 2);
      uint64_t const left_flank = curr_left - left_new_val;
      bool const goes_overmax = curr_right + (diff - left_flank) > contig_max_len;
      r.start = curr_left - left_flank;
      r.end = goes_overmax ? contig_max_len : curr_right + (diff - left_flank);
    }
  }
  // window_builder.cpp:140-205: tile every padded region, de-duplicate, sort by (chrom, start, end), number
  std::vector<Window> BuildWindows() const {
    int64_t const window_len = prm_.window_length, step = StepSize(prm_);
    std::vector<Window> out;
    for (RegionSpec region : regions_) {
      PadInputRegion(region);
      int const ci = ref_->Find(region.chrom);
      if (static_cast<int64_t>(region.Length()) <= window_len) {
        out.push_back({ci, *region.start, *region.end, 0});
        continue;
      }
      int64_t cur = static_cast<int64_t>(*region.start);
      int64_t const max_pos = static_cast<int64_t>(*region.end);
      while (cur + window_len <= max_pos) {
        out.push_back({ci, static_cast<uint64_t>(cur), static_cast<uint64_t>(cur + window_len), 0});
        cur += step;
      }
    }
    auto key = [](Window const& w) { return std::make_tuple(w.chrom, w.start1, w.end1); };
    std::sort(out.begin(), out.end(), [&](Window const& a, Window const& b) { return key(a) < key(b); });
    out.erase(std::unique(out.begin(), out.end(), [&](Window const& a, Window const& b) { return key(a) == key(b); }), out.end());
    for (size_t i = 0; i < out.size(); ++i) out[i].genome_index = i;
    return out;
  }

 private:
  Reference const* ref_;
  Params prm_;
  std::vector<RegionSpec> regions_;
};

// ---- samples and reads -------------------------------------------------------------------------------------------------
enum class Tag : uint8_t { CTRL = 2, CASE = 4 };  // cbdg/label.h:13
struct SampleInfo {
  std::string name;
  Tag tag = Tag::CTRL;
  const AlignmentSource* source = nullptr;
  size_t index = 0;           // position in the (tag, name)-sorted sample list (core/sample_info.h:50-54)
  uint64_t sampled_reads = 0, sampled_bases = 0;
};
inline void SortSamples(std::vector<SampleInfo>& s) {
  std::sort(s.begin(), s.end(), [](SampleInfo const& a, SampleInfo const& b) {
    return a.tag != b.tag ? static_cast<uint8_t>(a.tag) < static_cast<uint8_t>(b.tag) : a.name < b.name;
  });
  for (size_t i = 0; i < s.size(); ++i) s[i].index = i;
}

struct Read {  // cbdg/read.h:22-60
  std::string qname, seq, sample_name;
  std::vector<uint8_t> qual;
  int64_t start0 = 0;
  int32_t chrom = -1;
  uint16_t flag = 0;
  uint8_t mapq = 0;
  Tag tag = Tag::CTRL;
  size_t sample_index = 0;
  uint32_t leading_clip = 0;
  bool passes = true;
  uint8_t mflags = 0;   // MA_RM_* (SamRecord::MetaFlags)
  int32_t isize = 0;    // InsertSize(): tlen
  Read() = default;
  Read(SamRecord const& a, std::string sname, Tag t, size_t sidx)
      : qname(a.qname), seq(a.seq), sample_name(std::move(sname)), qual(a.qual), start0(a.pos0), chrom(a.chrom),
        flag(a.flag), mapq(a.mapq), tag(t), sample_index(sidx), leading_clip(a.LeadingSoftClip()), passes(a.mapq >= 20),
        mflags(a.MetaFlags()), isize(a.InsertSize32()) {}
};

// read_collector.cpp:42-53: filter-pass status > sample tag > sample name > qname > chrom > position
inline bool CompareReadsByPriority(Read const& l, Read const& r) {
  if (l.passes != r.passes) return static_cast<int>(l.passes) > static_cast<int>(r.passes);
  if (l.tag != r.tag) return static_cast<uint8_t>(l.tag) < static_cast<uint8_t>(r.tag);
  if (l.sample_name != r.sample_name) return l.sample_name < r.sample_name;
  if (l.qname != r.qname) return l.qname < r.qname;
  if (l.chrom != r.chrom) return l.chrom < r.chrom;
  return l.start0 < r.start0;
}

// ---- active region detection (core/active_region_detector.cpp:85-232) ----------------------------------------------------
using CountMap = std::unordered_map<uint32_t, uint32_t>;
inline bool ParseMd(std::string_view md, const uint8_t* quals, size_t n_quals, int64_t start, CountMap* result) {
  if (start < 0) return false;
  std::string token;
  uint32_t genome_pos = static_cast<uint32_t>(start);
  for (char ch : md) {
    if (ch >= '0' && ch <= '9') {
      token += ch;
      continue;
    }
    long const step = token.empty() ? 0 : std::strtol(token.c_str(), nullptr, 10);
    genome_pos += static_cast<uint32_t>(step);
    token.clear();
    size_t const base_pos = static_cast<size_t>(genome_pos - start);
    if (base_pos >= n_quals) throw std::out_of_range("MD tag walks past the read");  // quals.at() in the reference
    if (quals[base_pos] < 20) continue;
    char const base = static_cast<char>(std::toupper(static_cast<unsigned char>(ch)));
    if (base == 'A' || base == 'C' || base == 'T' || base == 'G') {
      if (++(*result)[genome_pos] == 2) return true;
    }
  }
  return false;
}
inline bool ParseMd(std::string_view md, std::vector<uint8_t> const& quals, int64_t start, CountMap* result) {
  return ParseMd(md, quals.data(), quals.size(), start, result);
}
struct MutationAccumulator {
  CountMap mismatches, insertions, deletions, softclips;
  void ClearAll() {
    mismatches.clear();
    insertions.clear();
    deletions.clear();
    softclips.clear();
  }
  bool CheckAlignment(SamRecord const& a) {
    if (a.IsQcFail() || a.IsDuplicate() || a.IsUnmapped() || a.mapq == 0) return false;
    std::string_view md;
    if (a.Md(&md) && ParseMd(md, a.QualData(), a.QualSize(), a.pos0, &mismatches)) return true;
    uint32_t gpos = static_cast<uint32_t>(a.pos0);
    size_t const n_ops = a.NumCigar();  // (a raw-mode record: the CIGAR words of its bytes)
    for (size_t k = 0; k < n_ops; ++k) {
      CigarUnit const c = a.Cigar(k);
      if (c.ConsumesReference()) gpos += c.len;
      if (c.op == 'I' && ++insertions[gpos] == 2) return true;
      if (c.op == 'D' && ++deletions[gpos] == 2) return true;
      if (c.op == 'X' && ++mismatches[gpos] == 2) return true;
    }
    // soft clips: genome position of every clip (hts/alignment.cpp:288-361, use_padded = false)
    uint32_t ref_position = static_cast<uint32_t>(a.pos0);
    bool any = false;
    for (size_t k = 0; k < n_ops; ++k) {
      CigarUnit const c = a.Cigar(k);
      if (c.op == 'D' || c.op == 'M' || c.op == 'X' || c.op == 'N' || c.op == '=') ref_position += c.len;
      if (c.op == 'S' && ++softclips[ref_position] == 2) any = true;
    }
    return any;
  }
};
inline bool IsActiveRegion(std::vector<SampleInfo> const& samples, Window const& w) {
  MutationAccumulator acc;
  for (auto const& s : samples) {
    acc.ClearAll();
    bool hit = false;
    s.source->ForRegion(w.chrom, static_cast<int64_t>(w.start1), static_cast<int64_t>(w.end1), [&](SamRecord const& a) {
      if (!hit && acc.CheckAlignment(a)) hit = true;
    });
    if (hit) return true;
  }
  return false;
}

// ---- read collection (core/read_collector.cpp:106-309) -------------------------------------------------------------------
class ReadCollector {
 public:
  struct Params {
    double max_sample_cov = 1000.0;  // core/read_collector.h:27
    bool extract_pairs = false;
    bool raw_records = false;   // the sources are in raw mode: CollectRaw instead of CollectFlat
    bool packed_reads = false;  // CollectFlat emits the read bases as 4-bit codes (FlatBatch::seq4) instead of letters
  };
  struct Result {
    std::vector<Read> reads;
    std::vector<SampleInfo> samples;
  };
  ReadCollector(Params p, std::vector<SampleInfo> samples) : prm_(p), samples_(std::move(samples)) { SortSamples(samples_); }
  std::vector<SampleInfo> const& Samples() const { return samples_; }

  static bool Filtered(SamRecord const& a) { return a.IsQcFail() || a.IsDuplicate() || a.IsUnmapped() || a.mapq < 20; }

  Result CollectRegion(Window const& w) {
    std::vector<Read> out;
    double const max_sample_bases = prm_.max_sample_cov * static_cast<double>(w.Length());
    int64_t const s1 = static_cast<int64_t>(w.start1), e1 = static_cast<int64_t>(w.end1);
    for (auto& sinfo : samples_) {
      // pass 1: profile + downsample by qname, fixed seed (read_collector.cpp:147-216)
      uint64_t n_reads = 0, n_bases = 0;
      std::vector<uint64_t> hashes;
      std::unordered_map<uint64_t, std::pair<int32_t, int64_t>> expected_mates;
      std::unordered_set<uint64_t> seen;
      sinfo.source->ForRegion(w.chrom, s1, e1, [&](SamRecord const& a) {
        if (Filtered(a)) return;
        uint64_t const qh = HashQname(a.qname);
        n_reads += 1;
        n_bases += a.seq.size();
        hashes.push_back(qh);
        if (!prm_.extract_pairs) return;
        if (seen.count(qh)) {
          expected_mates.erase(qh);
          return;
        }
        seen.insert(qh);
        if (a.IsMateMapped() && (!a.IsMappedProperPair() || a.has_sa)) expected_mates.emplace(qh, std::make_pair(a.mate_chrom, a.mate_pos0));
      });
      double const bases_per_read = static_cast<double>(n_bases) / static_cast<double>(std::max<uint64_t>(n_reads, 1));
      uint64_t const max_reads = static_cast<uint64_t>(std::ceil(max_sample_bases / bases_per_read));
      uint64_t const sampled = std::min(n_reads, max_reads);
      std::shuffle(hashes.begin(), hashes.end(), std::mt19937_64{0});
      std::unordered_set<uint64_t> keep(hashes.begin(), hashes.begin() + static_cast<long>(sampled));
      // pass 2: deep copy of the kept reads
      uint64_t bases = 0;
      sinfo.source->ForRegion(w.chrom, s1, e1, [&](SamRecord const& a) {
        if (Filtered(a) || !keep.count(HashQname(a.qname))) return;
        out.emplace_back(a, sinfo.name, sinfo.tag, sinfo.index);
        bases += out.back().seq.size();
      });
      // pass 3: out-of-region mates of kept reads, ascending genomic order (read_collector.cpp:236-271)
      if (prm_.extract_pairs && !expected_mates.empty()) {
        for (auto it = expected_mates.begin(); it != expected_mates.end();) it = keep.count(it->first) ? std::next(it) : expected_mates.erase(it);
        std::vector<std::pair<uint64_t, std::pair<int32_t, int64_t>>> order(expected_mates.begin(), expected_mates.end());
        std::sort(order.begin(), order.end(), [](auto const& a, auto const& b) { return a.second < b.second; });
        for (auto const& [qh, loc] : order) {
          if (!expected_mates.count(qh)) continue;
          sinfo.source->ForRegion(loc.first, loc.second + 1, loc.second + 1, [&](SamRecord const& a) {
            auto const itr = expected_mates.find(HashQname(a.qname));
            if (itr == expected_mates.end()) return;
            out.emplace_back(a, sinfo.name, sinfo.tag, sinfo.index);
            bases += out.back().seq.size();
            expected_mates.erase(itr);
          });
        }
      }
      sinfo.sampled_reads = sampled;
      sinfo.sampled_bases = bases;
    }
    std::stable_sort(out.begin(), out.end(), CompareReadsByPriority);  // (ties -- the reference's std::sort leaves them unspecified -- in arrival order)
    return {std::move(out), samples_};
  }

  // The same window, flattened straight into `out` (what CollectRegion + FlatBatch::Add append), without materialising a Read
  // per alignment: the kept alignments are REFERENCES to the source's records (whole-file sources; an indexed source's records
  // are copied once into a per-call arena), sorted as references, and every output array is sized before it is filled.  The
  // reference-shaped path above costs ~3000 allocations per 60x/30x window (three strings and a vector per read, the hash
  // sets of both passes) and was what bounded the extract stage at ~0.5 ms of one core per window; tests/host/host_units.cpp
  // holds the two paths to byte-identical batches.  Returns false when the window's options need the general path
  // (extract_pairs: out-of-region mates).
  bool CollectFlat(Window const& w, std::string_view ref_seq, struct FlatBatch* out);
  // The same window for ma_flatten_records_batch (include/microasm.h): the same filters and the same seeded downsampling, but
  // no sort, no interning and no per-read arrays -- `out` gets the window's scalars, its reference bases and the kept records'
  // core bytes back to back in arrival order (FlatBatch::raw_blob: copied from the records) with their lengths and samples.  The sources must
  // be in raw mode (SamRecord::is_raw); returns false otherwise, and when the options need the general path (extract_pairs).
  bool CollectRaw(Window const& w, std::string_view ref_seq, struct FlatBatch* out);
  // The window's CANDIDATES for ma_select_records_batch (include/microasm.h): every record ForRegion visits, sample after
  // sample in arrival order, unfiltered, its whole block (the sources keep their tags: keep_tags) -- nothing is looked at here
  // but the lengths.  `out` is a raw_mode batch with cand_mode set; its read_off counts the candidates' bases, an upper bound
  // of what the selected ones hold.  Returns false when the sources are not in raw mode.
  bool CollectCandidates(Window const& w, std::string_view ref_seq, struct FlatBatch* out);
  struct Kept {
    const SamRecord* rec;
    uint64_t qh;
    uint32_t sample;  // position in samples_
    uint32_t order;   // arrival order
  };
  size_t SelectKept(Window const& w, std::vector<Kept>* kept, std::deque<SamRecord>* arena);

 private:
  Params prm_;
  std::vector<SampleInfo> samples_;
};

// ---- skip gates (core/variant_builder.cpp:107-132, :214-224) ---------------------------------------------------------------
enum class WindowStatus { RUN, SKIPPED_NONLY_REF_BASES, SKIPPED_REF_REPEAT_SEEN, SKIPPED_INACTIVE_REGION, SKIPPED_ANCHOR_COVERAGE };
inline bool HasExactRepeat(std::string_view seq, size_t k) {  // base::HasExactRepeat(SlidingView(seq, k))
  if (seq.size() < k) return false;
  std::unordered_set<std::string_view> seen;
  for (size_t i = 0; i + k <= seq.size(); ++i)
    if (!seen.insert(seq.substr(i, k)).second) return true;
  return false;
}
inline WindowStatus PreReadGate(std::string_view ref_seq, int max_k, bool skip_active_region, std::vector<SampleInfo> const& samples,
                                Window const& w) {
  if (std::all_of(ref_seq.begin(), ref_seq.end(), [](char b) { return b == 'N'; })) return WindowStatus::SKIPPED_NONLY_REF_BASES;
  if (HasExactRepeat(ref_seq, static_cast<size_t>(max_k))) return WindowStatus::SKIPPED_REF_REPEAT_SEEN;
  if (!skip_active_region && !IsActiveRegion(samples, w)) return WindowStatus::SKIPPED_INACTIVE_REGION;
  return WindowStatus::RUN;
}
inline double CrossSampleMeanCoverage(std::vector<SampleInfo> const& samples, uint64_t window_length) {  // core/sample_info.h:40-48
  uint64_t total = 0;
  for (auto const& s : samples) total += s.sampled_bases;
  return static_cast<double>(total) / static_cast<double>(window_length);
}

// ---- Flatten: windows + collected reads -> ma_batch_t ------------------------------------------------------------------------
// A vector whose resize() does not zero what it adds: the big byte arrays (100-200 KB per window, 400 MB per batch) are sized
// first and filled right after -- value-initialising them was a memset of every byte in front of the memcpy that overwrites it.
template <class T>
struct NoInitAlloc : std::allocator<T> {
  template <class U>
  struct rebind { using other = NoInitAlloc<U>; };
  NoInitAlloc() = default;
  template <class U>
  NoInitAlloc(NoInitAlloc<U> const&) {}
  template <class U, class... A>
  void construct(U* p_, A&&... a) {
    if constexpr (sizeof...(A) == 0) ::new (static_cast<void*>(p_)) U;
    else ::new (static_cast<void*>(p_)) U(std::forward<A>(a)...);
  }
};
#ifdef MA_BYTEVEC_STD  // (A/B knob of tools/dbg/extract_ab.py)
using ByteVec = std::vector<uint8_t>;
#else
using ByteVec = std::vector<uint8_t, NoInitAlloc<uint8_t>>;
#endif
// BAM's 4-bit code of a base letter; a letter that is none of "=ACMGRSVTWYHKDBN" (lower case included) is N, as in a BAM file
inline uint8_t BaseCode4(uint8_t letter) {
  static const std::array<uint8_t, 256> code_of = [] {
    std::array<uint8_t, 256> t{};
    t.fill(15);
    const char* letters = "=ACMGRSVTWYHKDBN";
    for (int i = 0; i < 16; ++i) t[static_cast<uint8_t>(letters[i])] = static_cast<uint8_t>(i);
    return t;
  }();
  return code_of[letter];
}
struct FlatBatch {
  ByteVec ref_bases, read_bases, read_quals;
  // packed_mode (ReadCollector::Params::packed_reads): read_bases stays empty.  A one-window batch of CollectFlat holds its
  // reads' 4-bit sequence bytes back to back in seq4 (read i: [seq4_off[i], seq4_off[i + 1]), (len + 1) / 2 bytes -- a BAM
  // record's own bytes, SAM text packed); CopyPlaced() copies each to its place in the batch's nibble array, bases4: byte
  // (read_off[r] + r) >> 1 (include/microasm.h: ma_packed_reads_t).  Add() and Append() work on letters and refuse such a batch.
  bool packed_mode = false;
  // raw_mode (ReadCollector::Params::raw_records, --raw-records): the batch is the INPUT of ma_flatten_records_batch
  // (include/microasm.h: ma_records_t) -- the kept records' core bytes in raw_blob, window after window in arrival order, with
  // rec_off / rec_len / rec_sample per record; read_win_off is rec_win_off.  The per-read arrays, read_off, read_quals and
  // bases4 are only SIZED here (CollectRaw knows every window's bases): the call fills them (`flat_out`), and the batch then
  // goes to the chained call as a packed one with 8-bit qualities (`packed_view`, `packed`, `meta`).  Built by CollectRaw +
  // PlaceHeader / CopyPlaced / SizeForPlaced only, sealed by SealRaw().
  bool raw_mode = false;
  // cand_mode (beside raw_mode; ReadCollector::CollectCandidates): the records are every window's CANDIDATES, the input of
  // ma_select_records_batch.  SealCandidates() makes the views of that call (`records`, `sel_params`, `sel_out`); after it ran,
  // UseSelected() points `records` and the batch views at the selected lists, so that ma_flatten_records_batch and the chained
  // call take the batch as they take a CollectRaw one, and fills sample_cov from the call's sums.
  bool cand_mode = false;
  std::vector<uint8_t> rec_keep, win_state, sel_sample;
  std::vector<uint32_t> win_len, win_sample_reads, sel_win_off, sel_len, sel_src;
  std::vector<uint64_t> win_sample_bases, sel_off;
  uint64_t n_selected = 0;
  ma_select_params_t sel_params{};
  ma_select_out_t sel_out{};
  ByteVec raw_blob;
  std::vector<uint64_t> rec_off;
  std::vector<uint32_t> rec_len;
  std::vector<uint8_t> rec_sample;
  std::vector<int32_t> win_chrom;
  std::vector<int64_t> win_start0;
  uint64_t n_bases_out = 0;
  ma_records_t records{};
  ma_flat_out_t flat_out{};
  ByteVec seq4;
  std::vector<uint64_t> seq4_off{0};
  std::vector<uint8_t> read_sample, read_flags;
  std::vector<uint32_t> ref_off{0}, read_win_off{0}, read_qname_id;
  std::vector<uint64_t> read_off{0};
  std::vector<int32_t> read_hint;
  // the read metadata of ma_read_meta_t, per read like read_hint: MAPQ, MA_RM_* bits, insert size (tlen), start (pos0)
  std::vector<uint8_t> read_mapq, read_mflags;
  std::vector<int32_t> read_isize, read_start;
  ma_read_meta_t meta{};  // (Seal)
  std::vector<Window> windows;
  std::vector<std::vector<double>> sample_cov;  // [window][sample] sampled bases / window length
  ma_batch_t view{};
  void Add(Window const& w, std::string_view ref_seq, std::vector<Read> const& reads, std::vector<SampleInfo> const* samples = nullptr) {
    if (packed_mode) throw std::logic_error("FlatBatch::Add: a packed_mode batch is built by CollectFlat + PlaceHeader / CopyPlaced only");
    windows.push_back(w);
    sample_cov.emplace_back();
    if (samples)
      for (auto const& s : *samples) sample_cov.back().push_back(static_cast<double>(s.sampled_bases) / static_cast<double>(w.Length()));
    ref_bases.insert(ref_bases.end(), ref_seq.begin(), ref_seq.end());
    ref_off.push_back(static_cast<uint32_t>(ref_bases.size()));
    std::unordered_map<std::string_view, uint32_t> names;  // (qname, role) de-duplication needs names only within a window
    names.reserve(reads.size());
    for (Read const& r : reads) {
      read_bases.insert(read_bases.end(), r.seq.begin(), r.seq.end());
      size_t const q0 = read_quals.size();
      read_quals.insert(read_quals.end(), r.qual.begin(), r.qual.end());
      for (size_t q = q0; q < read_quals.size(); ++q)
        if (read_quals[q] == 0xFF) read_quals[q] = 0;
      read_off.push_back(read_bases.size());
      read_qname_id.push_back(names.emplace(r.qname, static_cast<uint32_t>(names.size())).first->second);
      read_sample.push_back(static_cast<uint8_t>(r.sample_index));
      read_flags.push_back(static_cast<uint8_t>((r.passes ? MA_RF_PASS : 0) | (r.tag == Tag::CASE ? MA_RF_CASE : 0) |
                                                ((r.flag & 0x10) ? MA_RF_REV : 0)));
      // where base 0 of the read is expected on the window (include/microasm.h: read_hint)
      int64_t const hint = r.chrom == w.chrom ? r.start0 - static_cast<int64_t>(w.start1 - 1) - static_cast<int64_t>(r.leading_clip) : INT64_MIN;
      read_hint.push_back(hint > INT32_MIN && hint < INT32_MAX ? static_cast<int32_t>(hint) : MA_NO_HINT);
      read_mapq.push_back(r.mapq);
      read_mflags.push_back(r.mflags);
      read_isize.push_back(r.isize);
      read_start.push_back(static_cast<int32_t>(std::max<int64_t>(0, std::min<int64_t>(INT32_MAX, r.start0))));
    }
    read_win_off.push_back(static_cast<uint32_t>(read_qname_id.size()));
  }
  // Appends the windows of another (unsealed) batch -- what Add() on their reads would have appended: the extract stage's
  // workers flatten each window on their own thread, the ordered assembler only copies.
  void Append(FlatBatch const& o) {
    if (packed_mode || o.packed_mode) throw std::logic_error("FlatBatch::Append: not for packed_mode batches (PlaceHeader / CopyPlaced)");
    uint32_t const rb = static_cast<uint32_t>(ref_bases.size()), nr = static_cast<uint32_t>(read_qname_id.size());
    uint64_t const qb = read_bases.size();
    windows.insert(windows.end(), o.windows.begin(), o.windows.end());
    sample_cov.insert(sample_cov.end(), o.sample_cov.begin(), o.sample_cov.end());
    ref_bases.insert(ref_bases.end(), o.ref_bases.begin(), o.ref_bases.end());
    read_bases.insert(read_bases.end(), o.read_bases.begin(), o.read_bases.end());
    read_quals.insert(read_quals.end(), o.read_quals.begin(), o.read_quals.end());
    read_sample.insert(read_sample.end(), o.read_sample.begin(), o.read_sample.end());
    read_flags.insert(read_flags.end(), o.read_flags.begin(), o.read_flags.end());
    read_qname_id.insert(read_qname_id.end(), o.read_qname_id.begin(), o.read_qname_id.end());
    read_hint.insert(read_hint.end(), o.read_hint.begin(), o.read_hint.end());
    read_mapq.insert(read_mapq.end(), o.read_mapq.begin(), o.read_mapq.end());
    read_mflags.insert(read_mflags.end(), o.read_mflags.begin(), o.read_mflags.end());
    read_isize.insert(read_isize.end(), o.read_isize.begin(), o.read_isize.end());
    read_start.insert(read_start.end(), o.read_start.begin(), o.read_start.end());
    for (size_t i = 1; i < o.ref_off.size(); ++i) ref_off.push_back(rb + o.ref_off[i]);
    for (size_t i = 1; i < o.read_off.size(); ++i) read_off.push_back(qb + o.read_off[i]);
    for (size_t i = 1; i < o.read_win_off.size(); ++i) read_win_off.push_back(nr + o.read_win_off[i]);
  }
  // The same, in two steps, for the extract stage's ordered thread (round 6: its Append() -- 200 KB copied per window on ONE
  // thread -- bounded the whole stage at ~30 k windows/s whatever the number of collectors): PlaceHeader() appends only the
  // window's scalars and returns where its arrays go; once the batch is closed SizeForPlaced() sizes the arrays (no zero-fill
  // of the big ones) and any thread copies a window into its place with CopyPlaced() -- disjoint ranges, no locks.
  // (A batch is built EITHER this way or with Add() / Append(): the placed sizes below are counted by PlaceHeader() alone.)
  struct Place {
    size_t ref0, read0;
    uint64_t base0;
    size_t raw0 = 0;
  };
  Place PlaceHeader(FlatBatch const& o) {  // o holds ONE window (what CollectFlat / CollectRaw / Add produce)
    Place const pl{placed_ref_, placed_reads_, placed_bases_, placed_raw_};
    windows.insert(windows.end(), o.windows.begin(), o.windows.end());
    sample_cov.insert(sample_cov.end(), o.sample_cov.begin(), o.sample_cov.end());
    placed_ref_ += o.ref_bases.size();
    placed_reads_ += o.raw_mode ? o.rec_len.size() : o.read_qname_id.size();
    placed_raw_ += o.raw_blob.size();
    placed_bases_ += o.read_off.back();
    ref_off.push_back(static_cast<uint32_t>(placed_ref_));
    read_win_off.push_back(static_cast<uint32_t>(placed_reads_));
    return pl;
  }
  void SizeForPlaced() {
    ref_bases.resize(placed_ref_);
    if (raw_mode) {  // the records, and room for what the device makes of them (the nibble array is read in aligned words)
      raw_blob.resize(std::max<size_t>(placed_raw_, 1));
      rec_off.resize(placed_reads_); rec_len.resize(placed_reads_); rec_sample.resize(placed_reads_);
      bases4.resize((placed_bases_ + placed_reads_ + 1) / 2 + 8);
      read_quals.resize(placed_bases_ + 64);
      read_off.resize(placed_reads_ + 1);
    } else {
      if (packed_mode) bases4.assign(std::max<size_t>((placed_bases_ + placed_reads_ + 1) / 2, 1), 0);
      else read_bases.resize(placed_bases_);
      read_quals.resize(placed_bases_);
    }
    read_sample.resize(placed_reads_);
    read_flags.resize(placed_reads_);
    read_qname_id.resize(placed_reads_);
    read_hint.resize(placed_reads_);
    read_mapq.resize(placed_reads_); read_mflags.resize(placed_reads_);
    read_isize.resize(placed_reads_); read_start.resize(placed_reads_);
    read_off.resize(placed_reads_ + 1);
    read_off[0] = 0;
  }
  void CopyPlaced(FlatBatch const& o, Place const& pl) {
    if (!o.ref_bases.empty()) std::memcpy(ref_bases.data() + pl.ref0, o.ref_bases.data(), o.ref_bases.size());
    if (o.raw_mode) {
      if (!o.raw_blob.empty()) std::memcpy(raw_blob.data() + pl.raw0, o.raw_blob.data(), o.raw_blob.size());
      for (size_t i = 0; i < o.rec_len.size(); ++i) {
        rec_off[pl.read0 + i] = pl.raw0 + o.rec_off[i];
        rec_len[pl.read0 + i] = o.rec_len[i];
        rec_sample[pl.read0 + i] = o.rec_sample[i];
      }
      return;
    }
    size_t const nr = o.read_qname_id.size();
    if (nr == 0) return;
    if (packed_mode) {
      for (size_t i = 0; i < nr; ++i)  // reads start on byte boundaries: whole bytes, wherever the window lands in the batch
        std::memcpy(bases4.data() + ((pl.base0 + o.read_off[i] + pl.read0 + i) >> 1), o.seq4.data() + o.seq4_off[i],
                    static_cast<size_t>(o.seq4_off[i + 1] - o.seq4_off[i]));
    } else {
      std::memcpy(read_bases.data() + pl.base0, o.read_bases.data(), o.read_bases.size());
    }
    std::memcpy(read_quals.data() + pl.base0, o.read_quals.data(), o.read_quals.size());
    std::memcpy(read_sample.data() + pl.read0, o.read_sample.data(), nr);
    std::memcpy(read_flags.data() + pl.read0, o.read_flags.data(), nr);
    std::memcpy(read_qname_id.data() + pl.read0, o.read_qname_id.data(), nr * sizeof(uint32_t));
    std::memcpy(read_hint.data() + pl.read0, o.read_hint.data(), nr * sizeof(int32_t));
    std::memcpy(read_mapq.data() + pl.read0, o.read_mapq.data(), nr);
    std::memcpy(read_mflags.data() + pl.read0, o.read_mflags.data(), nr);
    std::memcpy(read_isize.data() + pl.read0, o.read_isize.data(), nr * sizeof(int32_t));
    std::memcpy(read_start.data() + pl.read0, o.read_start.data(), nr * sizeof(int32_t));
    for (size_t i = 1; i <= nr; ++i) read_off[pl.read0 + i] = pl.base0 + o.read_off[i];
  }
  size_t placed_ref_ = 0, placed_reads_ = 0, placed_raw_ = 0;
  uint64_t placed_bases_ = 0;
  // back to an empty batch that KEEPS its arrays' memory: a recycled batch does not fault 300 MB of fresh pages in again
  void Clear() {
    ref_bases.clear(); read_bases.clear(); read_quals.clear(); read_sample.clear(); read_flags.clear();
    ref_off.assign(1, 0); read_win_off.assign(1, 0); read_off.assign(1, 0);
    read_qname_id.clear(); read_hint.clear(); windows.clear(); sample_cov.clear();
    read_mapq.clear(); read_mflags.clear(); read_isize.clear(); read_start.clear();
    meta = ma_read_meta_t{};
    placed_ref_ = placed_reads_ = placed_raw_ = 0;
    placed_bases_ = 0;
    raw_blob.clear(); rec_off.clear(); rec_len.clear(); rec_sample.clear(); win_chrom.clear(); win_start0.clear();
    n_selected = 0;
    sel_params = ma_select_params_t{};
    sel_out = ma_select_out_t{};
    records = ma_records_t{};
    flat_out = ma_flat_out_t{};
    n_bases_out = 0;
    seq4.clear(); seq4_off.assign(1, 0); bases4.clear(); quals_packed.clear();
    packed = ma_packed_reads_t{};
    packed_view = ma_batch_t{};
    view = ma_batch_t{};
  }
  void Reserve(size_t n_win, size_t n_ref, size_t n_reads, size_t n_bases) {  // (Append then never re-allocates and copies what it holds)
    windows.reserve(n_win); sample_cov.reserve(n_win); ref_off.reserve(n_win + 1); read_win_off.reserve(n_win + 1);
    ref_bases.reserve(n_ref + 64); read_bases.reserve(n_bases + 64); read_quals.reserve(n_bases + 64);
    read_sample.reserve(n_reads); read_flags.reserve(n_reads); read_qname_id.reserve(n_reads); read_hint.reserve(n_reads); read_off.reserve(n_reads + 1);
    read_mapq.reserve(n_reads); read_mflags.reserve(n_reads); read_isize.reserve(n_reads); read_start.reserve(n_reads);
  }
  void Seal() {
    size_t const rb = ref_bases.size(), qb = read_quals.size();
    ref_bases.resize(rb + 64, 0);
    read_bases.resize(read_bases.size() + 64, 0);
    read_quals.resize(qb + 64, 0);
    view.n_windows = static_cast<int32_t>(windows.size());
    view.n_reads = static_cast<int64_t>(read_qname_id.size());
    view.ref_bases = ref_bases.data();
    view.ref_off = ref_off.data();
    view.read_win_off = read_win_off.data();
    view.read_off = read_off.data();
    view.read_bases = read_bases.data();
    view.read_quals = read_quals.data();
    view.read_qname_id = read_qname_id.data();
    view.read_sample = read_sample.data();
    view.read_flags = read_flags.data();
    view.read_hint = read_hint.data();
    meta.read_mapq = read_mapq.data(); meta.read_mflags = read_mflags.data();
    meta.read_isize = read_isize.data(); meta.read_start = read_start.data();
  }
  // The sample tables and reference maps of ma_records_t: one row per sample of the collector, in its order.  Built once.
  struct RawTables {
    std::vector<uint8_t> index, is_case;
    std::vector<uint32_t> rank;     // samples that tie in (tag, name) tie here, as in the comparator
    std::vector<int32_t> ref_map;   // [samples x n_refs] BAM refID -> chrom of the FASTA, -1 beyond a file's own list
    int32_t n_refs = 0;
  };
  // raw_mode, in place of Seal(): the views of ma_flatten_records_batch and of the chained call that takes its outputs
  void SealRaw(RawTables const& t) {
    ref_bases.resize(ref_bases.size() + 64, 0);
    size_t const nr = rec_len.size(), nw = windows.size();
    win_chrom.resize(nw); win_start0.resize(nw);
    for (size_t w = 0; w < nw; ++w) {
      win_chrom[w] = windows[w].chrom;
      win_start0[w] = static_cast<int64_t>(windows[w].start1) - 1;
    }
    read_sample.resize(nr); read_flags.resize(nr); read_qname_id.resize(nr); read_hint.resize(nr);
    read_mapq.resize(nr); read_mflags.resize(nr); read_isize.resize(nr); read_start.resize(nr);
    read_src.resize(nr);
    records = ma_records_t{};
    records.n_windows = static_cast<int32_t>(nw);
    records.n_records = static_cast<int64_t>(nr);
    records.blob = raw_blob.data(); records.blob_bytes = placed_raw_;
    records.rec_off = rec_off.data(); records.rec_len = rec_len.data(); records.rec_win_off = read_win_off.data();
    records.rec_sample = rec_sample.data();
    records.n_samples_in = static_cast<int32_t>(t.index.size());
    records.sample_index = t.index.data(); records.sample_case = t.is_case.data(); records.sample_rank = t.rank.data();
    records.n_refs = t.n_refs; records.ref_map = t.ref_map.data();
    records.win_chrom = win_chrom.data(); records.win_start0 = win_start0.data();
    flat_out = ma_flat_out_t{};
    flat_out.bases_cap = placed_bases_;
    flat_out.n_bases = &n_bases_out; flat_out.read_off = read_off.data();
    flat_out.bases4 = bases4.data(); flat_out.read_quals = read_quals.data();
    flat_out.read_qname_id = read_qname_id.data(); flat_out.read_sample = read_sample.data(); flat_out.read_flags = read_flags.data();
    flat_out.read_hint = read_hint.data(); flat_out.read_mapq = read_mapq.data(); flat_out.read_mflags = read_mflags.data();
    flat_out.read_isize = read_isize.data(); flat_out.read_start = read_start.data(); flat_out.read_src = read_src.data();
    view = ma_batch_t{};
    view.n_windows = static_cast<int32_t>(nw);
    view.n_reads = static_cast<int64_t>(nr);
    view.ref_bases = ref_bases.data(); view.ref_off = ref_off.data(); view.read_win_off = read_win_off.data();
    view.read_off = read_off.data(); view.read_qname_id = read_qname_id.data(); view.read_sample = read_sample.data();
    view.read_flags = read_flags.data(); view.read_hint = read_hint.data();
    packed_view = view;  // (read_bases / read_quals stay null: a packed batch)
    packed = ma_packed_reads_t{};
    packed.bases4 = bases4.data(); packed.quals = read_quals.data(); packed.qual_bits = 8;
    meta.read_mapq = read_mapq.data(); meta.read_mflags = read_mflags.data();
    meta.read_isize = read_isize.data(); meta.read_start = read_start.data();
  }
  std::vector<uint32_t> read_src;  // raw_mode: which record each read is (ma_flat_out_t::read_src)
  void SealCandidates(RawTables const& t, double max_sample_cov, uint32_t min_anchor_cov, bool skip_active_region) {
    SealRaw(t);
    size_t const nr = rec_len.size(), nw = windows.size(), ns = t.index.size();
    win_len.resize(nw);
    for (size_t w = 0; w < nw; ++w) win_len[w] = static_cast<uint32_t>(windows[w].Length());
    rec_keep.resize(std::max<size_t>(nr, 1)); win_state.resize(std::max<size_t>(nw, 1));
    win_sample_reads.resize(std::max<size_t>(nw * ns, 1)); win_sample_bases.resize(std::max<size_t>(nw * ns, 1));
    sel_win_off.resize(nw + 1);
    sel_off.resize(std::max<size_t>(nr, 1)); sel_len.resize(std::max<size_t>(nr, 1)); sel_sample.resize(std::max<size_t>(nr, 1));
    sel_src.resize(std::max<size_t>(nr, 1));
    sel_params = ma_select_params_t{max_sample_cov, min_anchor_cov, skip_active_region ? 1 : 0, win_len.data()};
    sel_out = ma_select_out_t{rec_keep.data(), win_state.data(), win_sample_reads.data(), win_sample_bases.data(), &n_selected,
                              sel_win_off.data(), sel_off.data(), sel_len.data(), sel_sample.data(), sel_src.data()};
  }
  void UseSelected() {
    size_t const nw = windows.size(), ns = static_cast<size_t>(records.n_samples_in);
    records.n_records = static_cast<int64_t>(n_selected);
    records.rec_off = sel_off.data(); records.rec_len = sel_len.data(); records.rec_win_off = sel_win_off.data();
    records.rec_sample = sel_sample.data();
    view.n_reads = static_cast<int64_t>(n_selected);
    view.read_win_off = sel_win_off.data();
    packed_view = view;
    for (size_t w = 0; w < nw; ++w) {
      sample_cov[w].assign(ns, 0.0);
      for (size_t s = 0; s < ns; ++s) sample_cov[w][s] = static_cast<double>(win_sample_bases[w * ns + s]) / static_cast<double>(windows[w].Length());
    }
  }
  // --packed-reads (include/microasm.h: ma_packed_reads_t), after Seal(): the batch's quality dictionary -- 4-bit codes into
  // the distinct Phred values in ascending order when there are at most 16 of them, the Phred bytes as they are (qual_bits =
  // 8) otherwise -- and, unless the batch was built in packed_mode (bases4 is in place then), the read bases packed from
  // read_bases.  packed_view is `view` without the two ASCII arrays: what ma_process_packed_batch / ma_prefetch_packed_batch
  // take beside `packed`.  The arrays hold at least one byte, so that a batch without read bases still has non-null members.
  ByteVec bases4, quals_packed;
  ma_packed_reads_t packed{};
  ma_batch_t packed_view{};
  void PackReads() {
    size_t const nr = read_off.empty() ? 0 : read_off.size() - 1;
    size_t const total = nr ? static_cast<size_t>(read_off[nr]) : 0, bytes = std::max<size_t>((total + nr + 1) / 2, 1);
    packed = ma_packed_reads_t{};
    std::array<uint8_t, 256> qcode{};
    std::array<bool, 256> seen{};
    for (size_t i = 0; i < total; ++i) seen[read_quals[i]] = true;
    int distinct = 0;
    for (int q = 0; q < 256; ++q) {
      if (!seen[static_cast<size_t>(q)]) continue;
      if (distinct < 16) {
        packed.qual_dict[distinct] = static_cast<uint8_t>(q);
        qcode[static_cast<size_t>(q)] = static_cast<uint8_t>(distinct);
      }
      ++distinct;
    }
    bool const q4 = distinct <= 16;
    if (!q4) std::memset(packed.qual_dict, 0, sizeof(packed.qual_dict));
    if (!packed_mode) bases4.assign(bytes, 0);
    quals_packed.assign(q4 ? bytes : 1, 0);
    for (size_t r = 0; r < nr; ++r) {
      size_t const o0 = static_cast<size_t>(read_off[r]), len = static_cast<size_t>(read_off[r + 1]) - o0, at = (o0 + r) >> 1;
      for (size_t j = 0; j < len; ++j) {
        unsigned const sh = (j & 1) ? 0u : 4u;
        if (!packed_mode) bases4[at + (j >> 1)] |= static_cast<uint8_t>(BaseCode4(read_bases[o0 + j]) << sh);
        if (q4) quals_packed[at + (j >> 1)] |= static_cast<uint8_t>(qcode[read_quals[o0 + j]] << sh);
      }
    }
    packed.bases4 = bases4.data();
    packed.quals = q4 ? quals_packed.data() : read_quals.data();
    packed.qual_bits = q4 ? 4 : 8;
    packed_view = view;
    packed_view.read_bases = nullptr;
    packed_view.read_quals = nullptr;
  }
};

// The kept set of a window, sample after sample in arrival order: the record filters and the seeded downsampling of
// read_collector.cpp:147-216, shared by CollectFlat and CollectRaw.  Sets every sample's sampled_reads / sampled_bases and
// returns the bases kept.  (A raw-mode record has its name's hash as a scalar: SamRecord::NameHash.)
inline size_t ReadCollector::SelectKept(Window const& w, std::vector<Kept>* kept_out, std::deque<SamRecord>* arena) {
  std::vector<Kept>& kept = *kept_out;
  double const max_sample_bases = prm_.max_sample_cov * static_cast<double>(w.Length());
  int64_t const s1 = static_cast<int64_t>(w.start1), e1 = static_cast<int64_t>(w.end1);
  size_t total_bases = 0;
  for (size_t si = 0; si < samples_.size(); ++si) {
    SampleInfo& sinfo = samples_[si];
    size_t const first = kept.size();
    uint64_t n_reads = 0, n_bases = 0;
#ifdef LANCET2_AMD_WITH_ZLIB
    bool const own = sinfo.source->indexed();
#else
    bool const own = false;
#endif
    sinfo.source->ForRegion(w.chrom, s1, e1, [&](SamRecord const& a) {
      if (Filtered(a)) return;
      const SamRecord* p = &a;
      if (own) {
        arena->push_back(a);
        p = &arena->back();
      }
      n_reads += 1;
      n_bases += a.SeqLen();
      kept.push_back(Kept{p, a.NameHash(), static_cast<uint32_t>(si), static_cast<uint32_t>(kept.size())});
    });
    double const bases_per_read = static_cast<double>(n_bases) / static_cast<double>(std::max<uint64_t>(n_reads, 1));
    uint64_t const max_reads = static_cast<uint64_t>(std::ceil(max_sample_bases / bases_per_read));
    uint64_t const sampled = std::min(n_reads, max_reads);
    if (sampled < n_reads) {  // coverage-capped: the same shuffle of the name hashes, the same kept set (read_collector.cpp:147-216)
      std::vector<uint64_t> hashes;
      hashes.reserve(n_reads);
      for (size_t i = first; i < kept.size(); ++i) hashes.push_back(kept[i].qh);
      std::shuffle(hashes.begin(), hashes.end(), std::mt19937_64{0});
      std::unordered_set<uint64_t> keep(hashes.begin(), hashes.begin() + static_cast<long>(sampled));
      size_t at = first;
      for (size_t i = first; i < kept.size(); ++i)
        if (keep.count(kept[i].qh)) kept[at++] = kept[i];
      kept.resize(at);
    }
    uint64_t bases = 0;
    for (size_t i = first; i < kept.size(); ++i) bases += kept[i].rec->SeqLen();
    sinfo.sampled_reads = sampled;
    sinfo.sampled_bases = bases;
    total_bases += bases;
  }
  return total_bases;
}

inline bool ReadCollector::CollectFlat(Window const& w, std::string_view ref_seq, FlatBatch* out) {
  if (prm_.extract_pairs) return false;
  struct Ref {
    const SamRecord* rec;
    uint64_t qh;
    uint64_t qpre;    // the name's first eight bytes, big-endian, zero-padded: its order is the names' order while it differs
    uint32_t sample;  // position in samples_
    uint32_t order;   // arrival order (ties of the comparator)
  };
  auto name_prefix = [](std::string const& q) {
    uint64_t v = 0;
    size_t const n = std::min<size_t>(q.size(), 8);
    for (size_t i = 0; i < n; ++i) v |= static_cast<uint64_t>(static_cast<unsigned char>(q[i])) << (56 - 8 * i);
    return v;
  };
  std::vector<Kept> sel;
  std::deque<SamRecord> arena;  // an indexed source hands out temporaries
  size_t const total_bases = SelectKept(w, &sel, &arena);
  std::vector<Ref> kept;
  kept.reserve(sel.size());
  for (Kept const& k : sel) kept.push_back(Ref{k.rec, k.qh, name_prefix(k.rec->qname), k.sample, k.order});
  // read_collector.cpp:42-53: filter-pass status > sample tag > sample name > qname > chrom > position (> arrival)
  std::sort(kept.begin(), kept.end(), [&](Ref const& l, Ref const& r) {
    bool const lp = l.rec->mapq >= 20, rp = r.rec->mapq >= 20;
    if (lp != rp) return static_cast<int>(lp) > static_cast<int>(rp);
    if (l.sample != r.sample) {
      SampleInfo const &ls = samples_[l.sample], &rs = samples_[r.sample];
      if (ls.tag != rs.tag) return static_cast<uint8_t>(ls.tag) < static_cast<uint8_t>(rs.tag);
      if (ls.name != rs.name) return ls.name < rs.name;
    }
    // (names: bytes compare as unsigned chars, a proper prefix sorts first -- what the zero-padded big-endian prefix orders by
    //  while it differs; the 5 500 comparisons of a window's sort were string comparisons, most of the collector's time)
    if (l.qpre != r.qpre) return l.qpre < r.qpre;
    if (l.qh != r.qh || l.rec->qname != r.rec->qname) return l.rec->qname < r.rec->qname;
    if (l.rec->chrom != r.rec->chrom) return l.rec->chrom < r.rec->chrom;
    if (l.rec->pos0 != r.rec->pos0) return l.rec->pos0 < r.rec->pos0;
    return l.order < r.order;
  });
  // ---- what FlatBatch::Add appends ----
  FlatBatch& fb = *out;
  fb.windows.push_back(w);
  fb.sample_cov.emplace_back();
  for (auto const& sm : samples_) fb.sample_cov.back().push_back(static_cast<double>(sm.sampled_bases) / static_cast<double>(w.Length()));
  fb.ref_bases.insert(fb.ref_bases.end(), ref_seq.begin(), ref_seq.end());
  fb.ref_off.push_back(static_cast<uint32_t>(fb.ref_bases.size()));
  size_t const nr = kept.size(), b0 = static_cast<size_t>(fb.read_off.back()), r0 = fb.read_qname_id.size();
  bool const packed = prm_.packed_reads;
  fb.packed_mode = packed;
  if (!packed) fb.read_bases.resize(b0 + total_bases);
  fb.read_quals.resize(b0 + total_bases);
  fb.read_off.reserve(fb.read_off.size() + nr);
  fb.read_qname_id.resize(r0 + nr);
  fb.read_sample.resize(r0 + nr);
  fb.read_flags.resize(r0 + nr);
  fb.read_hint.resize(r0 + nr);
  fb.read_mapq.resize(r0 + nr); fb.read_mflags.resize(r0 + nr); fb.read_isize.resize(r0 + nr); fb.read_start.resize(r0 + nr);
  // names -> ids in order of first appearance: open addressing on the name hash, the name itself compared on a hit
  size_t cap = 16;
  while (cap < 2 * nr + 2) cap <<= 1;
  std::vector<uint32_t> table(cap, 0xFFFFFFFFu);  // index into kept of the name's first appearance
  std::vector<uint32_t> id_of(nr);
  uint32_t n_names = 0;
  size_t at = b0;
  for (size_t i = 0; i < nr; ++i) {
    SamRecord const& a = *kept[i].rec;
    size_t const len = a.SeqLen();
    if (!packed) {
      std::memcpy(fb.read_bases.data() + at, a.seq.data(), len);
    } else if (a.packed) {  // a BAM record: its sequence bytes as they are
      fb.seq4.insert(fb.seq4.end(), a.seq4.begin(), a.seq4.end());
      fb.seq4_off.push_back(fb.seq4.size());
    } else {                // SAM text: packed here
      size_t const s0 = fb.seq4.size();
      fb.seq4.resize(s0 + (len + 1) / 2, 0);
      for (size_t x = 0; x < len; ++x)
        fb.seq4[s0 + (x >> 1)] |= static_cast<uint8_t>(BaseCode4(static_cast<uint8_t>(a.seq[x])) << ((x & 1) ? 0 : 4));
      fb.seq4_off.push_back(fb.seq4.size());
    }
    uint8_t* q = fb.read_quals.data() + at;
    size_t const nq = std::min(a.qual.size(), len);  // (the arrays are sized by SEQ; the parsers reject a mismatch)
    for (size_t x = 0; x < nq; ++x) q[x] = a.qual[x] == 0xFF ? 0 : a.qual[x];
    for (size_t x = nq; x < len; ++x) q[x] = 0;
    at += len;
    fb.read_off.push_back(at);
    size_t h = static_cast<size_t>(kept[i].qh * 0x9E3779B97F4A7C15ull >> 20) & (cap - 1);
    uint32_t id;
    for (;;) {
      uint32_t const e = table[h];
      if (e == 0xFFFFFFFFu) {
        table[h] = static_cast<uint32_t>(i);
        id = n_names++;
        break;
      }
      if (kept[e].qh == kept[i].qh && kept[e].rec->qname == a.qname) {
        id = id_of[e];
        break;
      }
      h = (h + 1) & (cap - 1);
    }
    id_of[i] = id;
    fb.read_qname_id[r0 + i] = id;
    SampleInfo const& sm = samples_[kept[i].sample];
    fb.read_sample[r0 + i] = static_cast<uint8_t>(sm.index);
    fb.read_flags[r0 + i] = static_cast<uint8_t>((a.mapq >= 20 ? MA_RF_PASS : 0) | (sm.tag == Tag::CASE ? MA_RF_CASE : 0) | ((a.flag & 0x10) ? MA_RF_REV : 0));
    int64_t const hint = a.chrom == w.chrom ? a.pos0 - static_cast<int64_t>(w.start1 - 1) - static_cast<int64_t>(a.LeadingSoftClip()) : INT64_MIN;
    fb.read_hint[r0 + i] = hint > INT32_MIN && hint < INT32_MAX ? static_cast<int32_t>(hint) : MA_NO_HINT;
    fb.read_mapq[r0 + i] = a.mapq;
    fb.read_mflags[r0 + i] = a.MetaFlags();
    fb.read_isize[r0 + i] = a.InsertSize32();
    fb.read_start[r0 + i] = a.Start32();
  }
  fb.read_win_off.push_back(static_cast<uint32_t>(fb.read_qname_id.size()));
  return true;
}

inline bool ReadCollector::CollectRaw(Window const& w, std::string_view ref_seq, FlatBatch* out) {
  if (prm_.extract_pairs) return false;
  std::vector<Kept> sel;
  std::deque<SamRecord> arena;
  size_t const total_bases = SelectKept(w, &sel, &arena);
  size_t bytes = 0;
  for (Kept const& k : sel) {
    if (!k.rec->is_raw) return false;
    bytes += k.rec->raw.size();
  }
  // the device sorts a window in LDS: more kept records than that (three samples at the default coverage cap of 1000x can get
  // there) cannot go this way -- say so here, by name, instead of letting the batch fail with MA_ERR_PARAM
  if (sel.size() > MA_FLATTEN_MAX_WINDOW)
    throw std::runtime_error("--raw-records: window " + std::to_string(w.start1) + "-" + std::to_string(w.end1) + " keeps " +
                             std::to_string(sel.size()) + " records, more than the " + std::to_string(MA_FLATTEN_MAX_WINDOW) +
                             " that ma_flatten_records_batch sorts per window: lower --max-sample-cov or run without --raw-records");
  FlatBatch& fb = *out;
  fb.raw_mode = true;
  fb.windows.push_back(w);
  fb.sample_cov.emplace_back();
  for (auto const& sm : samples_) fb.sample_cov.back().push_back(static_cast<double>(sm.sampled_bases) / static_cast<double>(w.Length()));
  fb.ref_bases.insert(fb.ref_bases.end(), ref_seq.begin(), ref_seq.end());
  fb.ref_off.push_back(static_cast<uint32_t>(fb.ref_bases.size()));
  size_t const r0 = fb.rec_len.size(), b0 = fb.raw_blob.size();
  fb.raw_blob.resize(b0 + bytes);
  fb.rec_off.resize(r0 + sel.size()); fb.rec_len.resize(r0 + sel.size()); fb.rec_sample.resize(r0 + sel.size());
  size_t at = b0;
  for (size_t i = 0; i < sel.size(); ++i) {
    std::vector<uint8_t> const& raw = sel[i].rec->raw;
    std::memcpy(fb.raw_blob.data() + at, raw.data(), raw.size());
    fb.rec_off[r0 + i] = at;
    fb.rec_len[r0 + i] = static_cast<uint32_t>(raw.size());
    fb.rec_sample[r0 + i] = static_cast<uint8_t>(sel[i].sample);
    at += raw.size();
  }
  fb.read_off.push_back(fb.read_off.back() + total_bases);  // (one entry per WINDOW here: what PlaceHeader adds up)
  fb.read_win_off.push_back(static_cast<uint32_t>(fb.rec_len.size()));
  return true;
}

inline bool ReadCollector::CollectCandidates(Window const& w, std::string_view ref_seq, FlatBatch* out) {
  FlatBatch& fb = *out;
  fb.raw_mode = fb.cand_mode = true;
  fb.windows.push_back(w);
  fb.sample_cov.emplace_back(samples_.size(), 0.0);  // (known once the device has counted: FlatBatch::UseSelected)
  fb.ref_bases.insert(fb.ref_bases.end(), ref_seq.begin(), ref_seq.end());
  fb.ref_off.push_back(static_cast<uint32_t>(fb.ref_bases.size()));
  uint64_t bases = 0;
  bool all_raw = true;
  // an in-memory source's records stay where they are: they are listed first and copied once the window's size is known; an
  // indexed source hands out temporaries, which are appended as they come
  std::vector<std::pair<const SamRecord*, uint8_t>> listed;
  size_t bytes = fb.raw_blob.size();
  for (size_t si = 0; si < samples_.size(); ++si) {
#ifdef LANCET2_AMD_WITH_ZLIB
    bool const own = samples_[si].source->indexed();
#else
    bool const own = false;
#endif
    samples_[si].source->ForRegion(w.chrom, static_cast<int64_t>(w.start1), static_cast<int64_t>(w.end1), [&](SamRecord const& a) {
      if (!a.is_raw) {
        all_raw = false;
        return;
      }
      bases += a.SeqLen();
      if (!own) {
        listed.emplace_back(&a, static_cast<uint8_t>(si));
        bytes += a.raw.size();
        return;
      }
      fb.rec_off.push_back(fb.raw_blob.size());
      fb.rec_len.push_back(static_cast<uint32_t>(a.raw.size()));
      fb.rec_sample.push_back(static_cast<uint8_t>(si));
      fb.raw_blob.insert(fb.raw_blob.end(), a.raw.begin(), a.raw.end());
    });
    if (own || listed.empty()) continue;
    size_t at = fb.raw_blob.size();
    size_t const r0 = fb.rec_len.size();
    fb.raw_blob.resize(bytes);
    fb.rec_off.resize(r0 + listed.size()); fb.rec_len.resize(r0 + listed.size()); fb.rec_sample.resize(r0 + listed.size());
    for (size_t i = 0; i < listed.size(); ++i) {
      std::vector<uint8_t> const& raw = listed[i].first->raw;
      std::memcpy(fb.raw_blob.data() + at, raw.data(), raw.size());
      fb.rec_off[r0 + i] = at;
      fb.rec_len[r0 + i] = static_cast<uint32_t>(raw.size());
      fb.rec_sample[r0 + i] = listed[i].second;
      at += raw.size();
    }
    listed.clear();
  }
  fb.read_off.push_back(fb.read_off.back() + bases);  // (one entry per WINDOW here: what PlaceHeader adds up)
  fb.read_win_off.push_back(static_cast<uint32_t>(fb.rec_len.size()));
  return all_raw;
}

// the tables of a collector's samples (its sorted order: rec_sample is a position in it)
inline FlatBatch::RawTables MakeRawTables(std::vector<SampleInfo> const& sorted) {
  FlatBatch::RawTables t;
  for (size_t i = 0; i < sorted.size(); ++i) {
    t.index.push_back(static_cast<uint8_t>(sorted[i].index));
    t.is_case.push_back(sorted[i].tag == Tag::CASE ? 1 : 0);
    bool const tie = i > 0 && sorted[i].tag == sorted[i - 1].tag && sorted[i].name == sorted[i - 1].name;
    t.rank.push_back(tie ? t.rank.back() : static_cast<uint32_t>(i));
#ifdef LANCET2_AMD_WITH_ZLIB
    t.n_refs = std::max(t.n_refs, static_cast<int32_t>(sorted[i].source->RefMap().size()));
#endif
  }
  t.ref_map.assign(std::max<size_t>(sorted.size() * static_cast<size_t>(t.n_refs), 1), -1);
#ifdef LANCET2_AMD_WITH_ZLIB
  for (size_t i = 0; i < sorted.size(); ++i) {
    std::vector<int> const& m = sorted[i].source->RefMap();
    for (size_t r = 0; r < m.size(); ++r) t.ref_map[i * static_cast<size_t>(t.n_refs) + r] = m[r];
  }
#endif
  return t;
}

// ---- the store between the workers and the output (core/variant_store.cpp) ---------------------------------------------------
struct VariantRecord {
  int chrom = -1;
  uint64_t pos1 = 0;
  std::string ref;
  std::vector<std::string> alts;
  double qual = 0.0;
  std::vector<std::vector<uint32_t>> ad;  // [sample][allele]
  size_t window_index = 0;
  // what the VCF record needs beyond the TSV line (filled by RecordsOfBatch; empty vectors = not available)
  std::vector<int32_t> alt_type, alt_length;        // AlleleType 0 SNV 1 INS 2 DEL 3 MNP 4 CPX; AltAllele::mLength
  std::vector<std::vector<uint32_t>> adf, adr, pl;  // [sample][allele] forward / reverse depths; [sample][genotype] PL
  std::vector<uint32_t> gq;                         // [sample]
  std::vector<double> sample_window_cov;            // [sample] sampled bases / window length (SDFC's denominator)
  std::string seq_cx, graph_cx;                     // INFO values as the reference formats them (empty: not annotated)
  // the read-level FORMAT statistics of ma_process_stats_batch (empty: not computed; NaN: missing, "." in the VCF)
  std::vector<std::vector<double>> npbq, cmlod;     // [sample][allele], [sample][ALT]
  std::vector<std::array<double, 4>> fmt_stat;      // [sample] BQCD, ASMD, AHDD, HSE
  // ... and of ma_process_meta_batch (empty: not computed -- the six are then written as missing)
  std::vector<std::vector<double>> rmq;             // [sample][allele]
  std::vector<std::array<double, 5>> fmt_mstat;     // [sample] SCA, FLD, RPCD, MQCD, FSSE
  double pdcv = std::numeric_limits<double>::quiet_NaN();  // MaxAltPathCv of the variant's component (NaN: none)
  uint64_t TotalCoverage() const {
    uint64_t t = 0;
    for (auto const& s : ad)
      for (uint32_t c : s) t += c;
    return t;
  }
  bool HasAltSupport() const {
    for (auto const& s : ad)
      for (size_t a = 1; a < s.size(); ++a)
        if (s[a] > 0) return true;
    return false;
  }
  // the flush-time rule of core/variant_store.cpp:62-66 / :88-92: no ALT support, or every ALT category is REF
  bool HasNoSupport() const {
    if (!HasAltSupport()) return true;
    if (alt_type.empty()) return false;  // categories not filled in (TSV-only callers): the depth rule alone
    for (int32_t t : alt_type)
      if (t >= 0) return false;
    return true;
  }
  std::string AsLine(Reference const& ref_) const {
    std::string l = ref_.chroms[static_cast<size_t>(chrom)].name + "\t" + std::to_string(pos1) + "\t" + ref + "\t";
    for (size_t a = 0; a < alts.size(); ++a) l += (a ? "," : "") + alts[a];
    char buf[64];
    std::snprintf(buf, sizeof buf, "\t%.6f", qual);
    l += buf;
    for (auto const& s : ad) {
      l += "\t";
      for (size_t a = 0; a < s.size(); ++a) l += (a ? "," : "") + std::to_string(s[a]);
    }
    return l;
  }
};
class VariantStore {
 public:
  using Key = std::tuple<int, uint64_t, std::string>;  // VariantCall::Identifier(): CHROM + POS + REF (variant_call.cpp:37)
  void AddVariants(std::vector<VariantRecord> variants) {
    for (auto& cur : variants) {
      Key key{cur.chrom, cur.pos1, cur.ref};
      auto prev = data_.find(key);
      if (prev == data_.end()) {
        data_.emplace(std::move(key), std::move(cur));
      } else if (prev->second.TotalCoverage() < cur.TotalCoverage()) {
        prev->second = std::move(cur);  // the better covered window likely assembled the more complete picture
      }
    }
  }
  // variant_store.cpp:46-79: everything that starts before the window's END on its chromosome, or on an earlier one
  std::vector<VariantRecord> ExtractBeforeWindow(Window const& w) {
    std::vector<VariantRecord> out;
    for (auto it = data_.begin(); it != data_.end();) {
      VariantRecord const& v = it->second;
      bool const before = v.chrom != w.chrom ? v.chrom < w.chrom : v.pos1 < w.end1;
      if (!before) {
        ++it;
        continue;
      }
      if (!v.HasNoSupport()) out.push_back(std::move(it->second));
      it = data_.erase(it);
    }
    return out;  // (std::map iterates in key order: coordinate-sorted already)
  }
  std::vector<VariantRecord> ExtractAll() {
    std::vector<VariantRecord> out;
    for (auto& kv : data_)
      if (!kv.second.HasNoSupport()) out.push_back(std::move(kv.second));
    data_.clear();
    return out;
  }
  size_t Size() const { return data_.size(); }

 private:
  std::map<Key, VariantRecord> data_;
};

// ---- VCF text (caller/variant_call.cpp:100-520, caller/sample_format_data.cpp:32-98, cli/vcf_header_builder.cpp:28-63) -------
// The record layout, INFO field and the FORMAT key are the reference's.  Of the 24 FORMAT values the engine's outputs give 18:
// GT, AD, ADF, ADR, DP, SB, SDFC, PRAD, PANG, PL and GQ from the allele depths, NPBQ, BQCD, ASMD, CMLOD, AHDD and HSE from
// ma_process_stats_batch (RecordsOfBatch's `fmt`) and PDCV from the assembly's comp_cxf.  The other six -- RMQ, SCA, FLD,
// RPCD, MQCD, FSSE -- come from ma_process_meta_batch over FlatBatch's read metadata (RecordsOfBatch's `fmeta`); a record
// built without them writes the six as missing (".").  Values pass through f32 where the reference stores f32, and are
// printed with its formats: RMQ %.1F per allele, SCA %.4f, FLD %.1f, RPCD / MQCD / FSSE %.4f (sample_format_data.cpp:32-98,
// variant_call.cpp:171-204, :366-379).
inline constexpr const char* kVcfFormatKey =
    "GT:AD:ADF:ADR:DP:RMQ:NPBQ:SB:SCA:FLD:RPCD:BQCD:MQCD:ASMD:SDFC:PRAD:PANG:CMLOD:FSSE:AHDD:HSE:PDCV:PL:GQ";
inline double PolarRadius(double ref_depth, double alt_depth) {  // base/polar_coords.h:149-151
  return std::log10(1.0 + std::sqrt((ref_depth * ref_depth) + (alt_depth * alt_depth)));
}
inline double PolarAngle(double alt_depth, double ref_depth) {  // base/polar_coords.h:189-262 (minimax atan2, as the reference)
  constexpr double A = 0.1963, B = -0.9817, kHalfPi = 1.57079632679489661923, kQuarterPi = 0.78539816339744830962, kEps = 1e-10;
  double const abs_y = std::abs(alt_depth) + kEps, abs_x = std::abs(ref_depth);
  double const ratio = (ref_depth - std::copysign(abs_y, ref_depth)) / (abs_y + abs_x);
  double const base = kHalfPi - std::copysign(kQuarterPi, ref_depth);
  return std::copysign(base + (((A * ratio * ratio) + B) * ratio), alt_depth);
}
inline std::pair<int, int> GenotypeOfPlIndex(size_t best) {  // variant_call.cpp:262-290 (htslib's bcf_gt2alleles walk)
  size_t klen = 0, dk = 1;
  while (klen < best) {
    dk++;
    klen += dk;
  }
  size_t const j = dk - 1;
  return {static_cast<int>(best - klen + j), static_cast<int>(j)};
}
inline std::string FormatComplexityScore(double v) {  // base/longdust_scorer.h:340-350
  char buf[64];
  std::snprintf(buf, sizeof buf, "%.3f", v);
  std::string t = buf;
  if (t.find('.') != std::string::npos) {
    t.erase(t.find_last_not_of('0') + 1);
    if (t.back() == '.') t.pop_back();
  }
  return t;
}
inline std::string VcfHeader(Reference const& ref, std::vector<SampleInfo> const& samples, bool case_ctrl, bool annotated,
                             std::string const& command_line, std::string const& ref_path) {
  std::string h = "##fileformat=VCFv4.5\n##source=lancet2_amd_pipeline_driver\n##commandLine=\"" + command_line + "\"\n##reference=\"" + ref_path + "\"\n";
  for (auto const& c : ref.chroms) h += "##contig=<ID=" + c.name + ",length=" + std::to_string(c.seq.size()) + ">\n";
  if (case_ctrl)
    h += "##INFO=<ID=SHARED,Number=0,Type=Flag,Description=\"Variant ALT seen in both case & control sample(s)\">\n"
         "##INFO=<ID=CTRL,Number=0,Type=Flag,Description=\"Variant ALT seen only in control sample(s)\">\n"
         "##INFO=<ID=CASE,Number=0,Type=Flag,Description=\"Variant ALT seen only in case sample(s)\">\n";
  h += "##INFO=<ID=TYPE,Number=A,Type=String,Description=\"Variant type (SNV, INS, DEL, MNP)\">\n"
       "##INFO=<ID=LENGTH,Number=A,Type=Integer,Description=\"Variant length in base pairs\">\n"
       "##INFO=<ID=MULTIALLELIC,Number=0,Type=Flag,Description=\"Indicates if the site has multiple ALT alleles\">\n";
  if (annotated)
    h += "##INFO=<ID=GRAPH_CX,Number=3,Type=String,Description=\"Graph complexity metrics: GEI,TipToPathCovRatio,MaxSingleDirDegree\">\n"
         "##INFO=<ID=SEQ_CX,Number=11,Type=String,Description=\"Sequence complexity features: ContextHRun,ContextEntropy,ContextFlankLQ,"
         "ContextHaplotypeLQ,DeltaHRun,DeltaEntropy,DeltaFlankLQ,TrAffinity,TrPurity,TrPeriod,IsStutterIndel\">\n";
  static const char* kFmt[][4] = {{"GT", "1", "String", "Genotype"}, {"AD", "R", "Integer", "Allele depth"},
      {"ADF", "R", "Integer", "Forward strand allele depth"}, {"ADR", "R", "Integer", "Reverse strand allele depth"},
      {"DP", "1", "Integer", "Total read depth"}, {"RMQ", "R", "Float", "RMS mapping quality per allele"},
      {"NPBQ", "R", "Float", "Normalized posterior base quality per allele (raw PBQ / allele depth)"},
      {"SB", "1", "Float", "Strand bias log odds ratio (Haldane-corrected, coverage-invariant)"},
      {"SCA", "1", "Float", "Soft clip asymmetry (ALT minus REF)"},
      {"FLD", "1", "Float", "Fragment length delta (signed mean ALT isize minus mean REF isize)"},
      {"RPCD", "1", "Float", "Read position Cohen's D effect size (. if untestable)"},
      {"BQCD", "1", "Float", "Base quality Cohen's D effect size (. if untestable)"},
      {"MQCD", "1", "Float", "Mapping quality Cohen's D effect size (. if untestable)"},
      {"ASMD", "1", "Float", "Allele-specific mismatch delta (mean ALT NM minus mean REF NM minus variant length)"},
      {"SDFC", "1", "Float", "Site depth fold change (sample DP / per-sample window mean coverage)"},
      {"PRAD", "1", "Float", "Polar radius: log10(1 + sqrt(AD_Ref^2 + AD_Alt^2))"},
      {"PANG", "1", "Float", "Polar angle: allele identity ratio atan2(AD_Alt, AD_Ref) in radians"},
      {"CMLOD", "A", "Float", "Continuous mixture log-odds score per ALT allele (base-quality-weighted LOD vs null)"},
      {"FSSE", "1", "Float", "Fragment start Shannon entropy [0,1]"}, {"AHDD", "1", "Float", "ALT-haplotype discordance delta"},
      {"HSE", "1", "Float", "Haplotype segregation entropy [0,1]"}, {"PDCV", "1", "Float", "Path depth coefficient of variation"},
      {"PL", "G", "Integer", "Phred-scaled genotype likelihoods (Dirichlet-Multinomial model)"},
      {"GQ", "1", "Integer", "Genotype quality (second-lowest PL from the Dirichlet-Multinomial model, capped at 99)"}};
  for (auto const& f : kFmt)
    h += std::string("##FORMAT=<ID=") + f[0] + ",Number=" + f[1] + ",Type=" + f[2] + ",Description=\"" + f[3] + "\">\n";
  h += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT";
  for (auto const& s : samples) h += "\t" + s.name;
  return h + "\n";
}
// one VCF data line (variant_call.cpp:503-518); tags: the samples' roles, for the SHARED / CTRL / CASE state (:392-423)
inline std::string AsVcfRecord(VariantRecord const& r, Reference const& ref, std::vector<Tag> const& tags, bool case_ctrl) {
  static const char* kType[] = {"SNV", "INS", "DEL", "MNP", "CPX"};
  auto join = [](auto const& v) {
    std::string s;
    for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + std::to_string(v[i]);
    return s;
  };
  std::string info;
  if (case_ctrl) {
    bool in_ctrl = false, in_case = false;
    for (size_t s = 0; s < r.ad.size() && s < tags.size(); ++s) {
      uint32_t alt = 0;
      for (size_t a = 1; a < r.ad[s].size(); ++a) alt += r.ad[s][a];
      if (alt > 0) (tags[s] == Tag::CASE ? in_case : in_ctrl) = true;
    }
    info += in_case && in_ctrl ? "SHARED;" : (in_case ? "CASE;" : (in_ctrl ? "CTRL;" : "NONE;"));
  }
  if (r.alts.size() > 1) info += "MULTIALLELIC;";
  info += "TYPE=";
  for (size_t a = 0; a < r.alt_type.size(); ++a) info += std::string(a ? "," : "") + (r.alt_type[a] >= 0 && r.alt_type[a] < 5 ? kType[r.alt_type[a]] : "REF");
  info += ";LENGTH=" + join(r.alt_length);
  if (!r.graph_cx.empty()) info += ";GRAPH_CX=" + r.graph_cx;
  if (!r.seq_cx.empty()) info += ";SEQ_CX=" + r.seq_cx;
  char buf[96];
  std::snprintf(buf, sizeof buf, "%.2f", r.qual);
  std::string line = ref.chroms[static_cast<size_t>(r.chrom)].name + "\t" + std::to_string(r.pos1) + "\t.\t" + r.ref + "\t";
  for (size_t a = 0; a < r.alts.size(); ++a) line += (a ? "," : "") + r.alts[a];
  line += std::string("\t") + buf + "\t.\t" + info + "\t" + kVcfFormatKey;
  for (size_t s = 0; s < r.ad.size(); ++s) {
    uint64_t dp = 0;
    for (uint32_t c : r.ad[s]) dp += c;
    if (dp == 0) {  // no read of this sample was assigned here: SampleFormatData::SetMissingSupport
      line += "\t./.:.:.:.:.:.:.:.:.:.:.:.:.:.:.:.:.:.:.:.:.:.:.:.";
      continue;
    }
    std::string gt = "./.", pl = ".";
    if (s < r.pl.size() && !r.pl[s].empty()) {
      size_t const best = static_cast<size_t>(std::min_element(r.pl[s].begin(), r.pl[s].end()) - r.pl[s].begin());
      auto const g = GenotypeOfPlIndex(best);
      gt = std::to_string(g.first) + "/" + std::to_string(g.second);
      pl = join(r.pl[s]);
    }
    double alt = 0.0;
    for (size_t a = 1; a < r.ad[s].size(); ++a) alt += r.ad[s][a];
    std::string sdfc = ".";
    if (s < r.sample_window_cov.size() && r.sample_window_cov[s] > 0.0) {
      std::snprintf(buf, sizeof buf, "%.2f", static_cast<double>(dp) / r.sample_window_cov[s]);
      sdfc = buf;
    }
    char polar[64];
    std::snprintf(polar, sizeof polar, "%.4f:%.4f", static_cast<double>(static_cast<float>(PolarRadius(r.ad[s][0], alt))),
                  static_cast<double>(static_cast<float>(PolarAngle(alt, r.ad[s][0]))));
    // SB = ln(((rf+1)(ar+1)) / ((rr+1)(af+1))), ALT summed over the non-REF alleles, stored as f32, printed {:.3f}
    // (caller/variant_support.cpp:197-237, variant_call.cpp:167, sample_format_data.cpp:82): a closed form of ADF / ADR
    std::string sb = ".";
    if (s < r.adf.size() && s < r.adr.size() && !r.adf[s].empty() && r.adf[s].size() == r.adr[s].size()) {
      int af = 0, ar = 0;
      for (size_t a = 1; a < r.adf[s].size(); ++a) {
        af += static_cast<int>(r.adf[s][a]);
        ar += static_cast<int>(r.adr[s][a]);
      }
      double const rf1 = static_cast<double>(static_cast<int>(r.adf[s][0]) + 1), rr1 = static_cast<double>(static_cast<int>(r.adr[s][0]) + 1);
      double const af1 = static_cast<double>(af + 1), ar1 = static_cast<double>(ar + 1);
      char sbuf[48];
      std::snprintf(sbuf, sizeof sbuf, "%.3f", static_cast<double>(static_cast<float>(std::log((rf1 * ar1) / (rr1 * af1)))));
      sb = sbuf;
    }
    // the read-level statistics: a number, or "." for a value that is missing (NaN) or was not computed
    auto num = [](double x, const char* spec, bool via_f32) {
      if (std::isnan(x)) return std::string(".");
      char nb[64];
      std::snprintf(nb, sizeof nb, spec, via_f32 ? static_cast<double>(static_cast<float>(x)) : x);
      return std::string(nb);
    };
    auto list = [&](std::vector<std::vector<double>> const& per_sample, const char* spec, bool via_f32) {
      if (s >= per_sample.size() || per_sample[s].empty()) return std::string(".");
      std::string t;
      for (size_t i = 0; i < per_sample[s].size(); ++i) t += (i ? "," : "") + num(per_sample[s][i], spec, via_f32);
      return t;
    };
    double const kNan = std::numeric_limits<double>::quiet_NaN();
    std::array<double, 4> const st = s < r.fmt_stat.size() ? r.fmt_stat[s] : std::array<double, 4>{kNan, kNan, kNan, kNan};
    std::array<double, 5> const mt = s < r.fmt_mstat.size() ? r.fmt_mstat[s] : std::array<double, 5>{kNan, kNan, kNan, kNan, kNan};
    line += "\t" + gt + ":" + join(r.ad[s]) + ":" + (s < r.adf.size() ? join(r.adf[s]) : ".") + ":" +
            (s < r.adr.size() ? join(r.adr[s]) : ".") + ":" + std::to_string(dp) + ":" + list(r.rmq, "%.1F", true) + ":" +
            list(r.npbq, "%.1F", true) + ":" + sb + ":" + num(mt[0], "%.4f", true) + ":" + num(mt[1], "%.1f", true) + ":" +
            num(mt[2], "%.4f", true) + ":" + num(st[0], "%.4f", true) + ":" + num(mt[3], "%.4f", true) + ":" +
            num(st[1], "%.3f", true) + ":" + sdfc + ":" + polar + ":" +
            list(r.cmlod, "%.4F", false) + ":" + num(mt[4], "%.4f", true) + ":" + num(st[2], "%.3f", true) + ":" + num(st[3], "%.4f", true) + ":" +
            num(r.pdcv, "%.4f", true) + ":" + pl + ":" + (s < r.gq.size() ? std::to_string(r.gq[s]) : ".");
  }
  return line;
}

// the engine's per-window outputs of one batch -> records: what VariantBuilder::CollectSupportedCalls hands to the store
// (core/variant_builder.cpp:184-199).  A genotyped variant WITHOUT ALT support in any sample never becomes a VariantCall there,
// so it is dropped HERE, before VariantStore::AddVariants: kept, it could replace a supported call of the same CHROM+POS+REF
// from the overlapping window by having more total coverage, and the flush would then drop both.  `supported_only = false`
// returns every record (tests; callers that want the raw per-window table).
inline std::vector<VariantRecord> RecordsOfBatch(const ma_params_t& p, FlatBatch const& fb, const ma_var_out_t& v, const ma_geno_out_t& q,
                                                 const ma_cx_out_t* cx = nullptr, bool supported_only = true,
                                                 const ma_fmt_out_t* fmt = nullptr, const ma_asm_out_t* asmb = nullptr,
                                                 const ma_fmt_meta_out_t* fmeta = nullptr) {
  std::vector<VariantRecord> out;
  int const MV = p.max_vars, MA = p.max_alts, S = p.num_samples, NA = MA + 1;
  for (size_t w = 0; w < fb.windows.size(); ++w) {
    const uint8_t* pool = v.allele_pool + w * static_cast<size_t>(p.max_allele_bytes);
    for (uint32_t x = 0; x < v.win_nvars[w]; ++x) {
      size_t const vi = w * static_cast<size_t>(MV) + x;
      VariantRecord r;
      r.chrom = fb.windows[w].chrom;
      r.pos1 = fb.windows[w].start1 + v.var_pos[vi];
      r.window_index = fb.windows[w].genome_index;
      r.ref.assign(reinterpret_cast<const char*>(pool) + v.var_ref_off[vi], v.var_ref_len[vi]);
      for (uint32_t a = 0; a < v.var_nalts[vi]; ++a)
        r.alts.emplace_back(reinterpret_cast<const char*>(pool) + v.alt_off[vi * MA + a], v.alt_len[vi * MA + a]);
      r.qual = q.var_qual[vi];
      r.ad.assign(static_cast<size_t>(S), {});
      r.adf.assign(static_cast<size_t>(S), {});
      r.adr.assign(static_cast<size_t>(S), {});
      uint32_t const K = v.var_nalts[vi] + 1, G = static_cast<uint32_t>(NA * (NA + 1) / 2);
      for (int s = 0; s < S; ++s) {
        for (uint32_t al = 0; al < K; ++al) {
          const uint32_t* c = q.allele_counts + ((vi * S + s) * NA + al) * 2;
          r.ad[static_cast<size_t>(s)].push_back(c[0] + c[1]);
          r.adf[static_cast<size_t>(s)].push_back(c[0]);
          r.adr[static_cast<size_t>(s)].push_back(c[1]);
        }
        if (q.var_pl) {
          const uint32_t* pl = q.var_pl + (vi * S + s) * G;
          r.pl.emplace_back(pl, pl + K * (K + 1) / 2);
        }
        if (q.var_gq) r.gq.push_back(q.var_gq[vi * S + s]);
        if (fmt) {  // the read-level statistics of this (variant, sample)
          size_t const cell = vi * S + s;
          if (fmt->fmt_npbq) r.npbq.emplace_back(fmt->fmt_npbq + cell * NA, fmt->fmt_npbq + cell * NA + K);
          if (fmt->fmt_cmlod) r.cmlod.emplace_back(fmt->fmt_cmlod + cell * MA, fmt->fmt_cmlod + cell * MA + (K - 1));
          if (fmt->fmt_stat) r.fmt_stat.push_back({fmt->fmt_stat[cell * 4], fmt->fmt_stat[cell * 4 + 1], fmt->fmt_stat[cell * 4 + 2], fmt->fmt_stat[cell * 4 + 3]});
        }
        if (fmeta) {  // ... and the six over the read metadata
          size_t const cell = vi * S + s;
          if (fmeta->fmt_rmq) r.rmq.emplace_back(fmeta->fmt_rmq + cell * NA, fmeta->fmt_rmq + cell * NA + K);
          if (fmeta->fmt_mstat) {
            const double* m = fmeta->fmt_mstat + cell * 5;
            r.fmt_mstat.push_back({m[0], m[1], m[2], m[3], m[4]});
          }
        }
      }
      if (asmb && asmb->comp_cxf) {  // PDCV: MaxAltPathCv of the variant's component, -1 = no ALT path
        double const cv = asmb->comp_cxf[(w * static_cast<size_t>(p.max_comps) + v.var_comp[vi]) * 4 + 3];
        if (cv >= 0.0) r.pdcv = cv;
      }
      for (uint32_t a = 0; a < v.var_nalts[vi]; ++a) {
        r.alt_type.push_back(v.alt_type[vi * MA + a]);
        r.alt_length.push_back(v.alt_length[vi * MA + a]);
      }
      if (supported_only && !r.HasAltSupport()) continue;  // variant_builder.cpp:189-194
      if (w < fb.sample_cov.size()) r.sample_window_cov = fb.sample_cov[w];
      if (cx) {  // caller/raw_variant.h:43-46, base/sequence_complexity.cpp:462-469
        const int32_t* ci = cx->seq_cx_i + vi * 4;
        const float* cf = cx->seq_cx_f + vi * 4;
        const double* cd = cx->seq_cx_d + vi * 3;
        const double* gx = cx->graph_cx + vi * 3;
        r.seq_cx = std::to_string(ci[0]) + "," + FormatComplexityScore(cf[0]) + "," + FormatComplexityScore(cd[0]) + "," +
                   FormatComplexityScore(cd[1]) + "," + std::to_string(ci[1]) + "," + FormatComplexityScore(cf[1]) + "," +
                   FormatComplexityScore(cd[2]) + "," + FormatComplexityScore(cf[2]) + "," + FormatComplexityScore(cf[3]) + "," +
                   std::to_string(ci[2]) + "," + std::to_string(ci[3]);
        r.graph_cx = FormatComplexityScore(gx[0]) + "," + FormatComplexityScore(gx[1]) + "," + std::to_string(static_cast<long long>(gx[2]));
      }
      out.push_back(std::move(r));
    }
  }
  return out;
}

// ---- graph snapshots: one DOT digraph per exported component (ma_assemble_graph_batch) --------------------------------------
// What the reference buffers per component with --out-graphs-tgz (cbdg/graph.cpp:216-223), drawn from the export's arrays and
// the assembly rows of the same call.  Per node: the stored sequence, its reverse complement, `slot:sign`, length and total
// read support; the component's two anchors are boxes.  Per stored edge: the signs on its tail and head side.  The edges of
// every haplotype's walk carry that haplotype's colour (walk 0 = REF); an edge on several walks carries all of them.  A walk
// is found from the row's bases alone: the walk from the source anchor that spells them, the first node whole and every next
// one minus its first k - 1 bases, a node read as stored when the edge's sign on its side is +, reverse complemented
// otherwise, every edge leaving on the sign the walk arrived with (max_flow.cpp:64-113).
namespace dot_detail {
inline std::string RevCompAscii(std::string_view s) {
  std::string out(s.size(), 'N');
  for (size_t i = 0; i < s.size(); ++i) {
    char const c = s[s.size() - 1 - i];
    out[i] = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c == 'a' ? 't' : c == 'c' ? 'g' : c == 'g' ? 'c' : c == 't' ? 'a' : (c == 'n' ? 'n' : 'N');
  }
  return out;
}
struct DotEdge {
  uint32_t src, dst, kind;
  std::vector<uint32_t> walks;  // haplotypes whose walk crosses it
};
}  // namespace dot_detail

inline constexpr const char* kDotWalkColours[8] = {"royalblue3", "firebrick2", "darkorange2", "seagreen4", "orchid3", "goldenrod3", "turquoise4", "sienna"};

// w: window index in the batch; comp: component slot (< win_ncomp[w]); k: win_k[w]; title: the graph's name.  Returns the empty
// string when the window's export is flagged (ma_gstatus) or holds no node of the component.
inline std::string RenderComponentDot(const ma_params_t& p, const ma_asm_out_t& a, const ma_graph_out_t& g, int w, uint32_t comp, uint32_t k,
                                      std::string const& title) {
  using dot_detail::DotEdge;
  size_t const W = static_cast<size_t>(w), MN = static_cast<size_t>(g.max_nodes), ME = static_cast<size_t>(g.max_edges),
               MS = static_cast<size_t>(g.max_seq_bytes), S = static_cast<size_t>(p.num_samples);
  if (g.win_gstatus[W] != 0) return {};
  uint32_t const nn = g.win_nnodes[W], ne = g.win_nedges[W];
  auto seq_of = [&](uint32_t s) {
    return std::string_view(reinterpret_cast<const char*>(g.seq_pool) + W * MS + g.node_seq_off[W * MN + s], g.node_len[W * MN + s]);
  };
  std::vector<uint32_t> mine;
  for (uint32_t s = 0; s < nn; ++s)
    if (g.node_comp[W * MN + s] == comp) mine.push_back(s);
  if (mine.empty()) return {};
  std::vector<DotEdge> edges;
  std::unordered_map<uint32_t, std::vector<size_t>> out_of;  // node slot -> its edges
  uint32_t source = UINT32_MAX;
  for (uint32_t e = 0; e < ne; ++e) {
    uint32_t const src = g.edge_src[W * ME + e];
    if (g.node_comp[W * MN + src] != comp) continue;
    out_of[src].push_back(edges.size());
    edges.push_back(DotEdge{src, g.edge_dst[W * ME + e], g.edge_kind[W * ME + e], {}});
  }
  for (uint32_t s : mine)
    if (g.node_flags[W * MN + s] & 1u) source = s;
  // the walk of every haplotype row of the component
  size_t const ci = W * static_cast<size_t>(p.max_comps) + comp;
  uint32_t const hap0 = a.comp_hap0[ci], nh = a.comp_nhaps[ci];
  for (uint32_t h = 0; h < nh && source != UINT32_MAX; ++h) {
    size_t const hi = W * static_cast<size_t>(p.max_haps) + hap0 + h;
    std::string_view const target(reinterpret_cast<const char*>(a.hap_bases) + hi * static_cast<size_t>(p.max_hap_len), a.hap_len[hi]);
    std::vector<size_t> walk, found;
    std::function<bool(uint32_t, uint32_t, size_t)> go = [&](uint32_t node, uint32_t sign, size_t pos) -> bool {
      if (pos == target.size() && (g.node_flags[W * MN + node] & 2u) && !walk.empty()) {
        found = walk;
        return true;
      }
      for (size_t ei : out_of[node]) {
        DotEdge const& e = edges[ei];
        if (((e.kind >> 1) & 1u) != sign) continue;
        std::string_view const ds = seq_of(e.dst);
        if (ds.size() + 1 < k) continue;  // (a node is never shorter than k)
        std::string const piece = (e.kind & 1u) ? dot_detail::RevCompAscii(ds).substr(k - 1) : std::string(ds.substr(k - 1));
        if (pos + piece.size() > target.size() || target.compare(pos, piece.size(), piece) != 0) continue;
        walk.push_back(ei);
        if (go(e.dst, e.kind & 1u, pos + piece.size())) return true;
        walk.pop_back();
      }
      return false;
    };
    for (uint32_t sign = 0; sign < 2 && found.empty(); ++sign) {
      std::string const first = sign ? dot_detail::RevCompAscii(seq_of(source)) : std::string(seq_of(source));
      if (target.size() >= first.size() && target.compare(0, first.size(), first) == 0) go(source, sign, first.size());
    }
    for (size_t ei : found) edges[ei].walks.push_back(h);
  }
  std::ostringstream os;
  os << "digraph \"" << title << "\" {\n  rankdir=LR;\n  node [fontname=\"monospace\", fontsize=9];\n";
  for (uint32_t s : mine) {
    size_t const i = W * MN + s;
    unsigned long long cov = 0;
    for (size_t x = 0; x < S; ++x) cov += g.node_cnt[i * S + x];
    std::string_view const sq = seq_of(s);
    uint8_t const fl = g.node_flags[i];
    os << "  n" << s << " [label=\"" << sq << "\\n" << dot_detail::RevCompAscii(sq) << "\\n" << s << ":" << (g.node_sign[i] ? '+' : '-')
       << " len=" << sq.size() << " cov=" << cov << "\"";
    if (fl & 1u) os << ", shape=box, style=filled, fillcolor=palegreen, xlabel=\"source\"";
    else if (fl & 2u) os << ", shape=box, style=filled, fillcolor=lightsalmon, xlabel=\"sink\"";
    else if (g.node_label[i] & 1u) os << ", style=filled, fillcolor=gray90";
    os << "];\n";
  }
  for (auto const& e : edges) {
    os << "  n" << e.src << " -> n" << e.dst << " [taillabel=\"" << (((e.kind >> 1) & 1u) ? '-' : '+') << "\", headlabel=\""
       << ((e.kind & 1u) ? '-' : '+') << "\"";
    if (!e.walks.empty()) {
      os << ", penwidth=2, color=\"";
      for (size_t x = 0; x < e.walks.size(); ++x) os << (x ? ":" : "") << kDotWalkColours[e.walks[x] % 8];
      os << "\"";
    }
    os << "];\n";
  }
  os << "}\n";
  return os.str();
}

// ---- MSA snapshots: the GFA and the FASTA of one exported component (ma_msa_graph_batch) ------------------------------------
// Character for character what MsaBuilder::BuildGfaString / BuildFastaString print (caller/msa_builder.cpp:44-102): a segment
// per POA node (its id + 1) followed by the links of its out-edges, a path per haplotype (ref0, hap1, ...) walked from
// hap_first along the edges that carry the haplotype's label; the gapped rows.  Both return the empty string when the
// window's export is flagged (ma_pstatus) or the component has no node.
inline std::string RenderComponentGfa(const ma_params_t& p, const ma_asm_out_t& a, const ma_poa_out_t& x, int w, uint32_t comp) {
  size_t const W = static_cast<size_t>(w), MN = static_cast<size_t>(x.max_pnodes), ME = static_cast<size_t>(x.max_pedges);
  size_t const ci = W * static_cast<size_t>(p.max_comps) + comp;
  uint32_t const nn = x.comp_npnodes[ci], ne = x.comp_npedges[ci];
  if (x.win_pstatus[W] != 0 || nn == 0) return {};
  size_t const nb = W * MN + x.comp_pnode0[ci], eb = W * ME + x.comp_pedge0[ci];
  std::vector<uint32_t> first_edge(nn + 1, ne);  // a node's edges are contiguous, nodes in id order
  for (uint32_t e = ne; e-- > 0;) first_edge[x.pedge_tail[eb + e]] = e;
  for (uint32_t v = nn; v-- > 0;) first_edge[v] = std::min(first_edge[v], first_edge[v + 1]);
  std::string out = "H\tVN:Z:1.0\n";
  for (uint32_t v = 0; v < nn; ++v) {
    out += "S\t" + std::to_string(v + 1) + "\t" + static_cast<char>(x.pnode_base[nb + v]) + "\n";
    for (uint32_t e = first_edge[v]; e < first_edge[v + 1]; ++e)
      out += "L\t" + std::to_string(v + 1) + "\t+\t" + std::to_string(x.pedge_head[eb + e] + 1) + "\t+\t0M\n";
  }
  uint32_t const hap0 = a.comp_hap0[ci], nh = a.comp_nhaps[ci];
  for (uint32_t h = 0; h < nh; ++h) {
    out += std::string("P\t") + (h == 0 ? "ref" : "hap") + std::to_string(h) + "\t";
    uint32_t cur = x.hap_first[W * static_cast<size_t>(p.max_haps) + hap0 + h];
    for (uint32_t steps = 0; cur < nn && steps < nn; ++steps) {
      out += (steps ? "," : "") + std::to_string(cur + 1) + "+";
      uint32_t next = UINT32_MAX;
      for (uint32_t e = first_edge[cur]; e < first_edge[cur + 1] && next == UINT32_MAX; ++e)
        if ((x.pedge_haps[eb + e] >> h) & 1u) next = x.pedge_head[eb + e];
      cur = next;
    }
    out += "\t*\n";
  }
  return out;
}

inline std::string RenderComponentFasta(const ma_params_t& p, const ma_asm_out_t& a, const ma_poa_out_t& x, int w, uint32_t comp) {
  size_t const W = static_cast<size_t>(w), MX = static_cast<size_t>(x.max_cols);
  size_t const ci = W * static_cast<size_t>(p.max_comps) + comp;
  if (x.win_pstatus[W] != 0 || x.comp_npnodes[ci] == 0) return {};
  uint32_t const hap0 = a.comp_hap0[ci], nh = a.comp_nhaps[ci], ncols = x.comp_ncols[ci];
  std::string out;
  for (uint32_t h = 0; h < nh; ++h) {
    const char* row = reinterpret_cast<const char*>(x.msa) + (W * static_cast<size_t>(p.max_haps) + hap0 + h) * MX;
    out += std::string(">") + (h == 0 ? "ref" : "hap") + std::to_string(h) + "\n" + std::string(row, ncols) + "\n";
  }
  return out;
}

// ---- probe variants: the reference's --probe-variants input and --probe-results output around ma_assemble_probe_batch ----
struct ProbeVariant {  // cbdg/probe_index.h:18-35
  std::string chrom, ref, alt;
  uint64_t start0 = 0;
  uint32_t raw_alt = 0;
};
// missed_variants.txt (cbdg/probe_index.cpp:144-204): a header line, then tab-separated chrom, 0-based start, end, ref, alt,
// type, length, classification, raw_alt_count, ...; like the reference a line of fewer than nine fields, or whose start or
// raw_alt_count is no number, is skipped, and a probe's id is its index among the lines that were taken
inline std::vector<ProbeVariant> LoadProbeVariants(std::string const& path) {
  std::ifstream in(path);
  if (!in) throw std::runtime_error("--probe-variants: cannot open " + path);
  std::vector<ProbeVariant> out;
  std::string line;
  std::getline(in, line);  // header
  while (std::getline(in, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    std::vector<std::string> f;
    for (size_t at = 0;;) {
      size_t const tab = line.find('\t', at);
      f.push_back(line.substr(at, tab == std::string::npos ? std::string::npos : tab - at));
      if (tab == std::string::npos) break;
      at = tab + 1;
    }
    auto number = [](std::string const& s, uint64_t* v) {
      if (s.empty() || s.find_first_not_of("0123456789") != std::string::npos || s.size() > 18) return false;
      *v = std::stoull(s);
      return true;
    };
    uint64_t start = 0, raw = 0;
    if (f.size() < 9 || !number(f[8], &raw) || raw > 65535 || !number(f[1], &start)) continue;
    ProbeVariant v;
    v.chrom = f[0]; v.ref = f[3]; v.alt = f[4];
    v.start0 = start; v.raw_alt = static_cast<uint32_t>(raw);
    out.push_back(std::move(v));
  }
  return out;
}

// the header of probe_results.tsv (cbdg/probe_results_writer.cpp:51-59), forty columns
inline constexpr const char* kProbeResultsHeader =
    "probe_id\tchrom\tpos\tref\talt\twindow\tn_raw_alt_reads\tkmer_size\tn_expected_alt_kmers\tn_alt_kmers_in_reads\t"
    "comp_id\tn_comp_nodes\tn_split_across_comps\tn_surviving_build\tn_surviving_lowcov1\tn_surviving_compress1\t"
    "n_surviving_lowcov2\tn_surviving_compress2\tn_surviving_tips\thap_indices\tis_traversal_limited\t"
    "is_graph_cycle\tis_graph_complex\tis_no_anchor\tis_short_anchor\tis_variant_in_anchor\t"
    "n_last_edge_kmers\tn_last_interior_kmers\tn_last_chain_gaps\t"
    "msa_shift_bp\tis_msa_exact_match\tis_msa_shifted\tis_msa_subsumed\t"
    "n_geno_true_alt_reads\tn_geno_total_ref_reads\tn_geno_reassigned_to_ref\t"
    "n_geno_reassigned_to_wrong_alt\tn_geno_non_overlapping\tis_geno_has_alt_support\tis_geno_no_overlap\n";

// The probes of one batch as ma_probes_t wants them.  A variant is activated in every window whose region holds its start
// (probe_tracker.cpp:259-266: same chromosome, region start <= start < region end) -- unless its REF allele runs past the
// window's end, an allele is longer than 256 bases or the window already has 256 probes (the call's limits): those are counted
// in `skipped`.  id[i] = the variant of probe i.
struct ProbeBatch {
  std::vector<uint32_t> win_off, pos, ref_len, alt_off, alt_len, id;
  std::vector<uint8_t> pool;
  size_t skipped = 0;
  ma_probes_t View() const {
    ma_probes_t v{};
    v.probe_win_off = win_off.data(); v.probe_pos = pos.data(); v.probe_ref_len = ref_len.data();
    v.probe_alt_off = alt_off.data(); v.probe_alt_len = alt_len.data(); v.alt_pool = pool.data();
    return v;
  }
};
template <class Windows, class ChromName>
inline ProbeBatch ActivateProbes(std::vector<ProbeVariant> const& variants, Windows const& windows, ChromName&& chrom_name) {
  ProbeBatch pb;
  pb.win_off.push_back(0);
  for (auto const& w : windows) {
    uint64_t const s0 = w.start1 - 1, e0 = w.end1;  // the window's bases, 0-based half-open
    std::string const& name = chrom_name(w.chrom);
    uint32_t taken = 0;
    for (size_t i = 0; i < variants.size(); ++i) {
      ProbeVariant const& v = variants[i];
      if (v.chrom != name || v.start0 < s0 || v.start0 >= e0) continue;
      if (v.start0 + v.ref.size() > e0 || v.ref.size() > 256 || v.alt.size() > 256 || taken == 256) {
        ++pb.skipped;
        continue;
      }
      pb.pos.push_back(static_cast<uint32_t>(v.start0 - s0));
      pb.ref_len.push_back(static_cast<uint32_t>(v.ref.size()));
      pb.alt_off.push_back(static_cast<uint32_t>(pb.pool.size()));
      pb.alt_len.push_back(static_cast<uint32_t>(v.alt.size()));
      pb.pool.insert(pb.pool.end(), v.alt.begin(), v.alt.end());
      pb.id.push_back(static_cast<uint32_t>(i));
      ++taken;
    }
    pb.win_off.push_back(static_cast<uint32_t>(pb.pos.size()));
  }
  pb.pool.push_back(0);  // (never empty: the call wants a pointer)
  for (auto* v : {&pb.pos, &pb.ref_len, &pb.alt_off, &pb.alt_len})
    if (v->empty()) v->push_back(0);
  return pb;
}

// The lines of probe i (window w of the batch, named `region`): one per row of comp_* -- one with comp_id "." for a window
// without a component, so that the reads' and the raw graph's counts are not lost.  Columns the engine does not produce are
// ".": n_comp_nodes, n_split_across_comps, build, compress1 / 2, lowcov2, the structural flags, the MSA and genotyper columns.
inline std::string RenderProbeLines(const ma_params_t& p, const ma_asm_out_t& a, const ma_probe_out_t& o, size_t i, int w, uint32_t probe_id,
                                    ProbeVariant const& v, std::string const& region) {
  size_t const MC = static_cast<size_t>(p.max_comps);
  uint32_t const ncomp = a.win_ncomp[w];
  std::string const head = std::to_string(probe_id) + "\t" + v.chrom + "\t" + std::to_string(v.start0) + "\t" + v.ref + "\t" + v.alt + "\t" + region +
                           "\t" + std::to_string(v.raw_alt) + "\t" + std::to_string(o.pb_k[i]) + "\t" + std::to_string(o.pb_alt_kmers[i]) + "\t" +
                           std::to_string(o.pb_in_reads[2 * i]) + "\t";
  std::string out;
  for (uint32_t c = 0; c < (ncomp ? ncomp : 1u); ++c) {
    const uint32_t* fin = o.pb_final + 4 * (i * MC + c);
    std::string haps;
    if (ncomp)
      for (uint32_t h = 0; h < 32; ++h)
        if (o.pb_hap_mask[i * MC + c] >> h & 1u) haps += (haps.empty() ? "" : ",") + std::to_string(h);
    auto fin_or_dot = [&](int x) { return ncomp ? std::to_string(fin[x]) : std::string("."); };
    out += head + (ncomp ? std::to_string(c) : std::string(".")) + "\t.\t.\t.\t" + std::to_string(o.pb_lowcov1[4 * i]) + "\t.\t.\t.\t" + fin_or_dot(0) +
           "\t" + (haps.empty() ? "." : haps) + "\t.\t.\t.\t.\t.\t.\t" + fin_or_dot(1) + "\t" + fin_or_dot(2) + "\t" + fin_or_dot(3) +
           "\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\n";
  }
  return out;
}

}  // namespace lancet2_amd::host
