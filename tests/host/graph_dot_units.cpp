// RenderComponentDot (lancet2_amd/host/pipeline_host.hpp) on the hand-written bubble of tests/test_graph_export_ref.py:
// seven nodes, a tip, the SNV branch stored reverse complemented with sign MINUS.  Built with g++ by tests/test_graph_dot.py.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../lancet2_amd/host/pipeline_host.hpp"

using namespace lancet2_amd::host;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

static size_t count_of(std::string const& hay, std::string const& needle) {
  size_t n = 0;
  for (size_t at = hay.find(needle); at != std::string::npos; at = hay.find(needle, at + needle.size())) ++n;
  return n;
}

int main() {
  constexpr uint32_t K = 5;
  ma_params_t p;
  std::memset(&p, 0, sizeof p);
  p.num_samples = 2; p.max_comps = 2; p.max_haps = 4; p.max_hap_len = 64; p.max_runs = 8;
  // S A B1 B2 C T X; B2 is stored as RevComp(ATTCACAAG) with sign MINUS
  const char* seqs[7] = {"ACGTACGGA", "CGGATTC", "ATTCGCAAG", "CTTGTGAAT", "CAAGTTGCA", "TGCATCGAT", "TGCAGG"};
  uint32_t const cnts[7][2] = {{10, 10}, {9, 11}, {6, 6}, {4, 4}, {10, 10}, {10, 10}, {1, 1}};
  uint8_t const sign[7] = {1, 1, 1, 0, 1, 1, 1}, label[7] = {7, 7, 7, 6, 7, 7, 4}, flags[7] = {1, 0, 0, 0, 0, 2, 0};
  std::vector<uint32_t> gst{0}, nn{7}, ne{14}, nsq{0}, comp(8, 0), off(8, 0), len(8, 0), cnt(16, 0), es, ed;
  std::vector<uint8_t> sg(8, 0), lb(8, 0), fl(8, 0), ek, pool(80, 0);
  uint32_t at = 0;
  for (int i = 0; i < 7; ++i) {
    off[i] = at; len[i] = static_cast<uint32_t>(std::strlen(seqs[i]));
    std::memcpy(pool.data() + at, seqs[i], len[i]);
    at += len[i];
    cnt[2 * i] = cnts[i][0]; cnt[2 * i + 1] = cnts[i][1];
    sg[i] = sign[i]; lb[i] = label[i]; fl[i] = flags[i];
  }
  nsq[0] = at;
  // stored edges (source, destination, kind = source sign << 1 | destination sign; MINUS = 1), mirrors included
  uint32_t const edges[14][3] = {{0, 1, 0}, {1, 2, 0}, {1, 3, 1}, {1, 0, 3}, {2, 4, 0}, {2, 1, 3}, {3, 4, 2}, {3, 1, 1},
                                 {4, 5, 0}, {4, 6, 0}, {4, 2, 3}, {4, 3, 2}, {5, 4, 3}, {6, 4, 3}};
  for (auto const& e : edges) { es.push_back(e[0]); ed.push_back(e[1]); ek.push_back(static_cast<uint8_t>(e[2])); }
  es.resize(16); ed.resize(16); ek.resize(16);
  ma_graph_out_t g{};
  g.max_nodes = 8; g.max_edges = 16; g.max_seq_bytes = 80;
  g.win_gstatus = gst.data(); g.win_nnodes = nn.data(); g.win_nedges = ne.data(); g.win_nseq = nsq.data();
  g.node_comp = comp.data(); g.node_seq_off = off.data(); g.node_len = len.data(); g.node_cnt = cnt.data();
  g.node_sign = sg.data(); g.node_label = lb.data(); g.node_flags = fl.data();
  g.edge_src = es.data(); g.edge_dst = ed.data(); g.edge_kind = ek.data(); g.seq_pool = pool.data();
  // the assembly rows: REF (through B1) and one ALT (through B2)
  std::string const ref_seq = "ACGTACGGATTCGCAAGTTGCATCGAT", alt_seq = "ACGTACGGATTCACAAGTTGCATCGAT";
  std::vector<uint32_t> ncomp{1}, wk{K}, hap0(2, 0), nhaps{2, 0}, hlen{27, 27, 0, 0};
  std::vector<uint8_t> bases(4 * 64, 0);
  std::memcpy(bases.data(), ref_seq.data(), 27);
  std::memcpy(bases.data() + 64, alt_seq.data(), 27);
  ma_asm_out_t a{};
  a.win_ncomp = ncomp.data(); a.win_k = wk.data(); a.comp_hap0 = hap0.data(); a.comp_nhaps = nhaps.data();
  a.hap_len = hlen.data(); a.hap_bases = bases.data();

  std::string const dot = RenderComponentDot(p, a, g, 0, 0, K, "chr1_1_30__c0__k5");
  CHECK(dot.rfind("digraph \"chr1_1_30__c0__k5\" {", 0) == 0);
  CHECK(count_of(dot, " [label=\"") == 7);                 // one statement per node
  CHECK(count_of(dot, " -> ") == 14);                      // one per stored edge, mirrors included
  CHECK(count_of(dot, "xlabel=\"source\"") == 1 && count_of(dot, "xlabel=\"sink\"") == 1);
  CHECK(dot.find("n0 [label=\"ACGTACGGA\\nTCCGTACGT\\n0:+ len=9 cov=20\", shape=box") != std::string::npos);
  CHECK(dot.find("n3 [label=\"CTTGTGAAT\\nATTCACAAG\\n3:- len=9 cov=8\"") != std::string::npos);
  CHECK(dot.find("n1 -> n3 [taillabel=\"+\", headlabel=\"-\", penwidth=2, color=\"firebrick2\"]") != std::string::npos);
  CHECK(dot.find("n3 -> n4 [taillabel=\"-\", headlabel=\"+\", penwidth=2, color=\"firebrick2\"]") != std::string::npos);
  CHECK(dot.find("n1 -> n2 [taillabel=\"+\", headlabel=\"+\", penwidth=2, color=\"royalblue3\"]") != std::string::npos);
  // the shared edges carry both walks' colours, the mirrors and the tip's edge none: 4 edges per walk, 2 of them shared
  CHECK(count_of(dot, "color=\"royalblue3:firebrick2\"") == 2);
  CHECK(count_of(dot, "color=\"royalblue3\"") == 2 && count_of(dot, "color=\"firebrick2\"") == 2);
  CHECK(count_of(dot, "penwidth=2") == 6);
  // a flagged window, or a component without nodes, renders nothing
  gst[0] = MA_G_NODE_OVERFLOW;
  CHECK(RenderComponentDot(p, a, g, 0, 0, K, "x").empty());
  gst[0] = 0;
  CHECK(RenderComponentDot(p, a, g, 0, 1, K, "x").empty());
  if (failures) return 1;
  std::printf("graph dot units ok\n");
  return 0;
}
