// RenderComponentDot (lancet2_amd/host/pipeline_host.hpp) on rows a test took from ma_assemble_graph_batch: reads the arrays of
// ONE window from raw files in a directory (one file per array, named after the struct member) and prints the DOT text of one
// component.  usage: graph_dot_render DIR COMP K NUM_SAMPLES MAX_COMPS MAX_HAPS MAX_HAP_LEN MAX_NODES MAX_EDGES MAX_SEQ_BYTES
// Built with g++ by tests/test_gpu_graph_export.py.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../lancet2_amd/host/pipeline_host.hpp"

using namespace lancet2_amd::host;

static std::vector<char> slurp(std::string const& dir, const char* name) {
  std::ifstream f(dir + "/" + name, std::ios::binary);
  if (!f) {
    std::fprintf(stderr, "graph_dot_render: no file %s\n", name);
    std::exit(2);
  }
  return std::vector<char>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc != 11) return 2;
  std::string const dir = argv[1];
  uint32_t const comp = static_cast<uint32_t>(std::atoi(argv[2])), k = static_cast<uint32_t>(std::atoi(argv[3]));
  ma_params_t p{};
  p.num_samples = std::atoi(argv[4]); p.max_comps = std::atoi(argv[5]); p.max_haps = std::atoi(argv[6]); p.max_hap_len = std::atoi(argv[7]);
  ma_graph_out_t g{};
  g.max_nodes = std::atoi(argv[8]); g.max_edges = std::atoi(argv[9]); g.max_seq_bytes = std::atoi(argv[10]);
  std::vector<std::vector<char>> keep;
  auto u32 = [&](const char* n) { keep.push_back(slurp(dir, n)); return reinterpret_cast<uint32_t*>(keep.back().data()); };
  auto u8 = [&](const char* n) { keep.push_back(slurp(dir, n)); return reinterpret_cast<uint8_t*>(keep.back().data()); };
  g.win_gstatus = u32("win_gstatus"); g.win_nnodes = u32("win_nnodes"); g.win_nedges = u32("win_nedges"); g.win_nseq = u32("win_nseq");
  g.node_comp = u32("node_comp"); g.node_seq_off = u32("node_seq_off"); g.node_len = u32("node_len"); g.node_cnt = u32("node_cnt");
  g.node_sign = u8("node_sign"); g.node_label = u8("node_label"); g.node_flags = u8("node_flags");
  g.edge_src = u32("edge_src"); g.edge_dst = u32("edge_dst"); g.edge_kind = u8("edge_kind"); g.seq_pool = u8("seq_pool");
  ma_asm_out_t a{};
  a.comp_hap0 = u32("comp_hap0"); a.comp_nhaps = u32("comp_nhaps"); a.hap_len = u32("hap_len"); a.hap_bases = u8("hap_bases");
  std::fputs(RenderComponentDot(p, a, g, 0, comp, k, "window").c_str(), stdout);
  return 0;
}
