// RenderComponentGfa / RenderComponentFasta (lancet2_amd/host/pipeline_host.hpp) on the arrays of ma_poa_out_t: reads them from
// raw files in a directory (one file per array, named after the struct member) and prints, for one component of one window,
// the GFA text, a line "==", and the FASTA text.
// usage: msa_text_render DIR WINDOW COMP MAX_COMPS MAX_HAPS MAX_PNODES MAX_PEDGES MAX_COLS.  Built with g++ by tests/test_msa_text.py.
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
    std::fprintf(stderr, "msa_text_render: no file %s\n", name);
    std::exit(2);
  }
  return std::vector<char>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc != 9) return 2;
  std::string const dir = argv[1];
  int const w = std::atoi(argv[2]);
  uint32_t const comp = static_cast<uint32_t>(std::atoi(argv[3]));
  ma_params_t p{};
  p.max_comps = std::atoi(argv[4]); p.max_haps = std::atoi(argv[5]);
  ma_poa_out_t x{};
  x.max_pnodes = std::atoi(argv[6]); x.max_pedges = std::atoi(argv[7]); x.max_cols = std::atoi(argv[8]);
  std::vector<std::vector<char>> keep;
  auto u32 = [&](const char* n) { keep.push_back(slurp(dir, n)); return reinterpret_cast<uint32_t*>(keep.back().data()); };
  auto u8 = [&](const char* n) { keep.push_back(slurp(dir, n)); return reinterpret_cast<uint8_t*>(keep.back().data()); };
  x.win_pstatus = u32("win_pstatus"); x.win_npnodes = u32("win_npnodes"); x.win_npedges = u32("win_npedges"); x.win_ncols = u32("win_ncols");
  x.comp_pnode0 = u32("comp_pnode0"); x.comp_npnodes = u32("comp_npnodes"); x.comp_pedge0 = u32("comp_pedge0");
  x.comp_npedges = u32("comp_npedges"); x.comp_ncols = u32("comp_ncols");
  x.pnode_base = u8("pnode_base"); x.pnode_rank = u32("pnode_rank"); x.pnode_col = u32("pnode_col"); x.pnode_haps = u32("pnode_haps");
  x.pedge_tail = u32("pedge_tail"); x.pedge_head = u32("pedge_head"); x.pedge_haps = u32("pedge_haps");
  x.hap_first = u32("hap_first"); x.msa = u8("msa");
  ma_asm_out_t a{};
  a.comp_hap0 = u32("comp_hap0"); a.comp_nhaps = u32("comp_nhaps");
  std::fputs(RenderComponentGfa(p, a, x, w, comp).c_str(), stdout);
  std::fputs("==\n", stdout);
  std::fputs(RenderComponentFasta(p, a, x, w, comp).c_str(), stdout);
  return 0;
}
