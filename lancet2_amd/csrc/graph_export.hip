// Graph export (ma_assemble_graph_batch): the pruned graph of every component that got a row of comp_*, written to the
// caller's arrays -- what the reference draws per component with --out-graphs-tgz (cbdg/graph.cpp:216-223).
//
// The clean kernels (clean.hip) work on one set of node arrays per active slot and prune a window's candidate components one
// after the other; components are disjoint, so when a kernel reports the window the arrays hold every reported component in
// the state its metrics and walks were computed from.  In a call that exports, the kernels leave a mark record per slot
// (graph_ws.h: kGxMark) -- which components got a row, their anchors, which route reported -- and the LDS images of
// k_clean_tail are written back to the cg_* arrays they were loaded from.  k_graph_export runs behind them in every pass,
// before the next pass reuses the workspace: a window is exported by the pass (k rung, capacity retry) that reported it and
// by no other, since only that pass's marks are non-zero.
//
// One wavefront per window, a lane per node: which nodes are exported and where their rows, edges and bases go are ballots
// and prefix sums in node order; then every lane writes its node's row, its edges and its sequence -- the node's slice list
// spelled in the stored orientation by the rule the haplotype writer uses (clean.hip: slice_base).
#include "graph_ws.h"

namespace ma {

namespace {

__global__ void k_graph_export_clear(ma_graph_out_t o, const u32* win_status, int n, int only_overflowed) {
  int const i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (only_overflowed && !(win_status[i] & MA_W_TABLE_OVERFLOW)) return;  // (the windows a capacity retry pass takes again)
  o.win_gstatus[i] = 0;
  o.win_nnodes[i] = 0;
  o.win_nedges[i] = 0;
  o.win_nseq[i] = 0;
}

__global__ __launch_bounds__(64) void k_graph_export(DBatch b, GraphWs ws, GxDev gx) {
  int const a = blockIdx.x;
  u32 const lane = threadIdx.x;
  const u32* mark = gx.mark + static_cast<size_t>(a) * kGxMark;
  u32 const m0 = mark[0];
  if (m0 == 0u) return;  // not reported by this pass
  u32 const rows = m0 & 0xFFu, route = (m0 >> 8) - 1u;
  int const w = static_cast<int>(ws.active[a]);
  u32 const K = static_cast<u32>(win_kmer(ws, w));
  u32 const S = static_cast<u32>(ws.num_samples);
  __shared__ u32 s_comp[16], s_src[16], s_snk[16];
  if (lane < rows && lane < 16u) {
    s_comp[lane] = mark[1 + 3 * lane];
    s_src[lane] = mark[2 + 3 * lane];
    s_snk[lane] = mark[3 + 3 * lane];
  }
  __syncthreads();

  // the arrays the reporting route left: the raw graph of k_clean, or the compact graph of the tail kernels (graph_ws.h)
  GxNodes const g = gx_nodes(b, ws, a, w, route);
  u32 const n = g.n, ecap = g.ecap;
  const u32 *cnt = g.cnt, *comp = g.comp, *len = g.len, *edge = g.edge;
  const u8 *nedge = g.nedge, *alive = g.alive, *label = g.label, *sign = g.sign;
  // work lists in the route's scratch: 3 n words
  u32* const scratch = g.scratch;
  u32* const slot_of = scratch;       // [n] node -> slot of the window's export, kNoNode: not exported
  u32* const seq_at = scratch + n;    // [n] where its bases start in the window's pool
  u32* const edge_at = scratch + 2 * static_cast<size_t>(n);  // [n] where its edges start

  auto row_of = [&](u32 i) -> u32 {  // the row of comp_* node i belongs to, kNoNode: none
    if (!alive[i]) return kNoNode;
    u32 const cc = comp[i];
    u32 r = kNoNode;
    for (u32 x = 0; x < rows && x < 16u; ++x)
      if (s_comp[x] == cc) r = x;
    return r;
  };
  unsigned long long const below = (1ull << lane) - 1ull;

  // ---- the needs ----
  u32 nn = 0, nseq = 0, ne = 0;
  for (u32 base = 0; base < n; base += 64) {
    u32 const i = base + lane;
    bool const in = i < n && row_of(i) != kNoNode;
    unsigned long long const m = __ballot(in);
    u32 const ln = in ? len[i] : 0u;
    u32 inc = ln;
#pragma unroll
    for (u32 o = 1; o < 64; o <<= 1) {
      u32 const y = __shfl_up(inc, o, 64);
      if (lane >= o) inc += y;
    }
    if (i < n) slot_of[i] = in ? nn + static_cast<u32>(__popcll(m & below)) : kNoNode;
    if (in) seq_at[i] = nseq + inc - ln;
    nn += static_cast<u32>(__popcll(m));
    nseq += static_cast<u32>(__shfl(inc, 63, 64));
  }
  __syncthreads();
  for (u32 base = 0; base < n; base += 64) {
    u32 const i = base + lane;
    bool const in = i < n && slot_of[i] != kNoNode;
    u32 c = 0;
    if (in) {
      u32 const nei = nedge[i] < ecap ? nedge[i] : ecap;
      for (u32 x = 0; x < nei; ++x) {
        u32 const d = edge[i * ecap + x] >> 2;
        c += d < n && slot_of[d] != kNoNode;  // (pruning erases the edges to a removed node: every stored edge qualifies)
      }
    }
    u32 inc = c;
#pragma unroll
    for (u32 o = 1; o < 64; o <<= 1) {
      u32 const y = __shfl_up(inc, o, 64);
      if (lane >= o) inc += y;
    }
    if (in) edge_at[i] = ne + inc - c;
    ne += static_cast<u32>(__shfl(inc, 63, 64));
  }
  u32 const MN = static_cast<u32>(gx.o.max_nodes), ME = static_cast<u32>(gx.o.max_edges), MS = static_cast<u32>(gx.o.max_seq_bytes);
  u32 const gst = (nn > MN ? MA_G_NODE_OVERFLOW : 0u) | (ne > ME ? MA_G_EDGE_OVERFLOW : 0u) | (nseq > MS ? MA_G_SEQ_OVERFLOW : 0u);
  if (lane == 0) {
    gx.o.win_gstatus[w] = gst;
    gx.o.win_nnodes[w] = nn;
    gx.o.win_nedges[w] = ne;
    gx.o.win_nseq[w] = nseq;
  }
  if (gst != 0u) return;  // none of the window's rows is defined; nothing is written
  if (lane == 0) atomicAdd(&gx.routes[route & 3u], 1ull);  // (only windows whose rows are written count as exported)

  // ---- the rows: every index below is < its need <= its cap ----
  size_t const n0 = static_cast<size_t>(w) * MN, e0 = static_cast<size_t>(w) * ME;
  u8* const seq = gx.o.seq_pool + static_cast<size_t>(w) * MS;
  for (u32 base = 0; base < n; base += 64) {
    u32 const i = base + lane;
    if (i >= n) continue;
    u32 const slot = slot_of[i];
    if (slot == kNoNode) continue;
    u32 const r = row_of(i);
    u32 const ln = len[i], at = seq_at[i];
    gx.o.node_comp[n0 + slot] = r;
    gx.o.node_seq_off[n0 + slot] = at;
    gx.o.node_len[n0 + slot] = ln;
    for (u32 s = 0; s < S; ++s) gx.o.node_cnt[(n0 + slot) * S + s] = cnt[i * S + s];
    gx.o.node_sign[n0 + slot] = sign[i];
    gx.o.node_label[n0 + slot] = label[i];
    gx.o.node_flags[n0 + slot] = static_cast<u8>((i == s_src[r] ? 1u : 0u) | (i == s_snk[r] ? 2u : 0u));
    u32 ea = edge_at[i];
    u32 const nei = nedge[i] < ecap ? nedge[i] : ecap;
    for (u32 x = 0; x < nei; ++x) {
      u32 const e = edge[i * ecap + x], d = e >> 2;
      if (d >= n || slot_of[d] == kNoNode || ea >= ne) continue;
      gx.o.edge_src[e0 + ea] = slot;
      gx.o.edge_dst[e0 + ea] = slot_of[d];
      gx.o.edge_kind[e0 + ea] = static_cast<u8>(e & 3u);
      ++ea;
    }
    // the node's sequence as stored (graph_ws.h: gx_spell_node)
    u32 pos = gx_spell_node(g, i, ln, K, [seq, at](u32 at_pos, u8 ch) { seq[at + at_pos] = ch; });
    for (; pos < ln; ++pos) seq[at + pos] = 'N';  // (a list shorter than the node's length: never seen; defined bytes all the same)
  }
}

}  // namespace

int run_graph_export_clear(ma_ctx* ctx, const GxDev& gx, const u32* win_status, int n, bool only_overflowed) {
  if (n == 0) return MA_OK;
  if (ctx->probe) return run_probe_clear(ctx, *ctx->probe, win_status, n, only_overflowed);  // (a probe call: gx.o has no arrays)
  hipLaunchKernelGGL(k_graph_export_clear, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, gx.o, win_status, n, only_overflowed ? 1 : 0);
  MA_HIP(ctx, hipGetLastError());
  return MA_OK;
}

int run_graph_export(ma_ctx* ctx, const DBatch& b, const GraphWs& ws, const GxDev& gx) {
  if (ws.n_active == 0) return MA_OK;
  if (ctx->probe) return run_probe_nodes(ctx, b, ws, gx.mark, *ctx->probe);  // the probes' rows instead of the graph's
  ctx->tic("k_graph_export");
  hipLaunchKernelGGL(k_graph_export, dim3(ws.n_active), dim3(64), 0, ctx->stream, b, ws, gx);
  ctx->toc();
  MA_HIP(ctx, hipGetLastError());
  return MA_OK;
}

}  // namespace ma
