"""An independent restatement of the front half of the assembly: reads and reference bytes to the pruned component graphs.

Input: one window of the batch dictionary synth.pack_batch makes (ref_bases, ref_off, read_win_off, read_off, read_bases,
read_quals, read_qname_id, read_sample, read_flags -- no hints), a k-mer size and the parameters (num_samples, min_node_cov,
min_anchor_cov, min_anchor_len).  Output: one entry per component that found both anchors and was pruned, in the order the
reference visits them, with every alive node (sequence, per-sample counts, sign, label, source / sink flags) and its edge list
-- the state ma_graph_out_t publishes -- and counters of what the window exercised.  Pure Python; imports neither the engine
nor the oracle and shares no code with either, nor with graph_export_ref.py beyond that file's revcomp.  It follows the
reference's cbdg/graph.cpp (BuildGraph, AddNodes, RemoveLowCovNodes, MarkConnectedComponents, FindSource / FindSink,
PruneComponent and what that calls), node.cpp, kmer.cpp, kmer.h and edge.h; the lines are named where each rule is restated.

Node order: wherever the reference iterates its hash map of nodes, nodes are visited here in first-insertion order -- the
k-mers of the reference window first, then those of the reads in batch order -- and the size sort of the components is stable:
the project's canonical order (DESIGN.md's data layout).  Bytes that are not ACGT stay in the k-mers; N
complements to N.

NOT restated: the choice of k (the repeat gate, the cycle test, the complexity gate and the ladder) and the walk search.
build_window is run at the k the window reported (win_k); why lower rungs were rejected stays with the oracle, and what the
walks over these graphs must look like stays with graph_export_ref.py.
"""
import decimal
import math

import numpy as np

from graph_export_ref import revcomp

RF_PASS, RF_CASE = 1, 2                            # read_flags bits (include/microasm.h: MA_RF_PASS, MA_RF_CASE)
L_REFERENCE, L_CTRL, L_CASE = 1, 2, 4              # label.h:13
PLUS, MINUS = 0, 1                                 # sign codes as in edge_kind: kind = source sign << 1 | destination sign
KIND_NAMES = ("++", "+-", "-+", "--")
FLAG_SOURCE, FLAG_SINK = 1, 2

# hts/phred_quality.cpp:15-300 keeps 10^(-q/10) as decimal literals of 28 digits, i.e. the correctly rounded doubles; pow() of
# the C library is not correctly rounded, so the table is made with decimal arithmetic
_ctx = decimal.Context(prec=60)
PHRED_ERR = [float(_ctx.power(decimal.Decimal(10), _ctx.divide(decimal.Decimal(-q), decimal.Decimal(10)))) for q in range(256)]

_ACGT_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _rc(seq: bytes) -> bytes:
    if not seq.translate(None, b"ACGT"):  # plain ACGT: the quick way
        return seq.translate(_ACGT_COMP)[::-1]
    return revcomp(seq)


def mirror_kind(kind):
    """RevEdgeKind (kmer.h:94-105): the same edge seen from its other end -- both signs turned and swapped"""
    return ((1 - (kind & 1)) << 1) | (1 - (kind >> 1))


class BNode:
    __slots__ = ("idx", "seq", "sign", "label", "counts", "edges", "comp", "alive", "ref_first")

    def __init__(self, idx, seq, sign, label, num_samples):
        self.idx, self.seq, self.sign, self.label = idx, seq, sign, label
        self.counts = [0] * num_samples
        self.edges = []        # (destination node index, kind) in list order; node.h:59-64 keeps the list free of duplicates
        self.comp, self.alive = 0, True
        self.ref_first = label == L_REFERENCE

    @property
    def total(self):
        return sum(self.counts)

    @property
    def all_singletons(self):  # node.cpp:38-42
        return any(c > 0 for c in self.counts) and all(c <= 1 for c in self.counts)

    def add_edge(self, e):
        if e not in self.edges:
            self.edges.append(e)

    def drop_edge(self, e):    # node.h:66-71
        if e in self.edges:
            self.edges.remove(e)

    def self_loop(self):       # node.cpp:114-116
        return any(d == self.idx for d, _ in self.edges)

    def in_direction(self, dflt):
        """node.cpp:118-127: the edges that leave on the stored sign (dflt) or on the other one"""
        want = self.sign if dflt else 1 - self.sign
        return [e for e in self.edges if (e[1] >> 1) == want]


class BuiltWindow(list):
    """the pruned components of one window -- dict(anchor, comp, source, sink, nodes=[dict(idx, seq, counts, sign, label,
    flags, edges=[(idx of the destination, kind)])]) each -- and .counters"""
    counters = None


def new_counters():
    return dict(mate_suppressed=0, mate_other_tag=0, gate_refused=0, gate_near_below=0, gate_near_above=0, singletons_with_cov=0,
                merges=[0, 0, 0, 0], tip_rounds=[], tips_one_under_k=0, dead_ends_at_k=0, ref_first_supported=0, non_acgt_nodes=0,
                reads_used=0, reads_filtered=0, nodes_built=0)


class _Graph:
    def __init__(self, k, params, counters, log=None):
        self.k, self.S = k, int(params.num_samples)
        self.min_node_cov, self.min_anchor_cov = int(params.min_node_cov), int(params.min_anchor_cov)
        self.nodes, self.by_seq = [], {}
        self.source = self.sink = None  # mSourceAndSinkIds = {0, 0}: no anchors yet (graph.cpp:109)
        self.cnt = counters
        self.log = log  # None, or a list that gets ("merge", absorber before, absorbed, kind, counts after) and
        #                 ("remove", why, sequence, counts) in the order they happen

    # ---- construction ------------------------------------------------------------------------------------------------
    def add_nodes(self, seq: bytes, label):
        """AddNodes (graph.cpp:311-341): one node per distinct canonical k-mer (kmer.cpp:17-28, 115-128: the k-mer itself if it
        is not above its reverse complement, sign PLUS; else the reverse complement, sign MINUS), kept as its FIRST inserter
        made it -- try_emplace changes neither sign nor label of a node that exists.  Returns the node of every k-mer of seq,
        in order; nothing when seq has no (k + 1)-mer."""
        k, L = self.k, len(seq)
        if L < k + 1:
            return []
        rc = _rc(seq)
        ids = []
        for o in range(L - k + 1):
            fwd, bwd = seq[o:o + k], rc[L - o - k:L - o]
            plus = fwd <= bwd
            canon = fwd if plus else bwd
            i = self.by_seq.get(canon)
            if i is None:
                i = len(self.nodes)
                self.by_seq[canon] = i
                self.nodes.append(BNode(i, canon, PLUS if plus else MINUS, label, self.S))
            ids.append(i)
        nodes = self.nodes
        for a, b in zip(ids, ids[1:]):  # one (k + 1)-mer each.  The kind comes from the STORED signs (graph.cpp:333-336)
            kind = (nodes[a].sign << 1) | nodes[b].sign
            nodes[a].add_edge((b, kind))
            nodes[b].add_edge((a, mirror_kind(kind)))
        return ids

    def kmer_error(self, prefix, quals, o):
        """graph.cpp:300: the expected errors of the k-mer at offset o -- a difference of two prefix sums, NOT a sum of its own"""
        return prefix[o + self.k] - prefix[o]

    @staticmethod
    def refused(raw):
        """graph.cpp:301-304: floor(raw) > 0, i.e. from exactly 1.0 on"""
        return math.floor(raw) > 0

    def build(self, ref: bytes, reads):
        """BuildGraph (graph.cpp:262-309).  reads: (bases, quals, qname id, sample, flags) in batch order."""
        k, cnt = self.k, self.cnt
        self.ref_ids = self.add_nodes(ref, L_REFERENCE)
        mate_mers = set()
        for bases, quals, qname, sample, flags in reads:
            if not flags & RF_PASS:  # PassesAlnFilters (graph.cpp:275)
                cnt["reads_filtered"] += 1
                continue
            cnt["reads_used"] += 1
            tag = L_CASE if flags & RF_CASE else L_CTRL
            prefix, acc = [0.0], 0.0  # std::partial_sum over f64, left to right (graph.cpp:280-285)
            for q in quals:
                acc += PHRED_ERR[q]
                prefix.append(acc)
            for o, i in enumerate(self.add_nodes(bases, tag)):
                raw = self.kmer_error(prefix, quals, o)
                if abs(raw - 1.0) <= 0.02:
                    cnt["gate_near_above" if raw >= 1.0 else "gate_near_below"] += 1
                key = (qname, i, tag)            # MateMer: qname, node, CTRL / CASE tag (graph.cpp:291-292)
                if self.refused(raw):
                    cnt["gate_refused"] += 1
                    continue
                if key in mate_mers:
                    cnt["mate_suppressed"] += 1
                    continue
                cnt["mate_other_tag"] += (qname, i, L_CASE + L_CTRL - tag) in mate_mers  # same qname and node, other tag: counted
                self.nodes[i].counts[sample] += 1  # IncrementReadSupport (node.cpp:18-24): the label is NOT touched
                mate_mers.add(key)
        cnt["nodes_built"] = len(self.nodes)
        for nd in self.nodes:
            cnt["ref_first_supported"] += nd.ref_first and nd.total > 0
            cnt["non_acgt_nodes"] += bool(nd.seq.translate(None, b"ACGT"))

    # ---- removal, components, anchors --------------------------------------------------------------------------------
    def remove(self, i):
        """RemoveNode (graph.cpp:347-361)"""
        nd = self.nodes[i]
        if not nd.alive:
            return
        for dst, kind in nd.edges:
            if dst != i and self.nodes[dst].alive:
                self.nodes[dst].drop_edge((i, mirror_kind(kind)))
        nd.alive, nd.edges = False, []

    def note(self, why, i):
        if self.log is not None:
            self.log.append(("remove", why, self.nodes[i].seq, tuple(self.nodes[i].counts)))

    def remove_low_cov(self, comp):
        """RemoveLowCovNodes (graph.cpp:363-390): all-singletons or total < min_node_cov, the anchors exempt"""
        gone = []
        for nd in self.nodes:
            if not nd.alive or nd.comp != comp or nd.idx in (self.source, self.sink):
                continue
            single = nd.all_singletons
            if single or nd.total < self.min_node_cov:
                gone.append(nd.idx)
                self.cnt["singletons_with_cov"] += single and nd.total >= self.min_node_cov
        for i in gone:
            self.note("low_cov", i)
            self.remove(i)

    def mark_components(self):
        """MarkConnectedComponents (graph.cpp:392-463): ids 1, 2, ... in discovery order, largest first, ties in id order"""
        sizes = []
        for nd in self.nodes:
            if not nd.alive or nd.comp:
                continue
            cid = len(sizes) + 1
            sizes.append(0)
            queue, at = [nd.idx], 0
            while at < len(queue):
                cur = self.nodes[queue[at]]
                at += 1
                if cur.comp:
                    continue
                cur.comp = cid
                sizes[cid - 1] += 1
                queue.extend(d for d, _ in cur.edges)
        return sorted(range(1, len(sizes) + 1), key=lambda c: -sizes[c - 1])  # (sorted() is stable)

    def find_anchor(self, comp, backwards):
        """FindSource / FindSink (graph.cpp:469-509): the first (last) reference k-mer whose node is alive, in the component
        and has total support >= min_anchor_cov.  Returns (node, reference offset) or None."""
        n = len(self.ref_ids)
        for r in (range(n - 1, -1, -1) if backwards else range(n)):
            nd = self.nodes[self.ref_ids[r]]
            if nd.alive and nd.comp == comp and nd.total >= self.min_anchor_cov:
                return nd.idx, r
        return None

    # ---- compression -------------------------------------------------------------------------------------------------
    def buddy_ok(self, src, conn):
        """IsPotentialBuddyEdge (graph.cpp:758-799)"""
        nb = self.nodes[conn[0]]
        if len(src.edges) == 1 and len(nb.edges) == 1 and src.edges[0][0] == nb.idx and nb.edges[0][0] == src.idx:
            return False
        if not 1 <= len(nb.edges) <= 2 or nb.self_loop():
            return False
        back = (src.idx, mirror_kind(conn[1]))
        dflt = (back[1] >> 1) == nb.sign
        if nb.in_direction(dflt) != [back]:
            return False
        onward = nb.in_direction(not dflt)
        if len(onward) != 1 or onward[0][0] == src.idx:
            return False
        return len(self.nodes[onward[0][0]].edges) <= 2

    def compressible_edge(self, src, dflt):
        """FindCompressibleEdge (graph.cpp:688-717)"""
        if not 1 <= len(src.edges) <= 2 or src.self_loop() or src.idx in (self.source, self.sink):
            return None
        ahead = src.in_direction(dflt)
        if len(ahead) != 1 or ahead[0][0] in (self.source, self.sink) or not self.buddy_ok(src, ahead[0]):
            return None
        behind = src.in_direction(not dflt)
        if len(behind) > 1 or (behind and not self.buddy_ok(src, behind[0])):
            return None
        return ahead[0]

    def merge(self, nd, other, kind):
        """Node::Merge (node.cpp:81-112) with Kmer::Merge / MergeCords (kmer.cpp:48-109, 130-139): the absorbed node's bases
        beyond the k - 1 shared ones go behind (++, +-) or in front (-+, --), reverse complemented when the two signs of the
        edge differ; labels are OR-ed; every count becomes the floored length-weighted mean, the absorbing node weighted with
        its length AFTER the merge (node.cpp:91 reads the length once mKmer.Merge has run)."""
        k, before = self.k, nd.seq
        piece = other.seq if kind in (0, 3) else _rc(other.seq)
        nd.seq = nd.seq + piece[k - 1:] if kind < 2 else piece[:len(piece) - k + 1] + nd.seq
        nd.label |= other.label
        a, b = len(nd.seq), len(other.seq)
        nd.counts = [(x * a + y * b) // (a + b) for x, y in zip(nd.counts, other.counts)]
        self.cnt["merges"][kind] += 1
        if self.log is not None:
            self.log.append(("merge", before, other.seq, KIND_NAMES[kind], tuple(nd.counts)))

    def compress_node(self, i, dflt, absorbed):
        """CompressNode (graph.cpp:600-645)"""
        nd = self.nodes[i]
        edge = self.compressible_edge(nd, dflt)
        while edge is not None:
            buddy = self.nodes[edge[0]]
            ssign, dsign = edge[1] >> 1, edge[1] & 1
            self.merge(nd, buddy, edge[1])
            nd.drop_edge(edge)
            back = (i, mirror_kind(edge[1]))
            for e in list(buddy.edges):
                if e == back:
                    continue
                nsign = ssign if (e[1] >> 1) == dsign else 1 - ssign  # graph.cpp:632-635
                new = (e[0], (nsign << 1) | (e[1] & 1))
                far = self.nodes[e[0]]
                nd.add_edge(new)
                far.add_edge((i, mirror_kind(new[1])))
                far.drop_edge((buddy.idx, mirror_kind(e[1])))
            absorbed.add(buddy.idx)
            edge = self.compressible_edge(nd, dflt)

    def compress(self, comp):
        """CompressGraph (graph.cpp:558-576)"""
        absorbed = set()
        for nd in self.nodes:
            if nd.alive and nd.comp == comp and nd.idx not in absorbed:
                self.compress_node(nd.idx, True, absorbed)
                self.compress_node(nd.idx, False, absorbed)
        for i in sorted(absorbed):
            self.remove(i)

    def remove_tips(self, comp):
        """RemoveTips (graph.cpp:801-840): nodes with at most one edge and fewer than k bases of their own, round after round
        with a compression after each, until a round finds none"""
        k, rounds = self.k, []
        while True:
            ends = [nd for nd in self.nodes if nd.alive and nd.comp == comp and nd.idx not in (self.source, self.sink)
                    and len(nd.edges) <= 1]
            tips = [nd.idx for nd in ends if len(nd.seq) - k + 1 < k]
            self.cnt["tips_one_under_k"] += sum(1 for nd in ends if len(nd.seq) - k + 1 == k - 1)
            self.cnt["dead_ends_at_k"] += sum(1 for nd in ends if len(nd.seq) - k + 1 == k)
            if not tips:
                break
            rounds.append(len(tips))
            for i in tips:
                self.note("tip", i)
                self.remove(i)
            self.compress(comp)
        self.cnt["tip_rounds"].append(rounds)

    def prune(self, comp):
        """PruneComponent (graph.cpp:515-540)"""
        self.compress(comp)
        self.remove_low_cov(comp)
        self.compress(comp)
        self.remove_tips(comp)

    def snapshot(self, comp, anchor):
        out = []
        for nd in self.nodes:
            if nd.alive and nd.comp == comp:
                flags = (FLAG_SOURCE if nd.idx == self.source else 0) | (FLAG_SINK if nd.idx == self.sink else 0)
                out.append(dict(idx=nd.idx, seq=nd.seq, counts=list(nd.counts), sign=nd.sign, label=nd.label, flags=flags,
                                edges=list(nd.edges)))
        return dict(anchor=anchor, comp=comp, source=self.source, sink=self.sink, nodes=out)


def window_inputs(arrs, w):
    """(reference bytes, [(bases, quals, qname id, sample, flags), ...]) of window w of a packed batch"""
    ref = bytes(arrs["ref_bases"][int(arrs["ref_off"][w]):int(arrs["ref_off"][w + 1])])
    reads = []
    for r in range(int(arrs["read_win_off"][w]), int(arrs["read_win_off"][w + 1])):
        a, b = int(arrs["read_off"][r]), int(arrs["read_off"][r + 1])
        reads.append((bytes(arrs["read_bases"][a:b]), bytes(arrs["read_quals"][a:b]), int(arrs["read_qname_id"][r]),
                      int(arrs["read_sample"][r]), int(arrs["read_flags"][r])))
    return ref, reads


def build_graph(ref, reads, k, params, log=None):
    """The k attempt of graph.cpp:125-184 minus its gates: build, first low-coverage pass, components, and for every component
    with both anchors (different nodes, spanning at least min_anchor_len reference bases) the pruning.  Returns a BuiltWindow."""
    out = BuiltWindow()
    out.counters = new_counters()
    g = _Graph(int(k), params, out.counters, log)
    g.build(ref, reads)
    g.remove_low_cov(0)
    for comp in g.mark_components():
        src, snk = g.find_anchor(comp, False), g.find_anchor(comp, True)
        if src is None or snk is None or src[0] == snk[0]:
            continue
        if snk[1] - src[1] + g.k < int(params.min_anchor_len):  # graph.h:182-185, graph.cpp:167-173
            continue
        g.source, g.sink = src[0], snk[0]
        g.prune(comp)
        out.append(g.snapshot(comp, src[1]))
    return out


def build_window(arrs, w, k, params):
    ref, reads = window_inputs(arrs, w)
    return build_graph(ref, reads, k, params)


def to_export_arrays(entries, num_samples, caps=None):
    """The chosen components of ONE window as the flat arrays of ma_graph_out_t (a batch of one window): entries[c] becomes
    component slot c.  Nodes component after component in first-insertion order, the edges of a node contiguous in list order,
    nodes in slot order.  graph_export_ref.window_nodes / check_window / graph_key take the result as window 0."""
    S = num_samples
    nn = sum(len(e["nodes"]) for e in entries)
    ne = sum(len(nd["edges"]) for e in entries for nd in e["nodes"])
    ns = sum(len(nd["seq"]) for e in entries for nd in e["nodes"])
    MN, ME, MS = caps or (max(nn, 1), max(ne, 1), max(ns, 1))
    assert nn <= MN and ne <= ME and ns <= MS
    gr = dict(max_nodes=MN, max_edges=ME, max_seq_bytes=MS, win_gstatus=np.zeros(1, np.uint32),
              win_nnodes=np.array([nn], np.uint32), win_nedges=np.array([ne], np.uint32), win_nseq=np.array([ns], np.uint32),
              node_comp=np.zeros(MN, np.uint32), node_seq_off=np.zeros(MN, np.uint32), node_len=np.zeros(MN, np.uint32),
              node_cnt=np.zeros(MN * S, np.uint32), node_sign=np.zeros(MN, np.uint8), node_label=np.zeros(MN, np.uint8),
              node_flags=np.zeros(MN, np.uint8), edge_src=np.zeros(ME, np.uint32), edge_dst=np.zeros(ME, np.uint32),
              edge_kind=np.zeros(ME, np.uint8), seq_pool=np.zeros(MS, np.uint8))
    slot = {}
    for e in entries:
        for nd in e["nodes"]:
            slot[nd["idx"]] = len(slot)
    at = ei = 0
    for c, e in enumerate(entries):
        for nd in e["nodes"]:
            s = slot[nd["idx"]]
            gr["node_comp"][s], gr["node_seq_off"][s], gr["node_len"][s] = c, at, len(nd["seq"])
            gr["seq_pool"][at:at + len(nd["seq"])] = np.frombuffer(nd["seq"], np.uint8)
            at += len(nd["seq"])
            gr["node_cnt"][s * S:(s + 1) * S] = nd["counts"]
            gr["node_sign"][s] = 1 if nd["sign"] == PLUS else 0
            gr["node_label"][s], gr["node_flags"][s] = nd["label"], nd["flags"]
            for dst, kind in nd["edges"]:
                gr["edge_src"][ei], gr["edge_dst"][ei], gr["edge_kind"][ei] = s, slot[dst], kind
                ei += 1
    return gr


def first_difference(got, want):
    """The first node or edge on which two graph_key values (graph_export_ref.graph_key) differ, from both sides, as text;
    None when they are equal."""
    if got == want:
        return None
    if sorted(got) != sorted(want):
        return f"component slots {sorted(got)} vs {sorted(want)}"
    for c in sorted(got):
        for what, a, b in (("node", got[c][0], want[c][0]), ("edge", got[c][1], want[c][1])):
            if a != b:
                only_a, only_b = sorted(a - b), sorted(b - a)
                return (f"component {c}: {len(only_a)} {what}s only on the first side, {len(only_b)} only on the second; "
                        f"first: {only_a[0] if only_a else None} | second: {only_b[0] if only_b else None}")
    return "unequal"
