"""Restatement of the SPOA state the POA stage builds for one component: spoa::Graph::AddAlignment, its DFS topological sort
and GenerateMultipleSequenceAlignment, in plain Python.

Input: the component's haplotypes (byte strings, the first one the REF haplotype).  The alignments are NOT restated: haplotype
h is aligned to the graph of haplotypes 0 .. h-1 by the oracle (orc_poa_align_dump, unit weights -- the alignment does not
depend on weights), and only the returned (node | -1, position | -1) pairs are used.  Everything the engine exports with
ma_msa_graph_batch follows from the pairs: letters by id, out-edge lists with label masks, aligned rings, rank order,
sequences()[h], MSA columns, MSA rows, paths -- plus the GFA and FASTA texts of caller/msa_builder.cpp:44-102.
Imports neither the engine nor torch."""
import ctypes as C

SCORING = (0, -6, -6, -2, -26, -1)  # caller/msa_builder.h:72-77


def _oracle():
    from harness import oracle
    return oracle()


def oracle_dump(seqs, lib=None, sc=SCORING):
    """orc_poa_align_dump: the graph of seqs[:-1] -- (letters by id, in-edge tails per node in order, rank order) -- and the
    alignment pairs of seqs[-1] against it"""
    lib = lib or _oracle()
    blob = b"".join(bytes(s) + b"\0" for s in seqs)
    cap = 64 * sum(len(s) for s in seqs) + 1024
    out = (C.c_int32 * cap)()
    n = lib.orc_poa_align_dump(blob, len(seqs), *sc, out, cap)
    assert n > 0
    w = list(out[:n])
    V = w[0]
    pos = 1
    base, preds = [], []
    for _ in range(V):
        base.append(w[pos])
        k = w[pos + 1]
        preds.append(w[pos + 2: pos + 2 + k])
        pos += 2 + k
    order = w[pos:pos + V]
    pos += V
    A = w[pos]
    pairs = [(w[pos + 1 + 2 * x], w[pos + 2 + 2 * x]) for x in range(A)]
    return base, preds, order, pairs


class PoaGraph:
    """spoa::Graph without weights: nodes by id, edges as (head, label mask) in Node::outedges order"""

    def __init__(self):
        self.base = []      # letter per node id
        self.out = []       # per node: [[head, mask], ...] in outedges order
        self.inn = []       # per node: tails in inedges order
        self.ring = []      # per node: aligned node ids in aligned_nodes order
        self.order = []     # rank_to_node
        self.seq_first = []  # sequences()

    def add_node(self, ch):
        self.base.append(ch)
        self.out.append([])
        self.inn.append([])
        self.ring.append([])
        return len(self.base) - 1

    def add_edge(self, tail, head, label):
        for e in self.out[tail]:
            if e[0] == head:
                e[1] |= 1 << label
                return
        self.out[tail].append([head, 1 << label])
        self.inn[head].append(tail)

    def add_sequence(self, seq, begin, end, label):
        if begin >= end:
            return None
        first = self.add_node(seq[begin])
        prev = first
        for i in range(begin + 1, end):
            cur = self.add_node(seq[i])
            self.add_edge(prev, cur, label)
            prev = cur
        return first

    def add_alignment(self, pairs, seq):
        seq = bytes(seq)
        if not seq:
            return
        label = len(self.seq_first)
        if not pairs:
            self.seq_first.append(self.add_sequence(seq, 0, len(seq), label))
            self.toposort()
            return
        valid = [p for _, p in pairs if p != -1]
        assert valid and all(0 <= p < len(seq) for p in valid)
        begin = self.add_sequence(seq, 0, valid[0], label)
        prev = len(self.base) - 1 if begin is not None else None
        last = self.add_sequence(seq, valid[-1] + 1, len(seq), label)
        for node, p in pairs:
            if p == -1:
                continue
            ch = seq[p]
            if node == -1:
                cur = self.add_node(ch)
            elif self.base[node] == ch:
                cur = node
            else:
                cur = next((k for k in self.ring[node] if self.base[k] == ch), None)
                if cur is None:
                    cur = self.add_node(ch)
                    for k in self.ring[node]:
                        self.ring[k].append(cur)
                        self.ring[cur].append(k)
                    self.ring[node].append(cur)
                    self.ring[cur].append(node)
            if begin is None:
                begin = cur
            if prev is not None:
                self.add_edge(prev, cur, label)
            prev = cur
        if last is not None:
            self.add_edge(prev, last, label)
        self.seq_first.append(begin)
        self.toposort()

    def toposort(self):
        n = len(self.base)
        marks = [0] * n
        ignored = [False] * n
        order = []
        for root in range(n):
            if marks[root]:
                continue
            stack = [root]
            while stack:
                cur = stack[-1]
                valid = True
                if marks[cur] != 2:
                    for t in self.inn[cur]:
                        if marks[t] != 2:
                            stack.append(t)
                            valid = False
                    if not ignored[cur]:
                        for a in self.ring[cur]:
                            if marks[a] != 2:
                                stack.append(a)
                                ignored[a] = True
                                valid = False
                    assert valid or marks[cur] != 1, "graph is not a DAG"
                    if valid:
                        marks[cur] = 2
                        if not ignored[cur]:
                            order.append(cur)
                            order.extend(self.ring[cur])
                    else:
                        marks[cur] = 1
                if valid:
                    stack.pop()
        assert len(order) == n
        self.order = order

    def successor(self, node, label):
        for head, mask in self.out[node]:
            if mask >> label & 1:
                return head
        return None

    def path(self, label):
        out = []
        cur = self.seq_first[label]
        while cur is not None:
            out.append(cur)
            cur = self.successor(cur, label)
        return out

    def columns(self):
        """GenerateMultipleSequenceAlignment's node_id_to_column and the number of columns"""
        col = [-1] * len(self.base)
        ncols = 0
        for v in self.order:
            if col[v] == -1:
                col[v] = ncols
                for a in self.ring[v]:
                    col[a] = ncols
                ncols += 1
        return col, ncols


def build(seqs, lib=None, on_step=None, sc=SCORING):
    """The graph after every haplotype of `seqs`; on_step(h, graph, dump) sees the graph of seqs[:h] beside the oracle's dump
    of it (h = 1 .. H-1) before haplotype h is added."""
    lib = lib or _oracle()
    g = PoaGraph()
    g.add_alignment([], seqs[0])
    for h in range(1, len(seqs)):
        dump = oracle_dump(seqs[:h + 1], lib, sc)
        if on_step:
            on_step(h, g, dump)
        g.add_alignment(dump[3], seqs[h])
    return g


def describe(g):
    """Everything ma_msa_graph_batch exports for the component, as Python lists"""
    n = len(g.base)
    col, ncols = g.columns()
    rank = [0] * n
    for r, v in enumerate(g.order):
        rank[v] = r
    paths = [g.path(h) for h in range(len(g.seq_first))]
    haps = [0] * n
    for h, pth in enumerate(paths):
        for v in pth:
            haps[v] |= 1 << h
    rows = []
    for pth in paths:
        row = bytearray(b"-" * ncols)
        for v in pth:
            row[col[v]] = g.base[v]
        rows.append(bytes(row))
    edges = [(t, e[0], e[1]) for t in range(n) for e in g.out[t]]
    return dict(base=list(g.base), rank=rank, col=col, haps=haps, edges=edges, rings=[list(r) for r in g.ring], order=list(g.order),
                seq_first=list(g.seq_first), ncols=ncols, rows=rows, paths=paths)


def component(seqs, lib=None, sc=SCORING):
    return describe(build(seqs, lib, sc=sc))


def _name(h):
    return ("ref" if h == 0 else "hap") + str(h)


def gfa_text(d):
    """MsaBuilder::BuildGfaString"""
    out = ["H\tVN:Z:1.0\n"]
    by_tail = {}
    for t, hd, _ in d["edges"]:
        by_tail.setdefault(t, []).append(hd)
    for v, ch in enumerate(d["base"]):
        out.append(f"S\t{v + 1}\t{chr(ch)}\n")
        for hd in by_tail.get(v, []):
            out.append(f"L\t{v + 1}\t+\t{hd + 1}\t+\t0M\n")
    for h, pth in enumerate(d["paths"]):
        out.append(f"P\t{_name(h)}\t" + ",".join(f"{v + 1}+" for v in pth) + "\t*\n")
    return "".join(out)


def fasta_text(d):
    """MsaBuilder::BuildFastaString over GenerateMultipleSequenceAlignment's rows"""
    return "".join(f">{_name(h)}\n{row.decode()}\n" for h, row in enumerate(d["rows"]))


def from_export(px, p, w, c, asm):
    """Component c of window w out of the arrays of ma_poa_out_t (dict of flat numpy arrays + the three caps), in describe()'s
    form; paths are recomputed from hap_first and the edge labels"""
    MC, MH = p.max_comps, p.max_haps
    MN, ME, MX = px["max_pnodes"], px["max_pedges"], px["max_cols"]
    ci = w * MC + c
    n0, nn = int(px["comp_pnode0"][ci]), int(px["comp_npnodes"][ci])
    e0, ne = int(px["comp_pedge0"][ci]), int(px["comp_npedges"][ci])
    ncols = int(px["comp_ncols"][ci])
    hap0, nh = int(asm["comp_hap0"][ci]), int(asm["comp_nhaps"][ci])
    ns = slice(w * MN + n0, w * MN + n0 + nn)
    es = slice(w * ME + e0, w * ME + e0 + ne)
    edges = list(zip(px["pedge_tail"][es].tolist(), px["pedge_head"][es].tolist(), px["pedge_haps"][es].tolist()))
    rank = px["pnode_rank"][ns].tolist()
    order = [0] * nn
    for v, r in enumerate(rank):
        order[r] = v
    seq_first = px["hap_first"][w * MH + hap0:w * MH + hap0 + nh].tolist()
    rows = [bytes(px["msa"][(w * MH + hap0 + h) * MX:(w * MH + hap0 + h) * MX + ncols]) for h in range(nh)]
    succ = {}
    for t, hd, m in edges:
        succ.setdefault(t, []).append((hd, m))
    paths = []
    for h in range(nh):
        pth, cur = [], seq_first[h]
        while cur is not None and len(pth) <= nn:
            pth.append(cur)
            cur = next((hd for hd, m in succ.get(cur, []) if m >> h & 1), None)
        paths.append(pth)
    return dict(base=px["pnode_base"][ns].tolist(), rank=rank, col=px["pnode_col"][ns].tolist(), haps=px["pnode_haps"][ns].tolist(),
                edges=edges, order=order, seq_first=seq_first, ncols=ncols, rows=rows, paths=paths)


EXPORT_KEYS = ("base", "rank", "col", "haps", "edges", "order", "seq_first", "ncols", "rows", "paths")


def to_export(p, windows, caps):
    """The restatement's components laid out as ma_poa_out_t wants them: windows = [[haplotype list, ...], ...]; returns
    (asm, px) -- asm holds comp_hap0 / comp_nhaps / win_ncomp / hap_len / hap_bases (what from_export and the host renderers read),
    px the export arrays as flat numpy arrays plus the three caps"""
    import numpy as np
    MC, MH, ML = p.max_comps, p.max_haps, p.max_hap_len
    MN, ME, MX = caps
    n = len(windows)
    u32 = lambda k: np.zeros(k, np.uint32)  # noqa: E731
    asm = dict(win_ncomp=u32(n), comp_hap0=u32(n * MC), comp_nhaps=u32(n * MC), hap_len=u32(n * MH), hap_bases=np.zeros(n * MH * ML, np.uint8))
    px = dict(win_pstatus=u32(n), win_npnodes=u32(n), win_npedges=u32(n), win_ncols=u32(n), comp_pnode0=u32(n * MC), comp_npnodes=u32(n * MC),
              comp_pedge0=u32(n * MC), comp_npedges=u32(n * MC), comp_ncols=u32(n * MC), pnode_base=np.zeros(n * MN, np.uint8),
              pnode_rank=u32(n * MN), pnode_col=u32(n * MN), pnode_haps=u32(n * MN), pedge_tail=u32(n * ME), pedge_head=u32(n * ME),
              pedge_haps=u32(n * ME), hap_first=u32(n * MH), msa=np.zeros(n * MH * MX, np.uint8),
              max_pnodes=MN, max_pedges=ME, max_cols=MX)
    for w, comps in enumerate(windows):
        asm["win_ncomp"][w] = len(comps)
        n0 = e0 = hap0 = 0
        for c, haps in enumerate(comps):
            d = component(haps)
            ci = w * MC + c
            nn, ne = len(d["base"]), len(d["edges"])
            assert n0 + nn <= MN and e0 + ne <= ME and d["ncols"] <= MX and hap0 + len(haps) <= MH
            asm["comp_hap0"][ci], asm["comp_nhaps"][ci] = hap0, len(haps)
            px["comp_pnode0"][ci], px["comp_npnodes"][ci], px["comp_pedge0"][ci], px["comp_npedges"][ci] = n0, nn, e0, ne
            px["comp_ncols"][ci] = d["ncols"]
            ns, es = slice(w * MN + n0, w * MN + n0 + nn), slice(w * ME + e0, w * ME + e0 + ne)
            px["pnode_base"][ns], px["pnode_rank"][ns], px["pnode_col"][ns], px["pnode_haps"][ns] = d["base"], d["rank"], d["col"], d["haps"]
            if ne:
                px["pedge_tail"][es], px["pedge_head"][es], px["pedge_haps"][es] = zip(*d["edges"])
            for h, seq in enumerate(haps):
                hi = w * MH + hap0 + h
                asm["hap_len"][hi] = len(seq)
                asm["hap_bases"][hi * ML:hi * ML + len(seq)] = np.frombuffer(bytes(seq), np.uint8)
                px["hap_first"][hi] = d["seq_first"][h]
                px["msa"][hi * MX:hi * MX + d["ncols"]] = np.frombuffer(d["rows"][h], np.uint8)
            n0, e0, hap0 = n0 + nn, e0 + ne, hap0 + len(haps)
        px["win_npnodes"][w], px["win_npedges"][w] = n0, e0
        px["win_ncols"][w] = max(int(x) for x in px["comp_ncols"][w * MC:(w + 1) * MC])
    return asm, px
