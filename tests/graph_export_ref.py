"""An independent restatement of what the clean stage derives from a pruned component graph.

Input: one window's rows of ma_graph_out_t (include/microasm.h) -- nodes, stored edges, sequences -- plus k, num_samples and
the window's reference bytes.  Output: the component metrics (comp_cx, comp_cxf), the REF row, and for every ALT row the walk
that spells it with its (confidence, nbases) runs and coverage statistics (hap_runs, hap_stats).  Pure Python / numpy; imports
neither the engine nor the oracle, and shares no code with either: it follows the reference's graph_complexity.cpp:16-93,
node.cpp:59-79, max_flow.cpp:64-113, path.cpp:39-70 and base/compute_stats.h as the issue that introduced the export states
them.  Python floats are IEEE doubles and nothing here is fused, so the f64 results round like the reference's scalar code.
"""
import math

import numpy as np

PLUS, MINUS = 0, 1            # sign codes inside edge_kind: kind = source sign << 1 | destination sign
LABEL_REFERENCE = 1           # node_label bit 0
FLAG_SOURCE, FLAG_SINK = 1, 2  # node_flags
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(seq: bytes) -> bytes:
    out = bytearray(seq.translate(_COMP)[::-1])
    for i, c in enumerate(seq[::-1]):
        if c not in b"ACGTacgt":
            out[i] = ord("n") if c == ord("n") else ord("N")
    return bytes(out)


class Node:
    __slots__ = ("slot", "comp", "seq", "counts", "sign", "label", "flags", "edges")

    def __init__(self, slot, comp, seq, counts, sign, label, flags):
        self.slot, self.comp, self.seq, self.counts = slot, comp, seq, [int(c) for c in counts]
        self.sign, self.label, self.flags = PLUS if sign else MINUS, int(label), int(flags)
        self.edges = []  # (dst slot, source sign, destination sign) in stored order

    @property
    def total(self):
        return sum(self.counts)

    @property
    def is_ref(self):
        return bool(self.label & LABEL_REFERENCE)

    def oriented(self, sign):
        """the sequence a walk reads on this node when the edge's sign on the node's side is `sign`"""
        return self.seq if sign == PLUS else revcomp(self.seq)


def window_nodes(gr, w, num_samples, caps=None):
    """The nodes of window w out of the arrays of ma_graph_out_t (flat numpy arrays; caps = (max_nodes, max_edges,
    max_seq_bytes), default gr["max_nodes"] ...).  Returns {slot: Node} with the edges attached."""
    MN, ME, MS = caps or (gr["max_nodes"], gr["max_edges"], gr["max_seq_bytes"])
    S = num_samples
    nn, ne = int(gr["win_nnodes"][w]), int(gr["win_nedges"][w])
    assert int(gr["win_gstatus"][w]) == 0 and nn <= MN and ne <= ME and int(gr["win_nseq"][w]) <= MS
    pool = gr["seq_pool"][w * MS:(w + 1) * MS]
    nodes = {}
    for s in range(nn):
        i = w * MN + s
        off, ln = int(gr["node_seq_off"][i]), int(gr["node_len"][i])
        assert off + ln <= int(gr["win_nseq"][w])
        nodes[s] = Node(s, int(gr["node_comp"][i]), bytes(pool[off:off + ln]), gr["node_cnt"][i * S:(i + 1) * S],
                        int(gr["node_sign"][i]), gr["node_label"][i], gr["node_flags"][i])
    for e in range(ne):
        i = w * ME + e
        src, dst, kind = int(gr["edge_src"][i]), int(gr["edge_dst"][i]), int(gr["edge_kind"][i])
        assert src < nn and dst < nn and kind < 4
        nodes[src].edges.append((dst, (kind >> 1) & 1, kind & 1))
    return nodes


def components(nodes):
    """{component slot: [Node, ...] in slot order}"""
    out = {}
    for s in sorted(nodes):
        out.setdefault(nodes[s].comp, []).append(nodes[s])
    return out


class Welford:  # base/compute_stats.h:75-125
    def __init__(self):
        self.n, self.m1, self.m2 = 0, 0.0, 0.0

    def add(self, x):
        old = self.n
        self.n += 1
        delta = x - self.m1
        nd = delta / float(self.n)
        self.m1 += nd
        self.m2 += delta * nd * float(old)

    @property
    def sd(self):
        return math.sqrt(self.m2 / float(self.n - 1)) if self.n >= 2 else 0.0


def median_u32(values):
    """base/compute_stats.h Median on unsigned integers: the middle one, or the floored mean of the two middle ones"""
    v = sorted(int(x) for x in values)
    if not v:
        return 0
    if len(v) == 1:
        return v[0]
    half = v[len(v) // 2]
    return half if len(v) % 2 == 1 else (half + v[len(v) // 2 - 1]) // 2


def confidence(counts, num_samples, is_ref):
    """Node::Confidence (node.cpp:59-79): the product is taken in f64, as there, and truncated"""
    counts = [int(c) for c in counts]
    if any(c > 0 for c in counts) and all(c <= 1 for c in counts):
        return 1
    total = sum(counts)
    if total == 0:
        return 0
    concordance = float(sum(1 for c in counts if c > 0)) / float(max(num_samples, 1))
    return int(float(total) * concordance) + (1 if is_ref else 0)


def complexity(comp_nodes):
    """graph_complexity.cpp:16-93 over the nodes of one component, in the order given"""
    nn, ne, unitigs, bp, maxdeg = 0, 0, 0, 0, 0
    cov, tip, uni = Welford(), Welford(), Welford()
    for nd in comp_nodes:
        nn += 1
        d = sum(1 for (_, ss, _) in nd.edges if ss == nd.sign)
        o = len(nd.edges) - d
        ne += d + o
        maxdeg = max(maxdeg, d, o)
        bp += d >= 2 or o >= 2
        unitigs += d == 1 and o == 1
        c = float(nd.total)
        cov.add(c)
        if d == 0 or o == 0:
            tip.add(c)
        elif d == 1 and o == 1:
            uni.add(c)
    ne //= 2
    return dict(cyclomatic=max(ne - nn + 1, 0) if ne >= nn else 0, branch_points=bp, max_dir_degree=maxdeg,
                unitig_ratio=(float(unitigs) / float(nn)) if nn else 0.0,
                coverage_cv=(cov.sd / cov.m1) if cov.n and cov.m1 > 0.0 else 0.0,
                tip_to_path=(tip.m1 / uni.m1) if tip.n and uni.n and uni.m1 > 0.0 else 0.0)


def ref_weight(comp_nodes, num_samples):
    confs = [confidence(nd.counts, num_samples, True) for nd in comp_nodes if nd.is_ref]
    return median_u32(confs) if confs else 1


def find_walks(comp_nodes, k, target: bytes, limit=2):
    """Every walk (up to `limit`) from the source-flagged node that spells `target` under BuildSequence's rule and ends at the
    sink-flagged node: [(node, sign), ...].  The first node is spelled whole, every next one minus its first k - 1 bases, each
    in the orientation of the edge's sign on its side; an edge leaves a node on the sign the walk arrived with."""
    by_slot = {nd.slot: nd for nd in comp_nodes}
    src = [nd for nd in comp_nodes if nd.flags & FLAG_SOURCE]
    assert len(src) == 1 and sum(1 for nd in comp_nodes if nd.flags & FLAG_SINK) == 1
    found = []
    for sign0 in (PLUS, MINUS):
        first = src[0].oriented(sign0)
        if not target.startswith(first):
            continue
        stack = [(src[0], sign0, len(first), [(src[0], sign0)])]
        while stack and len(found) < limit:
            nd, sign, pos, walk = stack.pop()
            if pos == len(target) and (nd.flags & FLAG_SINK) and len(walk) > 1:
                found.append(walk)
                continue
            for (dst, ss, ds) in nd.edges:
                if ss != sign:
                    continue
                dn = by_slot[dst]
                piece = dn.oriented(ds)[k - 1:]
                if target[pos:pos + len(piece)] == piece and pos + len(piece) <= len(target):
                    stack.append((dn, ds, pos + len(piece), walk + [(dn, ds)]))
    return found


def walk_runs(walk, k, num_samples):
    """(confidence, nbases) per node of the walk, as Path::mNodeWeights keeps them"""
    return [(confidence(nd.counts, num_samples, nd.is_ref), len(nd.seq) - (k - 1 if i else 0)) for i, (nd, _) in enumerate(walk)]


def expand_runs(runs):
    out = []
    for wgt, nb in runs:
        out.extend([int(wgt)] * int(nb))
    return out


def path_stats(totals):
    """Path::Finalize (path.cpp:39-70): mean, median, sd, cv, qcv, total"""
    st = Welford()
    for t in totals:
        st.add(float(t))
    mean, sd = st.m1, st.sd
    total = mean * float(st.n)
    cv = sd / mean if mean > 0.0 else 0.0
    med = float(median_u32(totals))
    qcv = 0.0
    if len(totals) >= 4:
        s = sorted(totals)
        q1, q3 = float(s[len(s) // 4]), float(s[(len(s) * 3) // 4])
        if q3 + q1 > 0.0:
            qcv = (q3 - q1) / (q3 + q1)
    return [mean, med, sd, cv, qcv, total]


def _cmp_f64(what, got, want, bad):
    got, want = float(got), float(want)
    if want == 0.0 or got == 0.0:
        if got != want:
            bad.append(f"{what}: {got!r} != {want!r} (a zero must be exact)")
    elif not abs(got - want) <= 1e-9 * abs(want):
        bad.append(f"{what}: {got!r} vs {want!r}")


def check_window(gr, w, asm, p, ref_bytes, k, caps=None):
    """Every check of the restatement for window w: the exported graph `gr` against the assembly arrays `asm` (the layout of
    ma_asm_out_t; the engine's or the oracle's).  p: the parameters (num_samples, max_comps, max_haps, max_hap_len, max_runs).
    Integers must be equal -- hap_runs per base --, f64 values within 1e-9 relative, zeros exact.  Returns a list of complaints."""
    bad = []
    S, MC, MH, ML, MR = p.num_samples, p.max_comps, p.max_haps, p.max_hap_len, p.max_runs
    ncomp = int(asm["win_ncomp"][w])
    nodes = window_nodes(gr, w, S, caps)
    comps = components(nodes)
    if sorted(comps) != list(range(ncomp)):
        return [f"w{w}: exported components {sorted(comps)} but win_ncomp = {ncomp}"]
    for c in range(ncomp):
        cn, ci, tag = comps[c], w * MC + c, f"w{w} c{c}"
        seqs = [nd.seq for nd in cn]
        if len(set(seqs)) != len(seqs):
            bad.append(f"{tag}: node sequences are not distinct")
        for nd in cn:
            for (dst, ss, ds) in nd.edges:  # mirror edges both present: dst -> src with both signs turned and swapped
                if nodes[dst].comp != c or (nd.slot, 1 - ds, 1 - ss) not in nodes[dst].edges:
                    bad.append(f"{tag}: edge {nd.slot}->{dst} has no mirror in the component")
        cx = complexity(cn)
        got_i = [int(x) for x in asm["comp_cx"][ci * 3:ci * 3 + 3]]
        if got_i != [cx["cyclomatic"], cx["branch_points"], cx["max_dir_degree"]]:
            bad.append(f"{tag}: comp_cx {got_i} vs {cx}")
        for x, name in enumerate(("unitig_ratio", "coverage_cv", "tip_to_path")):
            _cmp_f64(f"{tag} {name}", asm["comp_cxf"][ci * 4 + x], cx[name], bad)
        hap0, nh, anchor = int(asm["comp_hap0"][ci]), int(asm["comp_nhaps"][ci]), int(asm["comp_anchor"][ci])
        # REF row
        hi = w * MH + hap0
        hl = int(asm["hap_len"][hi])
        if bytes(asm["hap_bases"][hi * ML:hi * ML + hl]) != bytes(ref_bytes[anchor:anchor + hl]):
            bad.append(f"{tag}: REF row is not ref[anchor : anchor + hap_len]")
        runs = [(int(asm["hap_runs"][(hi * MR + r) * 2]), int(asm["hap_runs"][(hi * MR + r) * 2 + 1])) for r in range(int(asm["hap_nruns"][hi]))]
        if runs != [(ref_weight(cn, S), hl)]:
            bad.append(f"{tag}: REF runs {runs} vs weight {ref_weight(cn, S)} x {hl}")
        max_cv, has_alt = -1.0, False
        for h in range(1, nh):
            hi = w * MH + hap0 + h
            hl = int(asm["hap_len"][hi])
            target = bytes(asm["hap_bases"][hi * ML:hi * ML + hl])
            walks = find_walks(cn, k, target)
            if len(walks) != 1:
                bad.append(f"{tag} h{h}: {len(walks)} walks spell the row")
                continue
            walk = walks[0]
            runs = [(int(asm["hap_runs"][(hi * MR + r) * 2]), int(asm["hap_runs"][(hi * MR + r) * 2 + 1])) for r in range(int(asm["hap_nruns"][hi]))]
            if expand_runs(runs) != expand_runs(walk_runs(walk, k, S)):
                bad.append(f"{tag} h{h}: per-base weights differ: {runs} vs {walk_runs(walk, k, S)}")
            st = path_stats([nd.total for nd, _ in walk])
            for x, name in enumerate(("mean", "median", "sd", "cv", "qcv", "total")):
                _cmp_f64(f"{tag} h{h} {name}", asm["hap_stats"][hi * 6 + x], st[x], bad)
            max_cv = max(max_cv, st[3]) if has_alt else st[3]
            has_alt = True
        _cmp_f64(f"{tag} max_alt_cv", asm["comp_cxf"][ci * 4 + 3], max_cv if has_alt else -1.0, bad)
    return bad


def graph_key(gr, w, num_samples, caps=None):
    """The exported graph of window w in a form that does not depend on node order: per component the set of
    (sequence, counts, sign, label, flags) and the set of (source sequence, destination sequence, kind)."""
    nodes = window_nodes(gr, w, num_samples, caps)
    out = {}
    for c, cn in components(nodes).items():
        ns = frozenset((nd.seq, tuple(nd.counts), nd.sign, nd.label, nd.flags) for nd in cn)
        es = frozenset((nd.seq, nodes[d].seq, ss * 2 + ds) for nd in cn for (d, ss, ds) in nd.edges)
        assert len(ns) == len(cn)
        out[c] = (ns, es)
    return out


def as_numpy(d):
    return {k: (np.asarray(v) if not isinstance(v, int) else v) for k, v in d.items()}
