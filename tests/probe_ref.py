"""An independent restatement of ma_assemble_probe_batch's rows (include/microasm.h: ma_probe_out_t) from byte strings alone:
contexts, equality of k-mers, ALT-unique k-mers and their numbering, profiles -- after the reference's cbdg/probe_tracker.cpp
(ComputeFlankRange, BuildAltContext, CollectRefKmerHashes, GenerateAndTag, CountInReads, CountSurvivingKmers, CheckPaths) with
the header's two stated deviations: a k-mer that holds a byte other than A C G T equals nothing and is not counted, and every
ALT-unique k-mer is numbered, not only those in the graph at build time.

Pure Python over bytes; shares no code with the engine.  The raw graph after the first low-coverage pass is made by driving
graph_build_ref._Graph step by step (build, remove_low_cov(0)); the pruned components come to window_rows as lists of node
sequences (tests/probe_cases.py takes them from graph_build_cases.expected_arrays), the haplotypes as byte strings."""
import numpy as np

import graph_build_ref as gb

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
FIELDS = ("pb_k", "pb_alt_kmers", "pb_in_reads", "pb_lowcov1", "pb_final", "pb_hap_mask")


def canon(kmer: bytes):
    """the form two equal k-mers share: the smaller of the k-mer and its reverse complement; None for a k-mer that holds a byte
    other than A C G T -- it equals nothing"""
    if kmer.translate(None, b"ACGT"):
        return None
    rc = kmer.translate(_COMP)[::-1]
    return kmer if kmer <= rc else rc


def kmers(seq: bytes, k):
    return [seq[o:o + k] for o in range(len(seq) - k + 1)]


def contexts(ref: bytes, pos, ref_len, alt: bytes, k):
    """(REF context, ALT context): probe_tracker.cpp:62-96"""
    f = k - 1
    a, e = max(0, pos - f), min(len(ref), pos + ref_len + f)
    return ref[a:e], ref[a:pos] + alt + ref[pos + ref_len:e]


def alt_unique(ref: bytes, pos, ref_len, alt: bytes, k):
    """the ALT-unique k-mers in context order, in canonical form: index = offset j"""
    ref_ctx, alt_ctx = contexts(ref, pos, ref_len, alt, k)
    in_ref = {canon(m) for m in kmers(ref_ctx, k)}
    return [c for c in (canon(m) for m in kmers(alt_ctx, k)) if c is not None and c not in in_ref]


def profile(uniq, present):
    """CountSurvivingKmers (probe_tracker.cpp:602-654) of the offsets j whose k-mer is in the set `present`"""
    offs = [j for j, c in enumerate(uniq) if c in present]
    last = len(uniq) - 1
    edge = sum(1 for j in offs if j == 0 or j == last)
    gaps = sum(1 for a, b in zip(offs, offs[1:]) if b - a > 1)
    return [len(offs), edge, len(offs) - edge, gaps]


def canon_set(seqs, k):
    """every k-mer that occurs in one of the sequences, canonical"""
    out = set()
    for s in seqs:
        out.update(canon(m) for m in kmers(s, k))
    out.discard(None)
    return out


def in_reads(uniq, read_seqs, k):
    """CountInReads (probe_tracker.cpp:299-330): per occurrence in a read and per offset that holds the k-mer; and the reads
    that hold at least one.  ALL reads, whatever their flags."""
    times = {}
    for c in uniq:
        times[c] = times.get(c, 0) + 1
    occ = holders = 0
    for s in read_seqs:
        hits = sum(times.get(canon(m), 0) for m in kmers(s, k))
        occ += hits
        holders += hits > 0
    return [occ, holders]


def lowcov1_kmers(ref: bytes, reads, k, params):
    """the k-mers of the raw graph after BuildGraph and RemoveLowCovNodes(0) (graph.cpp:125-135): what pruned_at_lowcov1 counts"""
    g = gb._Graph(int(k), params, gb.new_counters())
    g.build(ref, reads)
    g.remove_low_cov(0)
    return canon_set([nd.seq for nd in g.nodes if nd.alive], k)


def window_rows(ref, reads, k, probes, max_comps, lowcov1, comp_nodes, comp_haps):
    """The rows of one window's probes [(pos, ref_len, alt)] at k: lowcov1 = lowcov1_kmers(...); comp_nodes = per comp_* row the
    node sequences of the pruned component, or None when the window's graph is not comparable (pb_final is then None); comp_haps
    = per comp_* row the haplotypes, REF first.  k == 0: zero rows."""
    MC = max_comps
    rows = []
    read_seqs = [r[0] for r in reads]
    node_sets = None if comp_nodes is None else [canon_set(seqs, k) for seqs in comp_nodes]
    for pos, ref_len, alt in probes:
        assert pos < len(ref) and pos + ref_len <= len(ref)
        if k == 0:
            rows.append(dict(pb_k=0, pb_alt_kmers=0, pb_in_reads=[0, 0], pb_lowcov1=[0] * 4, pb_final=[0] * (4 * MC), pb_hap_mask=[0] * MC))
            continue
        uniq = alt_unique(ref, pos, ref_len, alt, k)
        alt_ctx = contexts(ref, pos, ref_len, alt, k)[1]
        final = None
        if node_sets is not None:
            final = [0] * (4 * MC)
            for c, present in enumerate(node_sets):
                final[4 * c:4 * c + 4] = profile(uniq, present)
        mask = [0] * MC
        for c, haps in enumerate(comp_haps):
            mask[c] = sum(1 << h for h, hap in enumerate(haps) if alt_ctx in hap)
        rows.append(dict(pb_k=k, pb_alt_kmers=len(uniq), pb_in_reads=in_reads(uniq, read_seqs, k), pb_lowcov1=profile(uniq, lowcov1),
                         pb_final=final, pb_hap_mask=mask))
    return rows


def engine_row(po, p, max_comps):
    """probe p of ma_probe_out_t arrays, as window_rows lays a row out"""
    MC = max_comps
    return dict(pb_k=int(po["pb_k"][p]), pb_alt_kmers=int(po["pb_alt_kmers"][p]), pb_in_reads=[int(x) for x in po["pb_in_reads"][2 * p:2 * p + 2]],
                pb_lowcov1=[int(x) for x in po["pb_lowcov1"][4 * p:4 * p + 4]],
                pb_final=[int(x) for x in po["pb_final"][4 * MC * p:4 * MC * (p + 1)]],
                pb_hap_mask=[int(x) for x in po["pb_hap_mask"][MC * p:MC * (p + 1)]])


def compare(got_rows, want_rows, what=""):
    """every field of every row, exactly (a field the restatement left None is not comparable); -> complaints"""
    bad = []
    assert len(got_rows) == len(want_rows)
    for i, (g, w) in enumerate(zip(got_rows, want_rows)):
        for f in FIELDS:
            if w[f] is not None and g[f] != w[f]:
                bad.append(f"{what} probe {i} {f}: {g[f]} (got) vs {w[f]} (restatement)")
    return bad


def rows_to_arrays(rows, max_comps):
    """rows as the flat arrays of ma_probe_out_t (None fields as zeros)"""
    MC = max_comps
    flat = lambda f, width: np.asarray([x for r in rows for x in (r[f] if r[f] is not None else [0] * width)], dtype=np.uint32)  # noqa: E731
    return dict(pb_k=np.asarray([r["pb_k"] for r in rows], np.uint32), pb_alt_kmers=np.asarray([r["pb_alt_kmers"] for r in rows], np.uint32),
                pb_in_reads=flat("pb_in_reads", 2), pb_lowcov1=flat("pb_lowcov1", 4), pb_final=flat("pb_final", 4 * MC),
                pb_hap_mask=flat("pb_hap_mask", MC))
