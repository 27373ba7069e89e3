"""Pins tests/graph_export_ref.py -- the independent restatement the graph-export GPU tests check the engine with -- on two
hand-written graphs whose numbers are worked out below, and its two integer rules against the oracle's known-answer hooks."""
import ctypes as C
import math
import types

import numpy as np

import graph_export_ref as ref
from harness import oracle

K = 5
# A bubble with one tip, seven nodes, every overlap K - 1 = 4 bases:
#
#   S -> A -> B1 -> C -> T        S = source anchor, T = sink anchor; B1 carries the reference base, B2 the SNV
#             B2 ->  \-> X        X = a tip hanging off C
#
#   node  sequence     counts   total  label            d  o   class
#   S     ACGTACGGA    10,10    20     REF|CTRL|CASE    1  0   tip (o == 0)
#   A     CGGATTC       9,11    20     REF|CTRL|CASE    2  1   branch point
#   B1    ATTCGCAAG     6, 6    12     REF|CTRL|CASE    1  1   unitig
#   B2    ATTCACAAG     4, 4     8     CTRL|CASE        1  1   unitig
#   C     CAAGTTGCA    10,10    20     REF|CTRL|CASE    2  2   branch point
#   T     TGCATCGAT    10,10    20     REF|CTRL|CASE    0  1   tip (d == 0)
#   X     TGCAGG        1, 1     2     CASE             0  1   tip
#
# 7 forward edges + their 7 mirrors are stored: E / 2 = 7, V = 7 -> cyclomatic = 7 - 7 + 1 = 1; 2 branch points; the largest
# single-direction degree is 2; unitig ratio 2 / 7.
# coverage: mean 102 / 7; sum of squares 4 * 400 + 144 + 64 + 4 = 1812, minus 102^2 / 7 -> 325.714285...; / 6 -> variance;
#           CV = sqrt(54.285714...) / 14.571428... = 0.505639...
# tips S, T, X: mean (20 + 20 + 2) / 3 = 14; unitigs B1, B2: mean 10 -> tip / path = 1.4
# confidence (two samples, both with support: total x 2 / 2, + 1 on REFERENCE nodes; X is all singletons -> 1):
#   S 21, A 21, B1 13, B2 8, C 21, T 21, X 1
# REF row: median of the REFERENCE nodes' confidences {13, 21, 21, 21, 21} = 21, one run over the 27-base anchor
# ALT row (through B2): runs (21, 9) (21, 3) (8, 5) (21, 5) (21, 5); coverages 20 20 8 20 20: mean 17.6, median 20,
#   variance (4 * 400 + 64 - 5 * 17.6^2) / 4 = 28.8, sd = sqrt(28.8), cv = sd / 17.6, quartiles s[1] = s[3] = 20 -> qcv 0, total 88
NODES = [("S", b"ACGTACGGA", (10, 10), 7, ref.FLAG_SOURCE), ("A", b"CGGATTC", (9, 11), 7, 0), ("B1", b"ATTCGCAAG", (6, 6), 7, 0),
         ("B2", b"ATTCACAAG", (4, 4), 6, 0), ("C", b"CAAGTTGCA", (10, 10), 7, 0), ("T", b"TGCATCGAT", (10, 10), 7, ref.FLAG_SINK),
         ("X", b"TGCAGG", (1, 1), 4, 0)]
FORWARD = [("S", "A"), ("A", "B1"), ("A", "B2"), ("B1", "C"), ("B2", "C"), ("C", "T"), ("C", "X")]
REF_SEQ = b"ACGTACGGA" + b"TTC" + b"GCAAG" + b"TTGCA" + b"TCGAT"
ALT_SEQ = b"ACGTACGGA" + b"TTC" + b"ACAAG" + b"TTGCA" + b"TCGAT"
PARAMS = types.SimpleNamespace(num_samples=2, max_comps=2, max_haps=4, max_hap_len=64, max_runs=8)


def export_arrays(minus=()):
    """one window's ma_graph_out_t arrays for the bubble; nodes named in `minus` are stored reverse complemented with sign MINUS
    (the same graph: the edges that touch them carry MINUS on their side)"""
    caps = dict(max_nodes=8, max_edges=16, max_seq_bytes=80)
    idx = {name: i for i, (name, *_r) in enumerate(NODES)}
    gr = dict(caps, win_gstatus=np.zeros(1, np.uint32), win_nnodes=np.array([7], np.uint32), win_nedges=np.array([14], np.uint32),
              node_comp=np.zeros(8, np.uint32), node_seq_off=np.zeros(8, np.uint32), node_len=np.zeros(8, np.uint32),
              node_cnt=np.zeros(16, np.uint32), node_sign=np.zeros(8, np.uint8), node_label=np.zeros(8, np.uint8),
              node_flags=np.zeros(8, np.uint8), edge_src=np.zeros(16, np.uint32), edge_dst=np.zeros(16, np.uint32),
              edge_kind=np.zeros(16, np.uint8), seq_pool=np.zeros(80, np.uint8))
    at = 0
    for i, (name, seq, cnt, label, flags) in enumerate(NODES):
        stored = ref.revcomp(seq) if name in minus else seq
        gr["seq_pool"][at:at + len(stored)] = np.frombuffer(stored, np.uint8)
        gr["node_seq_off"][i], gr["node_len"][i] = at, len(stored)
        gr["node_cnt"][2 * i:2 * i + 2] = cnt
        gr["node_sign"][i], gr["node_label"][i], gr["node_flags"][i] = 0 if name in minus else 1, label, flags
        at += len(stored)
    gr["win_nseq"] = np.array([at], np.uint32)
    edges = []  # the edges of a node contiguous, nodes in slot order: forward edges, then the mirrors of the incoming ones
    sgn = lambda name: ref.MINUS if name in minus else ref.PLUS  # noqa: E731
    for name, *_r in NODES:
        for u, v in FORWARD:
            if u == name:
                edges.append((idx[u], idx[v], sgn(u) * 2 + sgn(v)))
        for u, v in FORWARD:
            if v == name:  # mirror: both signs turned and swapped
                edges.append((idx[v], idx[u], (1 - sgn(v)) * 2 + (1 - sgn(u))))
    for e, (s, d, kind) in enumerate(edges):
        gr["edge_src"][e], gr["edge_dst"][e], gr["edge_kind"][e] = s, d, kind
    return gr


def asm_rows():
    p = PARAMS
    asm = dict(win_status=np.zeros(1, np.uint32), win_k=np.array([K], np.uint32), win_ncomp=np.array([1], np.uint32),
               comp_anchor=np.array([3, 0], np.uint32), comp_hap0=np.zeros(2, np.uint32), comp_nhaps=np.array([2, 0], np.uint32),
               comp_cx=np.zeros(6, np.uint32), comp_cxf=np.zeros(8), hap_len=np.zeros(4, np.uint32), hap_nruns=np.zeros(4, np.uint32),
               hap_stats=np.zeros(24), hap_bases=np.zeros(4 * p.max_hap_len, np.uint8), hap_runs=np.zeros(4 * p.max_runs * 2, np.uint32))
    sd = math.sqrt(28.8)
    asm["comp_cx"][:3] = (1, 2, 2)
    asm["comp_cxf"][:4] = (2.0 / 7.0, math.sqrt((1812.0 - 102.0 * 102.0 / 7.0) / 6.0) / (102.0 / 7.0), 1.4, sd / 17.6)
    for h, (seq, runs) in enumerate(((REF_SEQ, [(21, 27)]), (ALT_SEQ, [(21, 9), (21, 3), (8, 5), (21, 5), (21, 5)]))):
        asm["hap_len"][h], asm["hap_nruns"][h] = len(seq), len(runs)
        asm["hap_bases"][h * p.max_hap_len:h * p.max_hap_len + len(seq)] = np.frombuffer(seq, np.uint8)
        asm["hap_runs"][h * p.max_runs * 2:h * p.max_runs * 2 + 2 * len(runs)] = np.array(runs, np.uint32).ravel()
    asm["hap_stats"][6:12] = (17.6, 20.0, sd, sd / 17.6, 0.0, 88.0)
    return asm


REF_WINDOW = b"GGG" + REF_SEQ + b"CC"  # the anchor starts at offset 3 of the window


def test_bubble_with_a_tip():
    gr = export_arrays()
    cn = ref.components(ref.window_nodes(gr, 0, 2))[0]
    cx = ref.complexity(cn)
    assert (cx["cyclomatic"], cx["branch_points"], cx["max_dir_degree"]) == (1, 2, 2)
    assert cx["unitig_ratio"] == 2.0 / 7.0 and abs(cx["tip_to_path"] - 1.4) < 1e-15
    assert abs(cx["coverage_cv"] - math.sqrt((1812.0 - 102.0 * 102.0 / 7.0) / 6.0) / (102.0 / 7.0)) < 1e-12 and abs(cx["coverage_cv"] - 0.505639) < 1e-6
    assert [ref.confidence(nd.counts, 2, nd.is_ref) for nd in cn] == [21, 21, 13, 8, 21, 21, 1]
    assert ref.ref_weight(cn, 2) == 21
    walks = ref.find_walks(cn, K, ALT_SEQ)
    assert len(walks) == 1 and [nd.slot for nd, _ in walks[0]] == [0, 1, 3, 4, 5] and all(s == ref.PLUS for _, s in walks[0])
    assert ref.walk_runs(walks[0], K, 2) == [(21, 9), (21, 3), (8, 5), (21, 5), (21, 5)]
    assert [nd.slot for nd, _ in ref.find_walks(cn, K, REF_SEQ)[0]] == [0, 1, 2, 4, 5]
    assert ref.find_walks(cn, K, ALT_SEQ[:-1]) == []  # must end on the sink, with every base spelled
    st = ref.path_stats([20, 20, 8, 20, 20])
    assert st[0] == 17.6 and st[1] == 20.0 and abs(st[2] - math.sqrt(28.8)) < 1e-12 and st[4] == 0.0 and abs(st[5] - 88.0) < 1e-12
    assert ref.check_window(gr, 0, asm_rows(), PARAMS, REF_WINDOW, K) == []


def test_a_minus_signed_node_on_the_alt_walk():
    """B2 stored as its reverse complement CTTGTGAAT with sign MINUS: A -> B2 becomes +-, B2 -> C becomes -+ (and their mirrors
    +- and -+).  For B2 d counts the edges whose source sign is MINUS -- B2 -> C -- and o the other: still a unitig; every
    number of the table above stands, and the walk reads B2 reverse complemented."""
    gr = export_arrays(minus=("B2",))
    nodes = ref.window_nodes(gr, 0, 2)
    assert nodes[3].seq == b"CTTGTGAAT" and nodes[3].sign == ref.MINUS
    assert sorted(nodes[3].edges) == [(1, ref.PLUS, ref.MINUS), (4, ref.MINUS, ref.PLUS)]
    cn = ref.components(nodes)[0]
    assert ref.complexity(cn) == ref.complexity(ref.components(ref.window_nodes(export_arrays(), 0, 2))[0])
    walks = ref.find_walks(cn, K, ALT_SEQ)
    assert len(walks) == 1 and [(nd.slot, s) for nd, s in walks[0]] == [(0, 0), (1, 0), (3, ref.MINUS), (4, 0), (5, 0)]
    assert ref.check_window(gr, 0, asm_rows(), PARAMS, REF_WINDOW, K) == []
    # ... and the checks do see a wrong row: another weight on the ALT walk, a metric off by one, a zero that is not one
    for key, at, val in (("hap_runs", 2 * PARAMS.max_runs + 4, 9), ("comp_cx", 1, 3), ("hap_stats", 10, 1e-300)):
        asm = asm_rows()
        asm[key][at] = val
        assert ref.check_window(gr, 0, asm, PARAMS, REF_WINDOW, K), key


def test_confidence_and_median_against_the_oracle():
    lib = oracle()  # (the shared handle: called as tests/test_oracle_kat.py calls it, nothing declared on it)
    rng = np.random.default_rng(20240607)
    for it in range(400):
        S = int(rng.integers(1, 9))
        hi = (2, 4, 40, 3000, 1 << 20)[it % 5]
        counts = rng.integers(0, hi, size=S).astype(np.uint32)
        if it % 7 == 0:
            counts[rng.integers(0, S)] = 0
        for is_ref in (0, 1):
            want = lib.orc_confidence(counts.ctypes.data_as(C.c_void_p), S, S, is_ref) & 0xFFFFFFFF
            assert ref.confidence(counts, S, bool(is_ref)) == want, (counts, S, is_ref)
        vals = rng.integers(0, hi * 3, size=int(rng.integers(1, 40))).astype(np.uint32)
        assert ref.median_u32(vals) == lib.orc_median_u32(vals.ctypes.data_as(C.c_void_p), C.c_uint64(len(vals))), vals
