"""Pins tests/graph_build_ref.py -- the independent restatement of build + prune that tests/test_gpu_graph_build.py holds the
exported graphs to -- on a toy worked out by hand, chains it with tests/graph_export_ref.py against the oracle's assembly rows
on every case of tests/graph_build_cases.py (reads -> pruned graph -> rows, no engine, no GPU), asserts from its counters that
every case reaches the edge it was built for, shows that the `gate` window's graph changes under each wrong rule of the
expected-error gate, and that the comparison of the GPU file reports a changed count, a flipped label bit and a dropped edge."""
import functools
import types

import numpy as np
import pytest

import graph_build_cases as gc
import graph_build_ref as gb
import graph_export_ref as ref
from harness import OracleEngine

# ---- the toy: k = 5, a 22-base reference, thirteen reads, two samples (0 = CTRL, 1 = CASE) -------------------------------------
#
#   position   0         1         2
#              0123456789012345678901
#   REF        GGATCACAGTCTACACTGCTCA          18 k-mers r0 .. r17
#   ALT        GGATCACAGTCTCCACTGCTCA          REF with C at 12: five new k-mers a8 .. a12 between r7 and r13
#   TIP                 TCTACACTTCC            REF[9:17] + TCC: three new k-mers t13 t14 t15 behind r12
#
#   k-mer as read -> stored (sign): r0 GGATC -> GATCC (-), r1 GATCA (+), r2 ATCAC (+), r3 TCACA (+), r4 CACAG (+), r5 ACAGT (+),
#   r6 CAGTC (+), r7 AGTCT -> AGACT (-), r8 GTCTA (+), r9 TCTAC -> GTAGA (-), r10 CTACA (+), r11 TACAC -> GTGTA (-), r12 ACACT (+),
#   r13 CACTG (+), r14 ACTGC (+), r15 CTGCT -> AGCAG (-), r16 TGCTC -> GAGCA (-), r17 GCTCA (+);
#   a8 GTCTC -> GAGAC (-), a9 TCTCC -> GGAGA (-), a10 CTCCA (+), a11 TCCAC -> GTGGA (-), a12 CCACT -> AGTGG (-);
#   t13 CACTT -> AAGTG (-), t14 ACTTC (+), t15 CTTCC (+).  Every forward edge has the kind (sign of its source, sign of its
#   destination), its mirror both signs turned and swapped.
#
#   reads, in batch order (quality 30 = 0.001 a base unless said):
#     CTRL  q0 REF | q1 REF | q2, q3 REF[3:11] (r3 .. r6) | q4 REF[0:9] (r0 .. r4) with Q3 at its bases 1 and 5 |
#           q0 again: REF[0:8] (r0 .. r3), the mate of the first read
#     CASE  q5, q6 REF | q7, q8 ALT | q9, q10 TIP | q11 ALT, failing the filter
#   the gate: only the k-mer at offset 1 of q4 holds both Q3 bases: 2 x 0.5011872336272722 + 3 x 0.001 = 1.0053..., floor 1:
#     refused (and the one instance within 0.02 of 1.0, above); the others hold one: 0.505, counted.
#   mate-mers: the second q0 read finds (q0, node, CTRL) of r0 .. r3 in the set: four increments suppressed.
#   counts (CTRL, CASE) after the build: r0 3,4 | r1 2,4 (q4 refused) | r2 3,4 | r3 r4 5,4 | r5 r6 4,4 | r7 2,4 | r8 2,2 (neither
#     ALT nor TIP holds it) | r9 .. r12 2,4 (TIP) | r13 .. r17 2,4 (ALT) | a8 .. a12 0,2 | t13 .. t15 0,2.
#   labels: the reference inserted r0 .. r17 first -> REFERENCE only, whatever supports them later; a*, t* -> CASE only.
#   first low-coverage pass: every total is >= 2 and (0, 2) is no singleton: nothing goes.  One component; source r0 (total 7),
#     sink r17 (total 6), anchor start 0, 22 bases.
#   first compression, nodes in insertion order.  A node merges along an arm only if BOTH its arms lead to chain-interior nodes
#     whose onward neighbour has at most two edges; a neighbour with one edge (the anchors r0, r17; t15) is no buddy.
#       r1: its arm to r0 ends there -> never.   r2 absorbs r3 (++): ATCAC + A; the length is 6 AFTER the merge, so CTRL becomes
#       (3 x 6 + 5 x 5) // 11 = 3 -- with the length from before, (3 x 5 + 5 x 5) // 10 = 4 -- and CASE (4 x 6 + 4 x 5) // 11 = 4;
#       then r4: (3 x 7 + 5 x 5) // 12 = 3, (4 x 7 + 4 x 5) // 12 = 4; then r5: (3 x 8 + 4 x 5) // 13 = 3, (32 + 20) // 13 = 4: ATCACAGT
#       3,4.  r6 is no buddy: its onward neighbour r7 has three edges (r6, r8, a8).  r6, r8, r9, a8, a9: an arm meets r7 -> no.
#       r10, r11, r14, r15, a12, t13, t14: an arm meets r12 (r11, r13, t13) or r13 (r12, r14, a12) -> no.  r16: its arm to r17.
#       a10 absorbs a11 (+-): CTCCA + last base of revcomp(GTGGA) = CTCCAC, 0,2; a12 is no buddy (r13 behind it).
#       t15 (one edge, --) absorbs t14: first base of ACTTC in front: ACTTCC, 0,2; t13 is no buddy (r12 behind it).
#   second low-coverage pass and second compression: nothing.
#   tips: round 1 removes ACTTCC (one edge, 2 own bases < 5); t13 is left with one edge: round 2 removes it; now r12 has two
#     edges and the compression after round 2 lets r10 absorb r11 (+-): CTACA + C = CTACAC, (2 x 6 + 2 x 5) // 11 = 2,
#     (4 x 6 + 4 x 5) // 11 = 4; r12 is no buddy (r13 behind it).  Round 3 finds no tip.
#   left: 18 nodes, 18 forward edges and their mirrors.
TOY_K = 5
TOY_REF = b"GGATCACAGTCTACACTGCTCA"
TOY_ALT = b"GGATCACAGTCTCCACTGCTCA"
TOY_TIP = b"TCTACACTTCC"
TOY_PARAMS = types.SimpleNamespace(num_samples=2, min_node_cov=2, min_anchor_cov=3, min_anchor_len=10)
P, M = gb.PLUS, gb.MINUS
R, CASE = gb.L_REFERENCE, gb.L_CASE
TOY_NODES = {  # name: (stored sequence, counts, sign, label, flags)
    "r0": (b"GATCC", (3, 4), M, R, ref.FLAG_SOURCE), "r1": (b"GATCA", (2, 4), P, R, 0), "r2-5": (b"ATCACAGT", (3, 4), P, R, 0),
    "r6": (b"CAGTC", (4, 4), P, R, 0), "r7": (b"AGACT", (2, 4), M, R, 0), "r8": (b"GTCTA", (2, 2), P, R, 0), "r9": (b"GTAGA", (2, 4), M, R, 0),
    "r10-11": (b"CTACAC", (2, 4), P, R, 0), "r12": (b"ACACT", (2, 4), P, R, 0), "r13": (b"CACTG", (2, 4), P, R, 0),
    "r14": (b"ACTGC", (2, 4), P, R, 0), "r15": (b"AGCAG", (2, 4), M, R, 0), "r16": (b"GAGCA", (2, 4), M, R, 0),
    "r17": (b"GCTCA", (2, 4), P, R, ref.FLAG_SINK), "a8": (b"GAGAC", (0, 2), M, CASE, 0), "a9": (b"GGAGA", (0, 2), M, CASE, 0),
    "a10-11": (b"CTCCAC", (0, 2), P, CASE, 0), "a12": (b"AGTGG", (0, 2), M, CASE, 0)}
TOY_FORWARD = [("r0", "r1"), ("r1", "r2-5"), ("r2-5", "r6"), ("r6", "r7"), ("r7", "r8"), ("r8", "r9"), ("r9", "r10-11"), ("r10-11", "r12"),
               ("r12", "r13"), ("r13", "r14"), ("r14", "r15"), ("r15", "r16"), ("r16", "r17"),
               ("r7", "a8"), ("a8", "a9"), ("a9", "a10-11"), ("a10-11", "a12"), ("a12", "r13")]


def toy_reads():
    def read(seq, qname, sample, qual=None, passing=True):
        q = bytes(qual) if qual is not None else bytes([30] * len(seq))
        return seq, q, qname, sample, (gb.RF_PASS if passing else 0) | (gb.RF_CASE if sample == 1 else 0)
    return [read(TOY_REF, 0, 0), read(TOY_REF, 1, 0), read(TOY_REF[3:11], 2, 0), read(TOY_REF[3:11], 3, 0),
            read(TOY_REF[:9], 4, 0, [30, 3, 30, 30, 30, 3, 30, 30, 30]), read(TOY_REF[:8], 0, 0),
            read(TOY_REF, 5, 1), read(TOY_REF, 6, 1), read(TOY_ALT, 7, 1), read(TOY_ALT, 8, 1),
            read(TOY_TIP, 9, 1), read(TOY_TIP, 10, 1), read(TOY_ALT, 11, 1, passing=False)]


def test_toy_worked_by_hand():
    log = []
    bw = gb.build_graph(TOY_REF, toy_reads(), TOY_K, TOY_PARAMS, log)
    assert len(bw) == 1 and bw[0]["anchor"] == 0
    by_idx = {nd["idx"]: nd for nd in bw[0]["nodes"]}
    got_nodes = {(nd["seq"], tuple(nd["counts"]), nd["sign"], nd["label"], nd["flags"]) for nd in by_idx.values()}
    assert got_nodes == set(TOY_NODES.values())
    want_edges = set()
    for a, b in TOY_FORWARD:
        (sa, _, ga, *_r), (sb, _, gb_, *_r2) = TOY_NODES[a], TOY_NODES[b]
        want_edges |= {(sa, sb, ga * 2 + gb_), (sb, sa, (1 - gb_) * 2 + (1 - ga))}
    got_edges = [(nd["seq"], by_idx[d]["seq"], kind) for nd in by_idx.values() for d, kind in nd["edges"]]
    assert len(got_edges) == 36 and set(got_edges) == want_edges
    # a merged node keeps its absorber's orientation: ATCACAGT is above its reverse complement ACTGTGAT, and stays as it is
    assert TOY_NODES["r2-5"][0] > ref.revcomp(TOY_NODES["r2-5"][0]) and all(len(s) > TOY_K or s <= ref.revcomp(s) for s, *_ in got_nodes)
    assert log == [("merge", b"ATCAC", b"TCACA", "++", (3, 4)), ("merge", b"ATCACA", b"CACAG", "++", (3, 4)),
                   ("merge", b"ATCACAG", b"ACAGT", "++", (3, 4)), ("merge", b"CTCCA", b"GTGGA", "+-", (0, 2)),
                   ("merge", b"CTTCC", b"ACTTC", "--", (0, 2)), ("remove", "tip", b"ACTTCC", (0, 2)),
                   ("remove", "tip", b"AAGTG", (0, 2)), ("merge", b"CTACA", b"GTGTA", "+-", (2, 4))]
    c = bw.counters
    assert (c["mate_suppressed"], c["gate_refused"], c["gate_near_above"], c["gate_near_below"]) == (4, 1, 1, 0)
    assert (c["reads_used"], c["reads_filtered"], c["nodes_built"], c["ref_first_supported"]) == (12, 1, 26, 18)
    assert c["merges"] == [3, 2, 0, 1] and c["tip_rounds"] == [[1, 1]] and c["singletons_with_cov"] == 0
    # the layout: what graph_export_ref reads back is what went in, and its walk search spells both haplotypes over it
    gr = gb.to_export_arrays(list(bw), 2)
    nodes = ref.window_nodes(gr, 0, 2)
    assert {(nd.seq, tuple(nd.counts), nd.sign, nd.label, nd.flags) for nd in nodes.values()} == set(TOY_NODES.values())
    cn = ref.components(nodes)[0]
    assert len(ref.find_walks(cn, TOY_K, TOY_ALT)) == 1 and len(ref.find_walks(cn, TOY_K, TOY_REF)) == 1
    assert [len(nd.seq) for nd, _ in ref.find_walks(cn, TOY_K, TOY_ALT)[0]] == [5, 5, 8, 5, 5, 5, 5, 6, 5, 5, 5, 5, 5, 5]


def test_toy_rules_one_at_a_time():
    """what the toy's graph would be under each rule the issue names as unwatched: every one changes a node of the result"""
    base = gb.build_graph(TOY_REF, toy_reads(), TOY_K, TOY_PARAMS)
    key = lambda bw: {(nd["seq"], tuple(nd["counts"]), nd["label"]) for nd in bw[0]["nodes"]}  # noqa: E731
    reads = toy_reads()
    # the mate counted (another qname): r0, r2 and the r2-5 chain get one more CTRL read
    other = list(reads)
    other[5] = other[5][:2] + (99,) + other[5][3:]
    assert key(gb.build_graph(TOY_REF, other, TOY_K, TOY_PARAMS)) != key(base)
    # the gated k-mer let through (Q4 in place of Q3: 2 x 0.398 + 0.003 < 1): r1 becomes 3,4
    other = list(reads)
    other[4] = other[4][:1] + (bytes([30, 4, 30, 30, 30, 4, 30, 30, 30]),) + other[4][2:]
    got = gb.build_graph(TOY_REF, other, TOY_K, TOY_PARAMS)
    assert (b"GATCA", (3, 4), R) in key(got) and got.counters["gate_refused"] == 0
    # the filtered read counted: the ALT k-mers get 0,3
    other = list(reads)
    other[12] = other[12][:4] + (gb.RF_PASS | gb.RF_CASE,)
    assert (b"CTCCAC", (0, 3), CASE) in key(gb.build_graph(TOY_REF, other, TOY_K, TOY_PARAMS))


# ---- the cases: restatement -> graph_export_ref -> the oracle's rows -------------------------------------------------------------
CASE_NAMES = ("c2", "c3_ladder", "c5_three_samples", "c4_deep", "handmade")


@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    c = gc.cases()[name]
    return OracleEngine(c.params).assemble(c.arrs, c.n, c.nr)


def one_window(asm, w, n):
    """the rows of window w as a batch of one"""
    return {k: v[w * (len(v) // n):(w + 1) * (len(v) // n)] for k, v in asm.items()}


def compared_windows(name):
    c, asm = gc.cases()[name], oracle_rows(name)
    return [w for w in range(c.n) if gc.comparable(asm, w)]


def test_case_names():
    assert tuple(gc.cases()) == CASE_NAMES


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatements_explain_the_oracles_rows(name):
    c, asm = gc.cases()[name], oracle_rows(name)
    done = compared_windows(name)
    for w in done:
        k = int(asm["win_k"][w])
        gr = gc.expected_arrays(name, w, asm)
        refb = c.arrs["ref_bases"][int(c.arrs["ref_off"][w]):int(c.arrs["ref_off"][w + 1])]
        bad = ref.check_window(gr, 0, one_window(asm, w, c.n), c.params, refb, k)
        assert bad == [], f"{name} w{w} k={k}: " + "\n".join(bad[:10])
    # (a one-window set cannot reach four: the deep window must be compared itself)
    assert len(done) >= c.min_compared and 2 * len(done) >= c.n, (name, done)
    if c.handmade:
        assert done == list(range(c.n))
    if name == "c3_ladder":
        assert any(int(asm["win_k"][w]) > c.params.min_k for w in done)


def hm_counters(which):
    asm = oracle_rows("handmade")
    w = gc.HANDMADE.index(which)
    return gc.built("handmade", w, int(asm["win_k"][w])).counters


def hm_nodes(which):
    asm = oracle_rows("handmade")
    w = gc.HANDMADE.index(which)
    return [nd for e in gc.built("handmade", w, int(asm["win_k"][w])) for nd in e["nodes"]]


@functools.lru_cache(maxsize=None)
def unedited_counters(which):
    c = gc.cases()["handmade"]
    arrs, _n, _nr = gc.synth.pack_batch([gc.base_window(which)])
    return gb.build_window(arrs, 0, gc.K, c.params).counters


def test_mate_mer_cases_reach_the_set():
    plain = unedited_counters("mates")
    assert plain["mate_other_tag"] == 0
    # ten mates of 120 bases (96 k-mers each, less what the gate refuses) and two whole copies (126 each)
    assert hm_counters("mates_overlap")["mate_suppressed"] >= plain["mate_suppressed"] + 10 * 60 + 2 * 100
    # ten pairs that overlap by at least 90 bases: at least 66 shared k-mers a pair, less errors
    assert hm_counters("mates_same_role")["mate_suppressed"] >= plain["mate_suppressed"] + 10 * 40
    assert hm_counters("mates_same_role")["mate_other_tag"] == 0
    other = hm_counters("mates_other_role")
    assert other["mate_other_tag"] >= 10 * 40 and other["mate_suppressed"] == plain["mate_suppressed"]


def test_gate_case_sits_on_the_boundary():
    c = hm_counters("gate")
    assert c["gate_refused"] > 0 and c["gate_near_below"] >= 20 and c["gate_near_above"] >= 20, c
    q = gc.echo_pattern()
    assert list(q[:25]) == list(q[125:]) and (q[25:125] == 2).all()
    fresh, acc, prefix = 0.0, 0.0, [0.0]
    for x in q[:25]:
        fresh += gb.PHRED_ERR[int(x)]
    for x in q:
        acc += gb.PHRED_ERR[int(x)]
        prefix.append(acc)
    assert fresh == prefix[25] < 1.0 and prefix[150] - prefix[125] == 1.0 and prefix[125] > 64.0


def gate_window_key(reads=None):
    """graph_key-like view of the `gate` window's pruned graph (under whatever rules gb._Graph has at the moment), and the
    deciding k-mers of its three bubbles that a node of the graph holds"""
    c = gc.cases()["handmade"]
    ref_bytes, batch_reads = gb.window_inputs(c.arrs, gc.HANDMADE.index("gate"))
    bw = gb.build_graph(ref_bytes, reads if reads is not None else batch_reads, gc.K, c.params)
    assert len(bw) == 1
    nodes = bw[0]["nodes"]
    by_idx = {nd["idx"]: nd for nd in nodes}
    key = (frozenset((nd["seq"], tuple(nd["counts"]), nd["sign"], nd["label"], nd["flags"]) for nd in nodes),
           frozenset((nd["seq"], by_idx[d]["seq"], kind) for nd in nodes for d, kind in nd["edges"]))
    _wins, extra = gc.handmade()
    held = [any(km in nd["seq"] or km in ref.revcomp(nd["seq"]) for nd in nodes) for km in extra["gate_kmers"]]
    return key, held


def test_gate_case_decides_the_graph(monkeypatch):
    """The three bubbles of the `gate` window stand or fall with one verdict of the gate each (graph_build_cases.
    decisive_bubble), so a gate that sums afresh, that lets exactly 1.0 through, or whose threshold is off by 0.002 makes
    another graph -- which tests/test_gpu_graph_build.py then reports.  Each rule is changed alone, on the restatement."""
    truth, held = gate_window_key()
    # echo (exactly 1.0 as a prefix difference): refused, no bubble | 0.9985 .. 0.9999: counted, bubble | 1.0001 .. 1.0015: refused
    assert held == [False, True, False]
    k = gc.K

    def fresh_sum(self, prefix, quals, o):
        acc = 0.0
        for q in quals[o:o + k]:
            acc += gb.PHRED_ERR[q]
        return acc

    for what, attr, rule, want_held in (
            ("a fresh sum per k-mer", "kmer_error", fresh_sum, [True, True, False]),
            ("> 1.0 in place of floor() > 0", "refused", staticmethod(lambda raw: raw > 1.0), [True, True, False]),
            ("threshold 1.002", "refused", staticmethod(lambda raw: raw >= 1.002), [True, True, True]),
            ("threshold 0.998", "refused", staticmethod(lambda raw: raw >= 0.998), [False, False, False])):
        with monkeypatch.context() as m:
            m.setattr(gb._Graph, attr, rule)
            key, held = gate_window_key()
        assert key != truth and held == want_held, what
    assert gate_window_key()[0] == truth
    # the echo instance let through alone: one Q10 of the read's second pattern copy raised to Q11, the rules as they are
    c = gc.cases()["handmade"]
    _ref, reads = gb.window_inputs(c.arrs, gc.HANDMADE.index("gate"))
    echo = bytes(gc.echo_pattern())
    at = [i for i, r in enumerate(reads) if r[1] == echo]
    assert len(at) == 1
    q = bytearray(echo)
    q[125 + echo[125:].index(10)] = 11  # 0.1 -> 0.079
    reads[at[0]] = reads[at[0]][:1] + (bytes(q),) + reads[at[0]][2:]
    key, held = gate_window_key(reads)
    assert key != truth and held == [True, True, False]


def test_label_case_has_the_three_labels():
    nodes = hm_nodes("labels")
    _wins, extra = gc.handmade()
    case_only, ctrl_first = (alt[gc.K // 2:gc.K // 2 + gc.K] for alt in extra["label_alts"])  # the k-mer with the new base in its middle
    holds = lambda nd, s: s in nd["seq"] or s in ref.revcomp(nd["seq"])  # noqa: E731
    assert hm_counters("labels")["ref_first_supported"] > 0
    assert any(nd["label"] == gb.L_REFERENCE and sum(nd["counts"]) > 0 for nd in nodes)
    a = [nd for nd in nodes if holds(nd, case_only)]
    assert len(a) == 1 and a[0]["label"] == gb.L_CASE and a[0]["counts"][:2] == [0, 0] and a[0]["counts"][2] > 1
    b = [nd for nd in nodes if holds(nd, ctrl_first)]
    assert len(b) == 1 and b[0]["label"] == gb.L_CTRL and b[0]["counts"][2] > 0 and b[0]["counts"][0] > 0


def test_singleton_case_removes_covered_nodes():
    # 2k - 1 k-mers over the two planted bases, two or three reads each
    assert hm_counters("singletons")["singletons_with_cov"] >= unedited_counters("singletons")["singletons_with_cov"] + 2 * gc.K - 1


def test_tip_case_reaches_both_sides_of_k_and_keeps_the_self_loop():
    c = hm_counters("tips")
    rounds = c["tip_rounds"][0]
    assert c["tips_one_under_k"] > 0 and c["dead_ends_at_k"] > 0 and len(rounds) >= 2 and all(rounds), c
    assert sum(rounds) > sum(unedited_counters("tips")["tip_rounds"][0])
    nodes = hm_nodes("tips")
    _wins, extra = gc.handmade()
    kept, short = extra["tip_tails"]
    holds = lambda nd, s: s in nd["seq"] or s in ref.revcomp(nd["seq"])  # noqa: E731
    # k + 1 new bases: the last k-mer has one edge and cannot be absorbed (a buddy needs an onward edge), goes in the first round,
    # and leaves a dead end with exactly k bases of its own, which stays; with k new bases k - 1 are left, and go in the second
    tip = [nd for nd in nodes if holds(nd, kept[:gc.K])]
    assert len(tip) == 1 and len(tip[0]["seq"]) == 2 * gc.K - 1 and len(tip[0]["edges"]) == 1
    assert not any(holds(nd, short[:20]) for nd in nodes)
    loops = [nd for nd in nodes if any(d == nd["idx"] for d, _ in nd["edges"])]
    assert len(loops) == 1 and loops[0]["seq"] == b"A" * gc.K and len(loops[0]["edges"]) == 4


def test_n_and_filter_case():
    c, plain = hm_counters("nfilt"), unedited_counters("nfilt")
    assert c["non_acgt_nodes"] > 0 and plain["non_acgt_nodes"] == 0 and c["reads_filtered"] == plain["reads_filtered"] + 8
    assert any(b"N" in nd["seq"] for nd in hm_nodes("nfilt"))


def test_all_four_merge_kinds_everywhere():
    for name in CASE_NAMES:
        asm = oracle_rows(name)
        for w in compared_windows(name):
            assert min(gc.built(name, w, int(asm["win_k"][w])).counters["merges"]) > 0, (name, w)


def walked_slots(name, w):
    """(nodes, slots that some row of the window walks over -- the REF row too where a walk spells it)"""
    c, asm = gc.cases()[name], oracle_rows(name)
    p, k = c.params, int(asm["win_k"][w])
    nodes = ref.window_nodes(gc.expected_arrays(name, w, asm), 0, p.num_samples)
    walked = set()
    for comp, cn in ref.components(nodes).items():
        ci = w * p.max_comps + comp
        for h in range(int(asm["comp_nhaps"][ci])):
            hi = w * p.max_haps + int(asm["comp_hap0"][ci]) + h
            target = bytes(asm["hap_bases"][hi * p.max_hap_len:hi * p.max_hap_len + int(asm["hap_len"][hi])])
            for walk in ref.find_walks(cn, k, target):
                walked |= {nd.slot for nd, _ in walk}
    return nodes, walked


def test_some_compared_node_is_on_no_walk():
    w = gc.HANDMADE.index("tips")
    nodes, walked = walked_slots("handmade", w)
    off = [nd for s, nd in nodes.items() if s not in walked]
    assert walked and off and any(nd.total > 0 for nd in off)


# ---- the comparison of the GPU file can fail ---------------------------------------------------------------------------------------
def test_the_comparison_reports_a_count_a_label_bit_and_an_edge():
    name, w = "handmade", gc.HANDMADE.index("tips")
    c, asm = gc.cases()[name], oracle_rows(name)
    S = c.params.num_samples
    good = gc.expected_arrays(name, w, asm)
    want = ref.graph_key(good, 0, S)
    assert gb.first_difference(ref.graph_key(gc.expected_arrays(name, w, asm), 0, S), want) is None
    nodes, walked = walked_slots(name, w)
    off = next(s for s, nd in sorted(nodes.items()) if s not in walked and nd.total > 0)

    def changed(edit):
        gr = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        edit(gr)
        return gb.first_difference(ref.graph_key(gr, 0, S), want)

    def count_plus_one(gr):
        gr["node_cnt"][off * S + 1] += 1

    def label_bit(gr):
        gr["node_label"][off] ^= gb.L_CTRL

    def drop_edge(gr):
        ne = int(gr["win_nedges"][0])
        e = next(i for i in range(ne) if int(gr["edge_src"][i]) == off)
        for key in ("edge_src", "edge_dst", "edge_kind"):
            gr[key][e:ne - 1] = gr[key][e + 1:ne].copy()
        gr["win_nedges"][0] = ne - 1

    for edit, word in ((count_plus_one, "node"), (label_bit, "node"), (drop_edge, "edge")):
        said = changed(edit)
        assert said is not None and word in said, (edit.__name__, said)
