"""tests/probe_ref.py and tests/probe_cases.py without a GPU: the restatement is pinned on a k = 5 toy worked out by hand, every
case of probe_cases is shown to reach its edge on the oracle's assembly, and the comparison the GPU file relies on is shown to
report a count changed by one and a flipped mask bit."""
import copy

import pytest

import graph_build_cases as gc
import probe_cases as pc
import probe_ref as pr
from lancet2_amd import capi

@pytest.fixture(autouse=True, scope="module")
def the_call_the_restatement_is_for():
    """everything in this file pins what ma_assemble_probe_batch must return: without the call there is nothing to pin"""
    assert hasattr(capi.load_cdll(), "ma_assemble_probe_batch") and capi.Probes and capi.ProbeOut


TOY = b"AACCGGTTACGTAGCATCGA"  # G at 10; no 5-mer of it equals another or another's reverse complement around position 10


def test_toy_snv_insertion_deletion():
    # SNV 10 G>C: contexts ref[6:15] = TTACGTAGC and TTACCTAGC; all five ALT k-mers hold the new base and none is a REF one
    assert pr.contexts(TOY, 10, 1, b"C", 5) == (b"TTACGTAGC", b"TTACCTAGC")
    assert pr.alt_unique(TOY, 10, 1, b"C", 5) == [pr.canon(m) for m in (b"TTACC", b"TACCT", b"ACCTA", b"CCTAG", b"CTAGC")]
    # deletion 9 CGT>C: ALT context GTTA + C + AGCA; GTTAC is a REF k-mer, the four junction k-mers are not
    assert pr.contexts(TOY, 9, 3, b"C", 5) == (b"GTTACGTAGCA", b"GTTACAGCA")
    assert pr.alt_unique(TOY, 9, 3, b"C", 5) == [pr.canon(m) for m in (b"TTACA", b"TACAG", b"ACAGC", b"CAGCA")]
    # insertion 9 C>CTT: ALT context GTTA + CTT + GTAG, 7 k-mers of which the first is the REF's
    assert pr.contexts(TOY, 9, 1, b"CTT", 5) == (b"GTTACGTAG", b"GTTACTTGTAG")
    assert len(pr.alt_unique(TOY, 9, 1, b"CTT", 5)) == 6


def test_toy_context_clipped_at_both_ends():
    # a window of six bases: a = 0 and e = 6 both clip; ACTTA and CTTAC against ACGTA and CGTAC
    assert pr.contexts(b"ACGTAC", 2, 1, b"T", 5) == (b"ACGTAC", b"ACTTAC")
    assert len(pr.alt_unique(b"ACGTAC", 2, 1, b"T", 5)) == 2


def test_toy_reverse_complement_of_a_ref_kmer_is_not_alt_unique():
    # ACCGACGGT, 4 A>T -> ACCGTCGGT: ALT k-mer j is the reverse complement of REF k-mer 4 - j (ACCGT = rc(ACGGT), ...): none
    # is ALT-unique, where a forward-only comparison finds five
    ref = b"ACCGACGGT"
    alt_kmers, ref_kmers = pr.kmers(b"ACCGTCGGT", 5), pr.kmers(ref, 5)
    assert not set(alt_kmers) & set(ref_kmers)
    assert [pr.canon(m) for m in alt_kmers] == [pr.canon(m) for m in reversed(ref_kmers)]
    assert pr.alt_unique(ref, 4, 1, b"T", 5) == []


def test_toy_kmer_at_two_offsets_counts_at_both():
    # CGCGAAAAGCGC, 7 A>AAA: ALT context GAAAAAAGCGC; AAAAA at context offsets 1 and 2 is ALT-unique twice: offsets j = 0, 1
    ref = b"CGCGAAAAGCGC"
    assert pr.contexts(ref, 7, 1, b"AAA", 5)[1] == b"GAAAAAAGCGC"
    uniq = pr.alt_unique(ref, 7, 1, b"AAA", 5)
    assert uniq == [b"AAAAA", b"AAAAA"]
    # TTTTTT holds rc(AAAAA) at two positions: 2 positions x 2 offsets; one read holds one
    assert pr.in_reads(uniq, [b"TTTTTT", b"CGCGAAAAGC"], 5) == [4, 1]
    assert pr.profile(uniq, {b"AAAAA"}) == [2, 2, 0, 0]


def test_toy_n_equals_nothing():
    assert pr.alt_unique(TOY, 10, 1, b"N", 5) == []               # every ALT k-mer holds the N
    ref = TOY[:9] + b"N" + TOY[10:]
    assert pr.alt_unique(ref, 10, 1, b"C", 5) == [pr.canon(b"CTAGC")]  # TTANC .. NCTAG hold it, CTAGC does not
    uniq = pr.alt_unique(TOY, 10, 1, b"C", 5)
    # TTACCTAGC holds all five, TAGGT = rc(ACCTA) one; an N inside TTACNCTAGC leaves CTAGC only; the REF read none
    assert pr.in_reads(uniq, [b"TTACCTAGC", b"TAGGT", b"TTACGTAGC", b"TTACNCTAGC"], 5) == [7, 3]


def test_toy_profile_and_rows():
    uniq = pr.alt_unique(TOY, 9, 1, b"CTT", 5)
    assert pr.profile(uniq, {uniq[0], uniq[1], uniq[3], uniq[5]}) == [4, 2, 2, 2]   # survivors 0 1 . 3 . 5
    assert pr.profile(uniq, set()) == [0, 0, 0, 0]
    assert pr.profile(uniq[:1], {uniq[0]}) == [1, 1, 0, 0]                            # one k-mer: offset 0 IS n_alt - 1
    alt_hap = TOY[:10] + b"C" + TOY[11:]
    rows = pr.window_rows(TOY, [(alt_hap, b"", 0, 0, 1)], 5, [(10, 1, b"C"), (10, 1, b"T")], 2, pr.canon_set([alt_hap], 5),
                          [[TOY[2:15], alt_hap[5:]]], [[TOY, alt_hap], [alt_hap[::-1]]])
    assert rows[0] == dict(pb_k=5, pb_alt_kmers=5, pb_in_reads=[5, 1], pb_lowcov1=[5, 2, 3, 0], pb_final=[5, 2, 3, 0, 0, 0, 0, 0],
                           pb_hap_mask=[2, 0])
    assert rows[1]["pb_in_reads"] == [0, 0] and rows[1]["pb_hap_mask"] == [0, 0] and rows[1]["pb_final"] == [0] * 8
    assert pr.window_rows(TOY, [], 0, [(10, 1, b"C")], 2, set(), [], [])[0]["pb_k"] == 0


def test_structs_sit_where_the_header_puts_them(tmp_path):
    """ma_probes_t / ma_probe_out_t as gcc lays them out from include/microasm.h against the ctypes mirrors, field by field;
    the library exports the call"""
    import ctypes as C
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    structs = {"ma_probes_t": capi.Probes, "ma_probe_out_t": capi.ProbeOut}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "microasm.h"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ['  return 0;', '}']))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(capi.REPO, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"{cname}.{f}"
    assert set(capi.probe_out_spec(capi.default_params(), 3)) == {f for f, _ in capi.ProbeOut._fields_}
    assert hasattr(capi.load_cdll(), "ma_assemble_probe_batch")


@pytest.fixture(scope="module")
def handmade_rows():
    asm, _ = pc.oracle_run("handmade")
    return pc.expected_rows("handmade", asm)


def _row(rows, name, w, tag):
    hits = [r for r, p in zip(rows[w], pc.probes(name)[w]) if p[3] == tag]
    assert len(hits) == 1, (name, w, tag)
    return hits[0]


def test_handmade_reaches_its_edges(handmade_rows):
    """the figures measured on `handmade` at k = 25 with the oracle and graph_build_ref"""
    lists = pc.probes("handmade")
    ws, wt = pc.W_SINGLETONS, pc.W_TIPS
    assert (ws, wt) == (5, 6)
    s0 = _row(handmade_rows, "handmade", ws, "singleton0")
    assert next(p for p in lists[ws] if p[3] == "singleton0")[0] == 130
    assert (s0["pb_alt_kmers"], s0["pb_in_reads"][0], s0["pb_lowcov1"]) == (25, 75, [0, 0, 0, 0])
    short, kept = _row(handmade_rows, "handmade", wt, "tip_short"), _row(handmade_rows, "handmade", wt, "tip_kept")
    assert [p[0] for p in lists[wt] if p[3].startswith("tip_")] == [135, 330]
    assert (short["pb_alt_kmers"], short["pb_in_reads"][0], short["pb_lowcov1"], short["pb_final"][:4]) == (49, 75, [25, 1, 24, 0], [0, 0, 0, 0])
    assert (kept["pb_alt_kmers"], kept["pb_lowcov1"], kept["pb_final"][:4]) == (50, [26, 1, 25, 0], [26, 1, 25, 0])
    assert kept["pb_hap_mask"] == [0] * gc.cases()["handmade"].params.max_comps
    ins = [r for r, p in zip(handmade_rows[ws], lists[ws]) if p[:3] == (425, 1, b"GC")]
    assert len(ins) == 1 and ins[0]["pb_alt_kmers"] == 24   # of the 26 k-mers of its ALT context
    # the clipped decoys: 1, 2, 25 and 1 ALT-unique k-mers, none of them anywhere
    for w in range(len(lists)):
        decoys = [r for r, p in zip(handmade_rows[w], lists[w]) if p[3] == "decoy"]
        assert [r["pb_alt_kmers"] for r in decoys] == [1, 2, 25, 1], w
        for r, p in zip(handmade_rows[w], lists[w]):
            if p[3] == "absent":
                assert r["pb_in_reads"] == [0, 0] and r["pb_lowcov1"] == [0] * 4 and not any(r["pb_final"]) and not any(r["pb_hap_mask"]), (w, p)
    masks = [(p, any(r["pb_hap_mask"])) for w in range(len(lists)) for r, p in zip(handmade_rows[w], lists[w]) if p[3] == "oracle"]
    assert len(masks) == 17 and sum(m for _, m in masks) == 16
    assert [p[2] for p, m in masks if not m] == [b"N"]


@pytest.mark.parametrize("name", pc.NAMES)
def test_every_case_finds_its_variants_in_the_haplotypes(name):
    asm, _ = pc.oracle_run(name)
    rows, lists = pc.expected_rows(name, asm), pc.probes(name)
    c = pc.case(name)
    hits = [any(r["pb_hap_mask"]) for w in range(c.n) for r, p in zip(rows[w], lists[w]) if p[3] == "oracle"]
    print(name, "oracle-variant probes:", len(hits), "with a haplotype:", sum(hits), "k:", sorted({int(k) for k in asm["win_k"]}))
    assert hits and 2 * sum(hits) >= len(hits)
    for w in range(c.n):  # a probe a haplotype spells has every ALT-unique k-mer in that component's graph
        for r, p in zip(rows[w], lists[w]):
            if r["pb_final"] is not None:
                for ci, m in enumerate(r["pb_hap_mask"]):
                    if m:
                        assert r["pb_final"][4 * ci] == r["pb_alt_kmers"], (name, w, p)
    if name == "c3_ladder":
        assert max(int(k) for k in asm["win_k"]) > 32
    if name == "gap":
        g = _row(rows, name, 0, "gap")
        print("gap probe:", g)
        assert g["pb_alt_kmers"] == 45 and g["pb_lowcov1"] == [20, 2, 18, 1] and g["pb_final"][:4] == [20, 2, 18, 1]
        assert g["pb_lowcov1"][3] == 1 and not any(g["pb_hap_mask"])


def test_the_comparison_reports_a_changed_count_and_a_flipped_bit(handmade_rows):
    got = copy.deepcopy(handmade_rows)
    assert pc.compare_case("handmade", got, handmade_rows) == []
    got[pc.W_TIPS][0]["pb_in_reads"][0] += 1
    bad = pc.compare_case("handmade", got, handmade_rows)
    assert len(bad) == 1 and "w6 probe 0 pb_in_reads" in bad[0]
    got = copy.deepcopy(handmade_rows)
    got[2][1]["pb_hap_mask"][0] ^= 2
    got[3][0]["pb_final"][3] += 1
    bad = pc.compare_case("handmade", got, handmade_rows)
    assert len(bad) == 2 and "w2 probe 1 pb_hap_mask" in bad[0] and "w3 probe 0 pb_final" in bad[1]
    # the flat arrays of ma_probe_out_t and back
    flat = pr.rows_to_arrays(handmade_rows[0], 4)
    assert [pr.engine_row(flat, i, 4) for i in range(len(handmade_rows[0]))] == \
           [{k: (v if v is not None else [0] * 16) for k, v in r.items()} for r in handmade_rows[0]]
    assert capi.pack_probes([[(3, 1, b"AC")], [], [(0, 2, b"G")]])["probe_win_off"].tolist() == [0, 1, 1, 2]
