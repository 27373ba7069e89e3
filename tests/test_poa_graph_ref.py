"""tests/poa_graph_ref.py against the oracle's POA graph, step by step, and against hand-written MSA rows.

The restatement takes only the alignment pairs from the oracle; letters, in-edge lists and rank order of the graph it builds
from them must be the oracle's after every haplotype.  The four properties the export kernel leans on (poa.hip:
poa_export_component) are checked on every input."""
from functools import lru_cache

import pytest

import poa_cases
import poa_export_cases
import poa_graph_ref as ref
from harness import oracle

LINEAR = (3, -5, -3, -3, -3, -3)  # the engine of tests/caller/variant_set_test.cpp (tests/test_oracle_kat.py: poa_variants)


def in_lists(g):
    return [list(t) for t in g.inn]


def check_steps(seqs, sc=ref.SCORING):
    lib = oracle()

    def same(h, g, dump):
        base, preds, order, _ = dump
        assert g.base == base, h
        assert in_lists(g) == [list(p) for p in preds], h
        assert g.order == order, h

    g = ref.build(seqs, lib, on_step=same, sc=sc)
    same(len(seqs), g, ref.oracle_dump(list(seqs) + [b"A"], lib, sc))  # once more: the graph of ALL haplotypes
    return g


def check_properties(seqs, g):
    d = ref.describe(g)
    assert len(d["rows"]) == len(seqs)
    for h, row in enumerate(d["rows"]):
        assert len(row) == d["ncols"] and row.replace(b"-", b"") == bytes(seqs[h]), h
    # a haplotype's path is its member nodes sorted by rank
    for h, pth in enumerate(d["paths"]):
        members = [v for v in range(len(d["base"])) if d["haps"][v] >> h & 1]
        assert pth == sorted(members, key=lambda v: d["rank"][v]), h
        cols = [d["col"][v] for v in pth]
        assert all(a < b for a, b in zip(cols, cols[1:])), h  # strictly increasing along a path
    # out-edges in ascending order of their lowest label bit, no two share one
    for v, es in enumerate(g.out):
        low = [(m & -m).bit_length() for _, m in es]
        assert low == sorted(low) and len(set(low)) == len(low), v
        seen = 0
        for _, m in es:
            assert m and not (seen & m), v
            seen |= m
    # columns along rank: non-decreasing in steps of 0 or 1, from 0
    cols = [d["col"][v] for v in d["order"]]
    assert cols[0] == 0 and all(b - a in (0, 1) for a, b in zip(cols, cols[1:])) and cols[-1] + 1 == d["ncols"]
    return d


SEEDED = poa_export_cases.seeded_components()


@pytest.mark.parametrize("i", range(len(SEEDED)))
def test_seeded_component_matches_the_oracle_after_every_haplotype(i):
    seqs = SEEDED[i]
    assert 2 <= len(seqs) <= 9 and 30 <= len(seqs[0]) <= 400
    check_properties(seqs, check_steps(seqs))


@lru_cache(maxsize=None)
def case_windows():
    out = []
    for gname, g in poa_cases.groups().items():
        for w in g.windows:
            if not w.may_flag and w.max_len() <= 1100:
                out.append((f"{gname}:{w.name}", w))
    return out


def test_the_capacity_cases_hold_windows_of_every_group_up_to_1100_bases():
    names = [n for n, _ in case_windows()]
    assert len(names) >= 40 and {n.split(":")[0] for n in names} >= {"run", "degree", "ring", "headroom_1k", "multi"}


@pytest.mark.parametrize("k", range(len(case_windows())))
def test_capacity_case_window_matches_the_oracle_after_every_haplotype(k):
    _, w = case_windows()[k]
    for c in w.comps:
        seqs = c.haps()
        check_properties(seqs, check_steps(seqs))


# The seven known-answer inputs of the reference (tests/caller/variant_set_test.cpp:35-247), linear engine +3 / -5 / -3.
# Expected rows, by hand:
#  1 one substitution costs -5, two gaps -6: T and G share a column.
#  2 A and G match, T and C are skipped.
#  3 AGC: A, G, C match and three nodes are skipped -- the G in front (skip one, match, skip two) or the G behind (skip three,
#    match) score the same 0; the backtrack stands on the LAST G first and tries the diagonal first, so it is the G behind.
#  4 AA goes in between T and C: the only placement that keeps four matches.
#  5 two substitutions (-10) beat two skipped nodes and two inserted bases (-12).
#  6 three of AAAA meet T, C and a gap; from the end the backtrack takes diagonals while they explain the score -- G/G, A/C,
#    A/T, A/A -- so the base left over is the FIRST A, inserted in front of the graph's first node.
#  7 G and A join T's column one after the other; ACG skips that column.
KATS = [
    ([b"ATCG", b"AGCG"], [b"ATCG", b"AGCG"]),
    ([b"ATCG", b"AG"], [b"ATCG", b"A--G"]),
    ([b"ATGTGC", b"ACGTGC", b"AGC", b"ATGTAC"], [b"ATGTGC", b"ACGTGC", b"A---GC", b"ATGTAC"]),
    ([b"ATCG", b"ATAACG"], [b"AT--CG", b"ATAACG"]),
    ([b"ATCG", b"AAAG"], [b"ATCG", b"AAAG"]),
    ([b"ATCG", b"AAAAG"], [b"-ATCG", b"AAAAG"]),
    ([b"ATCG", b"AGCG", b"AACG", b"ACG"], [b"ATCG", b"AGCG", b"AACG", b"A-CG"]),
    ([b"ACGT", b"AGT"], [b"ACGT", b"A-GT"]),  # (not one of the seven: the example of the export's description)
]


@pytest.mark.parametrize("k", range(len(KATS)))
def test_known_answer_msa_rows(k):
    seqs, rows = KATS[k]
    g = check_steps(seqs, LINEAR)
    d = check_properties(seqs, g)
    assert d["rows"] == rows
    assert ref.fasta_text(d) == "".join(f">{'ref' if h == 0 else 'hap'}{h}\n{r.decode()}\n" for h, r in enumerate(rows))


def test_gfa_and_fasta_texts_of_a_substitution():
    d = ref.describe(check_steps([b"ATCG", b"AGCG"], LINEAR))
    assert ref.gfa_text(d) == ("H\tVN:Z:1.0\n"
                               "S\t1\tA\nL\t1\t+\t2\t+\t0M\nL\t1\t+\t5\t+\t0M\n"
                               "S\t2\tT\nL\t2\t+\t3\t+\t0M\n"
                               "S\t3\tC\nL\t3\t+\t4\t+\t0M\n"
                               "S\t4\tG\n"
                               "S\t5\tG\nL\t5\t+\t3\t+\t0M\n"
                               "P\tref0\t1+,2+,3+,4+\t*\n"
                               "P\thap1\t1+,5+,3+,4+\t*\n")
    assert ref.fasta_text(d) == ">ref0\nATCG\n>hap1\nAGCG\n"
    assert d["rings"][1] == [4] and d["rings"][4] == [1] and d["order"] == [0, 1, 4, 2, 3] and d["seq_first"] == [0, 0]
    assert d["edges"] == [(0, 1, 1), (0, 4, 2), (1, 2, 1), (2, 3, 3), (4, 2, 2)]
