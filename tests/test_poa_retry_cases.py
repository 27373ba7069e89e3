"""CPU guard of tests/test_gpu_poa_retry.py: the oracle alone over tests/poa_retry_cases.py, in the manner of
tests/test_poa_cases.py.  The oracle calls every window with status 0 (a case it flags itself -- an output cap -- would be a
broken case), shape() gives the degrees and rings the table claims from the edit lists, the special sites carry the allele
counts the table says, and the node counts lie on the side of the retry's capacities the table says.  The header declares
the two functions of the setting."""
import os
import re

import numpy as np
import pytest

import poa_cases as pc
import poa_retry_cases as rc
from harness import variants_of

GROUPS = tuple(rc.groups())
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "microasm.h")


def _hap_alleles(p, var, w, v):
    row = np.asarray(var["var_hap_allele"]).reshape(-1, p.max_vars, p.max_haps)[w, v]
    return {int(h): int(a) for h, a in enumerate(row) if a}


def test_the_table_is_what_the_docstring_says():
    names = [w.name for g in rc.groups().values() for w in g.windows]
    assert len(names) == len(set(names))
    by_kind = {k: {w.name for g in rc.groups().values() for w in g.windows if w.kind == k} for k in ("fit", "over")}
    assert by_kind["fit"] == {"out_degree_8", "in_degree_8", "ring_9", "ins_12x60", "width_then_nodes", "capped_between_two_fitting"}
    assert by_kind["over"] == {"out_degree_9", "in_degree_9", "ring_10", "ins_15x120"}
    for g in rc.groups().values():
        assert set(rc.MARKS) == set(rc.groups())
        for i, w in enumerate(g.windows):
            assert w.may_flag == (w.kind == "over") and w.kind in ("", "fit", "over"), w.name
            if w.kind:  # between ordinary windows
                assert 0 < i < len(g.windows) - 1 and not g.windows[i - 1].kind and not g.windows[i + 1].kind, w.name
        special = [w for w in g.windows if w.kind]
        assert rc.MARKS[g.name][0] + rc.MARKS[g.name][1] == len(special)
        assert rc.MARKS[g.name][2] == sum(w.kind == "over" for w in special)
        assert 3 <= len(g.windows) <= 11


@pytest.mark.parametrize("group", GROUPS)
def test_the_oracle_calls_every_window(group):
    g = rc.groups()[group]
    p = g.params
    var, status = rc.oracle_msa(group)
    assert not status.any(), status.tolist()
    for wi, w in enumerate(g.windows):
        got = variants_of(p, var, wi)
        assert len(got) >= 1, w.name
        for c in w.comps:
            assert all(pc.unique_place(c.ref, e) for edits in c.alts for e in edits), w.name
            assert len(set(c.haps())) == len(c.haps()) <= p.max_haps, w.name
            assert max(len(h) for h in c.haps()) <= p.max_hap_len
        if w.claims is not None:
            c0 = w.comps[0]
            assert pc.shape(c0.ref, c0.alts) == w.claims, (w.name, pc.shape(c0.ref, c0.alts))
            assert len(got) == 1 and len(got[0][2]) == w.n_alleles <= p.max_alts, (w.name, got)
            alleles = _hap_alleles(p, var, wi, 0)
            assert sorted(alleles) == list(range(1, w.n_alleles + 1)) and sorted(alleles.values()) == list(range(1, w.n_alleles + 1)), (w.name, alleles)
        if w.truth is not None:
            assert got == [t[:3] for t in w.truth], (w.name, got, w.truth)


def test_degrees_and_rings_at_eight_slots():
    """eight and nine edges out of / into one node; rings of nine and ten -- eight slots: eight edges, a node and eight aligned"""
    by = {w.name: w for n in ("degree8", "ring9") for w in rc.groups()[n].windows}
    shape = {k: pc.shape(w.comps[0].ref, w.comps[0].alts) for k, w in by.items()}
    for k in (8, 9):
        assert shape[f"out_degree_{k}"] == (k, 2, 1) and shape[f"in_degree_{k}"] == (2, k, 1)
        assert by[f"out_degree_{k}"].n_alleles == by[f"in_degree_{k}"].n_alleles == k - 1
    assert rc.groups()["degree8"].params.max_alts == 8  # (nine edges: eight ALT alleles, the cap exactly -- not an output overflow)
    assert shape["ring_9"] == (6, 6, 9) and shape["ring_10"] == (7, 7, 10)
    assert by["ring_9"].n_alleles == 8 and by["ring_10"].n_alleles == 9 <= rc.groups()["ring9"].params.max_alts == 12
    # every letter of the two ring sites occurs once, and no flank letter anywhere else in its haplotypes
    for name in ("ring_9", "ring_10"):
        c = by[name].comps[0]
        site = [h[300] for h in c.haps()]
        assert len(set(site)) == len(site) == int(name.split("_")[1])


def test_node_counts_against_the_capacities():
    """the capacity pass has 2680 nodes for 1060-base haplotypes (the first pass: 1323), the width pass 1704"""
    assert rc.node_capacity(1060, 4) == 2680 and rc.node_capacity(1060, 8) == 1704
    nodes = rc.groups()["nodes"]
    w12, w15 = (nodes.windows[nodes.by_name[n]] for n in ("ins_12x60", "ins_15x120"))
    assert pc.new_nodes(w12.comps[0].alts) == 720 and w12.max_len() == 1060
    assert 1060 + 263 < 1000 + 720 <= rc.node_capacity(1060, 4)
    assert pc.new_nodes(w15.comps[0].alts) == 1800 and w15.max_len() == 1120 and len(w15.comps[0].haps()) == 16
    assert 1000 + 1800 > rc.node_capacity(1120, 4)  # (the pass is sized from ITS longest haplotype: 1120 bases)
    both = rc.groups()["both"]
    w = both.windows[both.by_name["width_then_nodes"]]
    assert pc.shape(w.comps[0].ref, w.comps[0].alts)[0] == 6 and pc.new_nodes(w.comps[1].alts) == 480
    assert 1060 + 263 < 1000 + 480 <= rc.node_capacity(w.max_len(), 8)  # over for the first pass, held by the width pass
    w3 = both.windows[both.by_name["capped_between_two_fitting"]]
    assert [max(pc.shape(c.ref, c.alts)) for c in w3.comps] == [3, 6, 5]


def test_the_header_declares_the_setting():
    text = open(HEADER).read()
    assert re.search(r"\bint ma_set_poa_retry\(ma_ctx_t\* ctx, int on\);", text)
    assert re.search(r"\bint ma_last_poa_retry\(ma_ctx_t\* ctx, unsigned long long\* out, int cap\);", text)
    assert re.search(r"^#define MA_VERSION 3\b", text, re.M)
