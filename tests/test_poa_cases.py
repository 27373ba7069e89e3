"""CPU guard of tests/test_gpu_poa_cases.py: the oracle alone over tests/poa_cases.py.  The GPU test compares engine and
oracle; a case whose planted variants the oracle does not call, or whose graph does not have the degrees the table claims,
would pass for nothing.  So what every case is FOR is checked here without a GPU: the oracle's status is 0 everywhere (its POA
has none of the engine's widths), the biallelic cases give the truth that the construction fixes, the degree and ring cases
give one site with n alleles, and shape() -- from the edit lists, neither implementation -- gives the claimed degrees."""
import numpy as np
import pytest

import poa_cases as pc
from harness import variants_of

GROUPS = tuple(pc.groups())
EXPECTED_MAY_FLAG = {
    "out_degree_5", "out_degree_6", "in_degree_5", "in_degree_6", "ring_6",                  # over: a kPE width
    "ins_8x60", "over_between_two_fitting",                                                  # over: node capacity / in a window of three
    "ins_4x60", "ins_8x60_beside_2400", "snv_80_on_2400",                                    # fit depends on pn
    "length_3072", "length_3073", "length_4096", "length_2551", "length_2552",               # long
    "narrow_2400_then_17_haplotypes",                                                        # long for the kernels it takes
}


def _hap_alleles(p, var, w, v):
    row = np.asarray(var["var_hap_allele"]).reshape(-1, p.max_vars, p.max_haps)[w, v]
    return {int(h): int(a) for h, a in enumerate(row) if a}


def test_only_the_listed_cases_may_be_flagged():
    names = [w.name for g in pc.groups().values() for w in g.windows]
    assert len(names) == len(set(names))
    assert {w.name for g in pc.groups().values() for w in g.windows if w.may_flag} == EXPECTED_MAY_FLAG
    for g in pc.groups().values():
        for w in g.windows:
            assert (w.kind in ("over", "headroom", "long")) == w.may_flag and w.kind in ("", "over", "headroom", "long", "long_lab32"), w.name
            assert (w.kind == "long") == (w.max_len() >= (pc.LEN_EDGE_LAB32 + 1 if w.wide() else pc.LEN_EDGE)) and (w.kind == "long" or w.max_len() <= pc.COMMON_LEN_CEILING), w.name
            assert pc.may_flag_on("default", w)[0] == w.may_flag
            if not w.may_flag:  # on the forced LAB32 route the windows from that route's edge on are long cases, nothing else changes
                assert pc.may_flag_on("lab32", w)[0] == (w.max_len() >= pc.LEN_EDGE_LAB32), w.name


@pytest.mark.parametrize("group", GROUPS)
def test_the_oracle_calls_what_the_case_plants(group):
    g = pc.groups()[group]
    p = g.params
    var, status = pc.oracle_msa(group)
    assert not status.any(), status.tolist()
    print(f"\n{'case':28s} {'len':>5s} {'haps':>4s} out in ring new  vars  may_flag")
    for wi, w in enumerate(g.windows):
        c0 = w.comps[0]
        out_d, in_d, ring = pc.shape(c0.ref, c0.alts)
        got = variants_of(p, var, wi)
        print(f"{w.name:28s} {w.max_len():5d} {sum(len(c.haps()) for c in w.comps):4d} {out_d:3d} {in_d:2d} {ring:4d} "
              f"{pc.new_nodes(c0.alts):3d} {len(got):5d}  {w.kind or '-'}")
        for c in w.comps:
            assert all(pc.unique_place(c.ref, e) for edits in c.alts for e in edits), w.name
            assert len(set(c.haps())) == len(c.haps()), w.name
        if w.claims is not None:
            assert (out_d, in_d, ring) == w.claims, (w.name, out_d, in_d, ring)
            assert len(got) == 1 and len(got[0][2]) == w.n_alleles, (w.name, got)
            alleles = _hap_alleles(p, var, wi, 0)
            assert sorted(alleles) == list(range(1, w.n_alleles + 1)) and sorted(alleles.values()) == list(range(1, w.n_alleles + 1)), (w.name, alleles)
        if w.truth is not None:
            assert len(w.comps) == 1
            assert got == [t[:3] for t in w.truth], (w.name, got, w.truth)
            for v, t in enumerate(w.truth):
                assert _hap_alleles(p, var, wi, v) == t[3], (w.name, v)  # (the REF haplotype and the others carry none)


def test_degrees_are_what_the_table_says():
    """3, 4, 5 and 6 edges out of / into one node, rings of 4, 5 and 6 -- kPE = 4 edges, a node and 4 aligned ones"""
    by = {w.name: pc.shape(w.comps[0].ref, w.comps[0].alts) for n in ("degree", "ring") for w in pc.groups()[n].windows}
    for k in (3, 4, 5, 6):
        assert by[f"out_degree_{k}"] == (k, 2, 1) and by[f"in_degree_{k}"] == (2, k, 1)
    for k in (4, 5, 6):
        assert by[f"ring_{k}"] == (4, 4, k)
    assert pc.shape(b"ACGTACGT", [[("snv", 3, ord("A"))], [("del", 2, 3)], [("ins", 4, b"GG")]]) == (2, 3, 2)
    assert pc.shape(b"ACGTACGT", [[("del", 2, 3)], [("del", 2, 1)], [("snv", 2, ord("T"))]]) == (4, 3, 2)


def test_run_boundary_distances_and_length_classes_are_the_listed_ones():
    run = pc.groups()["run"]
    for d in (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300):
        w = run.windows[run.by_name[f"snv_pair_d{d}"]]
        (e1, e2), = w.comps[0].alts
        assert e2[1] - e1[1] == d and 600 <= len(w.comps[0].ref) <= 1000
    mnp = run.windows[run.by_name["snv_pair_d1"]].truth
    assert len(mnp) == 1 and len(mnp[0][1]) == 2 and len(mnp[0][2][0]) == 2
    length = pc.groups()["length"]
    assert sorted(len(w.comps[0].ref) for w in length.windows) == [1024, 1025, 1536, 1537, 2048, 2049, 2400, 3072, 3073, 4096]
    assert length.params.max_hap_len == 4096
    wl = pc.groups()["wide_long"]
    w = wl.windows[wl.by_name["narrow_2400_then_17_haplotypes"]]
    assert [len(c.haps()) for c in w.comps] == [3, 17] and w.max_len() == len(w.comps[0].ref) == 2400
    assert pc.LEN_EDGE_LAB32 < 2400 < pc.LEN_EDGE and max(x.max_len() for x in wl.windows if x is not w) < 1000
    head = pc.groups()["headroom_1k"]
    assert [pc.new_nodes(head.windows[head.by_name[n]].comps[0].alts) for n in ("ins_2x60", "ins_4x60", "ins_8x60")] == [120, 240, 480]
    assert max(w.max_len() for w in head.windows) == 1060
