"""CPU guard of tests/test_gpu_caps.py: the oracle alone over tests/cap_cases.py.  The GPU test compares engine and oracle under
every tight parameter set; a table without a window at a cap's edge, or an oracle whose results moved with the strides, would
let it pass for nothing.  So the yardstick is pinned here without a GPU: the table holds an exact fit, a window one over and a
window below for every cap; under every tight set the oracle flags exactly the windows whose need exceeds the cap, with the
cap's own bit and no other capacity bit; its results for the windows that fit do not depend on the strides; and the tiled
windows have their dropped walk where the table says (orc_walk_dispositions)."""
import numpy as np
import pytest

import cap_cases as cc
from harness import haplotypes_of, variants_of

TIGHT = cc.tight_sets()


@pytest.mark.parametrize("cap", tuple(cc.CAPS))
def test_table_holds_an_exact_fit_one_over_and_one_below(cap):
    key, _, bname, (lo, hi) = cc.CAPS[cap]
    nd = cc.needs(bname)[key]
    vals = cc.tight_values(cap)
    print(f"\n{cap}: needs {nd.tolist()} tight values {vals}")
    assert 1 <= len(vals) <= cc.MAX_TIGHT_SETS and all(lo <= c <= hi for c in vals)
    assert len(cc.batch(bname).names) == len(nd) <= 12
    full = [c for c in vals if (nd == c).any() and (nd == c + 1).any() and (nd < c).any()]
    if cap == "max_runs":  # (cap_cases: run counts come in steps, exact fit and one over are two contexts)
        assert not full
        c1 = cc.ONE_UNDER[cap]
        assert c1 in vals and c1 + 1 in vals and (nd == c1 + 1).any() and (nd < c1).any() and not (nd == c1).any()
    else:
        assert full, (cap, vals, nd.tolist())
    if cap == "max_comps":
        assert 1 in vals  # the run at max_comps = 1 is made: an exact fit for every assembled window but one


def test_the_named_windows_need_what_the_table_says():
    b = cc.batch("reads")
    nd = cc.needs("reads")
    at = {k: b.names.index(k) for k in cc.TILED}
    assert [int(nd["slots"][at[k]]) for k in cc.TILED] == [2, 2, 3, 4]
    assert [int(nd["comps"][at[k]]) for k in cc.TILED] == [1, 1, 1, 2]
    assert int(nd["hap_len"][at["alt_heavier"]]) + 1 == int(nd["hap_len"][at["two_alt_heavier"]]) == 601
    assert int(nd["slots"][b.names.index("unassembled")]) == 0
    assert sorted(set(nd["slots"].tolist())) == [0, 2, 3, 4, 5]
    pool = cc.needs("poa")["pool"]
    pb = cc.batch("poa")
    assert [int(pool[pb.names.index(k)]) for k in ("ins_62", "ins_63", "ins_2x60")] == [64, 65, 124]
    assert int(cc.needs("poa")["comps"][pb.names.index("two_components_3_4")]) == 2
    assert sorted(set(cc.needs("poa")["alts"].tolist())) == [1, 2, 3, 4]


def test_walk_order_of_the_tiled_windows():
    """alt_heavier and two_alt_heavier: the walk that spells the REF anchor is dropped BEHIND the last kept walk, so a component
    that fills its last slot still has a walk to come (clean.hip decides the overflow of max_haps after the dedup, like
    oracle/graph.cpp's BuildHaplotypes followed by oracle/capi.cpp's count); ref_heavier: it is dropped in front"""
    b = cc.batch("reads")
    fates = {k: cc.walk_dispositions("reads", b.names.index(k)) for k in cc.TILED}
    assert fates["alt_heavier"] == ["Kr"]
    assert fates["two_alt_heavier"] == ["KKr"]
    assert fates["ref_heavier"] == ["rK"]
    assert len(fates["two_islands"]) == 2 and all(f.count("K") == 1 for f in fates["two_islands"])
    assert cc.walk_dispositions("reads", b.names.index("unassembled")) == []


@pytest.mark.parametrize("cap,c", TIGHT, ids=[f"{cap}-{c}" for cap, c in TIGHT])
def test_oracle_flags_exactly_the_windows_over_the_cap(cap, c):
    key, bit, bname, _ = cc.CAPS[cap]
    b = cc.batch(bname)
    nd = cc.needs(bname)[key]
    p, asm, var, geno = cc.oracle_chain(bname, cap, c)
    p0, asm0, var0, geno0 = cc.oracle_chain(bname)
    assert getattr(p, cap) == c
    status = asm["win_status"]
    for w in range(b.n):
        want = bit if int(nd[w]) > c else 0
        assert int(status[w]) & cc.CAP_BITS == want, (cap, c, b.names[w], int(nd[w]), int(status[w]))
        assert int(status[w]) & ~cc.CAP_BITS == int(asm0["win_status"][w]) & ~cc.CAP_BITS, b.names[w]
        if want:
            continue
        # stride independence: what the oracle says of a window that fits does not move with the caps
        assert haplotypes_of(p, asm, w) == haplotypes_of(p0, asm0, w), (cap, c, b.names[w])
        assert variants_of(p, var, w) == variants_of(p0, var0, w), (cap, c, b.names[w])
        assert cc.calls_of(p, var, geno, w) == cc.calls_of(p0, var0, geno0, w), (cap, c, b.names[w])
