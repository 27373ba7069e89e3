"""CPU guard of tests/cx_chain_cases.py (the oracle alone, no GPU): the inputs of tests/test_gpu_cx_chain.py are what that test
takes them to be, and the Python layer exposes the chained annotation call."""
import numpy as np

from lancet2_amd import capi
from lancet2_amd.engine import Engine

import cx_chain_cases as cases


def test_chain_batch_carries_variants():
    c = cases.chain_case()
    nv = c.var["win_nvars"]
    assert int(nv.sum()) >= 6 and int((nv > 0).sum()) >= 3
    assert int((nv == 0).sum()) >= 1
    for gc in cases.GC_FRACS:
        used = cases.used_slots(c.params, nv)
        assert np.isfinite(c.cx[gc]["seq_cx_d"].reshape(-1, 3)[used]).all()
    # the two GC fractions are told apart by the values: a table that was not rebuilt shows
    used = cases.used_slots(c.params, nv)
    a, b = (c.cx[gc]["seq_cx_d"].reshape(-1, 3)[used] for gc in cases.GC_FRACS)
    assert not np.array_equal(a, b)


def _hap_lq(group, want, name):
    w = group.names.index(name)
    return float(want[group.name]["seq_cx_d"].reshape(group.n, group.params.max_vars, 3)[w, 0, 1])


def test_hap_lq_table():
    groups = {g.name: g for g in cases.hap_lq_groups()}
    want = cases.hap_lq_reference()
    values = []
    for g in groups.values():
        used = cases.used_slots(g.params, g.var["win_nvars"])
        col = want[g.name]["seq_cx_d"].reshape(-1, 3)[used, 1]
        assert np.isfinite(col).all(), g.name
        values += col.tolist()
    d, lg, multi = groups["default"], groups["long"], groups["multi"]
    assert d.params.max_hap_len == 2048 and lg.params.max_hap_len == 4096
    for name in ("len6", "all_n"):
        assert _hap_lq(d, want, name) == 0.0, name
    for name in ("homopolymer", "ac_repeat"):
        assert _hap_lq(d, want, name) > 0.0, name
    assert _hap_lq(lg, want, "doubled_unit") > 0.0
    assert len({round(v, 12) for v in values}) >= 6
    # the shapes are what their names say
    for name, length in (("len6", 6), ("len7", 7), ("len8", 8), ("len262", 262), ("len263", 263), ("len264", 264),
                         ("exact_fit", 2048), ("homopolymer", 2048)):
        assert len(cases.ref_haplotype(d, name)) == length, name
    homo = cases.kmer_counts(cases.ref_haplotype(d, "homopolymer"))
    assert homo[0] == 2042 and homo[1] == 0  # one bin of a word at 2042, the other half of that word at 0
    two = cases.kmer_counts(cases.ref_haplotype(d, "two_bins_one_word"))
    assert two[0] >= 2 and two[1] >= 2 and two[0] != two[1]  # AAAAAAA and AAAAAAC: codes 0 and 1, one word
    ac = cases.kmer_counts(cases.ref_haplotype(d, "ac_repeat"))
    code = lambda s: sum("ACGT".index(ch) << (2 * (6 - i)) for i, ch in enumerate(s))  # noqa: E731
    assert ac[code("ACACACA")] > 0 and ac[code("TGTGTGT")] == 0  # forward and reverse-complement bins differ
    scattered = cases.ref_haplotype(d, "scattered_n")
    assert 5 <= scattered.count("N") < len(scattered) // 8
    assert cases.ref_haplotype(d, "lower_case").islower()
    doubled = cases.kmer_counts(cases.ref_haplotype(lg, "doubled_unit"))
    assert 1900 <= int((doubled >= 2).sum()) <= cases.LIST_CAP  # just under the list cap, by construction
    assert len(cases.ref_haplotype(lg, "long_homopolymer")) == 4096
    # several components, and windows without a variant
    assert multi.asm["win_ncomp"].tolist() == [3, 1, 1, 2] and multi.var["win_nvars"].tolist() == [2, 1, 0, 2]
    assert set(multi.var["var_comp"][:2].tolist()) == {1}


def test_python_layer_exposes_the_chained_call():
    assert len(capi.PROCESS_CX_ARGTYPES) == 12
    assert callable(getattr(Engine, "process_cx")) and callable(getattr(Engine, "process_cx_device"))
    import os
    header = open(os.path.join(capi.REPO, "include", "microasm.h")).read()
    assert "int ma_process_cx_batch(" in header
