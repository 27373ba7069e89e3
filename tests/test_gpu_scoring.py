"""GPU parity of the genotype stage's second half -- k_assign, k_evidence, k_qual and, with statistics, k_evid_stats -- on the
hand-made variants of tests/scoring_cases.py (guarded on the CPU by tests/test_scoring_cases.py): windows whose reads x
variants exceed any fixed evidence table, five and seven alleles, one to eight samples, the SOLOR role layouts, a component
behind one without variants, small strides, and CIGARs that reach the variant region from every side.

Every case: records, CIGARs, assignments, score bit patterns, depths, PL and GQ equal to the oracle's, QUAL within 1e-9
(harness.compare_geno); the depths also equal to what the construction says; no window flag the oracle does not raise.
The genotype call is not split over lanes (ma_set_streams concerns ma_process_batch alone), so dense_among_others runs on the
one lane there is."""
import numpy as np
import pytest

import scoring_cases as sc
from format_stats_cases import compare_fmt
from harness import compare_geno

pytestmark = pytest.mark.gpu


def _engine(params):
    from lancet2_amd.engine import Engine
    return Engine(params)


def _fresh_asm(c):
    """(the engine copies win_status back into the caller's array: the shared case stays as it is)"""
    return dict(c.asm, win_status=c.asm["win_status"].copy())


def _depth_report(name, c, got):
    p = c.params
    want = sc.oracle_genotype(name)["allele_counts"]
    lost = want.astype(np.int64) - got.astype(np.int64)
    print(f"{name}: depths {int(got.sum())} of the oracle's {int(want.sum())}, {int((lost != 0).sum())} of "
          f"{int((want != 0).sum())} non-zero cells differ")
    per_win = lost.reshape(c.n, -1).sum(axis=1)
    for w in np.nonzero(per_win)[0]:
        per_var = lost.reshape(c.n, p.max_vars, -1)[w].sum(axis=1)
        print(f"  window {w}: {int(per_win[w])} reads not counted, variants {np.nonzero(per_var)[0][:12].tolist()} "
              f"lose {per_var[np.nonzero(per_var)[0][:12]].tolist()}")


@pytest.mark.parametrize("name", sc.NAMES)
def test_genotype_matches_the_oracle_and_the_construction(name):
    c = sc.case(name)
    want = sc.oracle_genotype(name)
    asm = _fresh_asm(c)
    eng = _engine(c.params)
    try:
        got = eng.genotype(c.arrs, c.n, c.nr, asm, c.var, debug=True)
        kernels = {k for k, _ in eng.kernel_times()}
    finally:
        eng.close()
    _depth_report(name, c, got["allele_counts"])
    assert {"k_assign", "k_evidence", "k_qual"} <= kernels
    bad = compare_geno(c.params, got, want, c.n, c.nr, c.var["win_nvars"], c.arrs["read_win_off"])
    assert not bad, "\n".join(bad[:20])
    if c.expected_counts is not None:
        assert np.array_equal(got["allele_counts"], c.expected_counts)
    extra = asm["win_status"] & ~c.asm["win_status"]  # (the oracle's genotype stage raises none)
    assert not extra.any(), extra.tolist()


@pytest.mark.parametrize("name", sc.STATS)
def test_genotype_stats_match_the_reference(name):
    c = sc.case(name)
    want = sc.stats_reference(name)
    eng = _engine(c.params)
    try:
        geno, fmt = eng.genotype_stats(c.arrs, c.n, c.nr, _fresh_asm(c), c.var)
        kernels = {k for k, _ in eng.kernel_times()}
    finally:
        eng.close()
    _depth_report(name, c, geno["allele_counts"])
    assert "k_evid_stats" in kernels
    assert np.array_equal(geno["allele_counts"], want["allele_counts"])
    assert np.array_equal(geno["allele_counts"], c.expected_counts)
    bad = compare_fmt(fmt, want, name)
    assert not bad, "\n".join(bad)


def test_calls_without_the_debug_taps_are_the_same():
    """the caller that passes no taps (the internal copy of the assignments, k_qual without the PL arrays in case/control mode)"""
    from harness import compare_geno_calls
    for name in ("dense_among_others", "five_alleles_case_control", "small_strides"):
        c = sc.case(name)
        eng = _engine(c.params)
        try:
            got = eng.genotype(c.arrs, c.n, c.nr, _fresh_asm(c), c.var, debug=False)
        finally:
            eng.close()
        bad = compare_geno_calls(got, sc.oracle_genotype(name))
        assert not bad, name + "\n" + "\n".join(bad)
