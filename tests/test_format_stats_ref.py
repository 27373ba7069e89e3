"""Pins tests/format_stats_ref.py -- the independent reference of the read-level FORMAT statistics -- before
tests/test_gpu_format_stats.py trusts it: against the oracle's per-read taps in the golden fixtures, against scipy's rank
test, against closed forms, and a guard that the GPU test's cases hold every condition worth testing.  CPU only."""
import ctypes as C
import math

import numpy as np
import pytest

from lancet2_amd import capi

import format_stats_cases as cases
import format_stats_ref as ref


def test_the_engine_exports_the_statistics_entry_points():
    lib = capi.load_cdll()
    assert hasattr(lib, "ma_genotype_stats_batch") and hasattr(lib, "ma_process_stats_batch")
    assert C.sizeof(capi.FmtOut) == 4 * C.sizeof(C.c_void_p)
    p = capi.default_params()
    spec = capi.fmt_out_spec(p, 3)
    cells = 3 * p.max_vars * p.num_samples
    assert {k: v[1] for k, v in spec.items()} == dict(ev_sums=cells * (p.max_alts + 1) * 3, fmt_npbq=cells * (p.max_alts + 1),
                                                      fmt_cmlod=cells * p.max_alts, fmt_stat=cells * 4)


@pytest.mark.parametrize("name", cases.GOLDEN)
def test_reference_reproduces_the_oracles_assignments(name):
    params, arrs, n, nr, asm, var, want = cases.genotype_case(name)
    taps = cases.load_golden(name)[4]["geno"]
    assert int(taps["aln_cigar"].reshape(-1, 1 + params.max_cigar)[:, 0].max()) <= params.max_cigar
    asg = want["asg"]
    assert int((asg["allele"] != 255).sum()) >= 85
    assert np.array_equal(asg["allele"], taps["asg_allele"])
    assert np.array_equal(asg["score"].view(np.uint64), taps["asg_score"].view(np.uint64))
    assert np.array_equal(want["allele_counts"], taps["allele_counts"])


@pytest.mark.parametrize("ref_vals, alt_vals", [
    ([30, 30, 31, 12, 40], [30, 12, 12, 41]),       # ties inside and across the groups
    ([7], [9, 9, 3]),                               # a single element
    ([20, 20, 20], [20, 20]),                       # all equal
    (list(range(0, 60, 3)), list(range(1, 50, 2))),
    ([255, 0, 0, 17], [0, 255]),
])
def test_rank_test_against_scipy(ref_vals, alt_vals):
    stats = pytest.importorskip("scipy.stats")
    ranks, tie = ref.mid_ranks(ref_vals + alt_vals)
    assert ranks == stats.rankdata(ref_vals + alt_vals).tolist()
    u = ref.mann_whitney_u_alt(ref_vals, alt_vals)
    assert u == stats.mannwhitneyu(alt_vals, ref_vals, alternative="two-sided", method="asymptotic").statistic
    _, counts = np.unique(ref_vals + alt_vals, return_counts=True)
    assert tie == float((counts.astype(np.int64) ** 3 - counts).sum())
    es = ref.mann_whitney_effect_size(ref_vals, alt_vals)
    if len(set(ref_vals + alt_vals)) == 1:
        assert es == 0.0  # zero variance: a genuine zero, not a missing value
    else:
        m, k = len(ref_vals), len(alt_vals)
        big_n = m + k
        var_u = m * k / 12.0 * ((big_n + 1) - tie / (big_n * (big_n - 1)))
        assert es == pytest.approx((u - m * k / 2.0) / math.sqrt(var_u) / math.sqrt(big_n), rel=1e-14)


def test_rank_test_is_missing_for_an_empty_group():
    assert ref.mann_whitney_effect_size([], [3, 4]) is None and ref.mann_whitney_effect_size([3], []) is None


def test_closed_forms():
    # NPBQ of n reads of one quality: log10(eps^n / (eps^n + (1 - eps)^n)) * -10 / n
    for q, n in ((30, 1), (30, 7), (12, 4), (2, 3)):
        eps = ref.PHRED[q]
        want = -10.0 * math.log10(eps ** n / (eps ** n + (1.0 - eps) ** n)) / n
        assert ref.raw_posterior_base_qual([q] * (n - n // 2), [q] * (n // 2)) / n == pytest.approx(want, rel=1e-12)
    assert ref.raw_posterior_base_qual([], []) == 0.0
    # CMLOD: no ALT reads -> 0; K < 2 -> 0
    assert ref.continuous_mixture_lods([([30, 31], [28]), ([], [])], [3, 0]) == [0.0, 0.0]
    assert ref.continuous_mixture_lods([([30], [])], [1]) == [0.0]
    # CMLOD with K = 3: written out for one read per allele, f = 1/3 each; the null of ALT 1 moves its third to the others
    q = 20
    eps = ref.PHRED[q]
    mm = eps / 2.0
    bonus = (1.0 - eps) - mm
    ll_mle = 3 * math.log10(mm + bonus / 3.0)
    ll_null = 2 * math.log10(mm + bonus / 2.0) + math.log10(max(1e-15, mm))
    lods = ref.continuous_mixture_lods([([q], []), ([], [q]), ([q], [])], [1, 1, 1])
    assert lods[0] == 0.0 and lods[1] == pytest.approx(ll_mle - ll_null, rel=1e-12) and lods[2] == pytest.approx(lods[1], rel=1e-12)
    # every read on the target ALT: nothing remains, the null puts everything on REF
    lod = ref.continuous_mixture_lods([([], []), ([q, q], [])], [0, 2])[1]
    assert lod == pytest.approx(2 * math.log10(eps + ((1.0 - eps) - eps)) - 2 * math.log10(eps), rel=1e-12)  # (K = 2: mismatch = eps)
    # HSE
    assert ref.alt_hap_entropy([2, 2, 2, 2], 5) == 0.0
    assert ref.alt_hap_entropy([0, 1, 2, 0, 1, 2], 3) == pytest.approx(1.0, rel=1e-15)
    assert ref.alt_hap_entropy([1, 2, 1, 2], 2) == pytest.approx(1.0, rel=1e-15)
    assert ref.alt_hap_entropy([1, 2], 4) is None and ref.alt_hap_entropy([1, 1, 1], 1) is None
    # ASMD / AHDD
    assert ref.mean_alt_minus_ref([1, 3], [10, 12, 14], 5.0) == (12.0 - 5.0) - 2.0
    assert ref.mean_alt_minus_ref([], [1]) is None and ref.mean_alt_minus_ref([1], []) is None


def test_local_score_tracks_both_sides_of_every_deletion_reached():
    """base_qual: a deletion BEFORE the variant still contributes the qualities on both sides of it"""
    q = np.zeros(40, np.uint8)
    quals = np.full(40, 30, np.uint8)
    quals[9], quals[10] = 7, 5  # the bases around the deletion
    target = np.zeros(43, np.uint8)
    cig = [(0, 10), (2, 3), (0, 30)]
    assert ref.local_score(cig, q, quals, target, 0, 25, 1)[3] == 5
    assert ref.local_score([(0, 40)], q, quals, target, 0, 25, 1)[3] == 30
    assert ref.local_score(cig, q, quals, target, 0, 5, 1)[3] == 30  # the walk stops before it reaches the deletion
    assert ref.local_score(cig, q, quals, target, 0, 25, 0)[3] == 0 and ref.local_score([], q, quals, target, 0, 25, 1)[3] == 0


def test_the_gpu_cases_hold_every_condition():
    """so that tests/test_gpu_format_stats.py cannot go empty: from the oracle alone, its cases hold a cell of every kind"""
    cells = {}
    for name in cases.GENOTYPE_CASES:
        params, arrs, n, nr, asm, var, want = cases.genotype_case(name)
        cells.update({(name,) + k: v for k, v in want["cells"].items()})
        if name == "c5_three_samples":
            assert params.num_samples == 3
        if name == "c4_indel50":
            assert max(np.diff(arrs["read_win_off"])) > 512  # several trips per thread of a 256-thread workgroup
        if name == "qual_extremes":  # both extremes sit on reads that are assigned somewhere
            quals = arrs["read_quals"]
            evid = {int(quals[int(arrs["read_off"][r])]) for r in range(nr)
                    if (want["asg"]["allele"][r * params.max_vars: (r + 1) * params.max_vars] != 255).any()}
            assert 0 in evid and 255 in evid
    params, arrs, n, nr, want = cases.process_case()
    cells.update({("process",) + k: v for k, v in want["cells"].items()})
    assert sum(c["n_ref"] > 0 and c["n_alt"] > 0 for k, c in cells.items() if k[0] == "process") >= 1
    vals = list(cells.values())
    assert any(c["n_ref"] > 0 and c["n_alt"] > 0 for c in vals)
    assert any(c["hse"] is not None and 0.0 < c["hse"] < 1.0 for c in vals)
    assert any(1 in c["alt_types"] and c["n_alt"] > 0 for c in vals)  # insertion
    assert any(2 in c["alt_types"] and c["n_alt"] > 0 for c in vals)  # deletion
    assert any(c["outside_del"] for c in vals)
    assert any(c["k"] == 3 and c["n_alt"] > 0 for k, c in cells.items() if k[0].startswith("two_alts"))
    assert any(c["removed"] > 0 for k, c in cells.items() if k[0] == "dedup")
    assert any(c["bqcd"] is None for c in vals)
    missing = 0
    for name in cases.GENOTYPE_CASES:
        params, arrs, n, nr, asm, var, want = cases.genotype_case(name)
        for w in range(n):
            for v in range(int(var["win_nvars"][w])):
                missing += sum((name, w, v, s) not in cells for s in range(params.num_samples))
    assert missing >= 1  # a sample without evidence at a variant that exists
