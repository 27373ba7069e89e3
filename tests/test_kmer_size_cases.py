"""CPU companion of tests/test_gpu_kmer_sizes.py: the oracle alone over the sweep's case table.  The sweep compares engine
and oracle; if the oracle assembled nothing at some k the comparison would hold trivially.  So the floor the GPU tests assert
(half the windows of a batch with a component of >= 2 haplotypes, a variant, win_k == K for every assembled window) is
checked here for every K on a machine without a GPU -- assembly and variant extraction only, the stages the floor reads."""
import pytest

import kmer_size_cases as kc
from harness import OracleEngine


def test_the_sweep_covers_the_sizes_the_kernels_treat_differently():
    ks = set(kc.SWEEP_KS + kc.HIGH_KS)
    assert {13, 15, 17, 19, 21, 23, 27, 29, 31, 33, 35, 47, 49, 61, 63, 65, 67, 79, 95, 97, 99, 111, 125, 127} <= ks
    assert {129, 191, 255} <= ks and set(kc.ROUTE_KS) == {31, 33, 65, 127}
    assert all(k & 1 for k in ks)


def test_the_mixed_batch_holds_every_kind_of_window():
    """soft clips / N (not staged in LDS) beside clean windows (staged), lower case, an STR, 250-base reads from K = 97"""
    for K in (25, 97, 127):
        wins = kc.main_windows(K)
        assert 8 <= len(wins) <= 12
        has_n = [any((r["seq"] == ord("N")).any() for r in w["reads"]) for w in wins]
        has_lower = [any((r["seq"] >= ord("a")).any() for r in w["reads"]) for w in wins]
        clean = [not a and not b for a, b in zip(has_n, has_lower)]
        assert sum(has_n) >= 2 and sum(has_lower) >= 1 and sum(clean) >= 3, (has_n, has_lower)
        assert any(b"CAG" * 10 in w["ref"].tobytes() for w in wins)
        assert any(max(len(r["seq"]) for r in w["reads"]) == 250 for w in wins) == (K >= 97)
        assert any(len(r["seq"]) == 150 for w in wins for r in w["reads"])
    assert all(len({r["sample"] for r in w["reads"]}) == 3 for w in kc.three_sample_windows(25))
    for K in kc.HIGH_KS:
        assert all(len(r["seq"]) - K + 1 > 50 for w in kc.main_windows(K)[:2] for r in w["reads"])


@pytest.mark.parametrize("K", kc.SWEEP_KS + kc.HIGH_KS)
def test_oracle_assembles_the_sweep_at_every_k(K):
    lines = []
    for name, params, arrs, n, nr in kc.sweep_batches(K):
        orc = OracleEngine(params)
        asm = orc.assemble(arrs, n, nr)
        var = orc.msa(arrs, n, nr, asm)
        assembled, multi, nvars, bad = kc.floor_of(K, asm, var, n)
        lines.append(f"k={K} {name}: {assembled}/{n} windows assembled, {multi}/{n} with >= 2 haplotypes, {nvars} variants")
        assert not bad, bad
    print("\n".join(lines))  # (pytest -s: the table a reader of the sweep wants to see)
