"""CPU companion of tests/test_gpu_scoring.py: the oracle alone over tests/scoring_cases.py.  The GPU test compares engine
and oracle; a case whose reads found no haplotype, or whose edge never occurs, would pass for nothing.  So what every case is
FOR is checked here on a machine without a GPU: the depths the construction fixes, the number of evidence keys of the dense
windows, the CIGAR shapes under the variant region, the allele counts K."""
import time

import numpy as np
import pytest

import scoring_cases as sc

DENSE_KEYS = dict(dense_over=9600, dense_exact=8192, dense_exact_plus_one=8193)


def _hits(c, geno):
    """-> [(read, haplotype slot, rs, re, [(op, len)])] of every alignment the oracle reported"""
    p = c.params
    rec = geno["aln_rec"].reshape(c.nr, p.max_haps, 6)
    cig = geno["aln_cigar"].reshape(c.nr, p.max_haps, 1 + p.max_cigar)
    out = []
    for r, h in zip(*np.nonzero(rec[:, :, 0])):
        n_ops = int(cig[r, h, 0])
        assert n_ops <= p.max_cigar
        out.append((int(r), int(h), int(rec[r, h, 2]), int(rec[r, h, 3]), [(int(x) & 15, int(x) >> 4) for x in cig[r, h, 1:1 + n_ops]]))
    return out


@pytest.mark.parametrize("name", sc.NAMES)
def test_the_oracle_sees_what_the_case_is_for(name):
    c = sc.case(name)
    t0 = time.perf_counter()
    geno = sc.oracle_genotype(name)
    seconds = time.perf_counter() - t0
    p = c.params
    hits = _hits(c, geno)  # (asserts that no CIGAR exceeds max_cigar)
    assert len(hits) > 0
    if c.expected_counts is not None:
        bad = np.nonzero(geno["allele_counts"] != c.expected_counts)[0]
        assert bad.size == 0, (bad[:8].tolist(), geno["allele_counts"][bad[:8]].tolist(), c.expected_counts[bad[:8]].tolist())
        assert c.expected_counts.sum() > 0
    keys = sc.key_count(c, geno)
    print(f"{name}: {c.nr} reads, {len(hits)} hits, {keys} evidence keys, {seconds:.2f} s")
    if name in DENSE_KEYS:
        assert keys == DENSE_KEYS[name]
        assert c.n == 1 and c.nr * int(c.var["win_nvars"][0]) >= keys
    assert seconds < 2.0


def test_the_dense_window_among_others_is_not_the_largest():
    c = sc.case("dense_among_others")
    geno = sc.oracle_genotype("dense_among_others")
    reads = np.diff(c.arrs["read_win_off"].astype(np.int64))
    assigned = (geno["asg_allele"].reshape(c.nr, c.params.max_vars) != 255).sum(axis=1)
    keys = [int(assigned[int(c.arrs["read_win_off"][w]):int(c.arrs["read_win_off"][w + 1])].sum()) for w in range(c.n)]
    assert c.n == 5 and keys[2] == 9600 and reads[2] == 160 and reads.max() == 300 and reads.argmax() != 2
    assert c.var["win_nvars"].tolist() == [1, 1, 60, 0, 1] and keys[3] == 0 and all(keys[w] == reads[w] for w in (0, 1, 4))


def test_dedup_assigns_the_ignored_sample():
    c = sc.case("dedup")
    geno = sc.oracle_genotype("dedup")
    beyond = np.nonzero(c.arrs["read_sample"][:c.nr] >= c.params.num_samples)[0]
    assert len(beyond) == 5 and (geno["asg_allele"].reshape(c.nr, -1)[beyond, 0] != 255).all()
    total = int((geno["asg_allele"].reshape(c.nr, -1)[:, 0] != 255).sum())
    assert total == c.nr and int(c.expected_counts.sum()) == c.nr - 5 - 6 - 3  # ignored, second mates, third reads


@pytest.mark.parametrize("name,k", [("five_alleles", 5), ("five_alleles_case_control", 5), ("seven_alleles", 7)])
def test_the_allele_cases_reach_their_k(name, k):
    c = sc.case(name)
    geno = sc.oracle_genotype(name)
    p = c.params
    NA, S = p.max_alts + 1, p.num_samples
    w, v = 0, 0
    assert int(c.var["var_nalts"][w * p.max_vars + v]) + 1 == k
    depth = geno["allele_counts"].reshape(-1, S, NA, 2)[w * p.max_vars + v].sum(axis=2)  # [sample][allele]
    with_evidence = depth.sum(axis=1) > 0
    assert (depth[with_evidence] > 0).sum(axis=1).max() == k  # a sample that holds every allele
    G = NA * (NA + 1) // 2
    pl = geno["var_pl"].reshape(-1, S, G)[w * p.max_vars + v]
    gq = geno["var_gq"].reshape(-1, S)[w * p.max_vars + v]
    assert G == k * (k + 1) // 2
    for s in range(S):
        if with_evidence[s]:
            assert (pl[s] == 0).sum() >= 1 and (pl[s] > 0).sum() >= G - 2, (s, pl[s].tolist())
        else:
            assert not pl[s].any() and gq[s] == 0
    if name != "seven_alleles":
        assert (~with_evidence).sum() == 1 and int(c.asm["comp_hap0"][1]) == 3 and int(c.var["var_comp"][0]) == 1
    assert (geno["var_qual"][0] > 0) and bool(p.case_ctrl_mode) == (name == "five_alleles_case_control")


def test_solor_shapes_hold_the_four_role_layouts():
    c = sc.case("solor_shapes")
    geno = sc.oracle_genotype("solor_shapes")
    p = c.params
    S, NA = p.num_samples, p.max_alts + 1
    assert c.n == 4 and p.case_ctrl_mode == 1 and S == 8
    shapes = []
    for w in range(c.n):
        r0, r1 = int(c.arrs["read_win_off"][w]), int(c.arrs["read_win_off"][w + 1])
        smp = c.arrs["read_sample"][r0:r1]
        case_of = {int(s) for s, f in zip(smp, c.arrs["read_flags"][r0:r1]) if f & 2}
        depth = geno["allele_counts"].reshape(-1, S, NA, 2)[w * p.max_vars].sum(axis=2)
        seen = {s for s in range(S) if depth[s].sum() > 0}
        shapes.append((sorted(seen - case_of), sorted(seen & case_of), depth))
    assert len(shapes[0][0]) == 3 and len(shapes[0][1]) == 2
    assert len(shapes[1][0]) == 0 and len(shapes[1][1]) == 2
    assert any(shapes[2][2][s, 1:].sum() == 0 for s in shapes[2][1]) and any(shapes[2][2][s, 1:].sum() > 0 for s in shapes[2][1])
    r0, r1 = int(c.arrs["read_win_off"][3]), int(c.arrs["read_win_off"][4])
    roles_of_2 = {int(f) & 2 for s, f in zip(c.arrs["read_sample"][r0:r1], c.arrs["read_flags"][r0:r1]) if s == 2}
    assert roles_of_2 == {0, 2} and 2 in shapes[3][1]
    # the larger of the two case samples' SOLOR values, by hand, for the first window
    depth = shapes[0][2]
    ctrl_alt = sum(depth[s, 1:].sum() for s in shapes[0][0]) / 3.0 + 1.0
    ctrl_ref = sum(depth[s, 0] for s in shapes[0][0]) / 3.0 + 1.0
    solor = [np.log(((depth[s, 1:].sum() + 1.0) * ctrl_ref) / ((depth[s, 0] + 1.0) * ctrl_alt)) for s in shapes[0][1]]
    assert abs(geno["var_qual"][0] - max(solor)) < 1e-12 and min(solor) < max(solor)
    assert (geno["var_qual"].reshape(c.n, -1)[:, 0] > 0).all()


def test_region_edges_reach_the_region_from_every_side():
    c = sc.case("region_edges")
    geno = sc.oracle_genotype("region_edges")
    p = c.params
    MH, MA = p.max_haps, p.max_alts
    indel_inside = begins = ends = 0
    hits = _hits(c, geno)
    for r, h, rs, re_, cig in hits:
        if h == 0:
            vstart, vlen = int(c.var["var_ref_start"][0]), int(c.var["var_ref_len"][0])
        else:
            vstart, vlen = int(c.var["var_hap_start"][h]), int(c.var["alt_len"][int(c.var["var_hap_allele"][h]) - 1])
        tp, inside = rs, False
        for op, ln in cig:
            if op in (1, 2) and vstart <= tp < vstart + vlen:
                inside = True
            if op in (0, 2):
                tp += ln
        indel_inside += inside
        begins += vstart < rs < vstart + vlen
        ends += vstart < re_ < vstart + vlen
    quals = set(np.unique(c.arrs["read_quals"][:int(c.arrs["read_off"][c.nr])]).tolist())
    print(f"region_edges: {len(hits)} hits, {indel_inside} with an indel starting in the region, {begins} beginning and {ends} ending inside it")
    assert quals == set(sc.EDGE_PHRED)
    assert indel_inside >= 100 and begins >= 20 and ends >= 10
    assert [int(c.var["var_ref_len"][0])] + c.var["alt_len"][:2].tolist() == [7, 1, 16] and MH >= 3 and MA >= 2
    assigned = geno["asg_allele"].reshape(c.nr, -1)[:, 0]
    assert {0, 1, 2} <= set(assigned.tolist())


def test_clipped_ends_carry_soft_clips():
    c = sc.case("clipped_ends")
    geno = sc.oracle_genotype("clipped_ends")
    hits = _hits(c, geno)
    clipped = sum(any(op == 4 for op, _ in cig) for *_, cig in hits)
    assigned = (geno["asg_allele"].reshape(c.nr, -1)[:, :2] != 255).any(axis=1)
    print(f"clipped_ends: {len(hits)} hits, {clipped} with an S operation, {int(assigned.sum())} of {c.nr} reads assigned")
    assert clipped >= 40 and c.nr == 32 and assigned.all()


def test_first_wins_is_a_tie():
    """an ALT read's combined scores against the two haplotypes of its allele are equal: only the order decides"""
    import format_stats_ref as ref
    c = sc.case("first_wins")
    geno = sc.oracle_genotype("first_wins")
    asg = ref.assign_reads(c.params, c.arrs, c.n, c.asm, c.var, geno["aln_rec"], geno["aln_cigar"])
    MV = c.params.max_vars
    rec = geno["aln_rec"].reshape(c.nr, c.params.max_haps, 6)
    tied = 0
    for r in range(c.nr):
        if asg["allele"][r * MV] == 1:
            assert rec[r, 1, 0] and rec[r, 2, 0] and rec[r, 1, 1] == rec[r, 2, 1]  # both hit, the same score
            assert asg["hap_id"][r * MV] == 1
            tied += 1
    assert tied >= 16


@pytest.mark.parametrize("name", sc.STATS)
def test_the_statistics_reference_counts_what_the_oracle_counts(name):
    """tests/format_stats_ref.py re-derives every assignment from the oracle's alignments alone: its depths are the oracle's
    with a component whose comp_hap0 is 3, five alleles, and 9600 keys in a window (stats_reference asserts it)"""
    want = sc.stats_reference(name)
    assert want["allele_counts"].sum() > 0 and np.isfinite(want["fmt_npbq"]).all()
    if name == "five_alleles":
        assert {k for (_, _, _), cell in want["cells"].items() for k in [cell["k"]]} == {5}
    if name == "first_wins":  # 18 ALT reads on haplotype 1, none on 2, 9 on 3 -- 9 / 9 / 9 had the tie gone the other way
        hse = want["fmt_stat"].reshape(-1, 4)[:c_samples(name), 3]
        assert np.all(hse < 0.5 * np.log2(3.0))


def c_samples(name):
    return sc.case(name).params.num_samples
