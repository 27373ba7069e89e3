"""Hand-made inputs of the genotype stage's second half (k_assign, k_evidence, k_qual, k_evid_stats): the cases
tests/test_gpu_scoring.py runs against the oracle and tests/test_scoring_cases.py guards on the CPU.  Inputs only, seeded;
the assembly and variant arrays are written by hand (harness.handmade_genotype_case), so a case does not depend on what the
assembler makes of a window.

case(name) -> Case(params, arrs, n, nr, asm, var, expected_counts).  expected_counts (capi.geno_out_spec's allele_counts
layout, or None) is what the CONSTRUCTION says: distinct read names, every read cut from one haplotype and spanning the
site -- AD = the number of such reads per sample, allele and strand."""
import collections
import functools

import numpy as np

from lancet2_amd import capi, synth
from pin_cases import BASES, rand_dna

Case = collections.namedtuple("Case", "params arrs n nr asm var expected_counts")

DENSE = ("dense_over", "dense_exact", "dense_exact_plus_one")
NAMES = DENSE + ("dense_among_others", "dedup", "five_alleles", "five_alleles_case_control", "seven_alleles", "one_sample",
                 "small_strides", "solor_shapes", "region_edges", "clipped_ends", "first_wins")
# the cases that also go through Engine.genotype_stats (first_wins: the winning haplotype shows in HSE alone)
STATS = DENSE + ("dedup", "five_alleles", "first_wins")
EDGE_PHRED = (0, 1, 2, 11, 25, 37, 41, 93, 255)


def _other(b, step=1):
    return BASES[(BASES.index(bytes([b])) + step) % 4]


def _sub(seq, pos, step=1):
    b = bytearray(seq)
    b[pos] = _other(b[pos], step)
    return bytes(b)


def _read(seq, qual, qname, sample=0, role=0, rev=False):
    qual = np.full(len(seq), qual, np.uint8) if np.isscalar(qual) else np.asarray(qual, np.uint8)
    assert len(qual) == len(seq)
    return dict(seq=np.frombuffer(bytes(seq), np.uint8).copy(), qual=qual, qname=qname, sample=sample, role=role, rev=rev,
                passf=True, start=0, hint=capi.MA_NO_HINT)


def _snv(comp, pos, carriers=(1,)):
    return dict(comp=comp, ref_start=pos, ref_len=1, alts=[(1, {h: pos for h in carriers})])


class _Counts:
    """expected allele depths, filled read by read"""

    def __init__(self, p, n):
        self.p = p
        self.a = np.zeros(n * p.max_vars * p.num_samples * (p.max_alts + 1) * 2, np.uint32)

    def add(self, w, v, sample, allele, rev, k=1):
        p = self.p
        self.a[(((w * p.max_vars + v) * p.num_samples + sample) * (p.max_alts + 1) + allele) * 2 + int(bool(rev))] += k


def _finish(params, wins, specs, counts):
    from harness import handmade_genotype_case
    asm, var = handmade_genotype_case(params, specs)
    arrs, n, nr = synth.pack_batch(wins)
    return Case(params, arrs, n, nr, asm, var, None if counts is None else counts.a)


# ---- the evidence table: reads x variants of ONE window ----------------------------------------------------------------
def _dense_window(rng, n_reads, read_len, n_sites, spacing, qname0=0, extra=False):
    """a REF and an ALT haplotype that differ in n_sites SNVs `spacing` apart; every read spans all of them and alternates
    haplotype, sample and strand.  REF reads have no hit on the ALT haplotype (and the other way round): 5 x n_sites of cost.
    extra: one more 150-base REF read that overlaps the LAST site alone.
    -> (window, spec, [(read's haplotype, sample, rev, sites it is counted at)])"""
    first = 40
    last = first + (n_sites - 1) * spacing
    assert last - first < read_len - 8
    ref = rand_dna(rng, last + 160)
    alt = ref
    sites = [first + x * spacing for x in range(n_sites)]
    for s in sites:
        alt = _sub(alt, s)
    lo, hi = max(0, last + 3 - read_len), first - 2  # starts from which a read spans every site
    reads, who = [], []
    for i in range(n_reads):
        h, sample, rev = i & 1, (i >> 1) & 1, bool((i >> 2) & 1)
        st = lo + int(rng.integers(0, hi - lo + 1))
        reads.append(_read((alt if h else ref)[st:st + read_len], rng.integers(20, 42, read_len), qname0 + i, sample, sample, rev))
        who.append((h, sample, rev, range(n_sites)))
    if extra:
        reads.append(_read(ref[last - 1:last + 149], 30, qname0 + n_reads, 0, 0, False))
        who.append((0, 0, False, [n_sites - 1]))
    win = dict(ref=np.frombuffer(ref, np.uint8).copy(), reads=reads)
    spec = dict(comps=[[ref, alt]], vars=[_snv(0, s) for s in sites])
    return win, spec, who


def _plain_window(rng, n_reads, qname0=0, with_variant=True, layout=None):
    """REF + ALT haplotype of 420 bases with one SNV at 210; 150-base reads spanning it.  layout: [(haplotype, sample, role,
    rev)] per read, default alternating like the dense window"""
    ref = rand_dna(rng, 420)
    alt = _sub(ref, 210)
    layout = layout or [(i & 1, (i >> 1) & 1, (i >> 1) & 1, bool((i >> 2) & 1)) for i in range(n_reads)]
    reads, who = [], []
    for i, (h, sample, role, rev) in enumerate(layout):
        st = int(rng.integers(80, 196))
        reads.append(_read((alt if h else ref)[st:st + 150], rng.integers(20, 42, 150), qname0 + i, sample, role, rev))
        who.append((h, sample, rev, [0] if with_variant else []))
    win = dict(ref=np.frombuffer(ref, np.uint8).copy(), reads=reads)
    spec = dict(comps=[[ref, alt]], vars=[_snv(0, 210)] if with_variant else [])
    return win, spec, who


def _count_who(counts, w, who):
    for h, sample, rev, sites in who:
        for v in sites:
            counts.add(w, v, sample, h, rev)


def _dense(seed, n_reads, n_sites, spacing, extra=False):
    params = capi.default_params(min_k=25, max_k=25)
    win, spec, who = _dense_window(np.random.default_rng(seed), n_reads, 250, n_sites, spacing, extra=extra)
    counts = _Counts(params, 1)
    _count_who(counts, 0, who)
    return _finish(params, [win], [spec], counts)


def _dense_among_others():
    params = capi.default_params(min_k=25, max_k=25)
    rng = np.random.default_rng(9105)
    parts = [_plain_window(rng, 40, qname0=0), _plain_window(rng, 300, qname0=1000), _dense_window(rng, 160, 250, 60, 4, qname0=2000),
             _plain_window(rng, 48, qname0=3000, with_variant=False), _plain_window(rng, 33, qname0=4000)]
    counts = _Counts(params, len(parts))
    for w, (_, _, who) in enumerate(parts):
        _count_who(counts, w, who)
    return _finish(params, [x[0] for x in parts], [x[1] for x in parts], counts)


# ---- the evidence rule -------------------------------------------------------------------------------------------------
def _dedup():
    params = capi.default_params(min_k=25, max_k=25)
    rng = np.random.default_rng(77031)
    ref = rand_dna(rng, 420)
    alt = _sub(ref, 210)
    hap = (ref, alt)
    counts = _Counts(params, 1)
    reads = []

    def put(h, qname, sample, rev, counted):
        st = int(rng.integers(80, 196))
        reads.append(_read(hap[h][st:st + 150], rng.integers(20, 42, 150), qname, sample, sample & 1, rev))
        if counted:
            counts.add(0, 0, sample, h, rev)

    for i in range(6):  # mates of one name that support the same allele: one count, the strand of the first
        put(i & 1, 100 + i, 0, bool(i & 2), True)
        put(i & 1, 100 + i, 0, not (i & 2), False)
    for i in range(4):  # mates that support different alleles: both
        put(0, 200 + i, 1, False, True)
        put(1, 200 + i, 1, True, True)
    for i in range(4):  # one name in both samples: both
        put(1, 300 + i, 0, bool(i & 1), True)
        put(1, 300 + i, 1, bool(i & 1), True)
    for i in range(5):  # a sample beyond num_samples: assigned, never counted -- and its names shadow nobody's
        put(i & 1, 100 + i, 2, False, False)
    for i in range(3):  # the third read of a name, after another name in between
        put(1, 100 + 2 * i + 1, 0, True, False)
    win = dict(ref=np.frombuffer(ref, np.uint8).copy(), reads=reads)
    return _finish(params, [win], [dict(comps=[[ref, alt]], vars=[_snv(0, 210)])], counts)


# ---- many alleles, many samples ----------------------------------------------------------------------------------------
def _multi_allele_site(rng, kinds, pos=230, length=520):
    """-> (haplotypes [REF, one per kind], variant).  kinds: ("snv", step) | ("del", L) | ("ins", L); the REF allele spans
    the anchor base at `pos` and the longest deletion"""
    ref = rand_dna(rng, length)
    # (no base of the region repeats its neighbour: an indel there has one placement)
    b = bytearray(ref)
    for x in range(pos, pos + 8):
        while b[x] == b[x - 1]:
            b[x] = _other(b[x])
    ref = bytes(b)
    ref_len = 1 + max([k[1] for k in kinds if k[0] == "del"] or [0])
    haps, alts = [ref], []
    for h, (kind, x) in enumerate(kinds, start=1):
        if kind == "snv":
            haps.append(_sub(ref, pos, x))
            alts.append((ref_len, {h: pos}))
        elif kind == "del":
            haps.append(ref[:pos + 1] + ref[pos + 1 + x:])
            alts.append((ref_len - x, {h: pos}))
        else:
            ins = bytes(_other(ref[pos + 1], 2) if i == 0 else BASES[int(rng.integers(0, 4))] for i in range(x))
            haps.append(ref[:pos + 1] + ins + ref[pos + 1:])
            alts.append((ref_len + x, {h: pos}))
    return haps, dict(ref_start=pos, ref_len=ref_len, alts=alts)


def _allele_reads(rng, haps, depths, counts, w, v, pos, roles=None, qname0=0):
    """depths[sample][allele] reads of 150 bases cut from the allele's haplotype around `pos`, Phred 2 ... 41"""
    reads = []
    for sample, per_allele in enumerate(depths):
        for allele, d in enumerate(per_allele):
            for i in range(d):
                st = pos - int(rng.integers(40, 110))
                rev = bool((i + allele) & 1)
                reads.append(_read(haps[allele][st:st + 150], rng.integers(2, 42, 150), qname0 + len(reads), sample,
                                   roles[sample] if roles else 0, rev))
                counts.add(w, v, sample, allele, rev)
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def _five_alleles(case_ctrl):
    params = capi.default_params(min_k=25, max_k=25, num_samples=8, case_ctrl_mode=case_ctrl)
    rng = np.random.default_rng(50505)
    comp0 = [rand_dna(rng, 300) for _ in range(3)]  # three haplotypes, no variant: not genotyped, no records, no mask bits
    haps, site = _multi_allele_site(rng, [("snv", 1), ("snv", 2), ("snv", 3), ("del", 4)])
    base = (9, 5, 3, 1, 7)
    depths = [tuple(base[(a + s) % 5] for a in range(5)) if s != 5 else (0,) * 5 for s in range(8)]  # sample 5 is silent
    depths[2] = (6, 0, 0, 0, 4)
    counts = _Counts(params, 1)
    roles = [0, 0, 0, 1, 1, 1, 1, 1]
    reads = _allele_reads(rng, haps, depths, counts, 0, 0, site["ref_start"], roles)
    win = dict(ref=np.frombuffer(haps[0], np.uint8).copy(), reads=reads)
    return _finish(params, [win], [dict(comps=[comp0, haps], vars=[dict(site, comp=1)])], counts)


def _seven_alleles():
    params = capi.default_params(min_k=25, max_k=25, num_samples=3, max_alts=6, case_ctrl_mode=0)
    rng = np.random.default_rng(70707)
    haps, site = _multi_allele_site(rng, [("snv", 1), ("snv", 2), ("snv", 3), ("del", 1), ("del", 2), ("ins", 3)])
    depths = [(8, 3, 2, 1, 4, 2, 5), (5, 0, 6, 2, 0, 3, 1), (2, 4, 1, 3, 2, 6, 3)]
    counts = _Counts(params, 1)
    reads = _allele_reads(rng, haps, depths, counts, 0, 0, site["ref_start"])
    win = dict(ref=np.frombuffer(haps[0], np.uint8).copy(), reads=reads)
    return _finish(params, [win], [dict(comps=[haps], vars=[dict(site, comp=0)])], counts)


def _one_sample():
    params = capi.default_params(min_k=25, max_k=25, num_samples=1)
    rng = np.random.default_rng(1001)
    win, spec, who = _plain_window(rng, 37, layout=[(int(i % 3 == 0), 0, 1, bool(i & 1)) for i in range(37)])
    counts = _Counts(params, 1)
    _count_who(counts, 0, who)
    return _finish(params, [win], [spec], counts)


def _small_strides():
    """max_vars = 10: the byte-wise branch of k_assign's fill; max_alts = 2 with a three-allele site"""
    params = capi.default_params(min_k=25, max_k=25, max_vars=10, max_alts=2)
    rng = np.random.default_rng(2002)
    haps, site = _multi_allele_site(rng, [("snv", 1), ("snv", 3)])
    counts = _Counts(params, 1)
    reads = _allele_reads(rng, haps, [(7, 4, 2), (3, 5, 6)], counts, 0, 0, site["ref_start"], roles=[0, 1])
    win = dict(ref=np.frombuffer(haps[0], np.uint8).copy(), reads=reads)
    return _finish(params, [win], [dict(comps=[haps], vars=[dict(site, comp=0)])], counts)


def _solor_shapes():
    """case/control QUAL (SOLOR) over eight samples: [(sample, role, REF reads, ALT reads)] per window"""
    params = capi.default_params(min_k=25, max_k=25, num_samples=8, case_ctrl_mode=1)
    rng = np.random.default_rng(3003)
    shapes = [
        # three controls with evidence, two case samples: QUAL is the larger of the two SOLOR values
        [(0, 0, 9, 1), (1, 0, 7, 0), (2, 0, 5, 2), (4, 1, 6, 3), (6, 1, 2, 8)],
        # no control with evidence (cc = 1)
        [(3, 1, 4, 5), (7, 1, 6, 2)],
        # a case sample without ALT reads beside one with
        [(0, 0, 8, 1), (5, 1, 7, 0), (6, 1, 3, 4)],
        # a sample with reads of both roles counts as a case
        [(1, 0, 6, 1), (2, 0, 4, 1), (2, 1, 2, 3), (3, 0, 5, 0)],
    ]
    parts = []
    for w, shape in enumerate(shapes):
        layout = []
        for sample, role, n_ref, n_alt in shape:
            layout += [(0, sample, role, bool(i & 1)) for i in range(n_ref)] + [(1, sample, role, bool(i & 1)) for i in range(n_alt)]
        layout = [layout[i] for i in rng.permutation(len(layout))]
        parts.append(_plain_window(rng, len(layout), qname0=1000 * w, layout=layout))
    counts = _Counts(params, len(parts))
    for w, (_, _, who) in enumerate(parts):
        _count_who(counts, w, who)
    return _finish(params, [x[0] for x in parts], [x[1] for x in parts], counts)


# ---- score_at_variant's walk -------------------------------------------------------------------------------------------
def _region_edges():
    """one site: REF (7 bases), a 6-base deletion (1 base) and a 9-base insertion (16 bases).  30 reads of each haplotype;
    reads with a 2-base deletion or a 3-base insertion of their own at each of 12 offsets from 2 before the REF region to 2
    behind it; reads that begin, and reads that end, at each of 14 offsets across it; Phred from EDGE_PHRED"""
    params = capi.default_params(min_k=25, max_k=25)
    rng = np.random.default_rng(4004)
    haps, site = _multi_allele_site(rng, [("del", 6), ("ins", 9)])
    pos = site["ref_start"]
    reads = []

    def put(seq):
        i = len(reads)
        reads.append(_read(seq, rng.choice(EDGE_PHRED, len(seq)), i, i & 1, i & 1, bool(i & 2)))

    for h in range(3):
        for _ in range(30):
            st = pos - int(rng.integers(30, 120))
            put(haps[h][st:st + 150])
    for h in range(3):
        for off in range(-2, 10):
            at = pos + off
            src = haps[h]
            put((src[:at] + src[at + 2:])[at - 70:at + 80])                     # its own 2-base deletion at `at`
            put((src[:at] + rand_dna(rng, 3) + src[at:])[at - 70:at + 80])      # its own 3-base insertion before `at`
    for h in range(3):
        for off in range(-3, 11):
            put(haps[h][pos + off:pos + off + 150])     # begins at pos + off
            put(haps[h][pos + off - 149:pos + off + 1])  # ends on pos + off
    win = dict(ref=np.frombuffer(haps[0], np.uint8).copy(), reads=reads)
    return _finish(params, [win], [dict(comps=[haps], vars=[dict(site, comp=0)])], None)


def _clipped_ends():
    """an SNV 8 bases from the haplotypes' left end and a 2-base deletion 12 bases from their right end; reads hang over either
    end by 0 ... 60 foreign bases (overhang is the canonical aligner's only source of S operations)"""
    params = capi.default_params(min_k=25, max_k=25)
    rng = np.random.default_rng(5005)
    L = 330
    ref = bytearray(rand_dna(rng, L))
    dpos = L - 12 - 2  # the two deleted bases; the anchor before them
    for x in range(dpos - 1, dpos + 4):
        while ref[x] == ref[x - 1]:
            ref[x] = _other(ref[x])
    ref = bytes(ref)
    alt = _sub(ref, 8)
    alt = alt[:dpos] + alt[dpos + 2:]
    hap = (ref, alt)
    reads = []
    for h in range(2):
        for over in (0, 1, 5, 9, 12, 20, 35, 60):
            i = len(reads)
            reads.append(_read(rand_dna(rng, over) + hap[h][:150 - over], rng.choice(EDGE_PHRED[2:], 150), i, i & 1, i & 1, bool(i & 2)))
            reads.append(_read(hap[h][len(hap[h]) - (150 - over):] + rand_dna(rng, over), rng.choice(EDGE_PHRED[2:], 150), i + 1,
                               i & 1, i & 1, bool(i & 2)))
    win = dict(ref=np.frombuffer(ref, np.uint8).copy(), reads=reads)
    spec = dict(comps=[[ref, alt]], vars=[_snv(0, 8), dict(comp=0, ref_start=dpos - 1, ref_len=3, alts=[(1, {1: dpos - 1})])])
    return _finish(params, [win], [spec], None)


def _first_wins():
    """two ALT haplotypes carry the same allele and differ only 400 bases from the site, out of every read's reach: the two
    combined scores of an ALT read tie and the lower haplotype wins (HSE sees which one did)"""
    params = capi.default_params(min_k=25, max_k=25)
    rng = np.random.default_rng(6006)
    ref = rand_dna(rng, 760)
    alt1 = _sub(ref, 200)
    alt2 = _sub(alt1, 620)
    alt3 = _sub(_sub(ref, 200, 2), 630)  # a second allele on a haplotype of its own: HSE has something to spread over
    haps = [ref, alt1, alt2, alt3]
    counts = _Counts(params, 1)
    reads = []
    for i in range(36):
        h = (0, 1, 2, 3)[i % 4]
        st = int(rng.integers(70, 190))
        rev, sample = bool(i & 4), (i >> 3) & 1
        reads.append(_read(haps[h][st:st + 150], rng.integers(10, 42, 150), i, sample, sample, rev))
        counts.add(0, 0, sample, (0, 1, 1, 2)[h], rev)
    win = dict(ref=np.frombuffer(ref, np.uint8).copy(), reads=reads)
    spec = dict(comps=[haps], vars=[dict(comp=0, ref_start=200, ref_len=1, alts=[(1, {1: 200, 2: 200}), (1, {3: 200})])])
    return _finish(params, [win], [spec], counts)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "dense_over":
        return _dense(9101, 160, 60, 4)                  # 9600 keys
    if name == "dense_exact":
        return _dense(9102, 128, 64, 3)                  # 8192 keys
    if name == "dense_exact_plus_one":
        return _dense(9102, 128, 64, 3, extra=True)      # 8193 keys
    if name == "dense_among_others":
        return _dense_among_others()
    if name == "dedup":
        return _dedup()
    if name == "five_alleles":
        return _five_alleles(0)
    if name == "five_alleles_case_control":
        return _five_alleles(1)
    if name == "seven_alleles":
        return _seven_alleles()
    if name == "one_sample":
        return _one_sample()
    if name == "small_strides":
        return _small_strides()
    if name == "solor_shapes":
        return _solor_shapes()
    if name == "region_edges":
        return _region_edges()
    if name == "clipped_ends":
        return _clipped_ends()
    if name == "first_wins":
        return _first_wins()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle_genotype(name):
    """the oracle's genotype stage over the case, taps included: computed once per process, never modified"""
    from harness import OracleEngine
    c = case(name)
    return OracleEngine(c.params).genotype(c.arrs, c.n, c.nr, c.asm, c.var)


def key_count(c, geno):
    """(read, variant) pairs that file an evidence key: assigned, and of a sample the call counts"""
    assigned = geno["asg_allele"].reshape(c.nr, c.params.max_vars) != 255
    return int(assigned[np.asarray(c.arrs["read_sample"][:c.nr]) < c.params.num_samples].sum())


@functools.lru_cache(maxsize=None)
def stats_reference(name):
    """tests/format_stats_ref.py over the oracle's taps of the case (it walks any comp_hap0 and any K as it is)"""
    import format_stats_ref as ref
    c, taps = case(name), oracle_genotype(name)
    want = ref.format_stats(c.params, c.arrs, c.n, c.asm, c.var, taps["aln_rec"], taps["aln_cigar"])
    assert np.array_equal(want["allele_counts"], taps["allele_counts"]), name  # the reference's depths are the oracle's
    return want
