"""The cases tests/test_gpu_format_meta.py runs and tests/test_format_meta_ref.py guards: inputs of the genotype stage
(tests/scoring_cases.py: hand-made assembly and variant arrays) plus the four read-metadata arrays of ma_read_meta_t, and the
expected statistics -- tests/format_meta_ref.py over the ORACLE's alignment taps, computed once per process, never modified.

  * the STATS cases of tests/scoring_cases.py and its region_edges / clipped_ends windows, with metadata drawn from a fixed
    seed: mates that share a name get different metadata (dedup: only the first read counts), eight samples and five alleles
    (five_alleles), a variant start before the alignment start and inside a deletion of the winning CIGAR (region_edges), soft-
    clipped winning alignments (clipped_ends);
  * positions: reads of 100 and 150 bases placed so that the variant falls on chosen query positions -- ties across the two
    lengths (50/100 = 75/150, 30/100 = 45/150) and mirror pairs of the 1/3 against 2/3 kind (50 and 100 of 150);
  * shapes (one sample): a REF-only and an ALT-only cell, exactly 2 and exactly 3 ALT reads, all ALT starts in one 3-base bin,
    more than 20 distinct bins, all MAPQ equal;
  * sort_fit: k_evid_stats sorts a cell's keys (one per evidence read, one more per ALT read) in LDS up to 2048 of them: a window
    that files exactly 2048 and one that files 2049, 100-base reads, one variant.

The variant start can not lie beyond the END of the winning alignment: AssignReadToAlleles only scores alignments that overlap
the variant (genotyper.cpp:360-362: var_start < aln_ref_end).  That branch of CigarRefPosToQueryPos is pinned on the CPU
(tests/test_format_meta_ref.py).  (A CIGAR cut at max_cigar can end before the variant, but its window is flagged
MA_W_CIGAR_OVERFLOW and flagged windows have no expected values: tests/test_gpu_parity.py compares every OTHER window.)"""
import collections
import functools

import numpy as np

from lancet2_amd import capi
from pin_cases import rand_dna

import format_meta_ref as mref
import scoring_cases as sc

MetaCase = collections.namedtuple("MetaCase", "params arrs n nr asm var meta")

SEEDED = sc.STATS + ("region_edges", "clipped_ends")
HANDMADE = ("positions", "shapes", "sort_fit")
NAMES = SEEDED + HANDMADE
SORT_CAP = 2048  # kEvSortCap (lancet2_amd/csrc/evidence.h)
ISIZES = (-480, -150, 0, 0, 151, 320, 700)


def random_meta(seed, nr):
    rng = np.random.default_rng(seed)
    return dict(read_mapq=rng.integers(0, 61, nr).astype(np.uint8), read_mflags=rng.integers(0, 4, nr).astype(np.uint8),
                read_isize=rng.choice(ISIZES, nr).astype(np.int32), read_start=rng.integers(0, 400, nr).astype(np.int32))


def _positions():
    params = capi.default_params(min_k=25, max_k=25)
    rng = np.random.default_rng(8801)
    ref = rand_dna(rng, 560)
    pos = 280
    hap = (ref, sc._sub(ref, pos))
    reads = []
    for length, places in ((150, (50, 100, 75, 45, 105, 10, 140, 25, 125, 60, 90)), (100, (50, 30, 70, 10, 90, 25, 75, 40, 60))):
        for q in places:
            for h in (0, 1):
                for sample in (0, 1):
                    i = len(reads)
                    reads.append(sc._read(hap[h][pos - q:pos - q + length], rng.integers(20, 42, length), i, sample, sample, bool(i & 4)))
    win = dict(ref=np.frombuffer(ref, np.uint8).copy(), reads=reads)
    c = sc._finish(params, [win], [dict(comps=[list(hap)], vars=[sc._snv(0, pos)])], None)
    return c, random_meta(8802, c.nr)


def _shapes():
    params = capi.default_params(min_k=25, max_k=25, num_samples=1)
    rng = np.random.default_rng(8811)
    # (REF reads, ALT reads) per window
    shapes = [(6, 0), (0, 5), (4, 2), (4, 3), (10, 30), (8, 8)]
    parts = []
    for w, (n_ref, n_alt) in enumerate(shapes):
        layout = [(0, 0, 1, bool(i & 1)) for i in range(n_ref)] + [(1, 0, 1, bool(i & 1)) for i in range(n_alt)]
        parts.append(sc._plain_window(rng, len(layout), qname0=1000 * w, layout=layout))
    c = sc._finish(params, [x[0] for x in parts], [x[1] for x in parts], None)
    meta = random_meta(8812, c.nr)
    off = [int(x) for x in c.arrs["read_win_off"]]
    meta["read_start"][off[3] + 4:off[4]] = (300, 301, 302)                     # three ALT reads, one bin: FSSE = 0.0
    meta["read_start"][off[4] + 10:off[5]] = 3 * np.arange(30) + 1000           # 30 ALT reads, 30 bins
    meta["read_mapq"][off[5]:off[6]] = 37                                       # all MAPQ equal: MQCD = 0.0
    return c, meta


def _sort_fit():
    """keys = evidence reads + ALT reads: 1024 REF + 512 ALT = 2048, and one REF read more"""
    params = capi.default_params(min_k=25, max_k=25, num_samples=1)
    rng = np.random.default_rng(8821)
    parts = []
    for w, n_ref in enumerate((SORT_CAP // 2, SORT_CAP // 2 + 1)):
        ref = rand_dna(rng, 420)
        hap = (ref, sc._sub(ref, 210))
        reads = []
        for i in range(n_ref + SORT_CAP // 4):
            h = int(i >= n_ref)
            st = 210 - int(rng.integers(10, 90))  # (the site well inside every read: each one is assigned)
            reads.append(sc._read(hap[h][st:st + 100], 30, 10000 * w + i, 0, 1, bool(i & 1)))
        reads = [reads[i] for i in rng.permutation(len(reads))]
        parts.append((dict(ref=np.frombuffer(ref, np.uint8).copy(), reads=reads), dict(comps=[list(hap)], vars=[sc._snv(0, 210)])))
    c = sc._finish(params, [x[0] for x in parts], [x[1] for x in parts], None)
    return c, random_meta(8822, c.nr)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in SEEDED:
        c = sc.case(name)
        meta = random_meta(7000 + SEEDED.index(name), c.nr)
    elif name == "positions":
        c, meta = _positions()
    elif name == "shapes":
        c, meta = _shapes()
    elif name == "sort_fit":
        c, meta = _sort_fit()
    else:
        raise KeyError(name)
    return MetaCase(c.params, c.arrs, c.n, c.nr, c.asm, c.var, meta)


@functools.lru_cache(maxsize=None)
def oracle_taps(name):
    if name in SEEDED:
        return sc.oracle_genotype(name)
    from harness import OracleEngine
    c = case(name)
    return OracleEngine(c.params).genotype(c.arrs, c.n, c.nr, c.asm, c.var)


@functools.lru_cache(maxsize=None)
def reference(name):
    """tests/format_meta_ref.py over the oracle's taps of the case"""
    c, taps = case(name), oracle_taps(name)
    want = mref.meta_stats(c.params, c.arrs, c.n, c.asm, c.var, taps["aln_rec"], taps["aln_cigar"], c.meta)
    assert np.array_equal(want["allele_counts"], taps["allele_counts"]), name  # the reference's depths are the oracle's
    return want


def compare_meta(got, want, what):
    """integers exact, NaN positions identical, f64 within 1e-9 * max(1, |want|); prints the largest error of every array"""
    bad = []
    for key in ("ev_meta", "ev_rpcd", "fmt_rmq", "fmt_mstat"):
        if key not in got:
            continue
        g, x = got[key], want[key]
        if key.startswith("ev_"):
            print(f"{what} {key}: {int((g != x).sum())} of {len(x)} differ")
            if not np.array_equal(g, x):
                i = np.nonzero(g != x)[0][:6]
                bad.append(f"{key} differs at {i.tolist()}: got {g[i].tolist()} want {x[i].tolist()}")
            continue
        if not np.array_equal(np.isnan(g), np.isnan(x)):
            i = np.nonzero(np.isnan(g) != np.isnan(x))[0][:6]
            bad.append(f"{key} NaN positions differ at {i.tolist()}: got {g[i].tolist()} want {x[i].tolist()}")
            continue
        ok = ~np.isnan(x)
        err = np.abs(g[ok] - x[ok]) / np.maximum(1.0, np.abs(x[ok]))
        print(f"{what} {key}: max scaled error {err.max() if err.size else 0.0:.3e} over {int(ok.sum())} values")
        if err.size and not err.max() <= 1e-9:
            i = np.nonzero(ok)[0][np.argsort(-err)[:6]]
            bad.append(f"{key} off at {i.tolist()}: got {g[i].tolist()} want {x[i].tolist()}")
    return bad
