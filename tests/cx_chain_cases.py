"""Inputs of tests/test_gpu_cx_chain.py, guarded on the CPU by tests/test_cx_chain_cases.py.

(a) chain_case(): a synthetic batch like that of tests/test_gpu_format_meta.py (C1, six windows, k = 25) with seeded read
    metadata and its packed form, and the ORACLE's chain over it (assembly, variants, annotation at two GC fractions).
(b) hap_lq_groups(): hand-made assembly and variant arrays for the annotation stage alone, one window per case, chosen for
    k_hap_lq (LongdustQ, k = 7, of a component's REF haplotype): lengths around the first k-mer and around one trip of its 256
    threads, a haplotype that fills its slot, counts that meet in one LDS word, lists just under the cap, bases that are no
    k-mer, windows and components without a variant.  Computed once per process and never modified."""
import collections
import functools

import numpy as np

from lancet2_amd import capi, synth

import meta_stats_cases as mcases
from harness import OracleEngine, handmade_annotation_case, handmade_genotype_case

CHAIN_WINDOWS = 6
CHAIN_FIRST_INDEX = 930  # (from 900, where that test's batch starts, every window has a variant; from 930 window 3 has none)
GC_FRACS = (0.41, 0.30)
HAP_K = 7          # kHapK (lancet2_amd/csrc/annotate.hip)
LIST_CAP = 2048    # kListCap

ChainCase = collections.namedtuple("ChainCase", "params arrs meta packed n nr asm var cx")
LqGroup = collections.namedtuple("LqGroup", "name params names asm var n")


@functools.lru_cache(maxsize=None)
def chain_case():
    params = capi.default_params(min_k=25, max_k=25)
    arrs, n, nr = synth.make_config_batch("C1", CHAIN_WINDOWS, first_index=CHAIN_FIRST_INDEX)
    meta = mcases.random_meta(4242, nr)
    packed, twin = capi.pack_reads(arrs)
    assert all(np.array_equal(twin[k], arrs[k]) for k in ("read_bases", "read_quals"))  # (ACGT only: the same batch)
    orc = OracleEngine(params)
    asm = orc.assemble(arrs, n, nr)
    var = orc.msa(arrs, n, nr, asm)
    cx = {gc: orc.annotate(arrs, n, nr, asm, var, gc) for gc in GC_FRACS}
    return ChainCase(params, arrs, meta, packed, n, nr, asm, var, cx)


def used_slots(params, win_nvars):
    """[n * max_vars] bool: the variant slots the windows use"""
    return (np.arange(params.max_vars)[None, :] < np.asarray(win_nvars)[:, None]).reshape(-1)


# ---- (b) ---------------------------------------------------------------------------------------------------------------
def _rand(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _other(base):
    return "C" if base.upper() != "C" else "G"


def _snv_case(ref, pos=None):
    """a one-component window: `ref` and a haplotype that differs from it in one base"""
    pos = len(ref) // 2 if pos is None else pos
    alt = ref[:pos] + _other(ref[pos]) + ref[pos + 1:]
    return dict(haps=[ref, alt], ref_pos=pos, ref_len=1, alts=[(1, {1: pos})])


def distinct_kmer_unit(rng, n, k=HAP_K):
    """n bases none of whose k-mers occurs twice, the k - 1 that wrap round to the start included (a random walk that steps
    round k-mers it has seen): doubled, every one of its k-mers is counted exactly twice"""
    for _ in range(64):
        seq, seen = list(_rand(rng, k - 1)), set()
        while len(seq) < n:
            for b in rng.permutation(4):
                kmer = "".join(seq[-(k - 1):]) + "ACGT"[b]
                if kmer not in seen:
                    seen.add(kmer)
                    seq.append("ACGT"[b])
                    break
            else:
                break  # a dead end: start again
        if len(seq) < n:
            continue
        unit = "".join(seq)
        wrap = unit[-(k - 1):] + unit[:k - 1]
        extra = [wrap[i:i + k] for i in range(k - 1)]
        if len(set(extra)) == len(extra) and not seen & set(extra):
            return unit
    raise AssertionError("no unit found")


def kmer_counts(seq, k=HAP_K):
    """[4^k] occurrences of every k-mer of ACGT (either case) in seq, as LongdustQ counts them: in numpy, from the sequence"""
    code_of = np.full(256, 4, np.int64)
    for i, ch in enumerate("ACGT"):
        code_of[ord(ch)] = code_of[ord(ch.lower())] = i
    b = code_of[np.frombuffer(seq.encode(), np.uint8)]
    if len(b) < k:
        return np.zeros(4 ** k, np.int64)
    win = np.lib.stride_tricks.sliding_window_view(b, k)
    ok = (win < 4).all(axis=1)
    codes = (win[ok] * (4 ** np.arange(k - 1, -1, -1))).sum(axis=1)
    return np.bincount(codes, minlength=4 ** k)


def _single_cases():
    rng = np.random.default_rng(7301)
    cag = "CAG" * 100
    two_bins = _rand(rng, 60) + "A" * 12 + "C" + _rand(rng, 40) + "G" + "A" * 7 + "C" + _rand(rng, 40) + "G" + "A" * 7 + "C" + _rand(rng, 60)
    scattered = list(_rand(rng, 500) + "CAG" * 20)
    for i in range(11, len(scattered), 37):
        scattered[i] = "N"
    default = [("len6", _snv_case("ACGTAC", 2)), ("len7", _snv_case("ACGTACG", 3)), ("len8", _snv_case("AAAAAAAA", 4)),
               ("len262", _snv_case(cag[:262])), ("len263", _snv_case(cag[:263])), ("len264", _snv_case(cag[:264])),
               ("exact_fit", _snv_case(((_rand(rng, 700) + "CAG" * 40) * 3)[:2048])),
               ("homopolymer", _snv_case("A" * 2048, 1000)), ("two_bins_one_word", _snv_case(two_bins, 30)),
               ("ac_repeat", _snv_case("AC" * 150, 151)), ("scattered_n", _snv_case("".join(scattered), 250)),
               ("all_n", _snv_case("N" * 300, 150)), ("lower_case", _snv_case((_rand(rng, 200) + "CAG" * 30).lower(), 100))]
    unit = distinct_kmer_unit(rng, 2000)
    long_ = [("doubled_unit", _snv_case(unit + unit, 3000)), ("long_homopolymer", _snv_case("T" * 4096, 2000)),
             ("long_mixed", _snv_case(_rand(rng, 1500) + "CAG" * 300 + _rand(rng, 1500), 1700))]
    return default, long_


def _multi_windows():
    """three components with variants only in the middle one; then a window without a variant between two that have some"""
    rng = np.random.default_rng(7302)

    def comp(ref):
        pos = len(ref) // 2
        return [ref.encode(), (ref[:pos] + _other(ref[pos]) + ref[pos + 1:]).encode()], pos

    refs = [_rand(rng, 300) + "CAG" * 30, "AC" * 80 + _rand(rng, 200), _rand(rng, 150) + "T" * 40 + _rand(rng, 150),
            "GA" * 100 + _rand(rng, 120), _rand(rng, 400), "CCG" * 50 + _rand(rng, 200)]
    comps = [comp(r) for r in refs]

    def snv(c, pos):
        return dict(comp=c, ref_start=pos, ref_len=1, alts=[(1, {1: pos})])

    return [dict(comps=[comps[0][0], comps[1][0], comps[2][0]], vars=[snv(1, comps[1][1]), snv(1, comps[1][1] + 9)]),
            dict(comps=[comps[3][0]], vars=[snv(0, comps[3][1])]),
            dict(comps=[comps[4][0]], vars=[]),
            dict(comps=[comps[5][0], comps[0][0]], vars=[snv(0, comps[5][1]), snv(1, comps[0][1])])]


@functools.lru_cache(maxsize=None)
def hap_lq_groups():
    default, long_ = _single_cases()
    groups = []
    for name, params, cases in (("default", capi.default_params(min_k=25, max_k=25), default),
                                ("long", capi.default_params(min_k=25, max_k=25, max_hap_len=4096), long_)):
        asm, var = handmade_annotation_case(params, [c for _, c in cases])
        groups.append(LqGroup(name, params, tuple(k for k, _ in cases), asm, var, len(cases)))
    params = capi.default_params(min_k=25, max_k=25)
    wins = _multi_windows()
    asm, var = handmade_genotype_case(params, wins)
    groups.append(LqGroup("multi", params, ("middle_component", "before_empty", "empty", "after_empty"), asm, var, len(wins)))
    return tuple(groups)


def ref_haplotype(group, name):
    """the REF haplotype of the (single) component of a one-component case"""
    w = group.names.index(name)
    hi = w * group.params.max_haps
    L = int(group.asm["hap_len"][hi])
    return bytes(group.asm["hap_bases"][hi * group.params.max_hap_len: hi * group.params.max_hap_len + L]).decode()


def group_batch(group):
    """the batch arrays ma_annotate_batch wants: only the window count is read"""
    return dict(ref_off=np.zeros(group.n + 1, np.uint32), read_win_off=np.zeros(group.n + 1, np.uint32))


@functools.lru_cache(maxsize=None)
def hap_lq_reference(gc_frac=0.41):
    """group name -> the oracle's annotation of the group"""
    return {g.name: OracleEngine(g.params).annotate(group_batch(g), g.n, 0, g.asm, g.var, gc_frac) for g in hap_lq_groups()}
