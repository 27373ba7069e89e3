"""The caller's eight output caps (ma_params_t: max_comps, max_haps, max_hap_len, max_runs, max_vars, max_alts,
max_allele_bytes, max_cigar) at exact fit and one under the need: the case table of tests/test_gpu_caps.py, guarded on the CPU
by tests/test_cap_cases.py.  Inputs and needs only -- nothing here looks at either implementation's internals.

DESIGN section 7 promises that a window over a cap is flagged (MA_W_HAP_OVERFLOW for max_comps / max_haps, MA_W_LEN_OVERFLOW for
max_hap_len / max_runs, MA_W_VAR_OVERFLOW for max_vars / max_alts / max_allele_bytes, MA_W_CIGAR_OVERFLOW for max_cigar), that
it is flagged exactly when the oracle flags it, and that a window that fits equals the oracle bit for bit.

Batches (at most 12 windows of at most 1001 bases, 30x / 30x, a few thousand reads):

  reads   built from reads, for the four assembly caps: a window that does not assemble at k = 25 (needs nothing), three
          variant-dense C2 windows (components of 3 and 5 haplotypes), two dense C2 windows (run counts and haplotype lengths
          spread), a plain C2 window, a C4 window with a 50-base insertion and deletion at 30x, and four tiled windows
          (tiled_window below):
            alt_heavier      one SNV, the ALT haplotype three times as deep as REF: the oracle's sorted walks are "kept ALT, then
                             the walk that spells the REF anchor" -- 2 haplotypes with a dropped walk BEHIND the last kept one
            ref_heavier      the same with REF the deeper one: the REF-equal walk comes first
            two_alt_heavier  two ALT haplotypes (an SNV and, 10 bases on, a one-base insertion: one bubble holds the three of
                             them) both deeper than REF: 3 haplotypes, the REF-equal walk last, and the longest haplotype one
                             base longer than the other tiled windows' (601 against 600)
            two_islands      reads over the two ends of the window only, an SNV in each: two components of 2 haplotypes, so
                             that max_comps has a window one over and max_haps a cap that falls in the second component
  cigar   the indel-dense C2 windows of test_truncated_cigars_are_flagged_not_silent (every one of them has a CIGAR of 7
          operations), and the plain, the first variant-dense and the alt_heavier window again (4, 5 and 1)
  poa     hand-made components (harness.handmade_poa_case, the builders of tests/poa_cases.py) for the three variant caps: one
          site with 1, 2, 3 and 4 ALT alleles, windows of 6, 7 and 8 SNVs, two 60-base insertions (124 pool bytes), one of 62 and
          one of 63 bases (64 and 65: the parameter check refuses max_allele_bytes < 64), and a window of two components
          (3 + 4 variants) so that max_vars can fall inside the second one

needs(batch): what every window needs of every cap, from ONE run of the oracle under roomy caps (ROOMY).  tight_values(cap):
the distinct need values of the cap's batch that the parameter check admits (api.hip: max_comps >= 1, max_haps 2 .. 32,
max_hap_len >= 256, max_runs >= 8, max_alts 1 .. 15, max_allele_bytes >= 64, max_cigar 4 .. 64), thinned to at most six
(first the values with a window one over, then the smallest, the largest and the ones around the median).  The tight
parameter set of (cap, c) is the roomy set with that cap alone set to c, so that a context holds windows below the cap, at
exact fit and over it side by side.

max_comps: two_islands has two components, every other window one or none, so max_comps = 1 holds exact fits, one window one
over and one below.  max_runs is the one cap without a context that holds an exact fit AND a window exactly one over: a
haplotype's runs are the nodes of its walk, and those come in steps (a tiled window with one variant has 14, with two 19 or 24;
the synthetic windows 22, 32, ...), so no two needs are neighbours.  The table adds ONE_UNDER["max_runs"], the commonest need
less one, where those windows are over by exactly one run, next to the set at that need itself, where they fit exactly.

max_cigar: the oracle keeps the whole operation count of every read x haplotype alignment in aln_cigar[.., 0] and cuts the
operations it stores (oracle/capi.cpp, orc_genotype_batch), but raises no flag of its own; the flag's definition is
include/microasm.h's (a CIGAR of more than max_cigar operations among the alignments the genotyper scores).  oracle_chain()
ORs MA_W_CIGAR_OVERFLOW into the status of the windows whose recorded operation count exceeds max_cigar -- from the oracle's
own records, under the same tight set."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import poa_cases as pc
from harness import OracleEngine, handmade_poa_case
from lancet2_amd import capi, synth
from pin_cases import rand_dna

ROOMY = dict(max_comps=16, max_haps=32, max_hap_len=4096, max_runs=1024, max_vars=128, max_alts=15, max_allele_bytes=8192,
             max_cigar=64)
CAP_BITS = capi.MA_W_HAP_OVERFLOW | capi.MA_W_LEN_OVERFLOW | capi.MA_W_VAR_OVERFLOW | capi.MA_W_CIGAR_OVERFLOW
# cap -> (key of needs(), the flag of a window over it, the batch, the values the parameter check admits)
CAPS = {
    "max_comps": ("comps", capi.MA_W_HAP_OVERFLOW, "reads", (1, 1 << 20)),
    "max_haps": ("slots", capi.MA_W_HAP_OVERFLOW, "reads", (2, 32)),
    "max_hap_len": ("hap_len", capi.MA_W_LEN_OVERFLOW, "reads", (256, 1 << 20)),
    "max_runs": ("runs", capi.MA_W_LEN_OVERFLOW, "reads", (8, 1 << 20)),
    "max_vars": ("vars", capi.MA_W_VAR_OVERFLOW, "poa", (1, 1 << 20)),
    "max_alts": ("alts", capi.MA_W_VAR_OVERFLOW, "poa", (1, 15)),
    "max_allele_bytes": ("pool", capi.MA_W_VAR_OVERFLOW, "poa", (64, 1 << 20)),
    "max_cigar": ("cigar", capi.MA_W_CIGAR_OVERFLOW, "cigar", (4, 64)),
}
MAX_TIGHT_SETS = 6


def params(**caps):
    kw = dict(ROOMY, min_k=25, max_k=25)
    kw.update(caps)
    return capi.default_params(**kw)


# ---- tiled windows ----
TILE, READ_LEN = 10, 150


def tiled_window(ref, haplotypes):
    """A window whose reads are error-free 150-base tiles of the given haplotypes, one every 10 bases, strands alternating:
    haplotypes = [(haplotype bytes, copies, sample, role)] or (..., role, offset) for a haplotype that starts `offset` bases
    into the window.  Returns synth.make_window()'s dict, so synth.pack_batch takes it."""
    reads, name = [], 0
    for hap in haplotypes:
        seq, copies, sample, role = hap[:4]
        off = hap[4] if len(hap) > 4 else 0
        b = np.frombuffer(bytes(seq), np.uint8)
        for _ in range(copies):
            for i, s in enumerate(range(0, len(b) - READ_LEN + 1, TILE)):
                reads.append(dict(seq=b[s:s + READ_LEN].copy(), qual=np.full(READ_LEN, 37, np.uint8), qname=name, sample=sample,
                                  role=role, rev=bool(i & 1), passf=True, start=off + s, hint=off + s))
                name += 1
    reads.sort(key=lambda r: (0 if r["passf"] else 1, r["role"], r["sample"], r["qname"], r["start"]))
    return dict(ref=np.frombuffer(bytes(ref), np.uint8).copy(), reads=reads)


def _snv(ref, p, k=1):
    return pc.apply_edits(ref, [("snv", p, pc.other_base(ref[p], k))])


def _two_samples(hap, copies, off=0):
    return [(hap, copies, 0, 0, off), (hap, copies, 1, 1, off)]


def _tiled_windows():
    """-> {name: window}"""
    rng = np.random.default_rng(0xCA95)
    out = {}
    ref = rand_dna(rng, 600)
    alt = _snv(ref, 300)
    out["alt_heavier"] = tiled_window(ref, _two_samples(ref, 1) + _two_samples(alt, 3))
    out["ref_heavier"] = tiled_window(ref, _two_samples(ref, 3) + _two_samples(alt, 1))
    ref = rand_dna(rng, 600)
    while ref[309] == ref[310]:  # (an inserted copy of a neighbour could slide)
        ref = rand_dna(rng, 600)
    ins = pc.apply_edits(ref, [("ins", 310, bytes([next(x for x in b"ACGT" if x not in ref[309:311])]))])
    out["two_alt_heavier"] = tiled_window(ref, _two_samples(ref, 1) + _two_samples(_snv(ref, 300), 3) + _two_samples(ins, 3))
    ref = rand_dna(rng, 1001)
    left, right = ref[:400], ref[600:]
    out["two_islands"] = tiled_window(ref, _two_samples(left, 3) + _two_samples(_snv(left, 200), 3) +
                                      _two_samples(right, 3, 600) + _two_samples(_snv(right, 200), 3, 600))
    return out


TILED = ("alt_heavier", "ref_heavier", "two_alt_heavier", "two_islands")


@dataclass
class Batch:
    name: str
    arrs: dict
    n: int
    nr: int
    names: tuple       # a name per window
    asm: dict = None   # hand-made assembly buffers under the ROOMY strides (the poa batch); None: assembled from the reads


def _reads_batch():
    c2 = dict(synth.CONFIGS["C2"])
    wins, names = [], []
    for name, i in (("unassembled", 1200), ("very_dense_3", 1201), ("very_dense_5a", 1214), ("very_dense_5b", 1207)):
        wins.append(synth.make_window(i, **dict(c2, snv_rate=3e-2, indel_rate=4e-3)))
        names.append(name)
    for i in range(2):
        wins.append(synth.make_window(42_000 + i, **dict(c2, snv_rate=1e-2, indel_rate=2e-3)))
        names.append(f"dense_{i}")
    wins.append(_plain_window())
    names.append("plain")
    wins.append(synth.make_window(7, **dict(synth.CONFIGS["C4"], depths=(30, 30))))
    names.append("big_indel")
    tiled = _tiled_windows()
    for k in TILED:
        wins.append(tiled[k])
        names.append(k)
    arrs, n, nr = synth.pack_batch(wins)
    return Batch("reads", arrs, n, nr, tuple(names))


def _plain_window():
    return synth.make_window(500, **synth.CONFIGS["C2"])


def _cigar_batch():
    c2 = dict(synth.CONFIGS["C2"])
    wins = [synth.make_window(8800 + i, **dict(c2, indel_rate=1.5e-2, snv_rate=2e-3)) for i in range(4)]
    wins += [_plain_window(), synth.make_window(1201, **dict(c2, snv_rate=3e-2, indel_rate=4e-3)), _tiled_windows()["alt_heavier"]]
    arrs, n, nr = synth.pack_batch(wins)
    return Batch("cigar", arrs, n, nr, tuple(f"indel_dense_{i}" for i in range(4)) + ("plain", "very_dense_3", "alt_heavier"))


def _insertion(name, length, seed):
    """poa_cases._insertions with one insertion of `length` bases: 1 + (1 + length) pool bytes"""
    ref, alts = pc._draw_ref(seed, 1000, lambda r, g: [[("ins", 100, rand_dna(g, length))]])
    return pc.Window(name, [pc.Comp(ref, alts)])


def _poa_batch():
    two = [pc._snv_spread("unused_a", 3, 7101, 700, n_alts=2).comps[0], pc._snv_spread("unused_b", 4, 7102, 700, n_alts=2).comps[0]]
    two[1].anchor = pc.ANCHOR + 1000
    wins = [pc._out_degree(1, 7001), pc._out_degree(2, 7002), pc._out_degree(3, 7003), pc._ring(b"", 7004), pc._ring(b"N", 7005),
            pc._snv_spread("snv_6", 6, 7006, 700), pc._snv_spread("snv_7", 7, 7007, 700, n_alts=7), pc._snv_spread("snv_8", 8, 7008, 700, n_alts=4),
            pc._insertions("ins_2x60", 2, 7010), _insertion("ins_62", 62, 7011), _insertion("ins_63", 63, 7012),
            pc.Window("two_components_3_4", two)]
    n = len(wins)
    asm = handmade_poa_case(params(), [[(c.haps(), c.anchor) for c in w.comps] for w in wins])
    arrs, n2, nr = synth.make_config_batch("C1", n, first_index=77)
    assert n2 == n
    return Batch("poa", arrs, n, nr, tuple(w.name for w in wins), asm)


@lru_cache(maxsize=None)
def batch(name):
    b = {"reads": _reads_batch, "cigar": _cigar_batch, "poa": _poa_batch}[name]()
    for a in list(b.arrs.values()) + (list(b.asm.values()) if b.asm else []):
        a.setflags(write=False)
    return b


def fresh_asm(b, p):
    """the hand-made assembly buffers of a poa batch as a writable copy (the POA stage writes the window status); they are laid
    out with the ROOMY strides, which no tight set of a variant cap changes"""
    assert (p.max_comps, p.max_haps, p.max_hap_len, p.max_runs) == tuple(ROOMY[k] for k in ("max_comps", "max_haps", "max_hap_len", "max_runs"))
    return {k: np.array(v, copy=True) for k, v in b.asm.items()}


def _freeze(*dicts):
    for d in dicts:
        for a in d.values():
            a.setflags(write=False)


def _cigar_counts(p, b, geno):
    """-> per window the largest operation count the oracle recorded (0: no alignment)"""
    cnt = geno["aln_cigar"].reshape(b.nr, p.max_haps, 1 + p.max_cigar)[:, :, 0]
    rwo = b.arrs["read_win_off"]
    return np.array([int(cnt[rwo[w]:rwo[w + 1]].max()) if rwo[w + 1] > rwo[w] else 0 for w in range(b.n)])


@lru_cache(maxsize=None)
def oracle_chain(batch_name, cap=None, c=None):
    """-> (params, asm, var, geno) of the oracle on a batch under the roomy caps (cap None) or the tight set of (cap, c), read
    only.  geno has the per-call arrays; asm["win_status"] is the status after the three stages, MA_W_CIGAR_OVERFLOW derived from
    the oracle's own operation counts (module docstring)."""
    b = batch(batch_name)
    p = params(**({cap: c} if cap else {}))
    orc = OracleEngine(p)
    asm = fresh_asm(b, p) if b.asm else orc.assemble(b.arrs, b.n, b.nr)
    var = orc.msa(b.arrs, b.n, b.nr, asm)
    want_cigars = batch_name != "poa"  # (the reads of the poa batch belong to other haplotypes: nothing aligns)
    geno = orc.genotype(b.arrs, b.n, b.nr, asm, var, debug=want_cigars)
    if want_cigars:
        over = _cigar_counts(p, b, geno) > p.max_cigar
        asm["win_status"][over] |= np.uint32(capi.MA_W_CIGAR_OVERFLOW)
        geno = {k: v for k, v in geno.items() if k in ("allele_counts", "var_qual", "var_pl", "var_gq") or k == "aln_cigar"}
    _freeze(asm, var, geno)
    return p, asm, var, geno


@lru_cache(maxsize=None)
def needs(batch_name):
    """-> {key: int array per window}: components, haplotype slots, longest haplotype, most runs, variants, most ALT alleles,
    pool bytes, longest CIGAR -- what the window needs of each cap, from the oracle under ROOMY.  No window may be flagged there."""
    b = batch(batch_name)
    p, asm, var, geno = oracle_chain(batch_name)
    assert not (asm["win_status"] & CAP_BITS).any(), asm["win_status"].tolist()
    MC, MH, MV, MA = p.max_comps, p.max_haps, p.max_vars, p.max_alts
    out = {k: np.zeros(b.n, np.int64) for k in ("comps", "slots", "hap_len", "runs", "vars", "alts", "pool", "cigar")}
    for w in range(b.n):
        nc = int(asm["win_ncomp"][w])
        out["comps"][w] = nc
        slots = int(asm["comp_nhaps"][w * MC:w * MC + nc].sum())
        out["slots"][w] = slots
        if slots:
            out["hap_len"][w] = int(asm["hap_len"][w * MH:w * MH + slots].max())
            out["runs"][w] = int(asm["hap_nruns"][w * MH:w * MH + slots].max())
        nv = int(var["win_nvars"][w])
        out["vars"][w] = nv
        if nv:
            out["alts"][w] = int(var["var_nalts"][w * MV:w * MV + nv].max())
            out["pool"][w] = int(var["var_ref_len"][w * MV:w * MV + nv].sum()) + sum(
                int(var["alt_len"][(w * MV + v) * MA:(w * MV + v) * MA + int(var["var_nalts"][w * MV + v])].sum()) for v in range(nv))
    if "aln_cigar" in geno:
        out["cigar"] = _cigar_counts(p, b, geno).astype(np.int64)
    _freeze(out)
    return out


ONE_UNDER = {"max_runs": 13}  # (module docstring: 14 runs is the commonest need of the reads batch)


def tight_values(cap):
    """the values of `cap` the table runs: every distinct need of the cap's batch that the parameter check admits -- of more
    than MAX_TIGHT_SETS first those with a window exactly one over, then the smallest, the largest and the ones around the
    median -- and ONE_UNDER's"""
    key, _, bname, (lo, hi) = CAPS[cap]
    nd = {int(v) for v in needs(bname)[key]}
    vals = sorted(v for v in nd if lo <= v <= hi)
    if len(vals) > MAX_TIGHT_SETS:
        m = len(vals) // 2
        order = [v for v in vals if v + 1 in nd] + [vals[0], vals[-1]] + [vals[i] for d in range(len(vals)) for i in (m - d, m + d) if 0 <= i < len(vals)]
        vals = sorted(list(dict.fromkeys(order))[:MAX_TIGHT_SETS - (cap in ONE_UNDER)])
    if cap in ONE_UNDER:
        assert ONE_UNDER[cap] + 1 in nd and ONE_UNDER[cap] not in vals
        vals = sorted(vals + [ONE_UNDER[cap]])
    return tuple(vals)


def calls_of(p, var, geno, w):
    """-> per variant of window w its call-level results without their strides: (allele depths of the nalts + 1 alleles per
    sample and strand, the (nalts + 1)(nalts + 2) / 2 PLs per sample, GQ per sample, the bits of QUAL)"""
    MV, MA, S = p.max_vars, p.max_alts, p.num_samples
    NA, G = MA + 1, (MA + 1) * (MA + 2) // 2
    out = []
    for v in range(int(var["win_nvars"][w])):
        vi = w * MV + v
        K = int(var["var_nalts"][vi]) + 1
        ad = geno["allele_counts"][vi * S * NA * 2:(vi + 1) * S * NA * 2].reshape(S, NA, 2)[:, :K]
        pl = geno["var_pl"][vi * S * G:(vi + 1) * S * G].reshape(S, G)[:, :K * (K + 1) // 2]
        out.append((ad.tolist(), pl.tolist(), geno["var_gq"][vi * S:(vi + 1) * S].tolist(), int(geno["var_qual"][vi:vi + 1].view(np.uint64)[0])))
    return out


def tight_sets():
    """-> [(cap, c)] of the whole table"""
    return [(cap, c) for cap in CAPS for c in tight_values(cap)]


def most_exact_fits(cap):
    """the tight value of `cap` that the most windows of its batch need exactly"""
    key, _, bname, _ = CAPS[cap]
    nd = needs(bname)[key]
    return max(tight_values(cap), key=lambda c: (int((nd == c).sum()), -c))


def walk_dispositions(batch_name, w):
    """-> per component of window w the oracle's string of walk fates in MinWeight order: K kept, r equals the REF anchor, d
    duplicate (orc_walk_dispositions)"""
    import ctypes as C
    b = batch(batch_name)
    p = params()
    orc = OracleEngine(p)
    buf = C.create_string_buffer(4096)
    bs = capi.make_batch_struct(b.arrs, b.n, b.nr)
    nc = orc.lib.orc_walk_dispositions(C.byref(p), C.byref(bs), int(w), buf, len(buf))
    assert nc >= 0
    lines = buf.value.decode().split("\n")[:-1]
    assert len(lines) == nc
    return lines
