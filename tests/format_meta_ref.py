"""Independent reference of the six read-metadata FORMAT statistics (ma_genotype_meta_batch): RMQ, MQCD, SCA, FLD, RPCD and
FSSE, in plain Python.  It shares no code with oracle/ or the product.

Input: a batch, the assembly and variant arrays, the ORACLE's alignment taps (aln_rec, aln_cigar) and the four per-read
metadata arrays (ma_read_meta_t).  tests/format_stats_ref.py gives the winning haplotype and allele of every (read, variant)
and the evidence reads; this file adds, per evidence read and in the reference's order (citations are to the reference tree):

  * the folded position (caller/combined_scorer.cpp:96-105, hts/cigar_utils.h:104-139): qpos of the variant's start in the
    winning CIGAR, x = qpos / read length as a Python float (an IEEE double, like the reference's f64), min(x, 1.0 - x);
  * RMQ (caller/variant_support.cpp:184-194), MQCD and RPCD (base/mann_whitney.h:127-225: Python floats are sorted, as the
    reference sorts doubles), SCA (:261-279), FLD (:49-51, variant_support.h:361-387) and FSSE (variant_support.h:391-411,
    variant_support.cpp:358-363).

It also returns the integer tallies the engine writes to ev_meta / ev_rpcd.  tests/test_format_meta_ref.py pins this file
to closed forms and scipy before the GPU test trusts it."""
import math

import numpy as np

import format_stats_ref as ref

MA_RM_SOFTCLIP, MA_RM_PROPER = 1, 2
META_DTYPES = dict(read_mapq=np.uint8, read_mflags=np.uint8, read_isize=np.int32, read_start=np.int32)
MSTAT = ("SCA", "FLD", "RPCD", "MQCD", "FSSE")  # the order of fmt_mstat


def refpos_to_qpos(cig, ref_pos):
    """hts::CigarRefPosToQueryPos: M walks both, I and S advance the query, D the target; the first column at ref_pos decides;
    the end of the query when ref_pos lies beyond the CIGAR"""
    qp = tp = 0
    for op, ln in cig:
        if op == 0:
            if tp <= ref_pos < tp + ln:
                return qp + (ref_pos - tp)
            qp += ln
            tp += ln
        elif op in (1, 4):
            qp += ln
        elif op == 2:
            if tp <= ref_pos < tp + ln:
                return qp
            tp += ln
    return qp


def folded(qpos, rlen):
    x = float(qpos) / float(rlen) if rlen > 0 else 0.5
    return min(x, 1.0 - x)


def rank_tallies(ref_vals, alt_vals):
    """-> (2 x the ALT mid-rank sum, sum of t^3 - t over the tie groups) of the pooled values, as integers"""
    pooled = sorted([(x, 0) for x in ref_vals] + [(x, 1) for x in alt_vals], key=lambda p: p[0])
    rank2 = tie = 0
    i = 0
    while i < len(pooled):
        j = i
        while j < len(pooled) and pooled[j][0] == pooled[i][0]:
            j += 1
        t = j - i
        tie += t * t * t - t
        rank2 += sum(p[1] for p in pooled[i:j]) * (i + 1 + j)
        i = j
    return rank2, tie


def rms(mapqs):
    """VariantSupport::RmsMappingQual"""
    if not mapqs:
        return 0.0
    acc = 0.0
    for q in mapqs:
        acc = acc + float(q) * float(q)
    return math.sqrt(acc / float(len(mapqs)))


def soft_clip_asymmetry(ref_sc, ref_total, alt_sc, alt_total):
    alt_frac = float(alt_sc) / float(alt_total) if alt_total > 0 else 0.0
    ref_frac = float(ref_sc) / float(ref_total) if ref_total > 0 else 0.0
    return alt_frac - ref_frac


def start_entropy(starts, max_bins=20.0):
    """AltPooledEntropy over start / 3 (starts are not negative); None below 3 values"""
    if len(starts) < 3:
        return None
    counts = {}
    for s in starts:
        counts[int(s) // 3] = counts.get(int(s) // 3, 0) + 1
    total = float(len(starts))
    entropy = 0.0
    for b in sorted(counts):
        prob = counts[b] / total
        entropy -= prob * math.log2(prob)
    max_entropy = math.log2(min(total, max_bins))
    return entropy / max_entropy if max_entropy > 0.0 else 0.0


def read_positions(p, arrs, n, asm, var, aln_rec, aln_cigar, asg):
    """qpos of every assigned (read, variant): [n_reads * max_vars], -1 where the read is not assigned; and what the walk met:
    1 the variant starts before the alignment, 2 it starts inside a deletion of the CIGAR, 4 the CIGAR has a soft clip"""
    MC, MH, MV, MCG = p.max_comps, p.max_haps, p.max_vars, p.max_cigar
    nr = len(asg["allele"]) // MV
    rec = np.asarray(aln_rec).reshape(nr, MH, 6)
    cigs = np.asarray(aln_cigar).reshape(nr, MH, 1 + MCG)
    qpos = np.full(nr * MV, -1, np.int64)
    kind = np.zeros(nr * MV, np.uint8)
    for w in range(n):
        for r in range(int(arrs["read_win_off"][w]), int(arrs["read_win_off"][w + 1])):
            for v in range(int(var["win_nvars"][w])):
                i, vi = r * MV + v, w * MV + v
                if int(asg["allele"][i]) == 255:
                    continue
                h = int(asg["hap_id"][i])
                slot = int(asm["comp_hap0"][w * MC + int(var["var_comp"][vi])]) + h
                var_start = int(var["var_ref_start"][vi]) if h == 0 else int(var["var_hap_start"][vi * MH + h])
                aln_start = int(rec[r, slot, 2])
                cig = ref.decode_cigar(cigs[r, slot], MCG)
                qpos[i] = refpos_to_qpos(cig, max(0, var_start - aln_start))
                tp, in_del = 0, False
                for op, ln in cig:
                    in_del |= op == 2 and tp <= var_start - aln_start < tp + ln
                    tp += ln if op in (0, 2) else 0
                kind[i] = (1 if var_start < aln_start else 0) | (2 if in_del else 0) | (4 if any(op == 4 for op, _ in cig) else 0)
    return qpos, kind


def meta_stats(p, arrs, n, asm, var, aln_rec, aln_cigar, meta):
    """-> dict: ev_meta, ev_rpcd, fmt_rmq, fmt_mstat (capi.fmt_meta_out_spec layouts), allele_counts, qpos, and `cells`: per
    (w, v, sample) what the case guard of the tests reads"""
    MV, MA, S = p.max_vars, p.max_alts, p.num_samples
    NA = MA + 1
    asg = ref.assign_reads(p, arrs, n, asm, var, aln_rec, aln_cigar)
    ev, _ = ref.evidence_reads(p, arrs, n, var, asg)
    qpos, kind = read_positions(p, arrs, n, asm, var, aln_rec, aln_cigar, asg)
    cells_n = n * MV * S
    out = dict(ev_meta=np.zeros(cells_n * NA * 4, np.int64), ev_rpcd=np.zeros(cells_n * 4, np.uint64),
               fmt_rmq=np.zeros(cells_n * NA, np.float64), fmt_mstat=np.full(cells_n * 5, np.nan, np.float64),
               allele_counts=np.zeros(cells_n * NA * 2, np.uint32), qpos=qpos, cells={})
    rlen = lambda r: int(arrs["read_off"][r + 1]) - int(arrs["read_off"][r])  # noqa: E731
    for (w, v, s), by_allele in ev.items():
        vi = w * MV + v
        cell = vi * S + s
        k = int(var["var_nalts"][vi]) + 1
        per = []
        for a in range(k):
            reads = by_allele.get(a, [])
            mapq = [int(meta["read_mapq"][r]) for r in reads]
            sc = sum(1 for r in reads if int(meta["read_mflags"][r]) & MA_RM_SOFTCLIP)
            isz = [int(meta["read_isize"][r]) for r in reads
                   if int(meta["read_mflags"][r]) & MA_RM_PROPER and int(meta["read_isize"][r]) != 0]
            fold = [folded(int(qpos[r * MV + v]), rlen(r)) for r in reads]
            starts = [int(meta["read_start"][r]) for r in reads]
            per.append(dict(reads=reads, mapq=mapq, sc=sc, isz=isz, fold=fold, starts=starts))
            out["ev_meta"][(cell * NA + a) * 4:(cell * NA + a) * 4 + 4] = [sum(q * q for q in mapq), sc, len(isz), sum(isz)]
            out["fmt_rmq"][cell * NA + a] = rms(mapq)
            for r in reads:
                out["allele_counts"][(cell * NA + a) * 2 + int(bool(int(arrs["read_flags"][r]) & 4))] += 1
        pool = lambda key: [x for d in per[1:] for x in d[key]]  # noqa: E731
        n_ref, n_alt = len(per[0]["reads"]), len(pool("reads"))
        rank2, tie = rank_tallies(per[0]["fold"], pool("fold"))
        out["ev_rpcd"][cell * 4:cell * 4 + 4] = [n_ref, n_alt, rank2, tie]
        stats = (soft_clip_asymmetry(per[0]["sc"], n_ref, sum(d["sc"] for d in per[1:]), n_alt),
                 ref.mean_alt_minus_ref(per[0]["isz"], pool("isz")),
                 ref.mann_whitney_effect_size(per[0]["fold"], pool("fold")),
                 ref.mann_whitney_effect_size(per[0]["mapq"], pool("mapq")),
                 start_entropy(pool("starts")))
        for i, x in enumerate(stats):
            if x is not None:
                out["fmt_mstat"][cell * 5 + i] = x
        ref_lens, alt_lens = {rlen(r) for r in per[0]["reads"]}, {rlen(r) for r in pool("reads")}
        by_val = {}
        for d in per:
            for r, f in zip(d["reads"], d["fold"]):
                by_val.setdefault(f, set()).add((int(qpos[r * MV + v]), rlen(r)))
        # a tie group fed by two read lengths; two positions that mirror each other (q / L and (L - q) / L) and do NOT tie
        cross_tie = any(len({L for _, L in grp}) > 1 for grp in by_val.values())
        pairs = {(q, L) for grp in by_val.values() for q, L in grp}
        mirror = any((L - q, L) in pairs and q * 2 != L and folded(q, L) != folded(L - q, L) for q, L in pairs)
        out["cells"][(w, v, s)] = dict(n_ref=n_ref, n_alt=n_alt, k=k, stats=stats, cross_length_tie=cross_tie,
                                       untied_mirror=mirror, lens=sorted(ref_lens | alt_lens),
                                       bins=len({x // 3 for x in pool("starts")}),
                                       n_isz=(len(per[0]["isz"]), len(pool("isz"))),
                                       kinds=int(np.bitwise_or.reduce([kind[r * MV + v] for d in per for r in d["reads"]] or [0])),
                                       keys=n_ref + 2 * n_alt,
                                       pair_kinds={(bool(int(meta["read_mflags"][r]) & MA_RM_PROPER), int(np.sign(meta["read_isize"][r])))
                                                   for d in per for r in d["reads"]})
    return out
