"""Independent reference of the read-level FORMAT statistics (ma_genotype_stats_batch), in plain Python and numpy.

Shares no code with oracle/ or the product.  Input: a batch, the assembly and variant arrays, and the alignment taps of the
ORACLE's genotype stage (aln_rec, aln_cigar) -- never a tap of the code under test.  From those it re-derives, the long way
and in the reference's order (all citations are to the reference tree):

  * every read's winning assignment per variant (caller/genotyper.cpp:269-362, caller/combined_scorer.cpp:24-108,
    caller/local_scorer.cpp:166-305): allele, combined score, and the four per-read values base_qual, hap_id, own_nm, ref_nm;
  * the evidence reads (the lowest read index per variant, sample, allele and qname id) and the allele depths;
  * NPBQ (caller/posterior_base_qual.cpp:14-40, caller/variant_call.cpp:368-373), BQCD (base/mann_whitney.h:127-225: a sort
    and mid-ranks), CMLOD (caller/genotype_likelihood.cpp:141-196, :307-345), ASMD / AHDD (caller/variant_support.h:361-387,
    caller/variant_call.cpp:177-184) and HSE (caller/variant_support.h:389-411) with per-read loops.

tests/test_format_stats_ref.py pins this file against the oracle's taps and scipy before the GPU test trusts it."""
import math
import os
import re
import struct

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _phred_lut():
    txt = open(os.path.join(REPO, "include", "ma_phred_lut.inc")).read()
    bits = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{16})ULL", txt)]
    assert len(bits) == 256
    return [struct.unpack("<d", struct.pack("<Q", b))[0] for b in bits]


PHRED = _phred_lut()  # error probability of a Phred quality, the table every implementation shares
_ENC = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _ENC[_c] = _i
    _ENC[_c + 32] = _i


def _score(t, q):  # scoring_constants.h:35-41: match 1, mismatch -4, anything against N 0
    if t == 4 or q == 4:
        return 0
    return 1 if t == q else -4


def decode_cigar(words, max_cigar):
    """[n_ops, len << 4 | op ...] -> [(op, len)], op: 0 M, 1 I, 2 D, 4 S"""
    n = min(int(words[0]), max_cigar)
    return [(int(x) & 15, int(x) >> 4) for x in words[1:1 + n]]


def edit_distance(cig, q, t):
    """hts/cigar_utils.h:61-111 on encoded query / target"""
    ed = qp = tp = 0
    for op, ln in cig:
        if op == 0:
            k = max(0, min(ln, len(q) - qp, len(t) - tp))
            ed += int(np.count_nonzero(q[qp:qp + k] != t[tp:tp + k]))
            qp += ln
            tp += ln
        elif op == 1:
            ed += ln
            qp += ln
        elif op == 2:
            ed += ln
            tp += ln
        elif op == 4:
            qp += ln
    return ed


def local_score(cig, q, quals, target, aln_start, vstart, vlen):
    """ComputeLocalScore (caller/local_scorer.cpp:166-279) -> (pbq, raw, identity, base_qual)"""
    if not cig or vlen == 0:
        return 0.0, 0.0, 0.0, 0
    vend = vstart + vlen
    pbq = raw = 0.0
    matches = aligned = 0
    min_bq = 255
    tpos = qpos = 0
    nq = len(quals)
    for op, ln in cig:
        if aln_start + tpos >= vend and op in (0, 2):
            break
        if op == 0:
            lo = max(0, vstart - (aln_start + tpos))
            hi = min(ln, vend - (aln_start + tpos))
            for i in range(lo, hi):  # (the positions outside the region do nothing)
                qp, tp = qpos + i, tpos + i
                aligned += 1
                if not (qp >= len(q) or tp >= len(target)):
                    r = _score(int(target[tp]), int(q[qp]))
                    raw += float(r)
                    w = 1.0 - PHRED[int(quals[qp])] if qp < nq else 1.0
                    pbq += float(r) * w
                    matches += int(q[qp] == target[tp])
                if qp < nq:
                    min_bq = min(min_bq, int(quals[qp]))
            tpos += ln
            qpos += ln
        elif op == 1:
            if vstart <= aln_start + tpos < vend:
                for i in range(ln):
                    aligned += 1
                    if qpos + i < nq:
                        min_bq = min(min_bq, int(quals[qpos + i]))
                    pbq += 3.0
            qpos += ln
        elif op == 2:
            for i in range(ln):
                if vstart <= aln_start + tpos + i < vend:
                    aligned += 1
                    pbq += 3.0
            tpos += ln
            # the bases on both sides of the deletion, whether or not it lies in the region
            if qpos > 0 and qpos - 1 < nq:
                min_bq = min(min_bq, int(quals[qpos - 1]))
            if qpos < nq:
                min_bq = min(min_bq, int(quals[qpos]))
        elif op == 4:
            qpos += ln
    ident = matches / aligned if aligned > 0 else 0.0
    return pbq, raw, ident, (0 if min_bq == 255 else min_bq)


def assign_reads(p, arrs, n, asm, var, aln_rec, aln_cigar):
    """Winning assignment of every read at every variant of its window.  -> dict of arrays [n_reads * max_vars]:
    allele (255 = none), score (f64), base_qual, hap_id, own_nm, ref_nm, and has_outside_del (the winning CIGAR holds a
    deletion that does not overlap the variant)."""
    MC, MH, ML, MV, MA, MCG = p.max_comps, p.max_haps, p.max_hap_len, p.max_vars, p.max_alts, p.max_cigar
    nr = len(arrs["read_sample"])
    out = dict(allele=np.full(nr * MV, 255, np.uint8), score=np.zeros(nr * MV, np.float64),
               base_qual=np.zeros(nr * MV, np.uint32), hap_id=np.zeros(nr * MV, np.uint32),
               own_nm=np.zeros(nr * MV, np.uint32), ref_nm=np.zeros(nr * MV, np.uint32),
               has_outside_del=np.zeros(nr * MV, bool))
    rec = np.asarray(aln_rec).reshape(nr, MH, 6)
    cigs = np.asarray(aln_cigar).reshape(nr, MH, 1 + MCG)
    for w in range(n):
        nv = int(var["win_nvars"][w])
        if nv == 0 or (int(asm["win_status"][w]) & (1 | 128)):
            continue
        r0, r1 = int(arrs["read_win_off"][w]), int(arrs["read_win_off"][w + 1])
        for c in range(int(asm["win_ncomp"][w])):
            vs = [v for v in range(nv) if int(var["var_comp"][w * MV + v]) == c]
            if not vs:
                continue  # components without variants are not genotyped
            ci = w * MC + c
            hap0, nh = int(asm["comp_hap0"][ci]), int(asm["comp_nhaps"][ci])
            henc = []
            for h in range(nh):
                hi = w * MH + hap0 + h
                henc.append(_ENC[asm["hap_bases"][hi * ML: hi * ML + int(asm["hap_len"][hi])]])
            for r in range(r0, r1):
                o0, o1 = int(arrs["read_off"][r]), int(arrs["read_off"][r + 1])
                q = _ENC[arrs["read_bases"][o0:o1]]
                quals = arrs["read_quals"][o0:o1]
                rlen = o1 - o0
                alns = []
                for h in range(nh):
                    hit, score, rs, re_, _, _ = (int(x) for x in rec[r, hap0 + h])
                    if hit:
                        alns.append((h, score, rs, re_, decode_cigar(cigs[r, hap0 + h], MCG)))
                if not alns:
                    continue
                ref_nm = rlen  # combined_scorer.cpp:24-38
                for h, score, rs, re_, cig in alns:
                    if h != 0 or rs >= re_:
                        continue
                    ref_nm = edit_distance(cig, q, henc[0][rs:re_])
                    break
                best = {}
                for h, score, rs, re_, cig in alns:  # alignments in haplotype order, the first wins ties
                    for v in vs:
                        vi = w * MV + v
                        if h == 0:
                            vstart, vlen, allele = int(var["var_ref_start"][vi]), int(var["var_ref_len"][vi]), 0
                        else:
                            allele = int(var["var_hap_allele"][vi * MH + h])
                            if allele == 0:
                                continue
                            vstart = int(var["var_hap_start"][vi * MH + h])
                            vlen = int(var["alt_len"][vi * MA + allele - 1])
                        if not ((vstart + vlen) > rs and vstart < re_):
                            continue
                        target = henc[h][rs:re_]
                        pbq, raw, ident, bq = local_score(cig, q, quals, target, rs, vstart, vlen)
                        s5 = cig[0][1] if cig and cig[0][0] == 4 else 0
                        s3 = cig[-1][1] if len(cig) > 1 and cig[-1][0] == 4 else 0
                        global_adj = float(score) - float(s5 + s3) * 4
                        combined = float(int(global_adj - raw)) + pbq * ident
                        if v in best and combined <= best[v][0]:
                            continue
                        tp, outside = rs, False
                        for op, ln in cig:
                            if op == 2 and not (tp < vstart + vlen and tp + ln > vstart):
                                outside = True
                            if op in (0, 2):
                                tp += ln
                        best[v] = (combined, allele, bq, h, edit_distance(cig, q, target), outside)
                for v, (combined, allele, bq, h, own_nm, outside) in best.items():
                    i = r * MV + v
                    out["allele"][i] = allele
                    out["score"][i] = combined
                    out["base_qual"][i] = bq
                    out["hap_id"][i] = h
                    out["own_nm"][i] = own_nm
                    out["ref_nm"][i] = ref_nm
                    out["has_outside_del"][i] = outside
    return out


def evidence_reads(p, arrs, n, var, asg):
    """-> {(w, v, sample): {allele: [read indices, ascending]}}: the lowest read index of every (variant, sample, allele,
    qname id); reads of a sample index >= num_samples are ignored.  Also the number of reads the rule removed."""
    MV, S = p.max_vars, p.num_samples
    cells, removed = {}, {}
    for w in range(n):
        r0, r1 = int(arrs["read_win_off"][w]), int(arrs["read_win_off"][w + 1])
        for v in range(int(var["win_nvars"][w])):
            seen = set()
            for r in range(r0, r1):
                al, smp = int(asg["allele"][r * MV + v]), int(arrs["read_sample"][r])
                if al == 255 or smp >= S:
                    continue
                key = (smp, al, int(arrs["read_qname_id"][r]))
                if key in seen:
                    removed[(w, v, smp)] = removed.get((w, v, smp), 0) + 1
                    continue
                seen.add(key)
                cells.setdefault((w, v, smp), {}).setdefault(al, []).append(r)
    return cells, removed


# ---- the statistics, over lists of per-read values -------------------------------------------------------------------
def raw_posterior_base_qual(fwd, rev):
    if not fwd and not rev:
        return 0.0
    log_err = log_ok = 0.0
    for quals in (fwd, rev):
        for q in quals:
            eps = PHRED[q]
            log_err += math.log10(max(eps, 1e-300))
            log_ok += math.log10(max(1.0 - eps, 1e-300))
    max_log = max(log_err, log_ok)
    log_sum = max_log + math.log10(1.0 + math.pow(10.0, min(log_err, log_ok) - max_log))
    return -10.0 * (log_err - log_sum)


def mid_ranks(values):
    """1-based mid-ranks of `values` (ties share the mean of the ranks they span), and sum of t^3 - t over the tie groups"""
    order = sorted(range(len(values)), key=lambda i: values[i])
    ranks = [0.0] * len(values)
    tie = 0.0
    i = 0
    while i < len(order):
        j = i
        while j < len(order) and values[order[j]] == values[order[i]]:
            j += 1
        for k in range(i, j):
            ranks[order[k]] = (i + 1 + j) / 2.0
        t = float(j - i)
        tie += t * t * t - t
        i = j
    return ranks, tie


def mann_whitney_u_alt(ref_vals, alt_vals):
    ranks, _ = mid_ranks(list(ref_vals) + list(alt_vals))
    n_alt = float(len(alt_vals))
    return sum(ranks[len(ref_vals):]) - (n_alt * (n_alt + 1.0)) / 2.0


def mann_whitney_effect_size(ref_vals, alt_vals):
    """base/mann_whitney.h:127-225; None when either group is empty"""
    if not ref_vals or not alt_vals:
        return None
    n_ref, n_alt = float(len(ref_vals)), float(len(alt_vals))
    n_total = n_ref + n_alt
    _, tie = mid_ranks(list(ref_vals) + list(alt_vals))
    u_stat = mann_whitney_u_alt(ref_vals, alt_vals)
    mean_u = (n_ref * n_alt) / 2.0
    var_u = (n_ref * n_alt / 12.0) * ((n_total + 1.0) - (tie / (n_total * (n_total - 1.0))))
    if var_u <= 0.0:
        return 0.0
    return ((u_stat - mean_u) / math.sqrt(var_u)) / math.sqrt(n_total)


def _pileup_log_lk(quals_by_allele, frac, k):
    ll = 0.0
    for called_as in range(k):
        for strand in quals_by_allele[called_as]:  # fwd, then rev
            for q in strand:
                eps = PHRED[q]
                mismatch = eps / max(1, k - 1)
                bonus = (1.0 - eps) - mismatch
                ll += math.log10(max(1e-15, mismatch + frac[called_as] * bonus))
    return ll


def continuous_mixture_lods(quals_by_allele, depths):
    """caller/genotype_likelihood.cpp:307-345.  quals_by_allele[a] = (fwd quals, rev quals); -> one LOD per allele"""
    k = len(depths)
    lods = [0.0] * k
    total = sum(depths)
    if k < 2 or total == 0:
        return lods
    frac = [d / float(total) for d in depths]
    ll_mle = _pileup_log_lk(quals_by_allele, frac, k)
    for target in range(1, k):
        if depths[target] == 0:
            continue
        null = list(frac)
        mass = null[target]
        null[target] = 0.0
        remaining = 1.0 - mass
        if remaining <= 0.0:
            null[0] = 1.0
        else:
            null = [f / remaining for f in null]
        lods[target] = max(0.0, ll_mle - _pileup_log_lk(quals_by_allele, null, k))
    return lods


def mean_alt_minus_ref(ref_vals, alt_vals, offset=0.0):
    if not ref_vals or not alt_vals:
        return None
    ref_mean = sum(float(x) for x in ref_vals) / float(len(ref_vals))
    alt_mean = sum(float(x) for x in alt_vals) / float(len(alt_vals))
    return (alt_mean - offset) - ref_mean


def alt_hap_entropy(hap_ids, max_bins):
    """caller/variant_support.h:389-411 with the haplotype index as the bin; None below 3 reads or 2 haplotypes"""
    if len(hap_ids) < 3 or max_bins < 2:
        return None
    counts = {}
    for h in hap_ids:
        counts[h] = counts.get(h, 0) + 1
    total = float(len(hap_ids))
    entropy = 0.0
    for h in sorted(counts):
        prob = counts[h] / total
        entropy -= prob * math.log2(prob)
    max_entropy = math.log2(min(total, float(max_bins)))
    return entropy / max_entropy if max_entropy > 0.0 else 0.0


def format_stats(p, arrs, n, asm, var, aln_rec, aln_cigar):
    """-> dict: the product's four arrays (capi.fmt_out_spec layouts), allele_counts, the per-read assignment (`asg`) and
    `cells`: per (w, v, sample) a summary the case guard of the tests reads."""
    MC, MV, MA, S = p.max_comps, p.max_vars, p.max_alts, p.num_samples
    NA = MA + 1
    asg = assign_reads(p, arrs, n, asm, var, aln_rec, aln_cigar)
    ev, removed = evidence_reads(p, arrs, n, var, asg)
    out = dict(ev_sums=np.zeros(n * MV * S * NA * 3, np.uint32), fmt_npbq=np.zeros(n * MV * S * NA, np.float64),
               fmt_cmlod=np.zeros(n * MV * S * MA, np.float64), fmt_stat=np.full(n * MV * S * 4, np.nan, np.float64),
               allele_counts=np.zeros(n * MV * S * NA * 2, np.uint32), asg=asg, cells={})
    for (w, v, s), by_allele in ev.items():
        vi = w * MV + v
        cell = vi * S + s
        k = int(var["var_nalts"][vi]) + 1
        val = lambda name, r: int(asg[name][r * MV + v])  # noqa: E731
        rev = lambda r: bool(int(arrs["read_flags"][r]) & 4)  # noqa: E731
        quals, depths = [], []
        for a in range(k):
            reads = by_allele.get(a, [])
            fwd = [val("base_qual", r) for r in reads if not rev(r)]
            rv = [val("base_qual", r) for r in reads if rev(r)]
            quals.append((fwd, rv))
            depths.append(len(reads))
            out["allele_counts"][(cell * NA + a) * 2] = len(fwd)
            out["allele_counts"][(cell * NA + a) * 2 + 1] = len(rv)
            out["ev_sums"][(cell * NA + a) * 3: (cell * NA + a) * 3 + 3] = [
                sum(val(name, r) for r in reads) for name in ("base_qual", "ref_nm", "own_nm")]
            raw = raw_posterior_base_qual(fwd, rv)
            out["fmt_npbq"][cell * NA + a] = raw / float(len(reads)) if reads else 0.0
        lods = continuous_mixture_lods(quals, depths)
        out["fmt_cmlod"][cell * MA: cell * MA + k - 1] = lods[1:]
        ref_reads = by_allele.get(0, [])
        alt_reads = [r for a in range(1, k) for r in by_allele.get(a, [])]
        max_var_len = max([abs(int(var["alt_length"][vi * MA + a])) for a in range(k - 1)] or [0])
        nhaps = int(asm["comp_nhaps"][w * MC + int(var["var_comp"][vi])])
        stats = (mann_whitney_effect_size([val("base_qual", r) for r in ref_reads], [val("base_qual", r) for r in alt_reads]),
                 mean_alt_minus_ref([val("ref_nm", r) for r in ref_reads], [val("ref_nm", r) for r in alt_reads], float(max_var_len)),
                 mean_alt_minus_ref([val("own_nm", r) for r in ref_reads], [val("own_nm", r) for r in alt_reads]),
                 alt_hap_entropy([val("hap_id", r) for r in alt_reads], nhaps))
        for i, x in enumerate(stats):
            if x is not None:
                out["fmt_stat"][cell * 4 + i] = x
        out["cells"][(w, v, s)] = dict(
            n_ref=len(ref_reads), n_alt=len(alt_reads), k=k, removed=removed.get((w, v, s), 0), hse=stats[3], bqcd=stats[0],
            alt_types=[int(var["alt_type"][vi * MA + a]) for a in range(k - 1)],
            outside_del=any(bool(asg["has_outside_del"][r * MV + v]) for r in ref_reads + alt_reads))
    return out
