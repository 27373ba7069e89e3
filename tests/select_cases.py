"""Hand-made candidates for ma_select_records_batch, one rule of include/microasm.h each, shared by tests/test_select_ref.py
(the restatement against what the rule says) and tests/test_gpu_select.py (the kernels against the restatement).

A case is one window of one to six 10-base records at pos 100 with qualities of 30 unless said otherwise; `want` is
(mask, value) of its win_state, `keep` the rec_keep bytes where they are the point."""
import struct

import numpy as np

import flatten_ref
import select_ref as ref

A, LOW, CAP, MDR, EV, LST = (ref.MA_S_ACTIVE, ref.MA_S_LOW_COVERAGE, ref.MA_S_CAPPED, ref.MA_S_MD_RANGE, ref.MA_S_EVENTS,
                             ref.MA_S_LISTED)
C, E = ref.MA_SK_COLLECT, ref.MA_SK_ELIGIBLE


def md(text):
    return b"MDZ" + text + b"\0"


def rec(tags=b"", l_seq=10, pos=100, mapq=60, flag=0, cigar=None, qual=None, name=b"r", sample=0, cut=None):
    """-> (record bytes, input sample); cut: bytes taken off the record's end (rec_len ends inside the auxiliary fields)"""
    body = flatten_ref.encode_record(name, flag=flag, pos=pos, mapq=mapq, cigar=[(l_seq, "M")] if cigar is None else cigar,
                                     seq4=bytes((l_seq + 1) // 2), qual=bytes([30] * l_seq) if qual is None else bytes(qual), tags=tags)
    return (body if not cut else body[:-cut], sample)


def qual_with(at, value, l_seq=10):
    q = [30] * l_seq
    q[at] = value
    return q


def twice(**kw):
    return [rec(**kw), rec(**kw)]


B_ARRAY = b"XBBs" + struct.pack("<i", 3) + bytes(6) + b"YBBc" + struct.pack("<i", 2) + bytes(2) + b"ZBBf" + struct.pack("<i", 1) + bytes(4)
M3 = md(b"3A6")  # a mismatch at 103

# (label, records, win_len, (mask, value) of win_state, rec_keep or None)
RULES = [
    ("mapq 0", twice(tags=M3, mapq=0), 10, (A | LST, 0), [0, 0]),
    ("mapq 1", twice(tags=M3, mapq=1), 10, (A | LST, A | LST), [E, E]),  # active, and nothing collected: an empty listed range
    ("mapq 19", twice(tags=M3, mapq=19), 10, (A, A), [E, E]),
    ("mapq 20", twice(tags=M3, mapq=20), 10, (A | LST, A | LST), [C | E, C | E]),
    ("flag 0x200", twice(tags=M3, flag=0x200), 10, (A, 0), [0, 0]),
    ("flag 0x400", twice(tags=M3, flag=0x400), 10, (A, 0), [0, 0]),
    ("flag 0x4", twice(tags=M3, flag=0x4), 10, (A, 0), [0, 0]),
    ("other flags", twice(tags=M3, flag=0x1 | 0x2 | 0x10 | 0x100 | 0x800), 10, (A, A), [C | E, C | E]),
    ("one mismatch is not two", [rec(tags=M3)], 10, (A | LST, 0), None),
    ("^ run lands on one position", [rec(tags=md(b"3^AC6"))], 10, (A, A), None),
    ("^ alone adds nothing", twice(tags=md(b"3^N6")), 10, (A, 0), None),
    ("quality 19 at the mismatch", twice(tags=M3, qual=qual_with(3, 19)), 10, (A, 0), None),
    ("quality 20 at the mismatch", twice(tags=M3, qual=qual_with(3, 20)), 10, (A, A), None),
    ("the quality index ignores a leading clip", [rec(tags=M3, cigar=[(4, "S"), (6, "M")], qual=qual_with(3, 0)), rec(tags=M3, qual=qual_with(3, 0))],
     10, (A, 0), None),  # (qual[3] it is, not qual[3 + 4])
    ("lower-case letters", twice(tags=md(b"3a6")), 10, (A, A), None),
    ("not a base", twice(tags=md(b"3N6")), 10, (A, 0), None),
    ("0xFF qualities pass", twice(tags=M3, qual=[0xFF] * 10), 10, (A, A), None),
    ("pos -1: no MD walk", twice(tags=M3, pos=-1), 10, (A | MDR, 0), None),
    ("the walk ends on the last base", twice(tags=md(b"9A")), 10, (A | MDR, A), None),
    ("a walk past l_seq", [rec(tags=md(b"10A"))], 10, (A | MDR | LST, MDR), None),
    ("a walk past l_seq behind a hit", twice(tags=md(b"3A5A2C")), 10, (A | MDR | LST, A | MDR), None),
    ("a 9-digit number", twice(tags=md(b"000000003A")), 10, (A | MDR, A), None),
    ("a 10-digit number", [rec(tags=md(b"0000000003A"))], 10, (A | MDR | LST, MDR), None),
    ("trailing digits are never used", twice(tags=md(b"3A99999999999")), 10, (A | MDR, A), None),
    ("two MD tags: the last wins", [rec(tags=M3 + md(b"5A4")), rec(tags=md(b"5A4"))], 10, (A, A), None),
    ("two MD tags: the first does not", [rec(tags=md(b"5A4") + M3), rec(tags=md(b"5A4"))], 10, (A, 0), None),
    ("MD:H is not MD:Z", twice(tags=b"MDH3A\0"), 10, (A, 0), None),
    ("MD behind B arrays", twice(tags=B_ARRAY + M3), 10, (A, A), None),
    ("MD behind every scalar type", twice(tags=b"aaAxbbc\x01ccC\x01dds\x01\x02eeS\x01\x02ffi\x01\x02\x03\x04ggI\x01\x02\x03\x04hhf\x01\x02\x03\x04iiZtext\0jjH0A\0" + M3), 10, (A, A), None),
    ("a negative B count ends the walk", twice(tags=b"XBBs" + struct.pack("<i", -1) + M3), 10, (A, 0), None),
    ("an unknown type ends the walk", twice(tags=b"XX?" + M3), 10, (A, 0), None),
    ("an unterminated Z ends the walk", twice(tags=b"XYZabc"), 10, (A, 0), None),
    ("an unterminated MD", twice(tags=b"MDZ3A6"), 10, (A, 0), None),
    ("tags cut inside an int", twice(tags=b"NMi\x01\x00\x00\x00" + M3, cut=len(M3) + 2), 10, (A, 0), None),
    ("tags cut inside the MD string", twice(tags=b"NMi\x01\x00\x00\x00" + M3, cut=2), 10, (A, 0), None),
    ("tags cut inside a B array", twice(tags=B_ARRAY + M3, cut=len(M3) + 3), 10, (A, 0), None),
    ("tags cut behind the MD's NUL", twice(tags=M3 + b"NMi\x01\x00\x00\x00", cut=5), 10, (A, A), None),
    ("two tag bytes left", twice(tags=M3 + b"NM", cut=0), 10, (A, A), None),
    ("I after the advance", twice(cigar=[(5, "M"), (2, "I"), (3, "M")]), 10, (A, A), None),
    ("D after the advance", [rec(cigar=[(5, "M"), (2, "D"), (5, "M")]), rec(cigar=[(7, "M"), (1, "D"), (3, "M")], pos=99)], 10, (A, A), None),  # 107, 107
    ("D before the advance would meet", [rec(cigar=[(5, "M"), (2, "D"), (5, "M")]), rec(cigar=[(5, "M"), (1, "D"), (5, "M")])], 10, (A, 0), None),  # 107, 106
    ("X after the advance", [rec(cigar=[(5, "="), (1, "X"), (4, "=")]), rec(cigar=[(6, "M"), (4, "X")], pos=96)], 10, (A, A), None),  # 106, 106
    ("N advances, H P I S do not", [rec(cigar=[(2, "H"), (1, "S"), (2, "M"), (3, "I"), (0, "P"), (10, "N"), (4, "M"), (1, "I")]),
                                   rec(cigar=[(9, "M"), (1, "I")], pos=107)], 10, (A, A), None),  # I at 116 and 116
    ("a leading S sits on pos", [rec(cigar=[(3, "S"), (7, "M")]), rec(cigar=[(2, "S"), (8, "M")])], 10, (A, A), None),
    ("an S behind M sits behind it", [rec(cigar=[(7, "M"), (3, "S")]), rec(cigar=[(1, "S"), (9, "M")], pos=107)], 10, (A, A), None),
    ("X and MD meet on one position", [rec(cigar=[(5, "="), (1, "X"), (4, "=")], tags=md(b"6A3"))], 10, (A, A), None),
    ("I and D on one position are two multisets", [rec(cigar=[(5, "M"), (1, "I"), (4, "M")]), rec(cigar=[(3, "M"), (2, "D"), (7, "M")])], 10, (A, 0), None),
    ("S and MD on one position are two multisets", [rec(cigar=[(3, "M"), (7, "S")], tags=md(b"3A"))], 10, (A | MDR, 0), None),
    ("positions wrap at 2^32", [rec(pos=0x7FFFFFFF, cigar=[(0xFFFFFFF, "N"), (0xFFFFFFF, "N"), (0xFFFFFFF, "N"), (0xFFFFFFF, "N"),
                                                            (0xFFFFFFF, "N"), (0xFFFFFFF, "N"), (0xFFFFFFF, "N"), (0xFFFFFFF, "N"), (9, "N"), (10, "M"), (1, "I")]),
                                rec(pos=0, cigar=[(10, "M"), (1, "I")])], 10, (A, A), None),  # 0x7FFFFFFF + 8 (2^28 - 1) + 9 + 10 = 2^32 + 10
    ("position 0xFFFFFFFF is a position", twice(pos=0x7FFFFFFF, cigar=[(0xFFFFFFF, "N")] * 8 + [(8, "N"), (1, "I"), (10, "M")]), 10, (A, A), None),
    ("two samples, one event each", [rec(tags=M3, sample=0), rec(tags=M3, sample=1)], 10, (A | LST, 0), None),
    ("the same two in one sample", [rec(tags=M3, sample=1), rec(tags=M3, sample=1)], 10, (A | LST, A | LST), None),
    ("a hit in the second sample only", [rec(tags=M3, sample=0), rec(tags=md(b"5A4"), sample=1), rec(tags=md(b"5C4"), sample=1)], 10, (A, A), None),
    # max_sample_cov 4: reads > ceil(4 * win_len / 10)
    ("4 reads at the cap of 4", [rec(tags=M3)] * 4, 10, (A | CAP | LST, A | LST), None),
    ("5 reads over the cap of 4", [rec(tags=M3)] * 5, 10, (A | CAP | LST, A | CAP), None),
    ("5 reads at the cap of ceil(4.4)", [rec(tags=M3)] * 5, 11, (A | CAP | LST, A | LST), None),
    ("6 reads over the cap of ceil(4.4)", [rec(tags=M3)] * 6, 11, (A | CAP | LST, A | CAP), None),
    ("the cap is per sample", [rec(tags=M3, sample=0)] * 4 + [rec(tags=M3, sample=1)] * 4, 10, (A | CAP | LST, A | LST), None),
    ("uncollected reads do not count", [rec(tags=M3)] * 4 + [rec(tags=M3, mapq=19)] * 3, 10, (A | CAP | LST, A | LST), None),
    ("a window of length 0", [rec(tags=M3)], 0, (CAP | LOW, CAP), None),
]
RULE_PARAMS = dict(max_sample_cov=4.0, min_anchor_cov=0, skip_active_region=False)

# min_anchor_cov 3: (double)bases / (double)win_len < 3.0
COVERAGE = [
    ("30 bases over 10: at the bound", [rec(tags=M3)] * 3, 10, (A | LOW | LST, A | LST), None),
    ("30 bases over 11: under it", [rec(tags=M3)] * 3, 11, (A | LOW | LST, A | LOW), None),
    ("the sum is over the samples", [rec(tags=M3, sample=0)] * 2 + [rec(tags=M3, sample=1)], 10, (A | LOW | LST, A | LST), None),
    ("uncollected bases do not count", [rec(tags=M3)] * 2 + [rec(tags=M3, mapq=19)], 10, (A | LOW | LST, A | LOW), None),
    ("no candidate at all", [], 10, (A | LOW | LST, LOW), None),
]
COVERAGE_PARAMS = dict(max_sample_cov=1000.0, min_anchor_cov=3, skip_active_region=False)

# skip_active_region: every window is active and no event is looked at
SKIPPED = [
    ("no event needed", [rec()], 10, (A | LST, A | LST), None),
    ("no MD walk either", [rec(tags=md(b"10A"))], 10, (A | MDR | LST, A | LST), None),
    ("the filters still hold", [rec(mapq=0), rec(flag=0x4)], 10, (A | LST, A | LST), [0, 0]),
]
SKIPPED_PARAMS = dict(max_sample_cov=4.0, min_anchor_cov=0, skip_active_region=True)

BATCHES = {"rules": (RULES, RULE_PARAMS), "coverage": (COVERAGE, COVERAGE_PARAMS), "skip_active_region": (SKIPPED, SKIPPED_PARAMS)}


def lay_out(windows, n_samples=2, gap=b"\x99\x77\x55", reverse=False):
    """windows: lists of (bytes, sample) -> (rec arrays, n_windows, n_records, n_samples); every listing gets bytes of its own,
    3 junk bytes apart, so that records start at odd and even offsets"""
    blob, off, ln, smp, win_off = bytearray(b"\x01"), [], [], [], [0]
    for records in windows:
        for body, s in (reversed(records) if reverse else records):
            blob += gap
            off.append(len(blob))
            ln.append(len(body))
            smp.append(s)
            blob += body
        win_off.append(len(off))
    blob += gap
    arrays = dict(blob=np.frombuffer(bytes(blob), dtype=np.uint8).copy(), rec_off=np.array(off, dtype=np.uint64),
                  rec_len=np.array(ln, dtype=np.uint32), rec_win_off=np.array(win_off, dtype=np.uint32),
                  rec_sample=np.array(smp, dtype=np.uint8), n_samples_in=n_samples)
    return arrays, len(windows), len(off), n_samples


def batch(which, reverse=False):
    """-> (rec arrays, n_windows, n_records, n_samples, win_len, params, cases)"""
    cases, params = BATCHES[which]
    arrays, n, nr, ns = lay_out([c[1] for c in cases], reverse=reverse)
    return arrays, n, nr, ns, np.array([c[2] for c in cases], dtype=np.uint32), params, cases


# ---- the reads of a synthesised batch as candidates ---------------------------------------------------------------------------
def md_of(read, window_ref, hint):
    """the MD string of `read` laid on `window_ref` at `hint` without gaps (bases off the window's ends count as matches)"""
    at = np.arange(len(read)) + hint
    inside = (at >= 0) & (at < len(window_ref))
    differs = np.zeros(len(read), bool)
    differs[inside] = window_ref[at[inside]] != read[inside]
    out, last = [], -1
    for j in np.flatnonzero(differs):
        out.append(b"%d%c" % (j - last - 1, window_ref[at[j]]))
        last = int(j)
    out.append(b"%d" % (len(read) - last - 1))
    return b"".join(out)


def records_of_synth(arrs, n, nr, roles, rng, extras=True):
    """the reads of a lancet2_amd.synth batch as BAM records with NM and MD fields, each window's in a shuffled arrival order;
    extras: one candidate in eight is followed by a copy that a filter drops (duplicate, QC fail, unmapped, mapq 0 or 19).
    -> (the ma_records_t arrays, n_windows, n_records, win_len)"""
    from lancet2_amd import capi
    start0 = [10_000 + 2000 * w for w in range(n)]
    blob, off, ln, smp, win_off = bytearray(b"\x01"), [], [], [], [0]
    for w in range(n):
        window_ref = arrs["ref_bases"][int(arrs["ref_off"][w]):int(arrs["ref_off"][w + 1])]
        for r in rng.permutation(np.arange(int(arrs["read_win_off"][w]), int(arrs["read_win_off"][w + 1]))):
            o0, o1 = int(arrs["read_off"][r]), int(arrs["read_off"][r + 1])
            fl, hint, s = int(arrs["read_flags"][r]), int(arrs["read_hint"][r]), int(arrs["read_sample"][r])
            hinted = hint != capi.MA_NO_HINT
            text = md_of(arrs["read_bases"][o0:o1], window_ref, hint) if hinted else b"%d" % (o1 - o0)
            tags = b"NMi" + struct.pack("<i", text.count(b"A") + text.count(b"C") + text.count(b"G") + text.count(b"T")) + md(text)
            kw = dict(refid=0 if hinted else 1, pos=start0[w] + (hint if hinted else 0), cigar=[(o1 - o0, "M")],
                      seq4=flatten_ref.pack_seq(arrs["read_bases"][o0:o1]), qual=arrs["read_quals"][o0:o1].tobytes(),
                      tlen=int(rng.integers(-500, 500)), tags=tags)
            name = b"A00123:45:HXXXXXXXX:1:%d" % int(arrs["read_qname_id"][r])
            bodies = [flatten_ref.encode_record(name, flag=(0x10 if fl & capi.MA_RF_REV else 0) | 0x2, mapq=60 if fl & capi.MA_RF_PASS else 7, **kw)]
            if extras and int(rng.integers(0, 8)) == 0:
                flag, mapq = [(0x400, 60), (0x200, 60), (0x4, 60), (0, 0), (0, 19)][int(rng.integers(0, 5))]
                bodies.append(flatten_ref.encode_record(name + b"x", flag=flag, mapq=mapq, **kw))
            for body in bodies:
                blob += b"\x99" * (1 + len(blob) % 3)  # records at any alignment
                off.append(len(blob))
                ln.append(len(body))
                smp.append(s)
                blob += body
        win_off.append(len(off))
    blob += b"\x99\x77\x55"
    rec = dict(blob=np.frombuffer(bytes(blob), dtype=np.uint8).copy(), rec_off=np.array(off, dtype=np.uint64),
               rec_len=np.array(ln, dtype=np.uint32), rec_win_off=np.array(win_off, dtype=np.uint32), rec_sample=np.array(smp, dtype=np.uint8),
               sample_index=np.arange(len(roles), dtype=np.uint8), sample_case=np.array(roles, dtype=np.uint8),
               sample_rank=np.array([10 * role + s for s, role in enumerate(roles)], dtype=np.uint32),
               win_chrom=np.zeros(n, np.int32), win_start0=np.array(start0, dtype=np.int64), n_samples_in=len(roles))
    win_len = (arrs["ref_off"][1:n + 1] - arrs["ref_off"][:n]).astype(np.uint32)
    return rec, n, len(off), win_len
