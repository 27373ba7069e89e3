"""Plain-Python restatement of ma_flatten_records_batch (include/microasm.h): raw BAM alignment records and the window each
belongs to in, the read arrays of a batch out.  Parses the record bytes with `struct`, sorts with a key tuple, interns names
with a dict.  Imports neither the engine nor the host shell: tests hold both to it.

Also the inverse, encode_record(), for tests that make records by hand."""
import struct

import numpy as np

MA_RF_PASS, MA_RF_CASE, MA_RF_REV = 1, 2, 4
MA_RM_SOFTCLIP, MA_RM_PROPER = 1, 2
MA_NO_HINT = -(1 << 31)
MA_ERR_ARG, MA_ERR_PARAM = -1, -5
MAX_WINDOW = 16384
CIGAR_OPS = "MIDNSHP=X"
BASE_CODES = "=ACMGRSVTWYHKDBN"


class FlattenError(Exception):
    def __init__(self, rc, what, record=None, n_bases=None):
        super().__init__(what)
        self.rc, self.record, self.n_bases = rc, record, n_bases


def encode_record(name, flag=0, refid=0, pos=0, mapq=60, cigar=(), seq4=b"", l_seq=None, qual=b"", tlen=0, mrefid=-1, mpos=-1,
                  tags=b"", l_read_name=None):
    """one BAM alignment record from its refID field on (SAM specification 4.2, without block_size).  name: bytes without the
    NUL; cigar: (length, op letter) pairs; seq4: the packed sequence bytes; l_seq / l_read_name: the fields, when they are to
    differ from what the bytes hold"""
    name = bytes(name)
    l_seq = len(qual) if l_seq is None else l_seq
    words = b"".join(struct.pack("<I", (ln << 4) | CIGAR_OPS.index(op)) for ln, op in cigar)
    head = struct.pack("<iiBBHHHiiii", refid, pos, len(name) + 1 if l_read_name is None else l_read_name, mapq, 4680, len(cigar),
                       flag, l_seq, mrefid, mpos, tlen)
    return head + name + b"\0" + words + bytes(seq4) + bytes(qual) + bytes(tags)


def pack_seq(letters):
    """ASCII bases -> BAM's packed sequence bytes (high nibble first; the last low nibble of an odd length is 0)"""
    out = bytearray((len(letters) + 1) // 2)
    for i, ch in enumerate(letters):
        c = BASE_CODES.find(ch if isinstance(ch, str) else chr(int(ch)))
        out[i // 2] |= (c if c >= 0 else 15) << (0 if i % 2 else 4)
    return bytes(out)


def parse_record(blob, off, avail):
    """the fields the call reads of the record at blob[off:off + avail]; None: a bad record"""
    if off > len(blob) or avail > len(blob) - off or avail < 32:
        return None
    b = bytes(blob[off:off + avail])
    refid, pos, l_name, mapq, _bin, n_cigar, flag, l_seq, _mref, _mpos, tlen = struct.unpack_from("<iiBBHHHiiii", b, 0)
    if l_seq <= 0 or l_name == 0 or 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > avail:
        return None
    p = 32
    name = b[p:p + l_name - 1]
    p += l_name
    cigar = [(v >> 4, v & 15) for v in struct.unpack_from("<%dI" % n_cigar, b, p)]
    p += 4 * n_cigar
    seq4 = b[p:p + (l_seq + 1) // 2]
    p += (l_seq + 1) // 2
    qual = b[p:p + l_seq]
    return dict(refid=refid, pos=pos, mapq=mapq, flag=flag, l_seq=l_seq, tlen=tlen, name=name, cigar=cigar, seq4=seq4, qual=qual)


def flatten(rec, n_windows, n_records, n_refs=0, bases_cap=None):
    """rec: dict of the ma_records_t arrays (ref_map only with n_refs > 0).  Returns a dict of the ma_flat_out_t arrays, bases4
    and read_quals as long as what the call defines: (n_bases + n_records + 1) // 2 and n_bases bytes.  Raises FlattenError."""
    blob = np.asarray(rec["blob"], dtype=np.uint8).tobytes()
    rec_off = [int(x) for x in np.asarray(rec["rec_off"])[:n_records]]
    rec_len = [int(x) for x in np.asarray(rec["rec_len"])[:n_records]]
    win_off = [int(x) for x in np.asarray(rec["rec_win_off"])[:n_windows + 1]]
    smp = [int(x) for x in np.asarray(rec["rec_sample"])[:n_records]]
    s_index, s_case, s_rank = (np.asarray(rec[k]) for k in ("sample_index", "sample_case", "sample_rank"))
    n_samples = len(s_rank)
    ref_map = np.asarray(rec["ref_map"]).reshape(n_samples, n_refs) if n_refs > 0 and rec.get("ref_map") is not None else None
    if win_off[0] != 0 or win_off[-1] != n_records or any(b < a for a, b in zip(win_off, win_off[1:])):
        raise FlattenError(MA_ERR_ARG, "rec_win_off does not rise from 0 to n_records")
    for w in range(n_windows):
        if win_off[w + 1] - win_off[w] > MAX_WINDOW:
            raise FlattenError(MA_ERR_PARAM, "window %d is too large" % w)
    parsed, first_bad = [], None
    for i in range(n_records):
        r = parse_record(blob, rec_off[i], rec_len[i]) if smp[i] < n_samples else None
        if r is None and first_bad is None:
            first_bad = i
        parsed.append(r)
    n_bases = sum(r["l_seq"] for r in parsed if r is not None)
    if first_bad is not None:
        raise FlattenError(MA_ERR_ARG, "record %d is bad" % first_bad, record=first_bad, n_bases=n_bases)
    if bases_cap is not None and n_bases > bases_cap:
        raise FlattenError(MA_ERR_ARG, "%d bases do not fit %d" % (n_bases, bases_cap), n_bases=n_bases)

    def chrom_of(i):
        rid = parsed[i]["refid"]
        if rid < 0 or rid >= n_refs:
            return -1
        return int(ref_map[smp[i], rid]) if ref_map is not None else rid

    n = n_records
    out = dict(n_bases=np.array([n_bases], dtype=np.uint64), read_off=np.zeros(n + 1, dtype=np.uint64),
               bases4=np.zeros((n_bases + n + 1) // 2, dtype=np.uint8), read_quals=np.zeros(n_bases, dtype=np.uint8),
               read_qname_id=np.zeros(n, dtype=np.uint32), read_sample=np.zeros(n, dtype=np.uint8),
               read_flags=np.zeros(n, dtype=np.uint8), read_hint=np.zeros(n, dtype=np.int32), read_mapq=np.zeros(n, dtype=np.uint8),
               read_mflags=np.zeros(n, dtype=np.uint8), read_isize=np.zeros(n, dtype=np.int32),
               read_start=np.zeros(n, dtype=np.int32), read_src=np.zeros(n, dtype=np.uint32))
    at = 0
    for w in range(n_windows):
        members = list(range(win_off[w], win_off[w + 1]))
        members.sort(key=lambda i: (0 if parsed[i]["mapq"] >= 20 else 1, int(s_rank[smp[i]]), parsed[i]["name"], chrom_of(i),
                                    parsed[i]["pos"], i))
        ids = {}
        for k, i in enumerate(members):
            r, o = parsed[i], win_off[w] + k
            out["read_src"][o] = i
            out["read_qname_id"][o] = ids.setdefault(r["name"], len(ids))
            out["read_sample"][o] = s_index[smp[i]]
            out["read_flags"][o] = ((MA_RF_PASS if r["mapq"] >= 20 else 0) | (MA_RF_CASE if int(s_case[smp[i]]) == 1 else 0) |
                                    (MA_RF_REV if r["flag"] & 0x10 else 0))
            lead = r["cigar"][0][0] if r["cigar"] and r["cigar"][0][1] == 4 else 0
            hint = r["pos"] - int(rec["win_start0"][w]) - lead
            ok = chrom_of(i) == int(rec["win_chrom"][w]) and -(1 << 31) < hint < (1 << 31) - 1
            out["read_hint"][o] = hint if ok else MA_NO_HINT
            out["read_mapq"][o] = r["mapq"]
            clip = sum(ln for ln, op in r["cigar"] if op == 4) & 0xFFFFFFFF
            out["read_mflags"][o] = ((MA_RM_SOFTCLIP if float(clip) / float(r["l_seq"]) >= 0.06 else 0) |
                                     (MA_RM_PROPER if r["flag"] & 0x2 else 0))
            out["read_isize"][o] = r["tlen"]
            out["read_start"][o] = max(0, r["pos"])
            out["read_off"][o] = at
            b4 = (at + o) >> 1
            out["bases4"][b4:b4 + len(r["seq4"])] = np.frombuffer(r["seq4"], dtype=np.uint8)
            q = np.frombuffer(r["qual"], dtype=np.uint8).copy()
            q[q == 0xFF] = 0
            out["read_quals"][at:at + r["l_seq"]] = q
            at += r["l_seq"]
    out["read_off"][n] = at
    return out
