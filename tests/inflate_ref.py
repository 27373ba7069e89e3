"""Plain-Python restatement of ma_inflate_blocks_batch and ma_index_records_batch as include/microasm.h states them: the header
rules, the block states, the layout of raw, the record walk.  The payloads and CRCs are zlib's (decompressobj(-15), crc32),
which shares nothing with the kernels."""
import struct
import zlib

import numpy as np

MA_Z_HEADER, MA_Z_ISIZE, MA_Z_DATA, MA_Z_SHORT, MA_Z_CRC = 1, 2, 4, 8, 16
MA_X_BAD_RECORD = 1


class InflateError(Exception):
    """a call-level MA_ERR_ARG; .which: the block or stream it names, None for a capacity; .need: the capacity needed"""

    def __init__(self, text, which=None, need=None):
        super().__init__(text)
        self.which, self.need = which, need


def parse_member(m):
    """m: the bytes available for the member -> (state, data, crc, isize); data is None unless the state is 0"""
    bad = (MA_Z_HEADER, None, 0, 0)
    if len(m) < 20 or m[0] != 0x1f or m[1] != 0x8b or m[2] != 8 or not m[3] & 4:
        return bad
    xlen = m[10] | (m[11] << 8)
    if 12 + xlen + 8 > len(m):
        return bad
    at, total = 12, 0
    while at + 4 <= 12 + xlen:
        slen = m[at + 2] | (m[at + 3] << 8)
        if at + 4 + slen > 12 + xlen:
            return bad
        if m[at:at + 2] == b"BC" and slen == 2:
            total = (m[at + 4] | (m[at + 5] << 8)) + 1
        at += 4 + slen
    if total < 12 + xlen + 8 or total > len(m):
        return bad
    crc, isize = struct.unpack("<II", m[total - 8:total])
    if isize > 65536:
        return (MA_Z_ISIZE, None, crc, 0)
    return (0, m[12 + xlen:total - 8], crc, isize)


def zlib_inflate(data):
    """-> the payload of a whole raw DEFLATE stream; raises zlib.error on an invalid one and on one that needs more input.
    Bytes behind the end of the stream are not an error"""
    d = zlib.decompressobj(-15)
    out = d.decompress(data)
    if not d.eof:
        raise zlib.error("the stream needs more input")
    return out


def member_state(m):
    """-> (state, payload size, payload or None)"""
    state, data, crc, isize = parse_member(m)
    if state:
        return state, 0, None
    try:
        payload = zlib_inflate(data)
    except zlib.error:
        return MA_Z_DATA, isize, None
    if len(payload) > isize:
        return MA_Z_DATA, isize, None
    if len(payload) < isize:
        return MA_Z_SHORT, isize, None
    if zlib.crc32(payload) != crc:
        return MA_Z_CRC, isize, None
    return 0, isize, payload


def inflate(cblob, blk_off, blk_len, raw_cap=None):
    """-> dict of the arrays of ma_inflate_out_t; raw holds zeros in the ranges of flagged blocks, `defined` is the mask of the
    bytes that are defined"""
    blob = bytes(cblob)
    for b, (off, n) in enumerate(zip(blk_off, blk_len)):
        if int(off) + int(n) > len(blob):
            raise InflateError(f"block {b} does not lie inside cblob", which=b)
    parts, defined, states, offs = [], [], [], [0]
    for off, n in zip(blk_off, blk_len):
        state, size, payload = member_state(blob[int(off):int(off) + int(n)])
        states.append(state)
        parts.append(payload if payload is not None else bytes(size))
        defined.append(np.full(size, payload is not None, bool))
        offs.append(offs[-1] + size)
    if raw_cap is not None and offs[-1] > raw_cap:
        raise InflateError("raw_cap is under the need", need=offs[-1])
    return dict(raw=np.frombuffer(b"".join(parts), np.uint8), blk_raw_off=np.array(offs, np.uint64), blk_state=np.array(states, np.uint8),
                n_raw=np.array([offs[-1]], np.uint64), n_flagged=np.array([sum(s != 0 for s in states)], np.uint64),
                defined=np.concatenate(defined) if defined else np.zeros(0, bool))


def walk(raw, begin, end):
    """one stream -> ([(rec_off, rec_len)], state)"""
    found, p, n = [], int(begin), len(raw)
    while p < end:
        if n - p < 4:
            return found, MA_X_BAD_RECORD
        bs = struct.unpack_from("<I", raw, p)[0]
        if p + 4 + bs > n or bs < 32:
            return found, MA_X_BAD_RECORD
        l_name, n_cigar, l_seq = raw[p + 4 + 8], struct.unpack_from("<H", raw, p + 4 + 12)[0], struct.unpack_from("<I", raw, p + 4 + 16)[0]
        if 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > bs:
            return found, MA_X_BAD_RECORD
        found.append((p + 4, bs))
        p += 4 + bs
    return found, 0


def index(raw, str_begin, str_end, rec_cap=None):
    """-> dict of the arrays of ma_index_out_t"""
    raw = bytes(raw)
    for s, (b, e) in enumerate(zip(str_begin, str_end)):
        if int(b) > int(e) or int(e) > len(raw):
            raise InflateError(f"stream {s} has bad bounds", which=s)
    recs, states, offs = [], [], [0]
    for b, e in zip(str_begin, str_end):
        found, state = walk(raw, int(b), int(e))
        recs += found
        states.append(state)
        offs.append(len(recs))
    if rec_cap is not None and len(recs) > rec_cap:
        raise InflateError("rec_cap is under the need", need=len(recs))
    ref, pos, span = [], [], []
    for off, _ in recs:
        r, p = struct.unpack_from("<ii", raw, off)
        l_name, n_cigar = raw[off + 8], struct.unpack_from("<H", raw, off + 12)[0]
        words = struct.unpack_from(f"<{n_cigar}I", raw, off + 32 + l_name)
        ref.append(r)
        pos.append(p)
        span.append(sum(w >> 4 for w in words if w & 15 in (0, 2, 3, 7, 8)) & 0xFFFFFFFF)
    return dict(n_found=np.array([len(recs)], np.uint64), str_rec_off=np.array(offs, np.uint64), str_state=np.array(states, np.uint8),
                rec_off=np.array([o for o, _ in recs], np.uint64), rec_len=np.array([n for _, n in recs], np.uint32),
                rec_ref=np.array(ref, np.int32), rec_pos=np.array(pos, np.int32), rec_span=np.array(span, np.uint32))
