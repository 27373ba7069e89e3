"""BGZF members for ma_inflate_blocks_batch and record streams for ma_index_records_batch, one rule of include/microasm.h
each, shared by tests/test_inflate_cases.py (zlib and the restatement against what the rule says, the decode core on the host)
and tests/test_gpu_inflate.py (the kernels against zlib and the restatement).

A member case is (label, member bytes, expected blk_state, expected payload or None).  zlib made the streams of the first group;
the second group comes from the bit writer below, token lists with chosen code lengths, and states its payload from the tokens
alone; the corrupt group names the state bit each must get."""
import struct
import zlib

import numpy as np

import flatten_ref

HEADER, ISIZE, DATA, SHORT, CRC = 1, 2, 4, 8, 16  # MA_Z_*
BAD_RECORD = 1  # MA_X_BAD_RECORD


# ---- members ----------------------------------------------------------------------------------------------------------------------
def member(data, payload=b"", isize=None, crc=None, extra=None, magic=b"\x1f\x8b\x08\x04", bsize=None, pad=b""):
    """a BGZF member around the DEFLATE bytes `data`; `pad`: unused bytes between the stream and the trailer"""
    if extra is None:
        extra = b"BC\x02\x00" + struct.pack("<H", (12 + 6 + len(data) + len(pad) + 8 - 1 if bsize is None else bsize) & 0xFFFF)
    head = magic + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", len(extra)) + extra
    return head + data + pad + struct.pack("<II", zlib.crc32(payload) if crc is None else crc, len(payload) if isize is None else isize)


def with_bsize(extra_of, data, payload):
    """a member whose extra field is extra_of(BSIZE): the size depends on the extra field's own length"""
    n = len(extra_of(0))
    return member(data, payload, extra=extra_of(12 + n + len(data) + 8 - 1))


def deflate(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(payload) + c.flush()


EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# ---- the bit writer ---------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        """nbits of value, least significant first (header fields, extra bits)"""
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):
        """a Huffman code, most significant bit first"""
        for k in range(nbits - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """code lengths -> {symbol: (code, length)} (RFC 1951 section 3.2.2); works for over-subscribed and incomplete sets too"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def flat_lengths(symbols, n):
    """a complete code over `symbols`: lengths k or k + 1; -> a list of n lengths"""
    symbols = sorted(symbols)
    m = len(symbols)
    k = m.bit_length() - 1
    longer = 2 * (m - (1 << k))
    lens = [0] * n
    for i, s in enumerate(symbols):
        lens[s] = k if i < m - longer else k + 1
    return lens


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CLEN_LENS = [5] * 16 + [2, 3, 3]  # a complete code-length code: every length plainly, and the three repeat codes
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def len_symbol(length):
    if length == 258:
        return 28
    return max(i for i in range(28) if LEN_BASE[i] <= length)


def dist_symbol(dist):
    return max(i for i in range(30) if DIST_BASE[i] <= dist)


def put_tokens(w, tokens, lit_lens, dist_lens):
    """tokens: an int is a literal/length SYMBOL as it is (256 ends the block), ('m', length, distance) a match,
    ('raw', code, nbits) a bit pattern"""
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        elif t[0] == "raw":
            w.code(t[1], t[2])
        else:
            _, length, d = t
            ls, ds = len_symbol(length), dist_symbol(d)
            w.code(*lit[257 + ls])
            w.put(length - LEN_BASE[ls], LEN_EXTRA[ls])
            w.code(*dist[ds])
            w.put(d - DIST_BASE[ds], DIST_EXTRA[ds])


def dynamic(w, tokens, lit_lens, dist_lens, final=1, cl_seq=None, cl_lens=CLEN_LENS, hlit=None, hdist=None):
    """a dynamic block: the code lengths as cl_seq says -- (symbol, extra value) pairs of the code-length code, default every
    length plainly -- then the tokens.  hlit / hdist: the FIELD values, default from the lists' lengths"""
    w.put(final, 1)
    w.put(2, 2)
    w.put(len(lit_lens) - 257 if hlit is None else hlit, 5)
    w.put(len(dist_lens) - 1 if hdist is None else hdist, 5)
    last = max(i for i, s in enumerate(CLEN_ORDER) if cl_lens[s]) + 1 if any(cl_lens) else 4
    last = max(last, 4)
    w.put(last - 4, 4)
    for s in CLEN_ORDER[:last]:
        w.put(cl_lens[s], 3)
    cl = canonical(cl_lens)
    if cl_seq is None:
        cl_seq = [(l, None) for l in list(lit_lens) + list(dist_lens)]
    for s, extra in cl_seq:
        w.code(*cl[s])
        if s >= 16:
            w.put(extra, {16: 2, 17: 3, 18: 7}[s])
    put_tokens(w, tokens, lit_lens, dist_lens)


def fixed(w, tokens, final=1):
    w.put(final, 1)
    w.put(1, 2)
    put_tokens(w, tokens, FIXED_LIT, FIXED_DIST)


def stored(w, data, final=1, nlen=None):
    w.put(final, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put(len(data) ^ 0xFFFF if nlen is None else nlen, 16)
    w.out += data


def play(tokens):
    """the payload a token list stands for"""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            if t < 256:
                out.append(t)
        elif t[0] == "m":
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out)


def one_dynamic(tokens, lit_lens, dist_lens, **kw):
    w = Bits()
    dynamic(w, tokens, lit_lens, dist_lens, **kw)
    return w.bytes()


def _text(n, seed):
    """compressible bytes: words of a small alphabet"""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(65, 91, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))]
        if rng.integers(0, 7) == 0:
            out += bytes(rng.integers(0, 256, 3, dtype=np.uint8))
    return bytes(out[:n])


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def zlib_cases():
    text = _text(5000, 1)
    runs = b"".join(bytes([65 + i % 7]) * (1 + (i * 37) % 300) for i in range(40))
    out = [("level 0 (stored)", deflate(text, 0), text), ("Z_FIXED", deflate(text, 6, zlib.Z_FIXED), text),
           ("level 1", deflate(text, 1), text), ("level 9", deflate(text, 9), text), ("Z_RLE", deflate(runs, 6, zlib.Z_RLE), runs),
           ("Z_HUFFMAN_ONLY", deflate(text, 6, zlib.Z_HUFFMAN_ONLY), text), ("noise, level 6", deflate(_noise(3000, 2), 6), _noise(3000, 2))]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    parts = c.compress(text[:1500]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[1500:3100]) + c.flush(zlib.Z_SYNC_FLUSH) + \
        c.compress(text[3100:]) + c.flush()
    out.append(("several DEFLATE blocks, full and sync flush", parts, text))
    for n, what in ((1, "ISIZE 1"), (65280, "ISIZE 65280"), (65536, "ISIZE 65536")):
        payload = _text(n, 10 + n % 7)
        out.append((what, deflate(payload, 6), payload))
    out.append(("65000 bytes of noise, stored", deflate(_noise(65000, 3), 0), _noise(65000, 3)))
    return [(label, member(d, p), 0, p) for label, d, p in out]


def _nine_bit_tail():
    """a fixed block of 73 bits: the last byte holds one bit of the end-of-block code"""
    w = Bits()
    tokens = [200 + i for i in range(7)] + [256]
    fixed(w, tokens)
    assert w.n == 1
    return w.bytes(), play(tokens)


def hand_cases():
    out = []
    # literal codes of every length up to 15
    syms = list(range(65, 80)) + [256]
    lens = [0] * 257
    for i, s in enumerate(syms):
        lens[s] = min(i + 1, 15)
    tokens = [65 + (i * i) % 15 for i in range(300)] + [79, 78, 256]
    out.append(("literal codes of 15 bits", one_dynamic(tokens, lens, [0]), tokens))
    # one distance code of length 1; length 258 at distance 1
    lens = flat_lengths([120, 121, 256, 257, 285], 286)
    tokens = [120, ("m", 258, 1), 121, ("m", 3, 1), ("m", 258, 1), 256]
    out.append(("a single distance code of length 1, length 258 at distance 1", one_dynamic(tokens, lens, [1]), tokens))
    # copies that overlap their own output, at distances around the lane count
    w = Bits()
    tokens = list(b"abc") + [("m", 258, 3), ("m", 100, 2), ("m", 70, 65)] + list(range(70)) + [("m", 258, 63), ("m", 258, 64), ("m", 129, 65),
                                                                                         ("m", 64, 64), ("m", 65, 64), ("m", 3, 700), 256]
    fixed(w, tokens)
    out.append(("periodic fills", w.bytes(), tokens))
    # the far end of the window
    rng = np.random.default_rng(5)
    lens = flat_lengths([97, 98, 99, 100, 256, 257, 258], 259)
    tokens = [int(x) for x in rng.integers(97, 101, 32768)] + [("m", 3, 32768), 97, ("m", 4, 32768), 256]
    out.append(("length 3 at distance 32768 after 32768 literals", one_dynamic(tokens, lens, [0] * 29 + [1]), tokens))
    # repeats that run from the literal/length lengths into the distance lengths
    head = [(18, 65 - 11), (1, None), (2, None), (18, 138 - 11), (18, 51 - 11)]  # 65 zeros, 'A': 1, 'B': 2, 189 zeros
    tokens = [65, 66, 65, 65, 66, 256]
    lit = [0] * 65 + [1, 2] + [0] * 189
    out.append(("repeat 16 across the boundary", one_dynamic(tokens, lit + [2], [2, 2, 2, 2], cl_seq=head + [(2, None), (16, 1)]), tokens))
    out.append(("repeat 17 across the boundary", one_dynamic(tokens, lit + [2, 0], [0, 0, 1], cl_seq=head + [(2, None), (17, 0), (1, None)]), tokens))
    out.append(("repeat 18 across the boundary", one_dynamic(tokens, lit + [2, 0, 0, 0], [0] * 10 + [1],
                                                             cl_seq=head + [(2, None), (18, 2), (1, None)]), tokens))
    out.append(("HLIT 257 and HDIST 1, no distance code at all", one_dynamic(tokens, lit + [2], [0]), tokens))
    # stored blocks of LEN 0 and of the greatest LEN a member has room for: BSIZE is 16 bits wide, so a member is 65536 bytes at
    # the most, 26 of them header and trailer, 5 per stored block's own fields -- LEN 65535 cannot occur in a BGZF member
    w = Bits()
    big = _noise(65536 - 26 - 15, 6)
    stored(w, b"", final=0)
    stored(w, big, final=0)
    stored(w, b"", final=1)
    assert len(member(w.bytes())) == 65536
    out.append(("stored blocks of LEN 0 and LEN 65495: a member of 65536 bytes", w.bytes(), [b for b in big]))
    # mixed block types in one member, the bit position carried over a stored block
    w = Bits()
    fixed(w, [72, 105, 256], final=0)
    stored(w, b" there", final=0)
    dynamic(w, [65, 66, 256], lit + [2], [0], final=0)
    fixed(w, [("raw", 0, 0)] + [33, ("m", 5, 1), 256], final=1)
    out.append(("fixed, stored, dynamic, fixed in one member", w.bytes(), [b for b in b"Hi thereAB!!!!!!"]))
    data, payload = _nine_bit_tail()
    out.append(("the last byte holds one bit", data, [b for b in payload]))
    return [(label, member(d, play(t)), 0, play(t)) for label, d, t in out]


def layout_cases():
    """good members whose point is the header or what surrounds the stream"""
    text = _text(700, 20)
    d = deflate(text)
    return [
        ("the BGZF end-of-file member", EOF_MEMBER, 0, b""),
        ("unused bytes in front of the trailer", member(d, text, pad=b"\x00\xff\x13"), 0, text),
        ("another subfield in front of BC", with_bsize(lambda b: b"XY\x03\x00abc" + b"BC\x02\x00" + struct.pack("<H", b), d, text), 0, text),
        ("a BC subfield of another length is passed by", with_bsize(lambda b: b"BC\x01\x00z" + b"BC\x02\x00" + struct.pack("<H", b), d, text), 0, text),
        ("two BC subfields: the last counts", with_bsize(lambda b: b"BC\x02\x00\x05\x00" + b"BC\x02\x00" + struct.pack("<H", b), d, text), 0, text),
        ("three stray bytes behind the subfields", with_bsize(lambda b: b"BC\x02\x00" + struct.pack("<H", b) + b"\x01\x02\x03", d, text), 0, text),
        ("other FLG bits beside bit 2", member(d, text, magic=b"\x1f\x8b\x08\xff"), 0, text),
    ]


def corrupt_cases():
    text = _text(900, 30)
    d = deflate(text)
    good = member(d, text)
    lit = [0] * 65 + [1, 2] + [0] * 189 + [2]
    tokens = [65, 66, 256]
    out = []

    def header(label, m):
        out.append((label, m, HEADER, None))

    header("magic byte 0", b"\x1e" + good[1:])
    header("magic byte 1", good[:1] + b"\x8a" + good[2:])
    header("CM is not 8", member(d, text, magic=b"\x1f\x8b\x07\x04"))
    header("FLG without bit 2", member(d, text, magic=b"\x1f\x8b\x08\x03"))
    header("no BC subfield", with_bsize(lambda b: b"BD\x02\x00" + struct.pack("<H", b), d, text))
    header("no extra field at all", member(d, text, extra=b""))
    header("BC of length 3 alone", with_bsize(lambda b: b"BC\x03\x00" + struct.pack("<H", b) + b"\0", d, text))
    header("a subfield beyond the extra field", with_bsize(lambda b: b"BC\x02\x00" + struct.pack("<H", b) + b"XY\x09\x00ab", d, text))
    header("BSIZE + 1 under 12 + XLEN + 8", member(b"", b"", bsize=24))
    header("BSIZE + 1 over the bytes there are", member(d, text, bsize=len(good)))
    header("fewer than 20 bytes", good[:19])
    out.append(("ISIZE 65537", member(d, text, isize=65537), ISIZE, None))

    def data(label, stream, payload=b"", **kw):
        out.append((label, member(stream, payload, **kw), DATA, None))

    w = Bits()
    w.put(1, 1)
    w.put(3, 2)
    data("block type 3", w.bytes())
    w = Bits()
    stored(w, b"abcd", nlen=0x1234)
    data("stored LEN is not ~NLEN", w.bytes(), b"abcd")
    data("HLIT 287", one_dynamic(tokens, lit, [0], hlit=30), b"ABA")
    data("HDIST 31", one_dynamic(tokens, lit, [0], hdist=30), b"ABA")
    data("an over-subscribed code-length code", one_dynamic(tokens, lit, [0], cl_lens=[5] * 16 + [2, 2, 2]), b"AB")
    data("an incomplete code-length code", one_dynamic(tokens, lit, [0], cl_lens=[5] * 16 + [2, 3, 4]), b"AB")
    data("a code-length code of one code", one_dynamic([], [], [], cl_lens=[1] + [0] * 18, cl_seq=[(0, None)] * 258, hlit=0, hdist=0), b"")
    over = [0] * 65 + [1, 1] + [0] * 189 + [2]
    data("an over-subscribed literal/length code", one_dynamic(tokens, over, [0]), b"AB")
    under = [0] * 65 + [2, 2] + [0] * 189 + [2]
    data("an incomplete literal/length code", one_dynamic(tokens, under, [0]), b"AB")
    lit_m = flat_lengths([65, 66, 256, 257], 258)
    data("an over-subscribed distance code", one_dynamic(tokens, lit_m, [1, 1, 1]), b"AB")
    data("an incomplete distance code", one_dynamic(tokens, lit_m, [2, 2]), b"AB")
    head = [(18, 65 - 11), (1, None), (2, None), (18, 138 - 11), (18, 51 - 11), (2, None)]
    data("repeat 16 with no previous length", one_dynamic(tokens, lit, [0], cl_seq=[(16, 0)] + head[1:] + [(0, None)]), b"AB")
    data("a repeat past HLIT + HDIST", one_dynamic(tokens, lit, [0], cl_seq=head + [(17, 0)]), b"AB")
    data("no code for symbol 256", one_dynamic([65, 66], [0] * 65 + [1, 1] + [0] * 190, [0]), b"AB")
    for s in (286, 287):
        w = Bits()
        fixed(w, [65, s, 256])
        data(f"literal/length symbol {s}", w.bytes(), b"A")
    for s in (30, 31):
        w = Bits()
        fixed(w, [65, 257, ("raw", s, 5), 256])
        data(f"distance symbol {s}", w.bytes(), b"AAAA")
    w = Bits()
    fixed(w, [65, 66, ("m", 3, 3), 256])
    data("a distance in front of the block's output", w.bytes(), b"ABABA")
    data("a distance with no distance code", one_dynamic([65, ("raw", 3, 2), ("raw", 0, 1), 256], lit_m, [0]), b"AAAA")
    data("the other pattern of a single code of length 1", one_dynamic([65, ("raw", 3, 2), ("raw", 1, 1), 256], lit_m, [1]), b"AAAA")
    data("one byte short", d[:-1], text)
    tail, payload = _nine_bit_tail()
    data("one bit short", tail[:-1], payload)
    data("a stored block longer than the data", deflate(text, 0)[:-5], text)
    data("ISIZE one too small", d, text, isize=len(text) - 1, crc=zlib.crc32(text[:-1]))
    out.append(("ISIZE one too large", member(d, text, isize=len(text) + 1), SHORT, None))
    out.append(("ISIZE 5 of the end-of-file member's stream", member(b"\x03\x00", b"", isize=5), SHORT, None))
    for k in range(4):
        out.append((f"CRC byte {k} flipped", member(d, text, crc=zlib.crc32(text) ^ (0x40 << (8 * k))), CRC, None))
    return out


def all_members():
    return zlib_cases() + hand_cases() + layout_cases() + corrupt_cases()


def lay_out(members, rng=None, slack=0):
    """members -> (cblob, blk_off, blk_len): junk of odd lengths between them when rng is given; slack: blk_len beyond the member"""
    blob, off, length = bytearray(), [], []
    for k, m in enumerate(members):
        if rng is not None:
            blob += bytes(rng.integers(0, 256, 1 + 2 * int(rng.integers(0, 6)), dtype=np.uint8))
        off.append(len(blob))
        blob += m
        length.append(len(m))
    if rng is not None or slack:
        blob += bytes(max(slack, 7))
    length = [n + slack for n in length]
    return np.frombuffer(bytes(blob), np.uint8).copy(), np.array(off, np.uint64), np.array(length, np.uint32)


def dump(path, members):
    """the case table for tests/host/inflate_units.cpp: per case u32 member bytes, the member, u32 state, u32 payload bytes, payload"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(members)))
        for _, m, state, payload in members:
            p = payload if payload is not None else b""
            f.write(struct.pack("<I", len(m)) + m + struct.pack("<II", state, len(p)) + p)


# ---- record streams ---------------------------------------------------------------------------------------------------------------
def record(name=b"r", pos=100, ref=0, cigar=((10, "M"),), l_seq=10, tags=b"", flag=0):
    """-> block_size field + record"""
    body = flatten_ref.encode_record(name, flag=flag, pos=pos, mapq=60, cigar=list(cigar), seq4=bytes((l_seq + 1) // 2),
                                     qual=bytes([30] * l_seq), tags=tags, refid=ref)
    return struct.pack("<I", len(body)) + body


EVERY_OP = ((3, "M"), (2, "I"), (4, "D"), (100, "N"), (5, "S"), (6, "H"), (7, "P"), (8, "="), (9, "X"))  # span 3 + 4 + 100 + 8 + 9


def stream_cases():
    """-> (raw, str_begin, str_end, {label: stream}) -- hand-made records; what each stream must give is asserted in
    tests/test_inflate_cases.py"""
    raw, begin, end, names = bytearray(b"BAM\1 a header of some kind"), [], [], {}

    def add(label, b, e):
        names[label] = len(begin)
        begin.append(b)
        end.append(e)

    def put(recs):
        at = []
        for r in recs:
            at.append(len(raw))
            raw.extend(r)
        return at + [len(raw)]

    a = put([record(b"a%d" % i, pos=100 + i) for i in range(5)])
    add("no record", a[0], a[0])
    add("one record", a[0], a[0] + 1)
    add("ends exactly at a record's start", a[0], a[2])
    add("ends one byte behind a record's start", a[0], a[2] + 1)
    add("shares records with the stream in front", a[1], a[4])
    b = put([record(b"every", cigar=EVERY_OP, l_seq=27, pos=-1, ref=-1), record(b"none", cigar=(), l_seq=4, pos=2**31 - 1, ref=7),
             record(b"wrap", cigar=((2**28 - 1, "M"),) * 17, l_seq=3), record(b"tags", tags=b"NMi\1\0\0\0" + b"MDZ10\0")])
    add("every operation, no CIGAR, negative pos and refID, a span that wraps, tags", b[0], b[-1])
    c = put([record(b"ok"), struct.pack("<I", 31) + bytes(31)])
    add("block_size 31", c[0], c[-1])
    d = put([record(b"ok"), record(b"short")[:4 + 32 + 3]])
    raw[d[1]:d[1] + 4] = struct.pack("<I", 35)  # a block_size that does not hold the core
    add("a core beyond block_size", d[0], d[-1])
    e = put([record(b"ok"), record(b"huge")])
    raw[e[1] + 4 + 16:e[1] + 4 + 20] = struct.pack("<i", -1)  # l_seq -1: read as unsigned
    add("l_seq -1", e[0], e[-1])
    f = put([record(b"ok"), record(b"last")])
    raw[f[1]:f[1] + 4] = struct.pack("<I", len(raw) - f[1] - 4 + 1)  # one byte past the end of raw
    add("block_size past raw_bytes", f[0], f[-1])
    add("a block_size field cut by the end of raw", len(raw) - 3, len(raw))
    add("at the end of raw", len(raw), len(raw))
    return np.frombuffer(bytes(raw), np.uint8).copy(), np.array(begin, np.uint64), np.array(end, np.uint64), names
