"""Developer tool: what ma_inflate_blocks_batch and ma_index_records_batch cost, beside zlib on 16 host
threads -- what the host shell does today, a block at a time.
The records of tools/flatten_cost.py (C3 workload, 60x tumour / 30x normal, 64 synthesised windows encoded as BAM records, tiled
to 8192 windows), laid out as a BAM record stream (block_size in front of every record, no padding) and written as BGZF blocks
of at most 65280 payload bytes with Python's zlib (level 6); the 64 windows' blocks are tiled, so every window has bytes of its
own.  Timing mode 2, the median of three runs with the runs beside it: the kernels one by one, the whole call with host arrays
and with device arrays, compressed bytes up against inflated bytes, then ma_index_records_batch on the result, a stream per
window.
usage: python tools/inflate_cost.py [windows]"""
import os
import statistics
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import flatten_ref as ref  # noqa: E402
from harness import DeviceArena  # noqa: E402
from lancet2_amd import capi, synth  # noqa: E402
from lancet2_amd.engine import Engine  # noqa: E402

n_want = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
PAYLOAD = 65280
params = capi.default_params(min_k=25, max_k=25)
arrs, nw, nr = synth.make_config_batch("C3", 64, first_index=0)
rng = np.random.default_rng(1)
stream, win_at = bytearray(), [0]
order = np.concatenate([rng.permutation(np.arange(int(arrs["read_win_off"][w]), int(arrs["read_win_off"][w + 1]))) for w in range(nw)])
for w in range(nw):
    for r in order[int(arrs["read_win_off"][w]):int(arrs["read_win_off"][w + 1])]:
        o0, o1 = int(arrs["read_off"][r]), int(arrs["read_off"][r + 1])
        fl, hint = int(arrs["read_flags"][r]), int(arrs["read_hint"][r])
        name = b"A00123:45:HXXXXXXXX:1:%d:%d:%d" % (1101 + w % 7, 1000 + 37 * int(arrs["read_qname_id"][r]), 2000 + 11 * w)
        body = ref.encode_record(name, flag=(0x10 if fl & 4 else 0) | 0x3, refid=0, pos=100_000 + 2000 * w + (hint if hint != capi.MA_NO_HINT else 0),
                                 mapq=60 if fl & 1 else 7, cigar=[(o1 - o0, "M")], seq4=ref.pack_seq(arrs["read_bases"][o0:o1]),
                                 qual=arrs["read_quals"][o0:o1].tobytes(), tlen=300)
        stream += struct.pack("<I", len(body)) + body
    win_at.append(len(stream))
stream = bytes(stream)
members = []
for at in range(0, len(stream), PAYLOAD):
    data = stream[at:at + PAYLOAD]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    cdata = c.compress(data) + c.flush()
    members.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(cdata) + 25) + cdata + struct.pack("<II", zlib.crc32(data), len(data)))
times = max(1, n_want // nw)
one = np.frombuffer(b"".join(members), np.uint8)
one_off = np.cumsum([0] + [len(m) for m in members[:-1]]).astype(np.uint64)
cblob = np.tile(one, times)
blk_off = np.concatenate([one_off + np.uint64(t * one.size) for t in range(times)])
blk_len = np.tile(np.array([len(m) for m in members], np.uint32), times)
n_blocks, raw_bytes = len(blk_off), len(stream) * times
str_begin = np.concatenate([np.array(win_at[:-1], np.uint64) + np.uint64(t * len(stream)) for t in range(times)])
str_end = np.concatenate([np.array(win_at[1:], np.uint64) + np.uint64(t * len(stream)) for t in range(times)])
n_rec = nr * times
med = statistics.median
print(f"library {capi.LIB_PATH}: windows {nw * times} records {n_rec} blocks {n_blocks}; compressed {cblob.size} bytes up, "
      f"inflated {raw_bytes} bytes ({raw_bytes / cblob.size:.2f} x); the index brings {20 * n_rec} bytes back")


def show(what, runs):
    print(f"{what}: {med(runs):.2f} ms (runs {[round(x, 2) for x in runs]})")


# the yardstick: the same blocks, zlib on 16 threads (decompress releases the GIL)
deflated = [bytes(m[18:-8]) for m in members]


def inflate_some(k):
    return sum(len(zlib.decompressobj(-15).decompress(deflated[i % len(deflated)])) for i in range(k, n_blocks, 16))


walls = []
for _ in range(3):
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as pool:
        assert sum(pool.map(inflate_some, range(16))) == raw_bytes
    walls.append((time.perf_counter() - t0) * 1e3)
show("zlib, 16 host threads, no CRC", walls)
zlib_ms = med(walls)

eng = Engine(params)
try:
    def timed(fn):
        eng.timing_control(2)
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        t = {}
        for k, v in eng.kernel_times():
            t[k] = t.get(k, 0.0) + v
        return t, wall, out

    def report(what, fn):
        timed(fn)  # warm-up: workspaces
        runs = [timed(fn) for _ in range(3)]
        show(f"{what}, host arrays: kernels", [sum(t.values()) for t, _, _ in runs])
        show(f"{what}, host arrays: whole call", [w for _, w, _ in runs])
        for k in sorted({k for t, _, _ in runs for k in t}):
            show(f"    {k}", [t.get(k, 0.0) for t, _, _ in runs])
        return runs[0][2], med([sum(t.values()) for t, _, _ in runs])

    out, kernel_ms = report("ma_inflate_blocks_batch", lambda: eng.inflate_blocks(cblob, blk_off, blk_len, raw_cap=raw_bytes))
    assert int(out["n_flagged"][0]) == 0 and out["raw"][:len(stream)].tobytes() == stream and out["raw"][-len(stream):].tobytes() == stream
    print(f"    kernels against zlib on 16 threads: {zlib_ms / kernel_ms:.2f} x ({raw_bytes / kernel_ms / 1e6:.1f} GB/s inflated)")
    raw = out["raw"]
    idx, _ = report("ma_index_records_batch", lambda: eng.index_records(raw, str_begin, str_end, rec_cap=n_rec))
    assert int(idx["n_found"][0]) == n_rec and not idx["str_state"].any()
    del out, idx
    dev = Engine(params, memspace=capi.MA_MEM_DEVICE)
    arena = DeviceArena()
    try:
        ins = {k: arena.upload(v) for k, v in (("cblob", cblob), ("blk_off", blk_off), ("blk_len", blk_len), ("str_begin", str_begin), ("str_end", str_end))}
        io = {k: arena.alloc(int(sz) * np.dtype(dt).itemsize + 64) for k, (dt, sz) in capi.inflate_out_spec(n_blocks, raw_bytes).items()}
        xo = {k: arena.alloc(int(sz) * np.dtype(dt).itemsize + 64) for k, (dt, sz) in capi.index_out_spec(len(str_begin), n_rec).items()}
        bs, os_ = capi.make_bgzf_struct(ins, n_blocks, cblob.size), capi.make_inflate_out(io, raw_bytes)
        ss, xs = capi.make_streams_struct(dict(ins, raw=io["raw"]), len(str_begin), raw_bytes), capi.make_index_out(xo, n_rec)
        for what, fn in (("ma_inflate_blocks_batch", lambda: dev.inflate_blocks_device(bs, os_)),
                         ("ma_index_records_batch", lambda: (dev.index_records_device(ss, xs), dev.synchronize()))):
            walls = []
            for i in range(4):
                t0 = time.perf_counter()
                fn()
                walls.append((time.perf_counter() - t0) * 1e3)
            show(f"{what}, device arrays: whole call", walls[1:])
        assert int(arena.download(xo["n_found"], np.uint64, 1)[0]) == n_rec
    finally:
        dev.close()
        arena.close()
finally:
    eng.close()
