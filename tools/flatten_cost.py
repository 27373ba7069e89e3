"""Developer tool: what ma_flatten_records_batch costs.
C3 workload (60x tumour / 30x normal), 8192 windows, k = 25; timing mode 2, the median of three runs each: the kernels of the
call one by one, the whole call with host arrays and with device arrays, and ma_process_packed_batch (8-bit qualities) on the
arrays the call made -- the plain call, for the comparison with another build: MA_LIB=<the parent commit's libmicroasm.so>
times that leg alone with that library (it has no flatten call; the arrays then come from tests/flatten_ref.py).
The reads of 64 synthesised windows are encoded as BAM records (names in Illumina's form, one M operation) and tiled, blob
included, to the window count: every window reads its own bytes.
usage: python tools/flatten_cost.py [windows]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import flatten_ref as ref  # noqa: E402
from harness import DeviceArena  # noqa: E402
from lancet2_amd import capi, synth  # noqa: E402
from lancet2_amd.engine import Engine  # noqa: E402

n_want = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
params = capi.default_params(min_k=25, max_k=25)
arrs, nw, nr = synth.make_config_batch("C3", 64, first_index=0)
rng = np.random.default_rng(1)
blob, rec_off, rec_len = bytearray(), [], []
start0 = [100_000 + 2000 * w for w in range(nw)]
order = np.concatenate([rng.permutation(np.arange(int(arrs["read_win_off"][w]), int(arrs["read_win_off"][w + 1]))) for w in range(nw)])
for w in range(nw):
    for r in order[int(arrs["read_win_off"][w]):int(arrs["read_win_off"][w + 1])]:
        o0, o1 = int(arrs["read_off"][r]), int(arrs["read_off"][r + 1])
        fl, hint = int(arrs["read_flags"][r]), int(arrs["read_hint"][r])
        name = b"A00123:45:HXXXXXXXX:1:%d:%d:%d" % (1101 + w % 7, 1000 + 37 * int(arrs["read_qname_id"][r]), 2000 + 11 * w)
        body = ref.encode_record(name, flag=(0x10 if fl & 4 else 0) | 0x3, refid=0, pos=start0[w] + (hint if hint != capi.MA_NO_HINT else 0),
                                 mapq=60 if fl & 1 else 7, cigar=[(o1 - o0, "M")], seq4=ref.pack_seq(arrs["read_bases"][o0:o1]),
                                 qual=arrs["read_quals"][o0:o1].tobytes(), tlen=300)
        blob += b"\0" * (1 + len(blob) % 3)  # records at any alignment
        rec_off.append(len(blob))
        rec_len.append(len(body))
        blob += body
times = max(1, n_want // nw)
tiled, n, n_rec = synth.tile_batch(arrs, nw, nr, times)
one_blob = np.frombuffer(bytes(blob), dtype=np.uint8)
rec = dict(blob=np.tile(one_blob, times),
           rec_off=np.concatenate([np.array(rec_off, np.uint64) + np.uint64(t * len(one_blob)) for t in range(times)]),
           rec_len=np.tile(np.array(rec_len, np.uint32), times), rec_win_off=tiled["read_win_off"],
           rec_sample=np.tile(arrs["read_sample"][order], times), sample_index=np.array([0, 1], np.uint8),
           sample_case=np.array([0, 1], np.uint8), sample_rank=np.array([0, 1], np.uint32), win_chrom=np.zeros(n, np.int32),
           win_start0=np.tile(np.array(start0, np.int64), times))
total = int(arrs["read_off"][nr]) * times
eng = Engine(params)
has_call = hasattr(eng.lib, "ma_flatten_records_batch")
med = statistics.median
print(f"library {capi.LIB_PATH}: windows {n} records {n_rec} bases {total} blob {rec['blob'].size} bytes")
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

    if has_call:
        timed(lambda: eng.flatten_records(rec, n, n_rec, bases_cap=total, n_refs=1))  # warm-up: workspaces
        runs = [timed(lambda: eng.flatten_records(rec, n, n_rec, bases_cap=total, n_refs=1)) for _ in range(3)]
        flat = runs[0][2]
        print(f"ma_flatten_records_batch, host arrays: kernels {med([sum(t.values()) for t, _, _ in runs]):.3f} ms, "
              f"whole call {med([w for _, w, _ in runs]):.1f} ms")
        for k in sorted({k for t, _, _ in runs for k in t}):
            print(f"    {k}: {med([t.get(k, 0.0) for t, _, _ in runs]):.3f} ms")
        dev = Engine(params, memspace=capi.MA_MEM_DEVICE)
        arena = DeviceArena()
        try:
            rs = capi.make_records_struct(dict({k: arena.upload(v) for k, v in rec.items()}, n_samples_in=2), n, n_rec, 1, blob_bytes=rec["blob"].size)
            fs = capi.make_flat_struct({k: arena.alloc(int(sz) * np.dtype(dt).itemsize + 64) for k, (dt, sz) in capi.flat_out_spec(n_rec, total).items()}, total)
            walls = []
            for i in range(4):
                t0 = time.perf_counter()
                dev.flatten_records_device(rs, fs)
                walls.append((time.perf_counter() - t0) * 1e3)
            print(f"ma_flatten_records_batch, device arrays: whole call {med(walls[1:]):.2f} ms (runs {[round(x, 2) for x in walls[1:]]})")
        finally:
            dev.close()
            arena.close()
    else:
        small = ref.flatten({k: (v[:len(one_blob)] if k == "blob" else v) for k, v in rec.items()} | dict(
            rec_off=rec["rec_off"][:nr], rec_len=rec["rec_len"][:nr], rec_sample=rec["rec_sample"][:nr],
            rec_win_off=arrs["read_win_off"], win_chrom=rec["win_chrom"][:nw], win_start0=rec["win_start0"][:nw]), nw, nr, 1)
        flat = None
    # the plain packed call on the flattened arrays (this library's, or the restatement's 64 windows tiled for another build)
    if flat is not None:
        batch = dict(ref_bases=tiled["ref_bases"], ref_off=tiled["ref_off"], read_win_off=tiled["read_win_off"], read_off=flat["read_off"],
                     read_qname_id=flat["read_qname_id"], read_sample=flat["read_sample"], read_flags=flat["read_flags"], read_hint=flat["read_hint"])
        quals, b4 = flat["read_quals"], flat["bases4"]
    else:
        one = dict(ref_bases=arrs["ref_bases"], ref_off=arrs["ref_off"], read_win_off=arrs["read_win_off"], read_off=small["read_off"],
                   read_bases=np.zeros(int(small["n_bases"][0]) + 64, np.uint8), read_quals=np.concatenate([small["read_quals"], np.zeros(64, np.uint8)]),
                   read_qname_id=small["read_qname_id"], read_sample=small["read_sample"], read_flags=small["read_flags"], read_hint=small["read_hint"])
        codes = capi.unpack_nibbles(small["bases4"], small["read_off"])
        one["read_bases"][:len(codes)] = np.frombuffer(capi.BASE_CODES.encode(), np.uint8)[codes]
        batch, _, _ = synth.tile_batch(one, nw, nr, times)
        pk, _ = capi.pack_reads(batch, qual_bits=8)
        quals, b4 = pk["quals"], pk["bases4"]
    packed = dict(bases4=np.concatenate([b4, np.zeros(8, np.uint8)]), quals=np.concatenate([quals, np.zeros(64, np.uint8)]), qual_bits=8,
                  qual_dict=np.zeros(16, np.uint8))
    timed(lambda: eng.process_packed(batch, n, n_rec, packed))
    runs = [timed(lambda: eng.process_packed(batch, n, n_rec, packed)) for _ in range(3)]
    print(f"ma_process_packed_batch: kernels {med([sum(t.values()) for t, _, _ in runs]):.3f} ms, whole call "
          f"{med([w for _, w, _ in runs]):.1f} ms (runs {[round(w, 1) for _, w, _ in runs]})")
finally:
    eng.close()
