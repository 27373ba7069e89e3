"""ma_inflate_blocks_batch and ma_index_records_batch on the GPU, every output array, in both memory spaces: the payloads and
CRCs against zlib, the states, the layout and the record index against tests/inflate_ref.py -- the case table of
tests/inflate_cases.py, block counts around the workgroup's, errors, capacities, and the composition inflate -> index ->
flatten on device pointers over a BAM file.  The device route's arrays -- the compressed blob at an odd address and every
output -- sit between 256 junk bytes that must come back unchanged."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import flatten_ref
import inflate_cases as cases
import inflate_ref as ref
from harness import DeviceArena
from lancet2_amd import capi
from lancet2_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

GUARD, JUNK = 256, 0x5A
INFLATE_KERNELS = {"k_inf_header", "k_inf_scan", "k_inf_decode"}
INDEX_KERNELS = {"k_idx_count", "k_idx_scan", "k_idx_fill", "k_idx_fields"}
# what ma_last_kernel_times names after a plain ma_process_batch of case 1 of tests/test_gpu_graph_export.py (tests/test_gpu_select.py)
PLAIN_PROCESS_KERNELS = {"gate_kernel", "k_align_reg", "k_align_tb", "k_align_wave", "k_assign", "k_classify", "k_clean", "k_clean_chains",
                         "k_clean_tail", "k_dp_scatter", "k_evidence", "k_graph", "k_graph_gen", "k_insert", "k_mm_hbm", "k_mm_q", "k_plan",
                         "k_poa", "k_qual", "k_read_planes", "k_support", "k_vote"}
MEMBERS = cases.all_members()
REC_KEYS = ("rec_off", "rec_len", "rec_ref", "rec_pos", "rec_span")


@pytest.fixture(scope="module")
def gpu():
    class Box:
        pass
    box = Box()
    box.host = Engine(capi.default_params())
    box.dev = Engine(capi.default_params(), memspace=capi.MA_MEM_DEVICE)
    box.arena = DeviceArena()
    yield box
    box.host.close()
    box.dev.close()
    box.arena.close()


def guarded(box, arrays, odd=()):
    return {k: box.arena.upload_unaligned(v, shift=1 if k in odd else 0, guard=GUARD, junk=JUNK) for k, v in arrays.items()}


def check_guards(box, ptrs, sizes):
    for k, nbytes in sizes.items():
        front, behind = box.arena.download(ptrs[k] - GUARD, np.uint8, GUARD), box.arena.download(ptrs[k] + nbytes, np.uint8, GUARD)
        assert (front == JUNK).all() and (behind == JUNK).all(), f"the guard of {k} changed"


def device_call(box, call, make_in, make_out, ins, spec, cap, fill):
    """-> (rc, the output arrays as the call left them); the inputs and the guards of every array must come back unchanged"""
    arrays = {k: np.ascontiguousarray(v) for k, v in ins.items()}
    in_ptrs = guarded(box, arrays, odd=("cblob", "raw"))
    out_ptrs = guarded(box, {k: np.full(int(sz) * np.dtype(dt).itemsize, fill, np.uint8) for k, (dt, sz) in spec.items()})
    rc = call(box.dev.h, C.byref(make_in(in_ptrs)), C.byref(make_out(out_ptrs, cap)))
    box.dev.synchronize()
    check_guards(box, in_ptrs, {k: v.nbytes for k, v in arrays.items()})
    check_guards(box, out_ptrs, {k: int(sz) * np.dtype(dt).itemsize for k, (dt, sz) in spec.items()})
    for k, v in arrays.items():
        assert box.arena.download(in_ptrs[k], np.uint8, v.nbytes).tobytes() == v.tobytes(), k
    return rc, {k: box.arena.download(out_ptrs[k], dt, sz) for k, (dt, sz) in spec.items()}


def inflate_device(box, blob, off, length, cap, fill=0xC3):
    n = len(off)
    return device_call(box, box.dev.lib.ma_inflate_blocks_batch, lambda p: capi.make_bgzf_struct(p, n, blob.size), capi.make_inflate_out,
                       dict(cblob=blob, blk_off=off, blk_len=length), capi.inflate_out_spec(n, cap), cap, fill)


def index_device(box, raw, begin, end, cap, fill=0xC3):
    n = len(begin)
    return device_call(box, box.dev.lib.ma_index_records_batch, lambda p: capi.make_streams_struct(p, n, raw.size), capi.make_index_out,
                       dict(raw=raw, str_begin=begin, str_end=end), capi.index_out_spec(n, cap), cap, fill)


def assert_inflated(got, want, what):
    total = int(want["n_raw"][0])
    for k in ("blk_raw_off", "blk_state", "n_raw", "n_flagged"):
        assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k][:20], want[k][:20])
    keep = want["defined"]
    assert (got["raw"][:total][keep] == want["raw"][keep]).all(), (what, "raw")


def check_inflate(box, blob, off, length, slack=5):
    """both memory spaces against zlib and the restatement; -> the restatement's arrays"""
    want = ref.inflate(blob, off, length)
    total, n = int(want["n_raw"][0]), len(off)
    got = box.host.inflate_blocks(blob, off, length)
    names = {k for k, _ in box.host.kernel_times()}
    assert names == (INFLATE_KERNELS if n else {"k_inf_scan"}), names
    assert len(got["raw"]) == total
    assert_inflated(got, want, "host arrays")
    rc, dev = inflate_device(box, blob, off, length, total + slack)
    assert rc == 0, box.dev.lib.ma_last_error(box.dev.h)
    assert_inflated(dev, want, "device arrays")
    assert (dev["raw"][total:] == 0xC3).all()  # (behind the need: as the caller left it)
    # a flagged block is confined to its own range: what lies in the ranges of good blocks is exact, see assert_inflated
    return want


# ---- the case table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MEMBERS, ids=lambda m: m[0])
def test_member(gpu, case):
    """one member between two small good ones, at an odd offset with junk between them"""
    label, m, state, payload = case
    small = cases.member(cases.deflate(b"front"), b"front"), cases.member(cases.deflate(b"behind"), b"behind")
    blob, off, length = cases.lay_out([small[0], m, small[1]], np.random.default_rng(len(m)))
    want = check_inflate(gpu, blob, off, length)
    assert want["blk_state"].tolist() == [0, state, 0], label
    if state == 0:
        a, b = int(want["blk_raw_off"][1]), int(want["blk_raw_off"][2])
        assert want["raw"][a:b].tobytes() == payload


def test_blk_len_beyond_the_member(gpu):
    good = [m for m in MEMBERS if m[2] == 0 and len(m[1]) < 3000]
    blob, off, length = cases.lay_out([m[1] for m in good], np.random.default_rng(2), slack=9)
    want = check_inflate(gpu, blob, off, length)
    assert not want["blk_state"].any() and want["raw"].tobytes() == b"".join(m[3] for m in good)


@pytest.mark.parametrize("n_blocks", [0, 1, 63, 64, 65, 257])
def test_block_counts(gpu, n_blocks):
    rng = np.random.default_rng(100 + n_blocks)
    payloads = [cases._text(int(rng.integers(0, 900)), 200 + i) for i in range(n_blocks)]
    members = [cases.member(cases.deflate(p, level=int(rng.integers(0, 10))), p) for p in payloads]
    blob, off, length = cases.lay_out(members, rng)
    want = check_inflate(gpu, blob, off, length)
    assert want["raw"].tobytes() == b"".join(payloads) and int(want["n_flagged"][0]) == 0


def test_good_and_corrupt_blocks_mixed(gpu):
    """257 blocks, every case of the table that is not large among them, in a shuffled order: the good ones are exact, the
    corrupt ones flagged and confined to their ranges"""
    rng = np.random.default_rng(7)
    pool = [m for m in MEMBERS if len(m[1]) < 3000]
    picked = [pool[i] for i in rng.permutation(len(pool))] + [pool[int(i)] for i in rng.integers(0, len(pool), 257 - len(pool))]
    assert len(picked) == 257
    blob, off, length = cases.lay_out([m[1] for m in picked], rng)
    want = check_inflate(gpu, blob, off, length)
    assert want["blk_state"].tolist() == [m[2] for m in picked]
    assert int(want["n_flagged"][0]) == sum(m[2] != 0 for m in picked) > 50


def test_blocks_in_any_order_and_twice(gpu):
    good = [m for m in MEMBERS if m[2] == 0 and len(m[1]) < 3000][:6]
    blob, off, length = cases.lay_out([m[1] for m in good])
    order = [3, 3, 0, 5, 1, 0]
    want = check_inflate(gpu, blob, off[order], length[order])
    assert want["raw"].tobytes() == b"".join(good[i][3] for i in order)


# ---- capacities and errors -----------------------------------------------------------------------------------------------------
def _some_blocks():
    rng = np.random.default_rng(11)
    payloads = [cases._text(300 + 50 * i, 300 + i) for i in range(5)]
    return cases.lay_out([cases.member(cases.deflate(p), p) for p in payloads], rng), payloads


def test_raw_cap_at_exact_fit_and_one_under(gpu):
    (blob, off, length), payloads = _some_blocks()
    total = sum(len(p) for p in payloads)
    got = gpu.host.inflate_blocks(blob, off, length, raw_cap=total)
    assert got["raw"].tobytes() == b"".join(payloads)
    rc, dev = inflate_device(gpu, blob, off, length, total)
    assert rc == 0 and dev["raw"].tobytes() == b"".join(payloads)
    with pytest.raises(EngineError) as e:
        gpu.host.inflate_blocks(blob, off, length, raw_cap=total - 1)
    assert e.value.rc == capi.MA_ERR_ARG and "raw_cap" in str(e.value) and int(e.value.arrays["n_raw"][0]) == total
    assert not any(v.any() for k, v in e.value.arrays.items() if k != "n_raw")
    rc, dev = inflate_device(gpu, blob, off, length, total - 1)
    assert rc == capi.MA_ERR_ARG and int(dev["n_raw"][0]) == total
    assert all((v.view(np.uint8) == 0xC3).all() for k, v in dev.items() if k != "n_raw")
    assert gpu.host.inflate_blocks(blob, off, length, raw_cap=None)["raw"].tobytes() == b"".join(payloads)  # (re-submitted on the need)


@pytest.mark.parametrize("what", ["blk_len past the blob", "blk_off past the blob", "blk_off + blk_len wraps"])
def test_a_block_outside_the_blob(gpu, what):
    (blob, off, length), _ = _some_blocks()
    for b in (4, 2):  # two bad blocks: the first is named
        if what == "blk_len past the blob":
            length[b] = blob.size - int(off[b]) + 1
        elif what == "blk_off past the blob":
            off[b] = blob.size + 1
        else:
            off[b] = 2**64 - 1
    with pytest.raises(ref.InflateError) as e:
        ref.inflate(blob, off, length)
    assert e.value.which == 2
    with pytest.raises(EngineError) as e:
        gpu.host.inflate_blocks(blob, off, length, raw_cap=100_000)
    assert e.value.rc == capi.MA_ERR_ARG and "block 2 " in str(e.value)
    assert not any(v.any() for v in e.value.arrays.values())
    rc, dev = inflate_device(gpu, blob, off, length, 100_000)
    assert rc == capi.MA_ERR_ARG and "block 2 " in gpu.dev.lib.ma_last_error(gpu.dev.h).decode()
    assert all((v.view(np.uint8) == 0xC3).all() for v in dev.values())


def test_null_members_are_argument_errors(gpu):
    (blob, off, length), _ = _some_blocks()
    ins = dict(cblob=blob, blk_off=off, blk_len=length)
    out = capi.alloc_host(capi.inflate_out_spec(len(off), 10_000))
    call = gpu.host.lib.ma_inflate_blocks_batch

    def structs():
        return capi.make_bgzf_struct(ins, len(off), blob.size), capi.make_inflate_out(out, 10_000)
    a, b = structs()
    assert call(gpu.host.h, C.byref(a), C.byref(b)) == 0
    for key in ins:
        a, b = structs()
        setattr(a, key, None)
        assert call(gpu.host.h, C.byref(a), C.byref(b)) == capi.MA_ERR_ARG, key
    for key in out:
        a, b = structs()
        setattr(b, key, None)
        assert call(gpu.host.h, C.byref(a), C.byref(b)) == capi.MA_ERR_ARG, key
    a, b = structs()
    a.n_blocks = -1
    assert call(gpu.host.h, C.byref(a), C.byref(b)) == capi.MA_ERR_ARG
    assert call(gpu.host.h, None, C.byref(b)) == capi.MA_ERR_ARG and call(gpu.host.h, C.byref(a), None) == capi.MA_ERR_ARG
    raw, begin, end, _ = cases.stream_cases()
    ins = dict(raw=raw, str_begin=begin, str_end=end)
    out = capi.alloc_host(capi.index_out_spec(len(begin), 100))
    call = gpu.host.lib.ma_index_records_batch

    def structs():  # noqa: F811
        return capi.make_streams_struct(ins, len(begin), raw.size), capi.make_index_out(out, 100)
    a, b = structs()
    assert call(gpu.host.h, C.byref(a), C.byref(b)) == 0
    for key in ins:
        a, b = structs()
        setattr(a, key, None)
        assert call(gpu.host.h, C.byref(a), C.byref(b)) == capi.MA_ERR_ARG, key
    for key in out:
        a, b = structs()
        setattr(b, key, None)
        assert call(gpu.host.h, C.byref(a), C.byref(b)) == capi.MA_ERR_ARG, key


# ---- the record index ----------------------------------------------------------------------------------------------------------
def assert_indexed(got, want, what):
    total = int(want["n_found"][0])
    for k in ("n_found", "str_rec_off", "str_state"):
        assert got[k].tobytes() == want[k].tobytes(), (what, k)
    for k in REC_KEYS:
        assert got[k][:total].tobytes() == want[k].tobytes(), (what, k)


def check_index(box, raw, begin, end, slack=3):
    want = ref.index(raw, begin, end)
    total, n = int(want["n_found"][0]), len(begin)
    got = box.host.index_records(raw, begin, end)
    names = {k for k, _ in box.host.kernel_times()}
    assert names == INDEX_KERNELS - (set() if total else {"k_idx_fields"}) - (set() if n else {"k_idx_count", "k_idx_fill"}), names
    assert all(len(got[k]) == total for k in REC_KEYS)
    assert_indexed(got, want, "host arrays")
    rc, dev = index_device(box, raw, begin, end, total + slack)
    assert rc == 0, box.dev.lib.ma_last_error(box.dev.h)
    assert_indexed(dev, want, "device arrays")
    for k in REC_KEYS:
        assert (dev[k][total:].view(np.uint8) == 0xC3).all(), k
    return want


def test_record_streams(gpu):
    """the hand-made streams; what each must give is asserted of the restatement in tests/test_inflate_cases.py"""
    raw, begin, end, names = cases.stream_cases()
    want = check_index(gpu, raw, begin, end)
    assert int(want["str_state"].sum()) == 5
    one = np.array([names["one record"]])
    check_index(gpu, raw, begin[one], end[one])
    none = np.array([names["no record"], names["at the end of raw"]])
    check_index(gpu, raw, begin[none], end[none])
    check_index(gpu, raw, begin[:0], end[:0])


@pytest.mark.parametrize("n_streams", [63, 64, 65, 257, 700])
def test_stream_counts(gpu, n_streams):
    rng = np.random.default_rng(n_streams)
    recs = [cases.record(b"q%d" % i, pos=int(rng.integers(-1, 10**6)), ref=int(rng.integers(-1, 3)), l_seq=int(rng.integers(1, 40)),
                         cigar=[(int(rng.integers(1, 50)), "MIDNSHP=X"[int(k)]) for k in rng.integers(0, 9, int(rng.integers(0, 6)))]) for i in range(300)]
    starts = np.cumsum([0] + [len(r) for r in recs])
    raw = np.frombuffer(b"".join(recs), np.uint8)
    first = rng.integers(0, 300, n_streams)
    count = rng.integers(0, 9, n_streams)
    begin = starts[first].astype(np.uint64)
    end = np.minimum(begin + (starts[np.minimum(first + count, 300)] - starts[first]) + rng.integers(0, 2, n_streams), raw.size).astype(np.uint64)
    end = np.maximum(end, begin)
    want = check_index(gpu, raw, begin, end)
    assert not want["str_state"].any() and int(want["n_found"][0]) > n_streams


def test_rec_cap_at_exact_fit_and_one_under(gpu):
    raw, begin, end, _ = cases.stream_cases()
    want = ref.index(raw, begin, end)
    total = int(want["n_found"][0])
    assert_indexed(gpu.host.index_records(raw, begin, end, rec_cap=total), want, "exact fit, host arrays")
    rc, dev = index_device(gpu, raw, begin, end, total)
    assert rc == 0
    assert_indexed(dev, want, "exact fit, device arrays")
    with pytest.raises(EngineError) as e:
        gpu.host.index_records(raw, begin, end, rec_cap=total - 1)
    assert e.value.rc == capi.MA_ERR_ARG and "rec_cap" in str(e.value) and int(e.value.arrays["n_found"][0]) == total
    assert not any(v.any() for k, v in e.value.arrays.items() if k != "n_found")
    rc, dev = index_device(gpu, raw, begin, end, total - 1)
    assert rc == capi.MA_ERR_ARG and int(dev["n_found"][0]) == total
    assert all((v.view(np.uint8) == 0xC3).all() for k, v in dev.items() if k != "n_found")
    assert_indexed(gpu.host.index_records(raw, begin, end, rec_cap=None), want, "re-submitted on the need")


@pytest.mark.parametrize("what", ["str_begin > str_end", "str_end > raw_bytes"])
def test_bad_stream_bounds(gpu, what):
    raw, begin, end, _ = cases.stream_cases()
    for s in (6, 3):  # two bad streams: the first is named
        if what == "str_begin > str_end":
            begin[s] = end[s] + 1
        else:
            end[s] = raw.size + 1
    with pytest.raises(EngineError) as e:
        gpu.host.index_records(raw, begin, end, rec_cap=100)
    assert e.value.rc == capi.MA_ERR_ARG and "stream 3 " in str(e.value)
    assert not any(v.any() for v in e.value.arrays.values())
    rc, dev = index_device(gpu, raw, begin, end, 100)
    assert rc == capi.MA_ERR_ARG and "stream 3 " in gpu.dev.lib.ma_last_error(gpu.dev.h).decode()
    assert all((v.view(np.uint8) == 0xC3).all() for v in dev.values())


# ---- composition: a BAM file inflated, indexed and flattened on device pointers ----------------------------------------------------
def _members_of(data):
    off, length, at = [], [], 0
    while at < len(data):
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        off.append(at)
        length.append(bsize)
        at += bsize
    return np.array(off, np.uint64), np.array(length, np.uint32)


def _bai_chunks(path):
    """-> [(virtual begin, virtual end)] of every bin of every reference"""
    b = open(path, "rb").read()
    n_ref = struct.unpack_from("<i", b, 4)[0]
    at, out = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", b, at)[0]
        at += 4
        for _ in range(n_bin):
            _, n_chunk = struct.unpack_from("<Ii", b, at)
            at += 8
            for _ in range(n_chunk):
                out.append(struct.unpack_from("<QQ", b, at))
                at += 16
        n_intv = struct.unpack_from("<i", b, at)[0]
        at += 4 + 8 * n_intv
    return out


def test_bam_file_inflated_indexed_and_flattened_on_the_device(gpu, tmp_path):
    """the BAM fixture of tests/test_pipeline_host.py in blocks of 3000 payload bytes (records straddle them): its members
    inflated on the device, one stream behind the BAM header and one per BAI chunk indexed there, and the first stream's
    rec_off / rec_len handed to ma_flatten_records_batch on the same raw buffer -- against a Python walk of the zlib-inflated
    file and flatten_ref on those bytes, byte for byte"""
    from test_pipeline_host import sam_to_bam, write_fixture
    write_fixture(str(tmp_path))
    bam = str(tmp_path / "tumor.bam")
    n_members = sam_to_bam(str(tmp_path / "tumor.sam"), bam, with_index=True, block_bytes=3000)
    data = open(bam, "rb").read()
    blk_off, blk_len = _members_of(data)
    assert len(blk_off) == n_members > 100
    # the yardstick: zlib, member after member
    payloads = [zlib.decompressobj(-15).decompress(data[int(o) + 18:int(o) + int(n) - 8]) for o, n in zip(blk_off, blk_len)]
    raw = b"".join(payloads)
    raw_off = np.cumsum([0] + [len(p) for p in payloads])
    l_text = struct.unpack_from("<i", raw, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 4 + struct.unpack_from("<i", raw, at)[0] + 4
    walked, p = [], at
    while p < len(raw):
        bs = struct.unpack_from("<I", raw, p)[0]
        walked.append((p + 4, bs))
        p += 4 + bs
    assert p == len(raw) and len(walked) > 1000
    block_of = {int(o): i for i, o in enumerate(blk_off)}
    block_of[len(data)] = len(blk_off)

    def place(v):
        return int(raw_off[block_of[v >> 16]]) + (v & 0xFFFF)
    chunks = _bai_chunks(bam + ".bai")
    begin = np.array([at] + [place(a) for a, _ in chunks], np.uint64)
    end = np.array([len(raw)] + [place(b) for _, b in chunks], np.uint64)
    assert any(lo < int(b) < lo + 4 + bs for (lo, bs) in [(o - 4, n) for o, n in walked[:400]] for b in raw_off[1:-1])  # a record straddles a join
    arena, dev = gpu.arena, gpu.dev
    blob = np.frombuffer(data, np.uint8)
    ins = guarded(gpu, dict(cblob=blob, blk_off=blk_off, blk_len=blk_len), odd=("cblob",))
    cap = len(raw)
    out = {k: arena.alloc(int(sz) * np.dtype(dt).itemsize + 64) for k, (dt, sz) in capi.inflate_out_spec(len(blk_off), cap).items()}
    dev.inflate_blocks_device(capi.make_bgzf_struct(ins, len(blk_off), blob.size), capi.make_inflate_out(out, cap))
    assert {k for k, _ in dev.kernel_times()} == INFLATE_KERNELS
    assert int(arena.download(out["n_raw"], np.uint64, 1)[0]) == len(raw) and int(arena.download(out["n_flagged"], np.uint64, 1)[0]) == 0
    assert arena.download(out["raw"], np.uint8, len(raw)).tobytes() == raw
    streams = {k: arena.upload(v) for k, v in (("str_begin", begin), ("str_end", end))}
    want = ref.index(raw, begin, end)
    total = int(want["n_found"][0])
    assert want["rec_off"][:len(walked)].tolist() == [o for o, _ in walked] and want["rec_len"][:len(walked)].tolist() == [n for _, n in walked]
    assert not want["str_state"].any() and total > len(walked)  # (the chunks list the records again)
    idx = {k: arena.alloc(int(sz) * np.dtype(dt).itemsize + 64) for k, (dt, sz) in capi.index_out_spec(len(begin), total).items()}
    dev.index_records_device(capi.make_streams_struct(dict(streams, raw=out["raw"]), len(begin), len(raw)), capi.make_index_out(idx, total))
    assert {k for k, _ in dev.kernel_times()} == INDEX_KERNELS
    assert_indexed({k: arena.download(idx[k], dt, sz) for k, (dt, sz) in capi.index_out_spec(len(begin), total).items()}, want, "the file")
    # the first stream's records, one window, to the flatten call: rec_off / rec_len are the index call's own device arrays
    nr = len(walked)
    rest = dict(rec_win_off=np.array([0, nr], np.uint32), rec_sample=np.zeros(nr, np.uint8), sample_index=np.zeros(1, np.uint8),
                sample_case=np.ones(1, np.uint8), sample_rank=np.zeros(1, np.uint32), win_chrom=np.zeros(1, np.int32),
                win_start0=np.array([1000], np.int64))
    rec = dict(rest, blob=np.frombuffer(raw, np.uint8), rec_off=want["rec_off"][:nr], rec_len=want["rec_len"][:nr])
    flat_want = flatten_ref.flatten(rec, 1, nr)
    bases_cap = int(flat_want["n_bases"][0])
    rest_ptrs = {k: arena.upload(v) for k, v in rest.items()}
    rs = capi.make_records_struct(dict(rest_ptrs, blob=out["raw"], rec_off=idx["rec_off"], rec_len=idx["rec_len"], n_samples_in=1), 1, nr,
                                  blob_bytes=len(raw))
    fp = {k: arena.alloc(int(sz) * np.dtype(dt).itemsize + 64) for k, (dt, sz) in capi.flat_out_spec(nr, bases_cap).items()}
    dev.flatten_records_device(rs, capi.make_flat_struct(fp, bases_cap))
    dev.synchronize()
    for k, (dt, sz) in capi.flat_out_spec(nr, bases_cap).items():
        cut = {"bases4": (bases_cap + nr + 1) // 2, "read_quals": bases_cap}.get(k, len(flat_want[k]))
        assert arena.download(fp[k], dt, sz)[:cut].tobytes() == flat_want[k].tobytes(), k


# ---- the plain calls are what they were ------------------------------------------------------------------------------------------
def test_plain_process_names_the_kernels_it_named(gpu):
    import test_gpu_graph_export as gx
    (blob, off, length), _ = _some_blocks()
    params, arrs, n, nr, _ = gx.case1()
    eng = Engine(params)
    try:
        eng.inflate_blocks(blob, off, length)
        eng.process(arrs, n, nr)
        names = {k for k, _ in eng.kernel_times()}
    finally:
        eng.close()
    assert names == PLAIN_PROCESS_KERNELS
    assert not names & (INFLATE_KERNELS | INDEX_KERNELS)
