"""ma_flatten_records_batch on the GPU against tests/flatten_ref.py, byte for byte, in both memory spaces: synthetic reads
encoded as BAM records with generated names and CIGARs, at odd blob offsets, with junk between the records, shuffled within
each window.  The device route's arrays sit between 256 junk bytes that must come back unchanged.

The sort has two instances: windows of up to 1024 records (k_rec_sort) and of up to 16384 (k_rec_sort_large); 1024 and 1025
are in the size list for that."""
import ctypes as C
import functools

import numpy as np
import pytest

import flatten_ref as ref
from harness import DeviceArena
from lancet2_amd import capi, synth
from lancet2_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

GUARD, JUNK = 256, 0x5A
FLAT_KEYS = tuple(capi.flat_out_spec(1, 1))
FLATTEN_KERNELS = {"k_rec_check", "k_rec_fields", "k_rec_sort", "k_rec_scan", "k_rec_gather"}
# what ma_last_kernel_times names after a plain ma_process_batch of case 1 of tests/test_gpu_graph_export.py, taken with the
# library of the commit before this call existed
PLAIN_PROCESS_KERNELS = {"gate_kernel", "k_align_reg", "k_align_tb", "k_align_wave", "k_assign", "k_classify", "k_clean", "k_clean_chains",
                         "k_clean_tail", "k_dp_scatter", "k_evidence", "k_graph", "k_graph_gen", "k_insert", "k_mm_hbm", "k_mm_q", "k_plan",
                         "k_poa", "k_qual", "k_read_planes", "k_support", "k_vote"}
PREFIX = b"A00123:45:HXXXXXXXX:1:"


# ---- records ---------------------------------------------------------------------------------------------------------------
def read(rng, name, l_seq=150, sample=0, mapq=60, flag=0, refid=0, pos=1000, cigar=None, tlen=0, qual=None, tags=b""):
    seq4 = bytes(rng.integers(0, 256, (l_seq + 1) // 2, dtype=np.uint8))
    qual = bytes(rng.integers(0, 42, l_seq, dtype=np.uint8)) if qual is None else bytes(qual)
    cigar = [(l_seq, "M")] if cigar is None else cigar
    body = ref.encode_record(name, flag=flag, refid=refid, pos=pos, mapq=mapq, cigar=cigar, seq4=seq4, qual=qual, tlen=tlen, tags=tags)
    return dict(bytes=body, sample=sample)


def lay_out(windows, rng, samples=((0, 0, 0), (1, 1, 1)), win_chrom=None, win_start0=None, shuffle=True, n_refs=2, ref_map=None):
    """windows: lists of read() dicts (one dict in two windows: one record, listed twice).  samples: (index, case, rank) per
    input sample.  Returns the ma_records_t arrays: records at odd and even offsets, junk before, between and behind them,
    each window's records in a shuffled (arrival) order."""
    blob = bytearray(rng.integers(0, 256, 1 + 2 * int(rng.integers(0, 4)), dtype=np.uint8).tobytes())
    placed, rec_off, rec_len, rec_sample, win_off = {}, [], [], [], [0]
    for recs in windows:
        order = list(range(len(recs)))
        if shuffle:
            rng.shuffle(order)
        for i in order:
            r = recs[i]
            if id(r) not in placed:
                blob += rng.integers(0, 256, int(rng.integers(1, 12)), dtype=np.uint8).tobytes()
                if len(blob) % 2 == 0 and len(placed) % 3:
                    blob += b"\xAA"  # (two records in three start at an odd offset)
                placed[id(r)] = (len(blob), len(r["bytes"]))
                blob += r["bytes"]
            off, ln = placed[id(r)]
            rec_off.append(off)
            rec_len.append(ln)
            rec_sample.append(r["sample"])
        win_off.append(len(rec_off))
    blob += rng.integers(0, 256, 7, dtype=np.uint8).tobytes()
    n = len(windows)
    out = dict(blob=np.frombuffer(bytes(blob), dtype=np.uint8).copy(), rec_off=np.array(rec_off, dtype=np.uint64),
               rec_len=np.array(rec_len, dtype=np.uint32), rec_win_off=np.array(win_off, dtype=np.uint32),
               rec_sample=np.array(rec_sample, dtype=np.uint8),
               sample_index=np.array([s[0] for s in samples], dtype=np.uint8),
               sample_case=np.array([s[1] for s in samples], dtype=np.uint8),
               sample_rank=np.array([s[2] for s in samples], dtype=np.uint32),
               win_chrom=np.array(win_chrom if win_chrom is not None else [0] * n, dtype=np.int32),
               win_start0=np.array(win_start0 if win_start0 is not None else [900] * n, dtype=np.int64))
    if ref_map is not None:
        out["ref_map"] = np.array(ref_map, dtype=np.int32)
    return out, n, len(rec_off), n_refs


# ---- the two routes ---------------------------------------------------------------------------------------------------------
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


def upload_records(arena, rec, n, nr, n_refs):
    """the input arrays on the device, the blob at an odd address; -> (struct, pointers)"""
    ptrs = {k: arena.upload_unaligned(v, shift=1 if k == "blob" else 0, guard=GUARD, junk=JUNK) for k, v in rec.items()}
    return capi.make_records_struct(dict(ptrs, n_samples_in=len(rec["sample_rank"])), n, nr, n_refs, blob_bytes=rec["blob"].size), ptrs


def flatten_device(box, rec, n, nr, n_refs, bases_cap, fill=0):
    """-> (rc, arrays as the call left them, device pointers, spec); checks the guards of every output array"""
    rs, _ = upload_records(box.arena, rec, n, nr, n_refs)
    spec = capi.flat_out_spec(nr, bases_cap)
    ptrs = {k: box.arena.upload_unaligned(np.full(int(sz) * np.dtype(dt).itemsize, fill, np.uint8).view(dt), shift=0, guard=GUARD, junk=JUNK)
            for k, (dt, sz) in spec.items()}
    rc = box.dev.lib.ma_flatten_records_batch(box.dev.h, C.byref(rs), C.byref(capi.make_flat_struct(ptrs, bases_cap)))
    box.dev.synchronize()
    for k, (dt, sz) in spec.items():
        nbytes = int(sz) * np.dtype(dt).itemsize
        front, behind = box.arena.download(ptrs[k] - GUARD, np.uint8, GUARD), box.arena.download(ptrs[k] + nbytes, np.uint8, GUARD)
        assert (front == JUNK).all() and (behind == JUNK).all(), f"the guard of {k} changed"
    return rc, {k: box.arena.download(ptrs[k], dt, sz) for k, (dt, sz) in spec.items()}, ptrs, spec


def assert_equal(got, want, nr, what):
    total = int(want["n_bases"][0])
    assert int(got["n_bases"][0]) == total, what
    for k in FLAT_KEYS:
        cut = {"bases4": (total + nr + 1) // 2, "read_quals": total}.get(k, len(want[k]))
        assert got[k][:cut].tobytes() == want[k].tobytes(), (what, k)


def check(box, case, slack=3):
    """both memory spaces against the restatement; -> the restatement's arrays"""
    rec, n, nr, n_refs = case
    want = ref.flatten(rec, n, nr, n_refs)
    cap = int(want["n_bases"][0]) + slack
    got = box.host.flatten_records(rec, n, nr, bases_cap=cap, n_refs=n_refs)
    names = {k for k, _ in box.host.kernel_times()}
    assert names - {"k_rec_sort_large"} == FLATTEN_KERNELS - ({"k_rec_fields", "k_rec_sort"} if nr == 0 else set()), names
    assert_equal(got, want, nr, "host arrays")
    rc, dev, _, _ = flatten_device(box, rec, n, nr, n_refs, cap)
    assert rc == 0, box.dev.lib.ma_last_error(box.dev.h)
    assert_equal(dev, want, nr, "device arrays")
    assert not dev["read_quals"][int(want["n_bases"][0]):].any()  # (behind the need: as the caller left it)
    return want


# ---- sort and name edges ----------------------------------------------------------------------------------------------------
def _edge_windows(rng):
    long64 = bytes(rng.integers(33, 127, 64, dtype=np.uint8))
    return {
        "proper prefixes": [read(rng, b"r1"), read(rng, b"r10"), read(rng, b"r1\x80"), read(rng, b"r"), read(rng, b"r1", pos=5)],
        "equal in the first 8, 16 and 64 bytes": [read(rng, long64[:8] + b"b"), read(rng, long64[:8] + b"a"), read(rng, long64[:16] + b"z"),
                                                  read(rng, long64[:16] + b"y"), read(rng, long64 + b"2"), read(rng, long64 + b"1"),
                                                  read(rng, long64), read(rng, long64[:8])],
        "bytes of 0x80 and more": [read(rng, b"n\xff"), read(rng, b"n\x7f"), read(rng, b"n\x80x"), read(rng, b"n\x80"), read(rng, b"\xfe"),
                                   read(rng, b"n")],
        "mates in two pass groups and two samples": [read(rng, b"mate", mapq=60, sample=0), read(rng, b"mate", mapq=3, sample=1),
                                                     read(rng, b"other", mapq=60, sample=1), read(rng, b"mate", mapq=60, sample=1),
                                                     read(rng, b"a", mapq=19, sample=0), read(rng, b"other", mapq=20, sample=0)],
        "full ties": [read(rng, b"same", pos=77, refid=1) for _ in range(6)] + [read(rng, b"same", pos=76, refid=1), read(rng, b"same", pos=77, refid=0)],
    }


@pytest.mark.parametrize("which", ["proper prefixes", "equal in the first 8, 16 and 64 bytes", "bytes of 0x80 and more",
                                   "mates in two pass groups and two samples", "full ties"])
def test_sort_and_name_edges(gpu, which):
    rng = np.random.default_rng(11)
    recs = _edge_windows(rng)[which]
    want = check(gpu, lay_out([recs], rng))
    if which in ("mates in two pass groups and two samples", "full ties"):  # (in the order written down: read_src can be stated)
        want = check(gpu, lay_out([recs], rng, shuffle=False))
    if which == "mates in two pass groups and two samples":
        # one id for the name wherever its reads sort: sample 0 pass, sample 1 pass (mate, other), then the two that fail
        assert want["read_src"].tolist() == [0, 5, 3, 2, 4, 1] and want["read_qname_id"].tolist() == [0, 1, 0, 1, 2, 0]
    if which == "full ties":
        assert want["read_src"].tolist() == [7, 6, 0, 1, 2, 3, 4, 5]  # chrom, pos, then arrival


def test_soft_clip_fraction_boundary(gpu):
    """the kernel's f64 division at the rule's edge: 9 of 150 clipped bases is 6 % exactly and sets MA_RM_SOFTCLIP, 8 of 150
    leaves it clear; every S operation counts, H never does, and the leading clip of the hint is the FIRST operation only"""
    rng = np.random.default_rng(15)
    recs = [read(rng, b"a", cigar=[(9, "S"), (141, "M")]), read(rng, b"b", cigar=[(8, "S"), (142, "M")]),
            read(rng, b"c", cigar=[(4, "S"), (141, "M"), (5, "S")], flag=0x2), read(rng, b"d", cigar=[(50, "H"), (150, "M")]),
            read(rng, b"e", l_seq=50, cigar=[(3, "S"), (47, "M")], flag=0x2), read(rng, b"f", l_seq=50, cigar=[(2, "S"), (48, "M")]),
            read(rng, b"g", cigar=[(5, "H"), (10, "S"), (140, "M")])]
    want = check(gpu, lay_out([recs], rng))
    S, P = capi.MA_RM_SOFTCLIP, capi.MA_RM_PROPER
    assert want["read_mflags"].tolist() == [S, 0, S | P, 0, S | P, 0, S]
    assert want["read_hint"].tolist() == [91, 92, 96, 100, 97, 98, 100]


def test_full_ties_follow_arrival(gpu):
    rng = np.random.default_rng(12)
    recs = [read(rng, b"same", pos=77) for _ in range(7)]
    want = check(gpu, lay_out([recs], rng))
    assert want["read_src"].tolist() == list(range(7)) and not want["read_qname_id"].any()


def test_sample_rank_reverses_the_index_order(gpu):
    rng = np.random.default_rng(13)
    samples = ((5, 0, 30), (6, 1, 20), (7, 0, 10))  # (read_sample, case, rank)
    recs = [read(rng, b"q%d" % (i % 4), sample=i % 3) for i in range(8)]
    want = check(gpu, lay_out([recs], rng, samples=samples))
    assert want["read_sample"].tolist() == sorted(want["read_sample"].tolist(), reverse=True)
    assert set(want["read_flags"][want["read_sample"] == 6].tolist()) == {capi.MA_RF_PASS | capi.MA_RF_CASE}


def test_ref_map_and_foreign_chrom(gpu):
    """per-sample refID -> chrom tables; a refID outside them is chrom -1: no hint, and it sorts first among equal names"""
    rng = np.random.default_rng(14)
    ref_map = [[1, 0, 2], [2, 1, 0]]  # sample 0, sample 1
    recs = [read(rng, b"x", sample=0, refid=0), read(rng, b"x", sample=0, refid=1), read(rng, b"x", sample=0, refid=2),
            read(rng, b"x", sample=1, refid=2), read(rng, b"x", sample=1, refid=3), read(rng, b"x", sample=1, refid=-1),
            read(rng, b"x", sample=1, refid=0)]
    want = check(gpu, lay_out([recs], rng, n_refs=3, ref_map=np.array(ref_map).reshape(-1), win_chrom=[0]))
    hinted = want["read_hint"] != capi.MA_NO_HINT
    assert int(hinted.sum()) == 2  # sample 0 / refID 1 and sample 1 / refID 2 map to chrom 0


# ---- sizes ------------------------------------------------------------------------------------------------------------------
def _sized_window(rng, size, distinct=None):
    distinct = max(1, size * 2 // 3) if distinct is None else distinct
    names = [PREFIX + b"%d:%d:%d" % (1101 + int(rng.integers(0, 3)), int(rng.integers(1000, 30000)), int(rng.integers(1000, 30000)))
             for _ in range(distinct)]
    out = []
    for i in range(size):
        ln = int(rng.integers(30, 152))
        clip = int(rng.integers(0, 20))
        cigar = [(clip, "S"), (ln - clip, "M")] if clip and i % 3 == 0 else ([(ln - clip, "M"), (clip, "S")] if clip else None)
        out.append(read(rng, names[i % distinct], l_seq=ln, sample=int(rng.integers(0, 2)), mapq=int(rng.choice([0, 19, 20, 60])),
                        flag=int(rng.choice([0x1 | 0x2, 0x10, 0x2 | 0x10, 0])), refid=int(rng.integers(0, 2)),
                        pos=int(rng.integers(0, 3000)), cigar=cigar, tlen=int(rng.integers(-600, 600))))
    return out


@pytest.mark.parametrize("size", [0, 1, 2, 63, 64, 65, 1024, 1025])
def test_sizes(gpu, size):
    rng = np.random.default_rng(100 + size)
    windows = [_sized_window(rng, 5), _sized_window(rng, size), [], _sized_window(rng, 3)]
    want = check(gpu, lay_out(windows, rng, win_chrom=[0, 1, 0, 0]))
    assert len(want["read_src"]) == size + 8


def test_no_window_and_no_record(gpu):
    rng = np.random.default_rng(5)
    check(gpu, lay_out([], rng))
    check(gpu, lay_out([[], []], rng))


def test_5000_records_2500_names(gpu):
    rng = np.random.default_rng(5000)
    want = check(gpu, lay_out([_sized_window(rng, 5000, distinct=2500), _sized_window(rng, 70)], rng))
    assert int(want["read_qname_id"][:5000].max()) == 2499


@pytest.mark.parametrize("l_seq", [1, 2, 149, 150, 151, 608])
def test_read_lengths(gpu, l_seq):
    """odd and even nibble tails at odd and even places of the nibble array; 0xFF qualities become 0"""
    rng = np.random.default_rng(l_seq)
    recs = [read(rng, b"n%d" % i, l_seq=l_seq + (i % 2 if l_seq > 1 else 0), qual=[0xFF] * (l_seq + (i % 2 if l_seq > 1 else 0)) if i == 2 else None)
            for i in range(7)]
    want = check(gpu, lay_out([recs, recs[:3]], rng))
    assert not want["read_quals"][int(want["read_off"][2]):int(want["read_off"][3])].any()


def test_a_record_in_two_windows(gpu):
    rng = np.random.default_rng(21)
    shared = [read(rng, b"s%d" % i, pos=1400 + i) for i in range(4)]
    a, b = [read(rng, b"a%d" % i) for i in range(3)], [read(rng, b"b%d" % i) for i in range(3)]
    case = lay_out([a + shared, shared + b], rng, win_start0=[900, 1300])
    rec, n, nr, _ = case
    assert len(set(rec["rec_off"].tolist())) == 10 and nr == 14  # uploaded once, listed twice
    want = check(gpu, case)
    by_off = {}
    for o in range(nr):
        by_off.setdefault(int(rec["rec_off"][want["read_src"][o]]), []).append(int(want["read_hint"][o]))
    assert sorted(len(v) for v in by_off.values()) == [1] * 6 + [2] * 4
    assert all(v[0] - v[1] == 400 for v in by_off.values() if len(v) == 2)  # the hint is the window's


# ---- error paths ------------------------------------------------------------------------------------------------------------
def _expect(gpu, case, rc, bases_cap, word):
    """the call fails with `rc` in both memory spaces, names `word`, and leaves the caller's arrays alone; -> n_bases it reported"""
    rec, n, nr, n_refs = case
    with pytest.raises(EngineError) as e:
        gpu.host.flatten_records(rec, n, nr, bases_cap=bases_cap, n_refs=n_refs)
    assert e.value.rc == rc and word in str(e.value), str(e.value)
    assert not any(v.any() for k, v in e.value.arrays.items() if k != "n_bases")
    got_rc, dev, _, _ = flatten_device(gpu, rec, n, nr, n_refs, bases_cap, fill=0xC3)
    assert got_rc == rc and word in gpu.dev.lib.ma_last_error(gpu.dev.h).decode()
    for k, v in dev.items():
        if k != "n_bases":
            assert (v.view(np.uint8) == 0xC3).all(), k
    return e.value.n_bases, int(dev["n_bases"][0])


def test_l_seq_overruns_rec_len(gpu):
    rng = np.random.default_rng(31)
    recs = [read(rng, b"r%d" % i) for i in range(9)]
    rec, n, nr, n_refs = lay_out([recs[:5], recs[5:]], rng, shuffle=False)
    blob = rec["blob"]
    for i in (6, 3):  # l_seq of records 3 and 6 claims 2^20 bases; the first bad one is named
        blob[int(rec["rec_off"][i]) + 16:int(rec["rec_off"][i]) + 20] = np.frombuffer(np.int32(1 << 20).tobytes(), dtype=np.uint8)
    _expect(gpu, (rec, n, nr, n_refs), capi.MA_ERR_ARG, 9 * 150, "record 3 ")
    with pytest.raises(ref.FlattenError) as e:
        ref.flatten(rec, n, nr, n_refs)
    assert e.value.record == 3


@pytest.mark.parametrize("what", ["rec_len past the blob", "rec_len under the core", "l_seq 0", "l_read_name 0", "no such sample"])
def test_other_bad_records(gpu, what):
    rng = np.random.default_rng(32)
    recs = [read(rng, b"r%d" % i) for i in range(6)]
    rec, n, nr, n_refs = lay_out([recs], rng, shuffle=False)
    at = int(rec["rec_off"][4])
    if what == "rec_len past the blob":
        rec["rec_len"][4] = rec["blob"].size - at + 1
    elif what == "rec_len under the core":
        rec["rec_len"][4] -= 1
    elif what == "l_seq 0":
        rec["blob"][at + 16:at + 20] = 0
    elif what == "l_read_name 0":
        rec["blob"][at + 8] = 0
    else:
        rec["rec_sample"][4] = 2
    _expect(gpu, (rec, n, nr, n_refs), capi.MA_ERR_ARG, 6 * 150, "record 4 ")


def test_bases_cap_one_under_the_need(gpu):
    rng = np.random.default_rng(33)
    case = lay_out([_sized_window(rng, 40), _sized_window(rng, 9)], rng)
    need = int(ref.flatten(*case)["n_bases"][0])
    assert _expect(gpu, case, capi.MA_ERR_ARG, need - 1, "bases_cap") == (need, need)
    check(gpu, case, slack=0)  # ... and the exact fit passes


def test_a_window_of_the_cap_and_one_more(gpu):
    """the cap's own size passes (one record listed 16384 times: ties all the way down to arrival), one more is MA_ERR_PARAM"""
    rng = np.random.default_rng(34)
    one = read(rng, b"only", l_seq=3)
    rec, n, nr, n_refs = lay_out([[one]], rng)
    big = dict(rec)
    for count, ok in ((capi.FLATTEN_MAX_WINDOW, True), (capi.FLATTEN_MAX_WINDOW + 1, False)):
        for k in ("rec_off", "rec_len", "rec_sample"):
            big[k] = np.repeat(rec[k][:1], count + 2)
        big["rec_win_off"] = np.array([0, 2, count + 2], dtype=np.uint32)
        big["win_chrom"], big["win_start0"] = np.zeros(2, np.int32), np.zeros(2, np.int64)
        case = (big, 2, count + 2, n_refs)
        if ok:
            want = check(gpu, case)
            assert want["read_src"].tolist() == list(range(count + 2))
        else:
            _expect(gpu, case, capi.MA_ERR_PARAM, 3 * (count + 2), "window 1 ")


def test_a_window_list_that_does_not_rise(gpu):
    rng = np.random.default_rng(35)
    rec, n, nr, n_refs = lay_out([_sized_window(rng, 4), _sized_window(rng, 4)], rng)
    for bad in ([0, 5, 4 + 4 - 1], [1, 4, 8], [0, 9, 8]):
        rec["rec_win_off"] = np.array(bad, dtype=np.uint32)
        _expect(gpu, (rec, n, nr, n_refs), capi.MA_ERR_ARG, 8 * 152, "rec_win_off")


def test_null_members_are_argument_errors(gpu):
    rng = np.random.default_rng(36)
    rec, n, nr, n_refs = lay_out([_sized_window(rng, 4)], rng)
    out = capi.alloc_host(capi.flat_out_spec(nr, 4 * 152))
    for cls_key in ("blob", "rec_win_off", "sample_rank", "win_start0"):
        rs = capi.make_records_struct(rec, n, nr, n_refs)
        setattr(rs, cls_key, None)
        assert gpu.host.lib.ma_flatten_records_batch(gpu.host.h, C.byref(rs), C.byref(capi.make_flat_struct(out, 4 * 152))) == capi.MA_ERR_ARG
    for key in ("n_bases", "bases4", "read_src"):
        fs = capi.make_flat_struct(out, 4 * 152)
        setattr(fs, key, None)
        assert gpu.host.lib.ma_flatten_records_batch(gpu.host.h, C.byref(capi.make_records_struct(rec, n, nr, n_refs)), C.byref(fs)) == capi.MA_ERR_ARG


# ---- composition: flattened on the device, processed from the same pointers ---------------------------------------------------
def _records_of_batch(arrs, n, nr, roles, rng):
    """the reads of a synth batch as BAM records: names from the window-local name ids, POS from the hint"""
    win_start0 = [10_000 + 2000 * w for w in range(n)]
    windows = []
    for w in range(n):
        recs = []
        for r in range(int(arrs["read_win_off"][w]), int(arrs["read_win_off"][w + 1])):
            o0, o1 = int(arrs["read_off"][r]), int(arrs["read_off"][r + 1])
            fl, hint, s = int(arrs["read_flags"][r]), int(arrs["read_hint"][r]), int(arrs["read_sample"][r])
            body = ref.encode_record(PREFIX + b"%d" % int(arrs["read_qname_id"][r]), flag=(0x10 if fl & capi.MA_RF_REV else 0) | 0x2,
                                     refid=0 if hint != capi.MA_NO_HINT else 1, pos=win_start0[w] + (hint if hint != capi.MA_NO_HINT else 0),
                                     mapq=60 if fl & capi.MA_RF_PASS else 7, cigar=[(o1 - o0, "M")], seq4=ref.pack_seq(arrs["read_bases"][o0:o1]),
                                     qual=arrs["read_quals"][o0:o1].tobytes(), tlen=int(rng.integers(-500, 500)))
            recs.append(dict(bytes=body, sample=s))
        windows.append(recs)
    samples = tuple((s, role, 10 * role + s) for s, role in enumerate(roles))
    return lay_out(windows, rng, samples=samples, win_start0=win_start0)


OUT_CLASSES = (capi.GateOut, capi.AsmOut, capi.VarOut, capi.GenoOut, capi.FmtOut, capi.FmtMetaOut, capi.CxOut)


def _chain_specs(p, n, nr):
    return [capi.gate_out_spec(n), capi.asm_out_spec(p, n), capi.var_out_spec(p, n), capi.geno_out_spec(p, n, nr, debug=False),
            capi.fmt_out_spec(p, n), capi.fmt_meta_out_spec(p, n), capi.cx_out_spec(p, n)]


@pytest.mark.parametrize("cfg,n_windows", [("C2", 8), ("C5", 4)])
def test_flattened_batch_goes_to_the_chained_call(cfg, n_windows):
    from harness import variants_of
    import cx_chain_cases
    import packed_reads_cases
    from test_gpu_graph_export import assert_same_assembly
    p = packed_reads_cases.params(cfg)
    arrs, n, nr = synth.make_config_batch(cfg, n_windows, first_index=70_000)
    rng = np.random.default_rng(77)
    rec, n, nr, n_refs = _records_of_batch(arrs, n, nr, synth.CONFIGS[cfg]["roles"], rng)
    want = ref.flatten(rec, n, nr, n_refs)
    total = int(want["n_bases"][0])
    flat_arrs = dict(ref_bases=arrs["ref_bases"], ref_off=arrs["ref_off"], read_win_off=rec["rec_win_off"], read_off=want["read_off"],
                     read_qname_id=want["read_qname_id"], read_sample=want["read_sample"], read_flags=want["read_flags"],
                     read_hint=want["read_hint"])
    quals = np.concatenate([want["read_quals"], np.zeros(64, np.uint8)])
    packed = dict(bases4=np.concatenate([want["bases4"], np.zeros(8, np.uint8)]), quals=quals, qual_bits=8, qual_dict=np.zeros(16, np.uint8))
    meta = {k: want[k] for k in capi.META_DTYPES}
    host = Engine(p)
    try:
        ref_out = host.process_cx(flat_arrs, n, nr, meta=meta, packed=packed)
    finally:
        host.close()
    assert int(ref_out[2]["win_nvars"].sum()) > 0  # (the comparison is of calls that found something)
    specs = _chain_specs(p, n, nr)
    eng = Engine(p, memspace=capi.MA_MEM_DEVICE)
    arena = DeviceArena()
    try:
        rs, _ = upload_records(arena, rec, n, nr, n_refs)
        fspec = capi.flat_out_spec(nr, total + 64)
        fp = {k: arena.alloc(int(sz) * np.dtype(dt).itemsize + 64) for k, (dt, sz) in fspec.items()}
        eng.flatten_records_device(rs, capi.make_flat_struct(fp, total + 64))
        names = {k for k, _ in eng.kernel_times()}
        refs = {k: arena.upload(arrs[k]) for k in ("ref_bases", "ref_off")}
        win_off = arena.upload(rec["rec_win_off"])

        def run(batch_ptrs, pk_ptrs, meta_ptrs):
            ptrs = [{k: arena.alloc(int(sz) * np.dtype(dt).itemsize) for k, (dt, sz) in spec.items()} for spec in specs]
            structs = [capi.fill_struct(cls, x) for cls, x in zip(OUT_CLASSES, ptrs)]
            b = capi.make_batch_struct(dict(refs, read_win_off=win_off, **batch_ptrs), n, nr)
            eng.process_cx_device(b, capi.make_packed_struct(dict(pk_ptrs, qual_bits=8, qual_dict=np.zeros(16, np.uint8))),
                                  capi.fill_struct(capi.ReadMeta, meta_ptrs), *structs[:6], structs[6])
            eng.synchronize()
            return [{k: arena.download(pt[k], dt, sz) for k, (dt, sz) in spec.items()} for spec, pt in zip(specs, ptrs)]

        batch_keys = ("read_off", "read_qname_id", "read_sample", "read_flags", "read_hint")
        got = run({k: fp[k] for k in batch_keys}, dict(bases4=fp["bases4"], quals=fp["read_quals"]), {k: fp[k] for k in capi.META_DTYPES})
        # ... and the same call on the restatement's arrays, uploaded: both wrote into zeroed device arrays, every byte is defined
        twin = run({k: arena.upload(want[k]) for k in batch_keys}, dict(bases4=arena.upload(packed["bases4"]), quals=arena.upload(quals)),
                   {k: arena.upload(want[k]) for k in capi.META_DTYPES})
    finally:
        eng.close()
        arena.close()
    assert FLATTEN_KERNELS <= names
    for g, t, spec in zip(got, twin, specs):
        for k in spec:
            assert g[k].tobytes() == t[k].tobytes(), k
    # against Engine.process_cx on host arrays, in what the two calls define: the staging buffers of the host route are not
    # cleared, so unused variant slots and the tails of the haplotype arrays hold whatever the allocation held
    assert got[0]["max_approx"].tobytes() == ref_out[0]["max_approx"].tobytes() and got[0]["max_exact"].tobytes() == ref_out[0]["max_exact"].tobytes()
    assert_same_assembly(p, ref_out[1], got[1], n)
    assert got[2]["win_nvars"].tobytes() == ref_out[2]["win_nvars"].tobytes()
    for w in range(n):
        assert repr(variants_of(p, got[2], w)) == repr(variants_of(p, ref_out[2], w)), w
    used = cx_chain_cases.used_slots(p, got[2]["win_nvars"])
    for i in (3, 4, 5, 6):
        for k in specs[i]:
            a, b = (x[k].view(np.uint8).reshape(len(used), -1)[used] for x in (got[i], ref_out[i]))
            assert np.array_equal(a, b), k


# ---- the plain calls are what they were -------------------------------------------------------------------------------------
def test_plain_process_names_the_kernels_it_named():
    import test_gpu_graph_export as gx
    params, arrs, n, nr, _ = gx.case1()
    eng = Engine(params)
    try:
        eng.process(arrs, n, nr)
        names = {k for k, _ in eng.kernel_times()}
    finally:
        eng.close()
    assert names == PLAIN_PROCESS_KERNELS
    assert not names & (FLATTEN_KERNELS | {"k_rec_sort_large"})


# ---- the driver, end to end --------------------------------------------------------------------------------------------------
def test_driver_prints_the_same_records_from_raw_records(tmp_path):
    """pipeline_driver --raw-records: every batch flattened on the device, then the chained call -- the VCF and the TSV lines
    are those of --packed-reads --read-meta, whose batches the host collector flattens"""
    import subprocess
    import test_pipeline_host as host
    exe = host.driver(tmp_path)
    host.write_fixture(str(tmp_path))
    for name in ("normal", "tumor"):
        host.sam_to_bam(str(tmp_path / (name + ".sam")), str(tmp_path / (name + ".bam")))
    texts, outs = [], []
    base = [exe, "--reference", str(tmp_path / "ref.fa"), "--normal", str(tmp_path / "normal.bam"), "--tumor", str(tmp_path / "tumor.bam"),
            "--region", "chr1:1-6000", "--min-kmer", "25", "--max-kmer", "25", "--batch-windows", "3"]
    for tag, extra in (("packed", ["--packed-reads", "--read-meta"]), ("raw", ["--raw-records"])):
        vcf = tmp_path / f"calls_{tag}.vcf"
        r = subprocess.run(base + ["--out-vcf", str(vcf)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = open(vcf, "rb").read().split(b"\n")
        texts.append(b"\n".join(x for x in lines if not x.startswith(b"##commandLine=")))
        r = subprocess.run(base + extra[:1], capture_output=True, text=True)  # ... and the plain records on the standard output
        assert r.returncode == 0, r.stderr
        outs.append([x for x in r.stdout.split("\n") if x.startswith("chr1\t")])
    assert texts[0] == texts[1] and sum(not x.startswith(b"#") for x in texts[1].split(b"\n") if x) >= 6
    assert outs[0] == outs[1] and len(outs[1]) >= 6
    assert b"RMQ" in texts[1]  # (the statistics over the read metadata are asked for: the flattened meta arrays are in use)
