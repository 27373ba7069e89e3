"""ma_select_records_batch on the GPU against tests/select_ref.py, every output array, in both memory spaces: the hand-made
rule cases of tests/select_cases.py, windows of every size around the block's, the event table at its capacity, errors, and the
composition select -> flatten -> chained call.  The device route's arrays -- the blob and every output -- sit between 256 junk
bytes that must come back unchanged."""
import ctypes as C
import struct

import numpy as np
import pytest

import flatten_ref
import select_cases as cases
import select_ref as ref
from harness import DeviceArena
from lancet2_amd import capi, synth
from lancet2_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

GUARD, JUNK = 256, 0x5A
SELECT_KERNELS = {"k_sel_check", "k_sel_fields", "k_sel_window", "k_sel_scan", "k_sel_gather"}
# what ma_last_kernel_times names after a plain ma_process_batch of case 1 of tests/test_gpu_graph_export.py, taken with the
# library of the commit before this call existed
PLAIN_PROCESS_KERNELS = {"gate_kernel", "k_align_reg", "k_align_tb", "k_align_wave", "k_assign", "k_classify", "k_clean", "k_clean_chains",
                         "k_clean_tail", "k_dp_scatter", "k_evidence", "k_graph", "k_graph_gen", "k_insert", "k_mm_hbm", "k_mm_q", "k_plan",
                         "k_poa", "k_qual", "k_read_planes", "k_support", "k_vote"}
WHOLE = ("rec_keep", "win_state", "win_sample_reads", "win_sample_bases", "n_selected", "sel_win_off")
LISTS = ("sel_off", "sel_len", "sel_sample", "sel_src")
WIDE = dict(max_sample_cov=1e9, min_anchor_cov=0, skip_active_region=False)


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


def upload_inputs(arena, rec, win_len):
    """the arrays the call reads on the device, the blob at an odd address, junk around each; -> pointers"""
    arrays = {k: np.ascontiguousarray(rec[k], dtype=capi.RECORDS_DTYPES[k]) for k in capi.SELECT_IN_KEYS}
    arrays["win_len"] = np.ascontiguousarray(win_len, dtype=np.uint32)
    return {k: arena.upload_unaligned(v, shift=1 if k == "blob" else 0, guard=GUARD, junk=JUNK) for k, v in arrays.items()}, arrays


def select_device(box, rec, n, nr, ns, win_len, params, fill=0):
    """-> (rc, arrays as the call left them); checks the guards of the blob and of every output array"""
    ins, arrays = upload_inputs(box.arena, rec, win_len)
    rs = capi.make_records_struct(dict(ins, n_samples_in=ns), n, nr, blob_bytes=arrays["blob"].size)
    spec = capi.select_out_spec(n, nr, ns)
    ptrs = {k: box.arena.upload_unaligned(np.full(int(sz) * np.dtype(dt).itemsize, fill, np.uint8).view(dt), shift=0, guard=GUARD, junk=JUNK)
            for k, (dt, sz) in spec.items()}
    rc = box.dev.lib.ma_select_records_batch(box.dev.h, C.byref(rs), C.byref(capi.make_select_params(ins["win_len"], **params)),
                                             C.byref(capi.fill_struct(capi.SelectOut, ptrs)))
    box.dev.synchronize()
    sizes = {k: int(sz) * np.dtype(dt).itemsize for k, (dt, sz) in spec.items()}
    sizes["blob"] = arrays["blob"].size
    for k, nbytes in sizes.items():
        p = ptrs.get(k, ins.get(k))
        front, behind = box.arena.download(p - GUARD, np.uint8, GUARD), box.arena.download(p + nbytes, np.uint8, GUARD)
        assert (front == JUNK).all() and (behind == JUNK).all(), f"the guard of {k} changed"
    assert box.arena.download(ins["blob"], np.uint8, arrays["blob"].size).tobytes() == arrays["blob"].tobytes()
    return rc, {k: box.arena.download(ptrs[k], dt, sz) for k, (dt, sz) in spec.items()}


def assert_equal(got, want, what):
    for k in WHOLE:
        assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k][:40], want[k][:40])
    total = int(want["n_selected"][0])
    for k in LISTS:
        assert got[k][:total].tobytes() == want[k].tobytes(), (what, k)


def check(box, case, params):
    """both memory spaces against the restatement; -> the restatement's arrays"""
    rec, n, nr, ns, win_len = case
    want = ref.select(rec, n, nr, ns, win_len, **params)
    got = box.host.select_records(rec, n, nr, win_len, **params)
    names = {k for k, _ in box.host.kernel_times()}
    assert names == SELECT_KERNELS - ({"k_sel_fields", "k_sel_gather"} if nr == 0 else set()) - ({"k_sel_window"} if n == 0 else set()), names
    assert_equal(got, want, "host arrays")
    assert all(len(got[k]) == int(want["n_selected"][0]) for k in LISTS)
    rc, dev = select_device(box, rec, n, nr, ns, win_len, params, fill=0xC3)
    assert rc == 0, box.dev.lib.ma_last_error(box.dev.h)
    assert_equal(dev, want, "device arrays")
    for k in LISTS:  # (behind the lists: as the caller left it)
        assert (dev[k][int(want["n_selected"][0]):].view(np.uint8) == 0xC3).all(), k
    return want


# ---- the rules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(cases.BATCHES))
def test_rules(gpu, which):
    """every hand-made case as one batch of small windows; what each must give is asserted of the restatement in
    tests/test_select_ref.py and of the kernels here"""
    arrays, n, nr, ns, win_len, params, rows = cases.batch(which)
    want = check(gpu, (arrays, n, nr, ns, win_len), params)
    for w, (label, _, _, (mask, value), _) in enumerate(rows):
        assert int(want["win_state"][w]) & mask == value, label
    check(gpu, cases.batch(which, reverse=True)[:5], params)


# ---- sizes ---------------------------------------------------------------------------------------------------------------------
def random_candidate(rng, length, i, quiet, sample):
    """quiet: record i keeps to positions of its own (no two events of the window can meet)"""
    pos = 10_000 + 400 * i if quiet else 10_000 + int(rng.integers(0, 300))
    shape = int(rng.integers(0, 5)) if length >= 3 else int(rng.integers(0, 2))
    if shape == 0:
        cigar = [(length, "M")]
    elif shape == 1:
        cigar = [(1, "S"), (length - 1, "M")] if length > 1 else [(1, "S")]
    elif shape == 2:
        cigar = [(length - 2, "M"), (1, "I"), (1, "M")]
    elif shape == 3:
        cigar = [(1, "M"), (3, "D"), (length - 1, "M")]
    else:
        cigar = [(length - 1, "M"), (1, "S")]
    spots = sorted(set(int(x) for x in rng.integers(0, length, int(rng.integers(0, 3)))))
    text, last = b"", -1
    for j in spots:
        if quiet and j == last + 1 and last >= 0:  # ("..C0A..": both letters land on one position, the walk's quirk)
            continue
        text += b"%d%c" % (j - last - 1, b"ACGTNacgt"[int(rng.integers(0, 9))])
        last = j
    text += b"%d" % (length - last - 1)
    tags = [b"NMi" + struct.pack("<i", len(spots)), cases.md(text), b"XBBS" + struct.pack("<i", 2) + bytes(4), b"RGZgrp\0"]
    order = rng.permutation(4)[:int(rng.integers(0, 5))]
    qual = rng.integers(0, 42, length, dtype=np.uint8)
    if i % 17 == 0:
        qual[:] = 0xFF
    return cases.rec(tags=b"".join(tags[k] for k in order), l_seq=length, pos=pos, mapq=int(rng.choice([0, 1, 19, 20, 60, 60])),
                     flag=int(rng.choice([0, 0, 0, 0x10, 0x3, 0x400, 0x200, 0x4])), cigar=cigar, qual=qual, sample=sample,
                     cut=int(rng.integers(1, 5)) if i % 11 == 0 and len(order) else None)


def sized_window(rng, size, length, quiet, n_samples=2):
    return [random_candidate(rng, length, i, quiet, int(rng.integers(0, n_samples))) for i in range(size)]


@pytest.mark.parametrize("size", [0, 1, 63, 64, 65, 1023, 1024, 1025, 5000])
def test_window_sizes(gpu, size):
    """a window of `size` candidates at each read length, quiet ones (every event on a position of its own: inactive,
    thousands of keys in the table) and loud ones, between small windows"""
    rng = np.random.default_rng(300 + size)
    windows = [sized_window(rng, 5, 151, False)]
    for length, quiet in ((1, True), (2, False), (151, True), (250, False), (151, False)):
        windows += [sized_window(rng, size, length, quiet), sized_window(rng, 3, 100, True)]
    arrays, n, nr, ns = cases.lay_out(windows)
    want = check(gpu, (arrays, n, nr, ns, np.full(n, 1001, np.uint32)), WIDE)
    assert not want["win_state"][1] & ref.MA_S_ACTIVE and not want["win_state"][5] & ref.MA_S_ACTIVE
    if size >= 1023:
        assert want["win_state"][9] & ref.MA_S_LISTED and int(want["n_selected"][0]) > size // 4
    assert not (want["win_state"] & ref.MA_S_HOST_BITS).any()


@pytest.mark.parametrize("n_samples", [1, 3])
def test_sample_counts(gpu, n_samples):
    rng = np.random.default_rng(40 + n_samples)
    windows = [sized_window(rng, 70, 151, quiet, n_samples) for quiet in (True, False, True)]
    arrays, n, nr, ns = cases.lay_out(windows, n_samples=n_samples)
    params = dict(max_sample_cov=3.0, min_anchor_cov=2, skip_active_region=False)
    want = check(gpu, (arrays, n, nr, ns, np.array([1001, 1001, 700], np.uint32)), params)
    assert len(want["win_sample_reads"]) == 3 * n_samples and want["win_sample_reads"].all()


def test_late_hits(gpu):
    """a window whose only hit is its last record, and one whose hit is in the second sample only"""
    rng = np.random.default_rng(50)
    quiet = [cases.rec(tags=cases.md(b"%dA%d" % (i % 100, 150 - i % 100)), l_seq=151, pos=10_000 + 400 * i, sample=0) for i in range(300)]
    last = cases.rec(tags=cases.md(b"7A143"), l_seq=151, pos=10_000 + 400 * 7, sample=0)  # meets record 7's mismatch
    other = [cases.rec(tags=cases.md(b"7A143"), l_seq=151, pos=10_000 + 400 * 7, sample=1),
             cases.rec(tags=cases.md(b"4C146"), l_seq=151, pos=10_000 + 400 * 7 + 3, sample=1)]
    windows = [quiet, quiet + [last], quiet + other[:1], quiet + other, sized_window(rng, 9, 100, True)]
    arrays, n, nr, ns = cases.lay_out(windows)
    want = check(gpu, (arrays, n, nr, ns, np.full(n, 1001, np.uint32)), WIDE)
    assert [bool(s & ref.MA_S_ACTIVE) for s in want["win_state"]] == [False, True, False, True, False]


def test_event_table_at_its_capacity(gpu):
    """64 records of 128 insertions each on positions of their own: MA_SELECT_EVENT_KEYS keys exactly -- not flagged; one more
    key: MA_S_EVENTS and an empty range.  The capacity is per (window, sample); a hit in another sample is still found"""
    per = 128
    assert 64 * per == capi.SELECT_EVENT_KEYS
    full = [cases.rec(l_seq=2 * per, cigar=[(1, "M"), (1, "I")] * per, pos=1000 * i) for i in range(64)]
    one = cases.rec(cigar=[(5, "M"), (1, "I"), (4, "M")], pos=90_000)
    mixed = [cases.rec(l_seq=2 * per, cigar=[(1, "M"), (1, "I"), (1, "D"), (1, "S")] * (per // 4) + [(per, "M")], pos=1000 * i,
                       tags=cases.md(b"1A" * (per // 4))) for i in range(64)]  # 32 keys in each multiset
    hit = [cases.rec(tags=cases.M3, sample=1), cases.rec(tags=cases.M3, sample=1)]
    quiet1 = [cases.rec(l_seq=2 * per, cigar=[(1, "M"), (1, "I")] * per, pos=1000 * i, sample=1) for i in range(64)]
    windows = [full, full + [one], full + [one] + hit, full + quiet1, mixed, mixed + [one], [one]]
    arrays, n, nr, ns = cases.lay_out(windows)
    want = check(gpu, (arrays, n, nr, ns, np.full(n, 1001, np.uint32)), WIDE)
    EV, A = ref.MA_S_EVENTS, ref.MA_S_ACTIVE
    assert [int(s) & (EV | A) for s in want["win_state"]] == [0, EV, A, 0, 0, EV, 0]
    assert [int(b - a) for a, b in zip(want["sel_win_off"], want["sel_win_off"][1:])] == [0, 0, 67, 0, 0, 0, 0]


def test_a_hit_behind_a_full_table_is_active_or_handed_back(gpu):
    """one sample with more keys than the table AND a position twice: the call reports MA_S_ACTIVE (it met the pair before
    the table filled) or MA_S_EVENTS (the table filled first and the host settles the window) -- include/microasm.h allows
    both, either is true to the host's answer, and the restatement marks such a window.  Every other window of the batch, a
    hit in a sample whose table does not overflow included, is what the restatement says"""
    per = 128
    full = [cases.rec(l_seq=2 * per, cigar=[(1, "M"), (1, "I")] * per, pos=1000 * i) for i in range(65)]  # 8320 keys
    pair = [cases.rec(tags=cases.M3, pos=500_000), cases.rec(tags=cases.M3, pos=500_000)]
    other = [cases.rec(tags=cases.M3, pos=500_000, sample=1), cases.rec(tags=cases.M3, pos=500_000, sample=1)]
    for order in (full + pair, pair + full):
        windows = [[cases.rec(tags=cases.M3)] * 2, full + other, order]  # the ambiguous window last: the lists in front of it stand
        arrays, n, nr, ns = cases.lay_out(windows)
        win_len = np.full(n, 1001, np.uint32)
        want = ref.select(arrays, n, nr, ns, win_len, **WIDE)
        assert want["either"].tolist() == [False, False, True]
        got = gpu.host.select_records(arrays, n, nr, win_len, **WIDE)
        rc, dev = select_device(gpu, arrays, n, nr, ns, win_len, WIDE)
        assert rc == 0
        for out in (got, dev):
            assert out["win_state"][:2].tolist() == want["win_state"][:2].tolist() == [ref.MA_S_ACTIVE | ref.MA_S_LISTED] * 2
            assert out["rec_keep"].tobytes() == want["rec_keep"].tobytes() and out["win_sample_reads"].tobytes() == want["win_sample_reads"].tobytes()
            assert out["sel_win_off"][:3].tolist() == want["sel_win_off"][:3].tolist()
            state, listed = int(out["win_state"][2]), int(out["sel_win_off"][3]) - int(out["sel_win_off"][2])
            assert (state, listed) in ((ref.MA_S_ACTIVE | ref.MA_S_LISTED, 67), (ref.MA_S_EVENTS, 0)), (state, listed)
            assert int(out["n_selected"][0]) == int(out["sel_win_off"][3])
            assert out["sel_src"][:int(want["sel_win_off"][2])].tolist() == want["sel_src"][:int(want["sel_win_off"][2])].tolist()


def test_a_record_in_two_windows(gpu):
    rng = np.random.default_rng(60)
    shared = twice = [cases.rec(tags=cases.M3, l_seq=10, pos=100, name=b"s%d" % i) for i in range(2)]
    a, b = sized_window(rng, 4, 50, True), sized_window(rng, 3, 50, True)
    arrays, n, nr, ns = cases.lay_out([a + shared, twice + b])
    for k in ("rec_off", "rec_len", "rec_sample"):  # the second window lists the bytes of the first one's records
        arrays[k][6:8] = arrays[k][4:6]
    want = check(gpu, (arrays, n, nr, ns, np.array([10, 10], np.uint32)), WIDE)
    assert want["win_state"].tolist() == [ref.MA_S_ACTIVE | ref.MA_S_LISTED] * 2
    assert want["sel_off"][want["sel_src"] == 4] == want["sel_off"][want["sel_src"] == 6]


def test_no_window_and_no_record(gpu):
    check(gpu, cases.lay_out([]) + (np.zeros(0, np.uint32),), WIDE)
    want = check(gpu, cases.lay_out([[], []]) + (np.array([10, 10], np.uint32),), dict(WIDE, min_anchor_cov=1))
    assert want["win_state"].tolist() == [ref.MA_S_LOW_COVERAGE] * 2
    check(gpu, cases.lay_out([[], []]) + (np.array([10, 0], np.uint32),), dict(WIDE, skip_active_region=True))


# ---- error paths ---------------------------------------------------------------------------------------------------------------
def _expect(gpu, case, params, word):
    """the call fails with MA_ERR_ARG in both memory spaces, names `word`, and leaves the caller's arrays alone"""
    rec, n, nr, ns, win_len = case
    with pytest.raises(EngineError) as e:
        gpu.host.select_records(rec, n, nr, win_len, **params)
    assert e.value.rc == capi.MA_ERR_ARG and word in str(e.value), str(e.value)
    assert not any(v.any() for v in e.value.arrays.values())
    rc, dev = select_device(gpu, rec, n, nr, ns, win_len, params, fill=0xC3)
    assert rc == capi.MA_ERR_ARG and word in gpu.dev.lib.ma_last_error(gpu.dev.h).decode()
    for k, v in dev.items():
        assert (v.view(np.uint8) == 0xC3).all(), k


@pytest.mark.parametrize("what", ["rec_len past the blob", "rec_off past the blob", "rec_len under the core", "l_seq 0", "l_seq huge",
                                  "l_read_name 0", "no such sample"])
def test_bad_records(gpu, what):
    rng = np.random.default_rng(70)
    arrays, n, nr, ns = cases.lay_out([sized_window(rng, 3, 151, False), sized_window(rng, 6, 151, False)])
    for i in (7, 4):  # two bad records: the first is named
        at = int(arrays["rec_off"][i])
        if what == "rec_len past the blob":
            arrays["rec_len"][i] = arrays["blob"].size - at + 1
        elif what == "rec_off past the blob":
            arrays["rec_off"][i] = arrays["blob"].size + 1
        elif what == "rec_len under the core":
            arrays["rec_len"][i] = ref.core_bytes(arrays["blob"][at:at + 32].tobytes()) - 1
        elif what == "l_seq 0":
            arrays["blob"][at + 16:at + 20] = 0
        elif what == "l_seq huge":
            arrays["blob"][at + 16:at + 20] = np.frombuffer(np.int32(1 << 30).tobytes(), dtype=np.uint8)
        elif what == "l_read_name 0":
            arrays["blob"][at + 8] = 0
        else:
            arrays["rec_sample"][i] = 2
    _expect(gpu, (arrays, n, nr, ns, np.full(n, 1001, np.uint32)), WIDE, "record 4 ")
    with pytest.raises(ref.SelectError) as e:
        ref.select(arrays, n, nr, ns, np.full(n, 1001, np.uint32))
    assert e.value.record == 4


def test_a_window_list_that_does_not_rise(gpu):
    rng = np.random.default_rng(71)
    arrays, n, nr, ns = cases.lay_out([sized_window(rng, 4, 60, False), sized_window(rng, 4, 60, False)])
    for bad in ([0, 5, 7], [1, 4, 8], [0, 9, 8]):
        arrays["rec_win_off"] = np.array(bad, dtype=np.uint32)
        _expect(gpu, (arrays, n, nr, ns, np.full(n, 1001, np.uint32)), WIDE, "rec_win_off")


def test_null_members_are_argument_errors(gpu):
    rng = np.random.default_rng(72)
    arrays, n, nr, ns = cases.lay_out([sized_window(rng, 4, 60, False)])
    win_len = np.full(n, 1001, np.uint32)
    out = capi.alloc_host(capi.select_out_spec(n, nr, ns))
    call = gpu.host.lib.ma_select_records_batch

    def structs():
        return capi.make_records_struct(arrays, n, nr), capi.make_select_params(win_len), capi.fill_struct(capi.SelectOut, out)
    rs, sp, so = structs()
    assert call(gpu.host.h, C.byref(rs), C.byref(sp), C.byref(so)) == 0
    for key in capi.SELECT_IN_KEYS:
        rs, sp, so = structs()
        setattr(rs, key, None)
        assert call(gpu.host.h, C.byref(rs), C.byref(sp), C.byref(so)) == capi.MA_ERR_ARG, key
    rs, sp, so = structs()
    sp.win_len = None
    assert call(gpu.host.h, C.byref(rs), C.byref(sp), C.byref(so)) == capi.MA_ERR_ARG
    for key, _ in capi.SelectOut._fields_:
        rs, sp, so = structs()
        setattr(so, key, None)
        assert call(gpu.host.h, C.byref(rs), C.byref(sp), C.byref(so)) == capi.MA_ERR_ARG, key
    assert call(gpu.host.h, C.byref(rs), None, C.byref(so)) == capi.MA_ERR_ARG
    for bad in (0, 257):
        rs, sp, so = structs()
        rs.n_samples_in = bad
        assert call(gpu.host.h, C.byref(rs), C.byref(sp), C.byref(so)) == capi.MA_ERR_ARG


# ---- the condition: the kernels do not pass by sending windows back ------------------------------------------------------------
def test_c3_windows_carry_no_host_bit(gpu):
    """the synth C3 shape (60x tumour / 30x normal): the restatement flags no window for the host, and neither do the kernels"""
    arrs, n, nr = synth.make_config_batch("C3", 16, first_index=0)
    rec, n, n_rec, win_len = cases.records_of_synth(arrs, n, nr, synth.CONFIGS["C3"]["roles"], np.random.default_rng(3))
    params = dict(max_sample_cov=1000.0, min_anchor_cov=5, skip_active_region=False)
    want = ref.select(rec, n, n_rec, 2, win_len, **params)
    assert not (want["win_state"] & ref.MA_S_HOST_BITS).any()
    assert (want["win_state"] & ref.MA_S_LISTED).all() and 0 < int(want["n_selected"][0]) < n_rec
    got = check(gpu, (rec, n, n_rec, 2, win_len), params)
    rc, dev = select_device(gpu, rec, n, n_rec, 2, win_len, params)
    assert rc == 0 and int((dev["win_state"] & ref.MA_S_HOST_BITS != 0).sum()) == 0
    assert (dev["win_state"] & ref.MA_S_LISTED).all() and got["win_state"].tobytes() == dev["win_state"].tobytes()


# ---- composition: selected on the device, flattened on the device, processed from the same pointers ----------------------------
def test_selected_lists_go_to_flatten_and_the_chained_call():
    """select -> flatten on the selected lists -> ma_process_cx_batch, all on device pointers, equals the same chain from the
    restatement's lists, uploaded, byte for byte.  The kept lists are the restatement's, not ReadCollector::CollectRaw's: the
    batch is synthesised, there is no BAM for the host shell to read.  tests/test_select_ref.py holds the restatement's lists
    to SelectKept's on the BAM fixture, and the driver test below runs the shell's own lists through the same chain"""
    import packed_reads_cases
    from test_gpu_flatten import OUT_CLASSES, _chain_specs
    cfg = "C2"
    p = packed_reads_cases.params(cfg)
    arrs, n, nr = synth.make_config_batch(cfg, 8, first_index=70_000)
    rec, n, n_rec, win_len = cases.records_of_synth(arrs, n, nr, synth.CONFIGS[cfg]["roles"], np.random.default_rng(78))
    params = dict(max_sample_cov=1000.0, min_anchor_cov=5, skip_active_region=False)
    want = ref.select(rec, n, n_rec, 2, win_len, **params)
    n_sel = int(want["n_selected"][0])
    assert (want["win_state"] & ref.MA_S_LISTED).all() and 0 < n_sel < n_rec  # (the filters dropped something)
    bases_cap = int(rec["rec_len"].astype(np.uint64).sum())
    eng = Engine(p, memspace=capi.MA_MEM_DEVICE)
    arena = DeviceArena()
    try:
        ins, _ = upload_inputs(arena, rec, win_len)
        rest = {k: arena.upload(rec[k]) for k in ("sample_index", "sample_case", "sample_rank", "win_chrom", "win_start0")}
        sel = {k: arena.alloc(int(sz) * np.dtype(dt).itemsize + 64) for k, (dt, sz) in capi.select_out_spec(n, n_rec, 2).items()}
        eng.select_records_device(capi.make_records_struct(dict(ins, n_samples_in=2), n, n_rec, blob_bytes=rec["blob"].size),
                                  capi.make_select_params(ins["win_len"], **params), capi.fill_struct(capi.SelectOut, sel))
        names = {k for k, _ in eng.kernel_times()}
        assert int(arena.download(sel["n_selected"], np.uint64, 1)[0]) == n_sel
        refs = {k: arena.upload(arrs[k]) for k in ("ref_bases", "ref_off")}
        specs = _chain_specs(p, n, n_sel)

        def chain(lists):
            """lists: device pointers of sel_off, sel_len, sel_win_off, sel_sample"""
            rs = capi.make_records_struct(dict(rest, blob=ins["blob"], rec_off=lists["sel_off"], rec_len=lists["sel_len"],
                                               rec_win_off=lists["sel_win_off"], rec_sample=lists["sel_sample"], n_samples_in=2),
                                          n, n_sel, 2, blob_bytes=rec["blob"].size)
            fp = {k: arena.alloc(int(sz) * np.dtype(dt).itemsize + 64) for k, (dt, sz) in capi.flat_out_spec(n_sel, bases_cap).items()}
            eng.flatten_records_device(rs, capi.make_flat_struct(fp, bases_cap))
            ptrs = [{k: arena.alloc(int(sz) * np.dtype(dt).itemsize) for k, (dt, sz) in spec.items()} for spec in specs]
            structs = [capi.fill_struct(cls, x) for cls, x in zip(OUT_CLASSES, ptrs)]
            b = capi.make_batch_struct(dict(refs, read_win_off=lists["sel_win_off"],
                                            **{k: fp[k] for k in ("read_off", "read_qname_id", "read_sample", "read_flags", "read_hint")}), n, n_sel)
            eng.process_cx_device(b, capi.make_packed_struct(dict(bases4=fp["bases4"], quals=fp["read_quals"], qual_bits=8, qual_dict=np.zeros(16, np.uint8))),
                                  capi.fill_struct(capi.ReadMeta, {k: fp[k] for k in capi.META_DTYPES}), *structs[:6], structs[6])
            eng.synchronize()
            flat = {k: arena.download(fp[k], dt, sz) for k, (dt, sz) in capi.flat_out_spec(n_sel, bases_cap).items()}
            return flat, [{k: arena.download(pt[k], dt, sz) for k, (dt, sz) in spec.items()} for spec, pt in zip(specs, ptrs)]

        got_flat, got = chain(sel)
        twin_flat, twin = chain({k: arena.upload(want[k]) for k in ("sel_off", "sel_len", "sel_win_off", "sel_sample")})
    finally:
        eng.close()
        arena.close()
    assert names == SELECT_KERNELS
    for k in got_flat:
        assert got_flat[k].tobytes() == twin_flat[k].tobytes(), k
    assert int(got[2]["win_nvars"].sum()) > 0  # (the comparison is of calls that found something)
    for g, t, spec in zip(got, twin, specs):
        for k in spec:
            assert g[k].tobytes() == t[k].tobytes(), k


# ---- the plain calls are what they were ------------------------------------------------------------------------------------------
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
    assert not names & SELECT_KERNELS


# ---- the driver, end to end --------------------------------------------------------------------------------------------------
def _thin(path, lo=4100, hi=5100, site=4701, keep_every=8):
    """of the SAM records that start in [lo, hi) only every eighth that covers `site` stays: a window there that is still
    active (the SNV at 4700) and under the anchor coverage"""
    out, k = [], 0
    for line in open(path):
        if line[0] != "@":
            pos1 = int(line.split("\t")[3])
            if lo <= pos1 < hi:
                covers = pos1 <= site < pos1 + 140
                k += covers
                if not covers or k % keep_every:
                    continue
        out.append(line)
    open(path, "w").write("".join(out))


@pytest.mark.parametrize("gates", [[], ["--window-size", "500", "--max-sample-cov", "55"]])
def test_driver_writes_the_same_vcf_with_device_select(tmp_path, gates):
    """pipeline_driver --raw-records --device-select: the candidates of every batch selected on the device, the selected lists
    flattened, then the chained call -- the VCF and the window counts are those of --raw-records, whose collector filters,
    detects active regions and gates on the host.  The second case thins the fixture around one variant and runs 500-base
    windows with --max-sample-cov 55: inactive windows, an active one under the anchor coverage, and capped ones, which come
    back to the host route"""
    import re
    import subprocess
    import test_pipeline_host as host
    exe = host.driver(tmp_path)
    host.write_fixture(str(tmp_path))
    for name in ("normal", "tumor"):
        if gates:
            _thin(str(tmp_path / (name + ".sam")))
        host.sam_to_bam(str(tmp_path / (name + ".sam")), str(tmp_path / (name + ".bam")))
    base = [exe, "--reference", str(tmp_path / "ref.fa"), "--normal", str(tmp_path / "normal.bam"), "--tumor", str(tmp_path / "tumor.bam"),
            "--region", "chr1:1-6000", "--min-kmer", "25", "--max-kmer", "25", "--batch-windows", "3", "--raw-records"] + gates
    texts, counts, back = [], [], None
    for tag, extra in (("host", []), ("device", ["--device-select"])):
        vcf = tmp_path / f"calls_{tag}.vcf"
        r = subprocess.run(base + ["--out-vcf", str(vcf)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = open(vcf, "rb").read().split(b"\n")
        texts.append(b"\n".join(x for x in lines if not x.startswith(b"##commandLine=")))
        counts.append(re.search(r"pipeline_driver: (\d+ windows \(.*records)\n", r.stderr).group(1))
        if extra:
            back = int(re.search(r"--device-select handed (\d+) windows back", r.stderr).group(1))
    assert texts[0] == texts[1] and sum(not x.startswith(b"#") for x in texts[1].split(b"\n") if x) >= (3 if gates else 6)
    assert counts[0] == counts[1], counts
    inactive, low = (int(x) for x in re.search(r"(\d+) inactive, (\d+) below anchor coverage", counts[1]).groups())
    n_windows = int(counts[1].split()[0])
    if gates:
        assert inactive >= 1 and low >= 1 and 0 < back < n_windows - inactive - low, (counts, back)
    else:
        assert back == 0
