"""tests/flatten_ref.py, the plain-Python restatement of ma_flatten_records_batch, on hand-made records for every rule of
include/microasm.h, and the call's ABI: the header declares and the library exports it, the two structs are laid out as
lancet2_amd/capi.py says.  Runs without a GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import flatten_ref as ref
from lancet2_amd import capi

HEADER = os.path.join(capi.REPO, "include", "microasm.h")


def one_window(records, samples=((0, 0, 0), (1, 1, 1)), win_chrom=0, win_start0=1000, n_refs=4, gap=b"\x99\x77\x55"):
    """records: (bytes, input sample) pairs -> the ma_records_t arrays of one window, records 3 junk bytes apart"""
    blob, off, ln = bytearray(b"\x01"), [], []
    for body, _ in records:
        blob += gap
        off.append(len(blob))
        ln.append(len(body))
        blob += body
    rec = dict(blob=np.frombuffer(bytes(blob), dtype=np.uint8).copy(), rec_off=np.array(off, dtype=np.uint64),
               rec_len=np.array(ln, dtype=np.uint32), rec_win_off=np.array([0, len(records)], dtype=np.uint32),
               rec_sample=np.array([s for _, s in records], dtype=np.uint8),
               sample_index=np.array([s[0] for s in samples], dtype=np.uint8), sample_case=np.array([s[1] for s in samples], dtype=np.uint8),
               sample_rank=np.array([s[2] for s in samples], dtype=np.uint32), win_chrom=np.array([win_chrom], dtype=np.int32),
               win_start0=np.array([win_start0], dtype=np.int64))
    return rec, 1, len(records), n_refs


def rec(name, l_seq=150, claim=None, **kw):
    """a record of l_seq bases; claim: what its l_seq field says, if not that"""
    if claim is not None:
        kw["l_seq"] = claim
    kw.setdefault("cigar", [(l_seq, "M")])
    kw.setdefault("qual", bytes(range(1, l_seq + 1)) if l_seq < 200 else bytes(l_seq))
    kw.setdefault("seq4", bytes((i * 37 + 1) & 0xFF for i in range((l_seq + 1) // 2)))
    return ref.encode_record(name, **kw)


def test_soft_clip_fraction_boundary():
    """9 of 150 bases clipped is 6 % exactly: set; 8 of 150 is not.  Every S operation counts, H never does"""
    got = ref.flatten(*one_window([(rec(b"a", cigar=[(9, "S"), (141, "M")]), 0), (rec(b"b", cigar=[(8, "S"), (142, "M")]), 0),
                                   (rec(b"c", cigar=[(4, "S"), (141, "M"), (5, "S")], flag=0x2), 0),
                                   (rec(b"d", cigar=[(50, "H"), (150, "M")]), 0), (rec(b"e", l_seq=50, cigar=[(3, "S"), (47, "M")], flag=0x2), 0)]))
    assert got["read_mflags"].tolist() == [ref.MA_RM_SOFTCLIP, 0, ref.MA_RM_SOFTCLIP | ref.MA_RM_PROPER, 0, ref.MA_RM_SOFTCLIP | ref.MA_RM_PROPER]


def test_leading_clip_is_the_first_operation_only():
    got = ref.flatten(*one_window([(rec(b"a", pos=1100, cigar=[(5, "H"), (10, "S"), (140, "M")]), 0),
                                   (rec(b"b", pos=1100, cigar=[(10, "S"), (140, "M")]), 0),
                                   (rec(b"c", pos=1100, cigar=[(140, "M"), (10, "S")]), 0), (rec(b"d", pos=1100, cigar=[]), 0)]))
    assert got["read_hint"].tolist() == [100, 90, 100, 100]
    assert got["read_mflags"].tolist() == [1, 1, 1, 0]  # (10 of 150 clipped wherever the S stands)


def test_mapq_19_and_20():
    got = ref.flatten(*one_window([(rec(b"a", mapq=19), 0), (rec(b"b", mapq=20), 0), (rec(b"c", mapq=19, flag=0x10), 1), (rec(b"d", mapq=255), 1)]))
    assert got["read_src"].tolist() == [1, 3, 0, 2]  # the passing reads first, then by sample rank
    assert got["read_flags"].tolist() == [ref.MA_RF_PASS, ref.MA_RF_PASS | ref.MA_RF_CASE, 0, ref.MA_RF_CASE | ref.MA_RF_REV]
    assert got["read_mapq"].tolist() == [20, 255, 19, 19]


def test_hint_overflow_and_foreign_chrom():
    top = (1 << 31) - 1
    cases = [(rec(b"a", pos=top, refid=0), 0), (rec(b"b", pos=top - 2, refid=0), 0),  # -> INT32_MAX (no hint), INT32_MAX - 2
             (rec(b"c", pos=0, refid=0), 0), (rec(b"d", pos=5, refid=1), 0), (rec(b"e", pos=5, refid=-1), 0), (rec(b"f", pos=5, refid=4), 0)]
    got = ref.flatten(*one_window(cases, win_start0=0))
    assert got["read_hint"].tolist() == [ref.MA_NO_HINT, top - 2, 0, ref.MA_NO_HINT, ref.MA_NO_HINT, ref.MA_NO_HINT]
    low = ref.flatten(*one_window([(rec(b"a", pos=0), 0), (rec(b"b", pos=1), 0), (rec(b"c", pos=2), 0)], win_start0=1 << 31))
    assert low["read_hint"].tolist() == [ref.MA_NO_HINT, -(1 << 31) + 1, -(1 << 31) + 2]  # INT32_MIN is MA_NO_HINT itself
    mapped = ref.flatten(*one_window([(rec(b"a", refid=2), 0), (rec(b"a", refid=0), 1)], win_chrom=7), )
    assert mapped["read_hint"].tolist() == [ref.MA_NO_HINT] * 2


def test_ref_map_names_the_chrom_per_sample():
    r, n, nr, _ = one_window([(rec(b"a", refid=1, pos=1010), 0), (rec(b"a", refid=1, pos=1010), 1)], win_chrom=3)
    r["ref_map"] = np.array([0, 3, 0, 1], dtype=np.int32)  # sample 0: refID 1 -> chrom 3; sample 1: refID 1 -> chrom 1
    got = ref.flatten(r, n, nr, 2)
    assert got["read_hint"].tolist() == [10, ref.MA_NO_HINT]


def test_pos_minus_one_and_tlen():
    got = ref.flatten(*one_window([(rec(b"a", pos=-1, tlen=-(1 << 31)), 0), (rec(b"b", pos=7, tlen=(1 << 31) - 1), 0)], win_start0=0))
    assert got["read_start"].tolist() == [0, 7] and got["read_hint"].tolist() == [-1, 7]
    assert got["read_isize"].tolist() == [-(1 << 31), (1 << 31) - 1]


def test_absent_qualities_and_the_nibble_layout():
    """0xFF qualities become 0; sequence bytes verbatim at byte (read_off[r] + r) >> 1, zero between the reads"""
    recs = [(rec(b"a", l_seq=3, qual=b"\xff\xff\xff", seq4=b"\x12\x3f"), 0), (rec(b"b", l_seq=4, qual=b"\x01\xff\x02\xfe", seq4=b"\x48\x21"), 0),
            (rec(b"c", l_seq=1, qual=b"\x09", seq4=b"\x8f"), 0)]
    got = ref.flatten(*one_window(recs))
    assert got["read_off"].tolist() == [0, 3, 7, 8] and int(got["n_bases"][0]) == 8
    assert got["read_quals"].tolist() == [0, 0, 0, 1, 0, 2, 0xFE, 9]
    # read 0 at byte 0 (two bytes), read 1 at (3 + 1) >> 1 = 2 (two bytes), read 2 at (7 + 2) >> 1 = 4, and (8 + 3 + 1) // 2 = 6 bytes
    assert got["bases4"].tolist() == [0x12, 0x3F, 0x48, 0x21, 0x8F, 0x00]


def test_names_order_and_ids():
    names = [b"r10", b"r1\x80", b"r1", b"r", b"r1", b"\xffz", b"r1"]
    got = ref.flatten(*one_window([(rec(nm, pos=100 - i), i % 2) for i, nm in enumerate(names)], samples=((0, 0, 5), (1, 0, 5))))
    # one sample rank for both samples: names decide, then chrom, pos (descending arrival here), then arrival
    assert [names[i] for i in got["read_src"]] == [b"r", b"r1", b"r1", b"r1", b"r10", b"r1\x80", b"\xffz"]
    assert got["read_src"].tolist()[1:4] == [6, 4, 2] and got["read_qname_id"].tolist() == [0, 1, 1, 1, 2, 3, 4]


def test_bad_records_and_capacity():
    good = rec(b"ok")
    for bad in (rec(b"x", claim=1 << 20), rec(b"x", l_seq=0, qual=b""), rec(b"x", l_read_name=0), rec(b"x")[:-1]):
        with pytest.raises(ref.FlattenError) as e:
            ref.flatten(*one_window([(good, 0), (bad, 0), (bad, 1)]))
        assert e.value.rc == ref.MA_ERR_ARG and e.value.record == 1
    r, n, nr, n_refs = one_window([(good, 0), (good, 1)])
    r["rec_len"][1] += 100  # past the blob
    with pytest.raises(ref.FlattenError) as e:
        ref.flatten(r, n, nr, n_refs)
    assert e.value.record == 1
    with pytest.raises(ref.FlattenError) as e:
        ref.flatten(*one_window([(good, 0), (good, 2)]))  # no such sample
    assert e.value.record == 1
    with pytest.raises(ref.FlattenError) as e:
        ref.flatten(*one_window([(good, 0), (good, 1)]), bases_cap=299)
    assert e.value.rc == ref.MA_ERR_ARG and e.value.n_bases == 300
    assert int(ref.flatten(*one_window([(good, 0), (good, 1)]), bases_cap=300)["n_bases"][0]) == 300
    tagged = ref.flatten(*one_window([(good + b"NMC\x03", 0)]))  # tags behind the core are not looked at
    assert int(tagged["n_bases"][0]) == 150


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_call():
    text = open(HEADER).read()
    assert "int ma_flatten_records_batch(ma_ctx_t* ctx, const ma_records_t* in, const ma_flat_out_t* out);" in text
    assert "typedef struct ma_records {" in text and "typedef struct ma_flat_out {" in text
    assert f"#define MA_FLATTEN_MAX_WINDOW {capi.FLATTEN_MAX_WINDOW}" in text and capi.FLATTEN_MAX_WINDOW >= 16384 == ref.MAX_WINDOW
    assert os.path.exists(capi.LIB_PATH), "libmicroasm.so is not built: run __graft_entry__.build()"
    lib = capi.load_cdll()
    assert hasattr(lib, "ma_flatten_records_batch")
    from lancet2_amd.engine import Engine
    assert callable(getattr(Engine, "flatten_records")) and callable(getattr(Engine, "flatten_records_device"))


@pytest.mark.parametrize("cname,cls", [("ma_records_t", capi.Records), ("ma_flat_out_t", capi.FlatOut)])
def test_struct_layout_matches_the_header(tmp_path, cname, cls):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    lines = ['#include <cstdio>', '#include <cstddef>', '#include "microasm.h"', 'int main() {',
             f'  std::printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'  std::printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.cpp"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got[cname]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname
    spec = capi.flat_out_spec(5, 40)
    assert set(spec) == {f for f, _ in capi.FlatOut._fields_} - {"bases_cap"} and spec["bases4"][1] == (40 + 5 + 1) // 2
    assert set(capi.records_spec(2, 5, 100, 3, n_refs=4)) == set(capi.RECORDS_DTYPES)


# ---- the restatement against the host shell ---------------------------------------------------------------------------------
def _load_dump(d):
    def arr(name, dt):
        return np.fromfile(os.path.join(d, name), dtype=dt)
    return arr


def test_restatement_equals_the_host_collector(tmp_path):
    """pipeline_driver --raw-records dumps the ma_records_t arrays of every batch; flatten_ref applied to them must give,
    byte for byte, the arrays ReadCollector::CollectFlat makes of the same windows (--packed-reads): the restatement is the
    host shell's semantics, and CollectRaw keeps the records CollectFlat keeps, in its arrival order"""
    from test_pipeline_host import driver, sam_to_bam, write_fixture
    exe = driver(tmp_path)
    write_fixture(str(tmp_path))
    for name in ("normal", "tumor"):
        sam_to_bam(str(tmp_path / (name + ".sam")), str(tmp_path / (name + ".bam")))
    dumps = {}
    for mode in ("--packed-reads", "--raw-records"):
        d = tmp_path / ("dump" + mode)
        d.mkdir()
        r = subprocess.run([exe, "--reference", str(tmp_path / "ref.fa"), "--normal", str(tmp_path / "normal.bam"),
                            "--tumor", str(tmp_path / "tumor.bam"), "--region", "chr1:1-6000", "--batch-windows", "4",
                            "--dump", str(d), "--extract-only", mode], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        dumps[mode] = d
    batches = sorted(os.listdir(dumps["--packed-reads"]))
    assert batches == sorted(os.listdir(dumps["--raw-records"])) and len(batches) >= 2
    n_reads = 0
    for b in batches:
        A, B = _load_dump(dumps["--packed-reads"] / b), _load_dump(dumps["--raw-records"] / b)
        for same in ("ref_bases.u8", "ref_off.u32", "windows.u64"):
            assert open(dumps["--packed-reads"] / b / same, "rb").read() == open(dumps["--raw-records"] / b / same, "rb").read(), same
        n_samples, n_refs = (int(x) for x in B("counts.i32", np.int32))
        rec = dict(blob=B("blob.u8", np.uint8), rec_off=B("rec_off.u64", np.uint64), rec_len=B("rec_len.u32", np.uint32),
                   rec_win_off=B("rec_win_off.u32", np.uint32), rec_sample=B("rec_sample.u8", np.uint8),
                   sample_index=B("sample_index.u8", np.uint8), sample_case=B("sample_case.u8", np.uint8),
                   sample_rank=B("sample_rank.u32", np.uint32), ref_map=B("ref_map.i32", np.int32),
                   win_chrom=B("win_chrom.i32", np.int32), win_start0=B("win_start0.i64", np.int64))
        assert len(rec["sample_rank"]) == n_samples == 2 and n_refs == 1
        n, nr = len(rec["win_chrom"]), len(rec["rec_off"])
        got = ref.flatten(rec, n, nr, n_refs)
        assert got["read_src"].tolist() != list(range(nr))  # (the records arrive unsorted: the sort is the call's)
        assert A("read_win_off.u32", np.uint32).tobytes() == rec["rec_win_off"].tobytes()
        total = int(got["n_bases"][0])
        for name, dt, key, cut in (("read_off.u64", np.uint64, "read_off", None), ("bases4.u8", np.uint8, "bases4", (total + nr + 1) // 2),
                                   ("read_quals.u8", np.uint8, "read_quals", total), ("read_qname_id.u32", np.uint32, "read_qname_id", None),
                                   ("read_sample.u8", np.uint8, "read_sample", None), ("read_flags.u8", np.uint8, "read_flags", None),
                                   ("read_hint.i32", np.int32, "read_hint", None), ("read_mapq.u8", np.uint8, "read_mapq", None),
                                   ("read_mflags.u8", np.uint8, "read_mflags", None), ("read_isize.i32", np.int32, "read_isize", None),
                                   ("read_start.i32", np.int32, "read_start", None)):
            want = A(name, dt)
            assert want[:cut].tobytes() == got[key].tobytes(), (b, name)
            assert not want[cut:].any() if cut is not None else True  # (behind the arrays: the host's padding)
        n_reads += nr
    assert n_reads > 1000


def test_raw_records_needs_bam_input(tmp_path):
    from test_pipeline_host import driver, write_fixture
    exe = driver(tmp_path)
    write_fixture(str(tmp_path))
    r = subprocess.run([exe, "--reference", str(tmp_path / "ref.fa"), "--normal", str(tmp_path / "normal.sam"), "--tumor",
                        str(tmp_path / "tumor.sam"), "--extract-only", "--raw-records"], capture_output=True, text=True)
    assert r.returncode == 2 and "is not a BAM file" in r.stderr


def test_collect_raw_keeps_what_collect_flat_keeps(tmp_path):
    """tests/host/raw_units.cpp: the two collectors on one BAM, with and without the coverage cap"""
    from test_pipeline_host import build, sam_to_bam, write_fixture
    write_fixture(str(tmp_path))
    for name in ("normal", "tumor"):
        sam_to_bam(str(tmp_path / (name + ".sam")), str(tmp_path / (name + ".bam")))
    exe, _ = build(tmp_path, "tests/host/raw_units.cpp", "raw_units", ["-DLANCET2_AMD_WITH_ZLIB", "-lz"])
    r = subprocess.run([exe, str(tmp_path / "ref.fa"), str(tmp_path / "normal.bam"), str(tmp_path / "tumor.bam")], capture_output=True, text=True)
    assert r.returncode == 0 and "raw units ok" in r.stdout, r.stdout + r.stderr
