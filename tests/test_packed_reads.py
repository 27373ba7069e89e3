"""Packed read input (ma_packed_reads_t, ma_process_packed_batch, ma_prefetch_packed_batch) without a GPU: the nibble layout
of capi.pack_reads, the two calls in the header and the library, the struct's layout against gcc, and the host shell's packer
and the kernel's per-lane step (both in tests/host/packed_units.cpp) against capi.pack_reads / a nibble-by-nibble decode."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from lancet2_amd import capi

import packed_reads_cases as cases

REPO = capi.REPO
HEADER = os.path.join(REPO, "include", "microasm.h")
LETTERS = cases.LETTERS


def _arrs(lens, bases=None, quals=None, seed=5):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    total = int(off[-1])
    bases = LETTERS[rng.integers(0, 16, total)] if bases is None else bases
    quals = rng.integers(0, 8, total).astype(np.uint8) * 5 if quals is None else quals
    pad = np.zeros(64, np.uint8)
    return dict(read_off=off, read_bases=np.concatenate([bases, pad]), read_quals=np.concatenate([quals.astype(np.uint8), pad]))


def _decode(packed, off):
    """nibble by nibble, from the layout rule as include/microasm.h states it -- independent of capi's vectorised code"""
    out = []
    for r in range(len(off) - 1):
        at = (int(off[r]) + r) >> 1
        for j in range(int(off[r + 1]) - int(off[r])):
            b = int(packed[at + j // 2])
            out.append(b & 15 if j & 1 else b >> 4)
    return np.array(out, dtype=np.uint8)


def test_pack_reads_round_trip_and_layout():
    lens = [1, 2, 7, 8, 9, 150, 151, 3, 150]
    total = sum(lens)
    bases = LETTERS[np.arange(total) % 16]  # all 16 codes, at even and odd positions of reads of every parity
    arrs = _arrs(lens, bases=bases)
    packed, twin = capi.pack_reads(arrs)
    off = arrs["read_off"]
    n = len(lens)
    assert packed["qual_bits"] == 4
    assert len(packed["bases4"]) == (total + n + 1) // 2 == len(packed["quals"])
    assert np.array_equal(LETTERS[_decode(packed["bases4"], off)], bases)
    assert np.array_equal(packed["qual_dict"][_decode(packed["quals"], off)], arrs["read_quals"][:total])
    assert np.array_equal(capi.unpack_nibbles(packed["bases4"], off), _decode(packed["bases4"], off))
    assert np.array_equal(twin["read_bases"].view(np.uint8), arrs["read_bases"].view(np.uint8))
    assert np.array_equal(twin["read_quals"].view(np.uint8), arrs["read_quals"].view(np.uint8))
    # reads start on byte boundaries and never overlap: read r owns bytes [(off[r] + r) >> 1, + (len + 1) // 2)
    end = 0
    for r, ln in enumerate(lens):
        at = (int(off[r]) + r) >> 1
        assert at >= end
        end = at + (ln + 1) // 2
    assert end <= len(packed["bases4"])
    # the unused low nibble of an odd read's last byte and the bytes between reads are zero here (the device ignores them)
    assert packed["bases4"][0] & 15 == 0
    # letters that BAM has no code for become N, in the packed form and in the twin
    odd = _arrs([4], bases=np.frombuffer(b"aXN.", dtype=np.uint8))
    p2, t2 = capi.pack_reads(odd)
    assert bytes(t2["read_bases"][:4]) == b"NNNN" and p2["bases4"].tolist() == [0xFF, 0xFF, 0]  # (4 + 1 + 1) // 2 bytes


def test_pack_reads_of_windows_without_reads():
    arrs = dict(read_off=np.zeros(1, np.uint64), read_bases=np.zeros(64, np.uint8), read_quals=np.zeros(64, np.uint8))
    packed, twin = capi.pack_reads(arrs)
    assert len(packed["bases4"]) == 0 and len(packed["quals"]) == 0 and packed["qual_bits"] == 4
    arrs = _arrs([0, 5, 0, 0, 6])  # reads of length zero in between
    packed, _ = capi.pack_reads(arrs)
    assert len(packed["bases4"]) == (11 + 5 + 1) // 2
    assert np.array_equal(LETTERS[_decode(packed["bases4"], arrs["read_off"])], arrs["read_bases"][:11])


def test_quality_dictionary_sixteen_values_fit_seventeen_do_not():
    q16 = np.concatenate([[0, 93], np.arange(2, 16)]).astype(np.uint8)  # sixteen distinct values, 0 and 93 among them
    arrs = _arrs([9, 7], quals=q16)
    packed, _ = capi.pack_reads(arrs)
    assert packed["qual_bits"] == 4 and packed["qual_dict"].tolist() == sorted(q16.tolist())
    assert np.array_equal(packed["qual_dict"][_decode(packed["quals"], arrs["read_off"])], q16)
    q17 = np.concatenate([q16, [40]]).astype(np.uint8)
    arrs = _arrs([9, 8], quals=q17)
    packed, _ = capi.pack_reads(arrs)
    assert packed["qual_bits"] == 8 and np.array_equal(packed["quals"][:17], q17)
    with pytest.raises(ValueError):
        capi.pack_reads(arrs, qual_bits=4)
    packed, _ = capi.pack_reads(_arrs([9, 7], quals=q16), qual_bits=8)  # 8 bits may always be asked for
    assert packed["qual_bits"] == 8
    s = capi.make_packed_struct(packed)
    assert s.qual_bits == 8 and s.bases4 == packed["bases4"].ctypes.data and s.quals == packed["quals"].ctypes.data


def test_header_declares_and_library_exports_the_packed_calls():
    text = open(HEADER).read()
    for name in ("ma_process_packed_batch", "ma_prefetch_packed_batch"):
        assert f"int {name}(ma_ctx_t* ctx, const ma_batch_t*" in text, name
    assert "#define MA_VERSION 3" in text and "typedef struct ma_packed_reads {" in text
    assert os.path.exists(capi.LIB_PATH), "libmicroasm.so is not built: run __graft_entry__.build()"
    lib = capi.load_cdll()
    for name in ("ma_process_packed_batch", "ma_prefetch_packed_batch"):
        assert getattr(lib, name) is not None


def test_packed_struct_offsets_match_the_compiled_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cname, cls = "ma_packed_reads_t", capi.PackedReads
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "microasm.h"', 'int main(void) {',
             f'  printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got[cname]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname


def _units(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "packed_units")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(REPO, "tests", "host", "packed_units.cpp"), "-I",
                           os.path.join(REPO, "include"), "-lpthread", "-o", exe])
    return exe


def test_kernel_step_and_host_packer(tmp_path):
    """tests/host/packed_units.cpp: the per-lane step of k_unpack_reads (csrc/unpack_core.h, the two GPU instructions restated
    in C++) against a nibble-by-nibble decode, then FlatBatch::PackReads of pipeline_host.hpp against capi.pack_reads on the
    reads of the test batches -- 4-bit and 8-bit qualities."""
    exe = _units(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "packed units ok" in r.stdout, r.stderr
    for cfg, bits in (("C2", 4), ("C2", 8), ("C5", 4)):
        arrs, n, nr, packed, twin = cases.batch(cfg, bits)
        off = arrs["read_off"]
        total = int(off[-1])
        fin, fout = tmp_path / "reads.bin", tmp_path / "packed.bin"
        with open(fin, "wb") as f:
            f.write(struct.pack("<Q", len(off)) + off.tobytes() + arrs["read_bases"][:total].tobytes() +
                    arrs["read_quals"][:total].tobytes())
        r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        blob = open(fout, "rb").read()
        nb, nq, got_bits = struct.unpack("<QQQ", blob[:24])
        assert got_bits == bits
        assert np.array_equal(np.frombuffer(blob[24:40], np.uint8), packed["qual_dict"])
        assert np.array_equal(np.frombuffer(blob[40:40 + nb], np.uint8), packed["bases4"])
        if bits == 4:
            assert np.array_equal(np.frombuffer(blob[40 + nb:40 + nb + nq], np.uint8), packed["quals"])
        else:
            assert nq == 1  # (the Phred bytes are passed as they are; the unused array is one byte, never null)


def test_bam_sequence_bytes_are_copied_to_the_reads_nibble_offset(tmp_path):
    """pipeline_driver --packed-reads --extract-only --dump (no device): the collector copies a BAM record's sequence bytes,
    undecoded, to byte (read_off[r] + r) >> 1 of the batch's nibble array, and packs SAM text to the same bytes -- both equal
    capi.pack_reads of the ASCII read_bases the run without the flag dumps; every other array is the same in all three runs."""
    import test_pipeline_host as host
    exe = host.driver(tmp_path)
    host.write_fixture(str(tmp_path))
    for name in ("normal", "tumor"):
        host.sam_to_bam(str(tmp_path / (name + ".sam")), str(tmp_path / (name + ".bam")))

    def run(ext, tag, extra):
        d = tmp_path / ("dump_" + tag)
        d.mkdir()
        r = subprocess.run([exe, "--reference", str(tmp_path / "ref.fa"), "--normal", str(tmp_path / ("normal." + ext)),
                            "--tumor", str(tmp_path / ("tumor." + ext)), "--region", "chr1:1-6000", "--batch-windows", "3",
                            "--dump", str(d), "--extract-only"] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return {(b, f): np.fromfile(str(d / b / f), dtype=np.uint8) for b in sorted(os.listdir(d)) for f in sorted(os.listdir(d / b))}

    plain = run("sam", "ascii", [])
    from_bam = run("bam", "bam4", ["--packed-reads"])
    from_sam = run("sam", "sam4", ["--packed-reads"])
    batches = sorted({b for b, _ in plain})
    assert len(batches) == 3 and from_bam.keys() == from_sam.keys() == plain.keys() | {(b, "bases4.u8") for b in batches}
    odd_starts = 0
    for b in batches:
        off = plain[(b, "read_off.u64")].view(np.uint64)
        total = int(off[-1])
        assert total > 0
        arrs = dict(read_off=off, read_bases=plain[(b, "read_bases.u8")], read_quals=plain[(b, "read_quals.u8")])
        want = capi.pack_reads(arrs)[0]["bases4"]
        assert np.array_equal(from_bam[(b, "bases4.u8")], want), b
        assert np.array_equal(from_sam[(b, "bases4.u8")], want), b
        assert np.array_equal(LETTERS[_decode(from_bam[(b, "bases4.u8")], off)], plain[(b, "read_bases.u8")][:total])
        odd_starts += int(np.count_nonzero((off[:-1] + np.arange(len(off) - 1, dtype=np.uint64)) & np.uint64(1)))
        for (bb, f), v in plain.items():
            if bb == b and f != "read_bases.u8":
                assert np.array_equal(from_bam[(bb, f)], v) and np.array_equal(from_sam[(bb, f)], v), (b, f)
        assert len(from_bam[(b, "read_bases.u8")]) == 64  # (no ASCII copy is kept: the pad alone)
    assert odd_starts > 0  # reads whose nibble index is odd still start on a byte: the rule's rounding was exercised
    r = subprocess.run([exe, "--reference", str(tmp_path / "ref.fa"), "--normal", str(tmp_path / "normal.sam"), "--packed-reads",
                        "--collect-reads", "--extract-only"], capture_output=True, text=True)
    assert r.returncode == 2 and "--packed-reads needs the flat collector" in r.stderr
