"""The case table of ma_inflate_blocks_batch / ma_index_records_batch (tests/inflate_cases.py) without a GPU: zlib inflates
every good member to the payload and CRC the case states and rejects every MA_Z_DATA member; the restatement
(tests/inflate_ref.py) gives every case the state it names; the decode core (lancet2_amd/csrc/inflate_core.h) does the same on
the host, in a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import inflate_cases as cases
import inflate_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = cases.all_members()
# MA_Z_DATA cases whose stream zlib takes: the rule is about ISIZE, which zlib never sees
ABOUT_ISIZE = {"ISIZE one too small"}


def test_labels_are_unique_and_every_state_occurs():
    labels = [m[0] for m in MEMBERS]
    assert len(set(labels)) == len(labels)
    assert {m[2] for m in MEMBERS} == {0, cases.HEADER, cases.ISIZE, cases.DATA, cases.SHORT, cases.CRC}


@pytest.mark.parametrize("case", [m for m in MEMBERS if m[2] == 0], ids=lambda m: m[0])
def test_zlib_inflates_every_good_member_to_its_payload(case):
    label, m, _, payload = case
    state, data, crc, isize = ref.parse_member(m)
    assert state == 0 and isize == len(payload)
    assert ref.zlib_inflate(data) == payload and zlib.crc32(payload) == crc


@pytest.mark.parametrize("case", [m for m in MEMBERS if m[2] == cases.DATA], ids=lambda m: m[0])
def test_zlib_rejects_every_data_case(case):
    label, m, _, _ = case
    state, data, crc, isize = ref.parse_member(m)
    assert state == 0
    if label in ABOUT_ISIZE:
        assert len(ref.zlib_inflate(data)) > isize
        return
    with pytest.raises(zlib.error):
        ref.zlib_inflate(data)


@pytest.mark.parametrize("case", MEMBERS, ids=lambda m: m[0])
def test_the_restatement_gives_every_case_its_state(case):
    label, m, want, payload = case
    state, size, got = ref.member_state(m)
    assert state == want
    if want == 0:
        assert got == payload and size == len(payload)
    elif want in (cases.HEADER, cases.ISIZE):
        assert size == 0
    else:
        assert size == struct.unpack("<I", m[-4:])[0]


def test_short_and_crc_cases_are_whole_streams():
    """MA_Z_SHORT and MA_Z_CRC are not MA_Z_DATA: zlib takes their streams to the end"""
    for label, m, want, _ in MEMBERS:
        if want in (cases.SHORT, cases.CRC):
            state, data, crc, isize = ref.parse_member(m)
            payload = ref.zlib_inflate(data)
            assert (len(payload) < isize) if want == cases.SHORT else (len(payload) == isize and zlib.crc32(payload) != crc), label


def test_restatement_lays_the_payloads_end_to_end():
    rng = np.random.default_rng(1)
    picked = [m for m in MEMBERS if len(m[1]) < 3000]
    blob, off, length = cases.lay_out([m[1] for m in picked], rng)
    length[[b for b, m in enumerate(picked) if m[2] == 0][::2]] += 1  # blk_len may pass the member's end
    got = ref.inflate(blob, off, length)
    at = 0
    for b, (label, m, want, payload) in enumerate(picked):
        assert got["blk_state"][b] == want and got["blk_raw_off"][b] == at, label
        size = struct.unpack("<I", m[-4:])[0] if want not in (cases.HEADER, cases.ISIZE) else 0
        if want == 0:
            assert got["raw"][at:at + size].tobytes() == payload and got["defined"][at:at + size].all()
        else:
            assert not got["defined"][at:at + size].any()
        at += size
    assert got["n_raw"][0] == at == got["blk_raw_off"][-1] and got["n_flagged"][0] == sum(m[2] != 0 for m in picked)
    with pytest.raises(ref.InflateError) as e:
        ref.inflate(blob, off, length, raw_cap=at - 1)
    assert e.value.need == at
    ref.inflate(blob, off, length, raw_cap=at)
    length[3] = blob.size - int(off[3]) + 1
    length[7] = blob.size
    with pytest.raises(ref.InflateError) as e:
        ref.inflate(blob, off, length)
    assert e.value.which == 3


def test_record_streams_by_hand():
    raw, begin, end, names = cases.stream_cases()
    got = ref.index(raw, begin, end)
    count = np.diff(got["str_rec_off"].astype(np.int64))

    def of(label):
        s = names[label]
        a, b = int(got["str_rec_off"][s]), int(got["str_rec_off"][s + 1])
        return int(got["str_state"][s]), {k: got[k][a:b] for k in ("rec_off", "rec_len", "rec_ref", "rec_pos", "rec_span")}

    assert of("no record")[0] == 0 and count[names["no record"]] == 0
    state, one = of("one record")
    assert state == 0 and one["rec_pos"].tolist() == [100] and one["rec_off"][0] == begin[names["one record"]] + 4
    assert of("ends exactly at a record's start")[1]["rec_pos"].tolist() == [100, 101]
    assert of("ends one byte behind a record's start")[1]["rec_pos"].tolist() == [100, 101, 102]
    shared = of("shares records with the stream in front")[1]
    assert shared["rec_pos"].tolist() == [101, 102, 103] and shared["rec_off"][0] == of("ends one byte behind a record's start")[1]["rec_off"][1]
    state, every = of("every operation, no CIGAR, negative pos and refID, a span that wraps, tags")
    assert state == 0 and every["rec_span"].tolist() == [3 + 4 + 100 + 8 + 9, 0, (17 * (2**28 - 1)) % 2**32, 10]
    assert every["rec_ref"].tolist() == [-1, 7, 0, 0] and every["rec_pos"].tolist() == [-1, 2**31 - 1, 100, 100]
    for label in ("block_size 31", "a core beyond block_size", "l_seq -1", "block_size past raw_bytes"):
        state, kept = of(label)
        assert state == cases.BAD_RECORD and len(kept["rec_off"]) == 1, label  # the record in front is kept, the bad one is not listed
    assert of("a block_size field cut by the end of raw")[0] == cases.BAD_RECORD
    assert of("at the end of raw")[0] == 0 and count[names["at the end of raw"]] == 0
    # a listed record is what ma_records_t takes: rec_off at refID, rec_len = block_size
    for off, n in zip(got["rec_off"], got["rec_len"]):
        assert struct.unpack_from("<I", raw, int(off) - 4)[0] == n
    total = int(got["n_found"][0])
    with pytest.raises(ref.InflateError) as e:
        ref.index(raw, begin, end, rec_cap=total - 1)
    assert e.value.need == total
    for bad_begin, bad_end in ((5, 4), (0, raw.size + 1)):
        b2, e2 = begin.copy(), end.copy()
        b2[2], e2[2] = bad_begin, bad_end
        with pytest.raises(ref.InflateError) as e:
            ref.index(raw, b2, e2)
        assert e.value.which == 2


def test_decode_core_on_the_host_under_sanitizers(tmp_path):
    """tests/host/inflate_units.cpp: parse_member, inflate_member and the sliced CRC of inflate_core.h over the whole case
    table, compiled with -fsanitize=address,undefined and run as a plain executable"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe, table = str(tmp_path / "inflate_units"), str(tmp_path / "cases.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(REPO, "tests", "host", "inflate_units.cpp"), "-I", os.path.join(REPO, "include"), "-o", exe])
    cases.dump(table, MEMBERS)
    r = subprocess.run([exe, table], capture_output=True, text=True)
    labels = [m[0] for m in MEMBERS]
    named = "\n".join(f"{line}  <- {labels[int(line.split()[1].rstrip(':'))]}" for line in r.stderr.splitlines() if line.startswith("case "))
    assert r.returncode == 0 and f"inflate units ok: {len(MEMBERS)} cases" in r.stdout, named + "\n" + r.stderr[-3000:]
