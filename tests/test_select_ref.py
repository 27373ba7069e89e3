"""tests/select_ref.py, the plain-Python restatement of ma_select_records_batch, on the hand-made candidates of
tests/select_cases.py -- every rule of include/microasm.h against what the rule says --, against IsActiveRegion's own control
flow in every record order, and the call's ABI: the header declares and the library exports it, the two structs are laid out
as lancet2_amd/capi.py says.  Runs without a GPU."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import select_cases as cases
import select_ref as ref
from flatten_ref import parse_record
from lancet2_amd import capi

HEADER = os.path.join(capi.REPO, "include", "microasm.h")


def run(which, reverse=False):
    arrays, n, nr, ns, win_len, params, rows = cases.batch(which, reverse=reverse)
    return ref.select(arrays, n, nr, ns, win_len, **params), arrays, rows


@pytest.mark.parametrize("which", list(cases.BATCHES))
@pytest.mark.parametrize("reverse", [False, True])
def test_every_rule_by_hand(which, reverse):
    got, arrays, rows = run(which, reverse)
    for w, (label, records, _, (mask, value), keep) in enumerate(rows):
        assert int(got["win_state"][w]) & mask == value, (label, int(got["win_state"][w]))
        a, b = int(arrays["rec_win_off"][w]), int(arrays["rec_win_off"][w + 1])
        if keep is not None:
            assert got["rec_keep"][a:b].tolist() == (keep[::-1] if reverse else keep), label
        listed = bool(got["win_state"][w] & ref.MA_S_LISTED)
        want = [i for i in range(a, b) if got["rec_keep"][i] & ref.MA_SK_COLLECT] if listed else []
        assert got["sel_src"][int(got["sel_win_off"][w]):int(got["sel_win_off"][w + 1])].tolist() == want, label
    assert int(got["n_selected"][0]) == int(got["sel_win_off"][-1]) == len(got["sel_src"])
    assert got["sel_off"].tolist() == arrays["rec_off"][got["sel_src"]].tolist()
    assert got["sel_len"].tolist() == arrays["rec_len"][got["sel_src"]].tolist()
    assert got["sel_sample"].tolist() == arrays["rec_sample"][got["sel_src"]].tolist()


def test_states_are_what_the_bits_say():
    got, _, rows = run("rules")
    for w, row in enumerate(rows):
        st = int(got["win_state"][w])
        assert bool(st & ref.MA_S_LISTED) == (bool(st & ref.MA_S_ACTIVE) and not st & (ref.MA_S_HOST_BITS | ref.MA_S_LOW_COVERAGE)), row[0]
        assert not (st & ref.MA_S_EVENTS and st & ref.MA_S_ACTIVE)


def test_sums_are_of_the_collected_records():
    got, arrays, rows = run("rules")
    blob = arrays["blob"].tobytes()
    for w in range(len(rows)):
        for s in range(2):
            mine = [i for i in range(int(arrays["rec_win_off"][w]), int(arrays["rec_win_off"][w + 1]))
                    if arrays["rec_sample"][i] == s and got["rec_keep"][i] & ref.MA_SK_COLLECT]
            assert int(got["win_sample_reads"][2 * w + s]) == len(mine)
            assert int(got["win_sample_bases"][2 * w + s]) == sum(parse_record(blob, int(arrays["rec_off"][i]), int(arrays["rec_len"][i]))["l_seq"] for i in mine)


def test_event_positions():
    """the positions themselves, not only whether two met"""
    def events(**kw):
        body, _ = cases.rec(**kw)
        return ref.record_events(parse_record(body, 0, len(body)), ref.find_md(body))
    M, I, D, S = ref.MISMATCH, ref.INSERTION, ref.DELETION, ref.SOFTCLIP
    assert events(tags=cases.md(b"3A2^CG1t0")) == ([(M, 103), (M, 105), (M, 105), (M, 106)], False)  # '^' itself: no base; 't' at 106
    assert events(cigar=[(2, "S"), (3, "M"), (1, "I"), (2, "D"), (1, "X"), (3, "="), (4, "N"), (1, "M"), (2, "S")]) == \
        ([(S, 100), (I, 103), (D, 105), (M, 106), (S, 114)], False)
    assert events(tags=cases.md(b"10A")) == ([], True) and events(tags=cases.md(b"9A")) == ([(M, 109)], False)
    assert events(tags=cases.md(b"3A6A")) == ([(M, 103), (M, 109)], False)  # (the number counts from the mismatch itself)
    assert events(tags=cases.md(b"3A7A")) == ([(M, 103)], True)


def test_event_positions_repeat_without_a_number():
    body, _ = cases.rec(tags=cases.md(b"3AC"))  # no number between two letters: the position stays
    assert ref.record_events(parse_record(body, 0, len(body)), ref.find_md(body)) == ([(ref.MISMATCH, 103), (ref.MISMATCH, 103)], False)


def test_set_definition_equals_the_early_returns_in_every_order():
    """IsActiveRegion returns at the first count that reaches two, MD before I/D/X before S within a record, record after
    record; MA_S_ACTIVE is 'some multiset of some sample holds a position twice'.  Both, for every order of every case's
    records and for the samples taken one after the other"""
    checked = 0
    for which in ("rules", "coverage"):
        got, arrays, rows = run(which)
        for w, (label, records, *_rest) in enumerate(rows):
            if len(records) > 5:
                continue
            by_sample = {}
            for body, s in records:
                if ref.record_bits(parse_record(body, 0, len(body))) & ref.MA_SK_ELIGIBLE:
                    ev, _ = ref.record_events(parse_record(body, 0, len(body)), ref.find_md(body))
                    # (CheckAlignment's order within a record: MD, then I / D / X, then S -- the MD events come first already)
                    by_sample.setdefault(s, []).append([e for e in ev if e[0] != ref.SOFTCLIP] + [e for e in ev if e[0] == ref.SOFTCLIP])
            for order in itertools.permutations(range(len(records))):
                lists = {s: list(v) for s, v in by_sample.items()}
                host = any(ref.host_answer([v[i] for i in _sub_order(order, len(v))]) for s, v in sorted(lists.items()))
                assert host == bool(got["win_state"][w] & ref.MA_S_ACTIVE), (label, order)
                checked += 1
    assert checked > 200


def _sub_order(order, n):
    return [i for i in order if i < n]


def test_event_table_capacity_is_a_property_of_the_kernel_not_of_the_answer():
    """more distinct keys than the table holds and no position twice: MA_S_EVENTS, not listed; at the capacity: inactive"""
    windows = [[cases.rec(cigar=[(1, "M"), (1, "I")] * 3 + [(4, "M")], pos=100 + 10 * i) for i in range(2)]]
    arrays, n, nr, ns = cases.lay_out(windows)
    for keys, want in ((6, 0), (5, ref.MA_S_EVENTS)):
        got = ref.select(arrays, n, nr, ns, np.array([10], np.uint32), max_sample_cov=1000.0, min_anchor_cov=0, event_keys=keys)
        assert int(got["win_state"][0]) == want and int(got["n_selected"][0]) == 0


def test_bad_records_are_named():
    good, _ = cases.rec(tags=cases.M3)
    arrays, n, nr, ns = cases.lay_out([[(good, 0), (good, 0), (good, 0)]])
    for what in ("core", "blob", "sample", "l_seq"):
        bad = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in arrays.items()}
        if what == "core":
            bad["rec_len"][1] = ref.core_bytes(good) - 1
        elif what == "blob":
            bad["rec_len"][1] = bad["blob"].size - int(bad["rec_off"][1]) + 1
        elif what == "sample":
            bad["rec_sample"][1] = 2
        else:
            at = int(bad["rec_off"][1]) + 16
            bad["blob"][at:at + 4] = 0
        with pytest.raises(ref.SelectError) as e:
            ref.select(bad, n, nr, ns, np.array([10], np.uint32))
        assert e.value.rc == ref.MA_ERR_ARG and e.value.record == 1
    arrays["rec_len"][1] = ref.core_bytes(good)  # the core alone is a good record: no tags, no MD
    assert int(ref.select(arrays, n, nr, ns, np.array([10], np.uint32), min_anchor_cov=0)["win_state"][0]) & ref.MA_S_ACTIVE
    arrays["rec_len"][2] = ref.core_bytes(good)
    assert not int(ref.select(arrays, n, nr, ns, np.array([10], np.uint32), min_anchor_cov=0)["win_state"][0]) & ref.MA_S_ACTIVE
    arrays["rec_win_off"][1] = 2
    with pytest.raises(ref.SelectError):
        ref.select(arrays, n, nr, ns, np.array([10], np.uint32))


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_call():
    text = open(HEADER).read()
    assert ("int ma_select_records_batch(ma_ctx_t* ctx, const ma_records_t* in, const ma_select_params_t* sp, "
            "const ma_select_out_t* out);") in text
    assert "typedef struct ma_select_params {" in text and "typedef struct ma_select_out {" in text
    assert f"#define MA_SELECT_EVENT_KEYS {capi.SELECT_EVENT_KEYS}" in text and capi.SELECT_EVENT_KEYS >= 8192 and capi.SELECT_EVENT_KEYS == ref.EVENT_KEYS
    for name in ("MA_SK_COLLECT", "MA_SK_ELIGIBLE", "MA_S_ACTIVE", "MA_S_LOW_COVERAGE", "MA_S_CAPPED", "MA_S_MD_RANGE", "MA_S_EVENTS", "MA_S_LISTED"):
        assert f"#define {name} {getattr(capi, name)}\n" in text and getattr(capi, name) == getattr(ref, name), name
    assert os.path.exists(capi.LIB_PATH), "libmicroasm.so is not built: run __graft_entry__.build()"
    lib = capi.load_cdll()
    assert hasattr(lib, "ma_select_records_batch")
    from lancet2_amd.engine import Engine
    assert callable(getattr(Engine, "select_records")) and callable(getattr(Engine, "select_records_device"))


@pytest.mark.parametrize("cname,cls", [("ma_select_params_t", capi.SelectParams), ("ma_select_out_t", capi.SelectOut)])
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
    spec = capi.select_out_spec(3, 7, 2)
    assert set(spec) == {f for f, _ in capi.SelectOut._fields_}
    assert spec["win_sample_bases"] == (np.uint64, 6) and spec["sel_win_off"] == (np.uint32, 4) and spec["sel_off"] == (np.uint64, 7)


# ---- the restatement against the host shell ---------------------------------------------------------------------------------
def test_restatement_equals_the_host_shell(tmp_path):
    """tests/host/select_units.cpp lists the candidates of 59 windows of the fixture BAMs (MD strings, indels, soft clips,
    mapq 7 reads) with ReadCollector::CollectCandidates and asks the shell itself: IsActiveRegion in both record orders,
    Filtered and CheckAlignment's filter per record, SelectKept's sums, whether a 12x cap bites, the coverage gate at two
    bounds.  The restatement must agree window for window and record for record"""
    from test_pipeline_host import build, sam_to_bam, write_fixture
    write_fixture(str(tmp_path))
    for name in ("normal", "tumor"):
        sam_to_bam(str(tmp_path / (name + ".sam")), str(tmp_path / (name + ".bam")))
    exe, _ = build(tmp_path, "tests/host/select_units.cpp", "select_units", ["-DLANCET2_AMD_WITH_ZLIB", "-lz"])
    out = tmp_path / "dump"
    out.mkdir()
    r = subprocess.run([exe, str(tmp_path / "ref.fa"), str(tmp_path / "normal.bam"), str(tmp_path / "tumor.bam"), str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "select units ok" in r.stdout, r.stdout + r.stderr
    rec = {k: np.fromfile(out / f"{k}.{ext}", dtype=dt) for k, ext, dt in (("blob", "u8", np.uint8), ("rec_off", "u64", np.uint64),
           ("rec_len", "u32", np.uint32), ("rec_win_off", "u32", np.uint32), ("rec_sample", "u8", np.uint8))}
    win_len, keep = np.fromfile(out / "win_len.u32", dtype=np.uint32), np.fromfile(out / "keep.u8", dtype=np.uint8)
    host = np.array([[int(x) for x in line.split()] for line in open(out / "windows.txt")])
    n, nr = len(win_len), len(rec["rec_off"])
    assert n == 59 == len(host) and nr > 3000 and (win_len == 200).all()
    assert (host[:, 0] == host[:, 1]).all() and 0 < host[:, 0].sum() < n  # both record orders; active and inactive windows
    wide = ref.select(rec, n, nr, 2, win_len, max_sample_cov=1000.0, min_anchor_cov=30)
    assert wide["rec_keep"].tolist() == keep.tolist() and len(set(keep.tolist())) >= 2
    assert ((wide["win_state"] & ref.MA_S_ACTIVE) != 0).astype(int).tolist() == host[:, 0].tolist()
    assert wide["win_sample_reads"].tolist() == host[:, [2, 4]].reshape(-1).tolist()
    assert wide["win_sample_bases"].tolist() == host[:, [3, 5]].reshape(-1).tolist()
    assert not (wide["win_state"] & ref.MA_S_HOST_BITS).any()
    assert ((wide["win_state"] & ref.MA_S_LOW_COVERAGE) != 0).astype(int).tolist() == host[:, 7].tolist()
    at60 = ref.select(rec, n, nr, 2, win_len, max_sample_cov=1000.0, min_anchor_cov=60)
    assert ((at60["win_state"] & ref.MA_S_LOW_COVERAGE) != 0).astype(int).tolist() == host[:, 8].tolist()
    assert 0 < host[:, 7].sum() + host[:, 8].sum() < 2 * n
    tight = ref.select(rec, n, nr, 2, win_len, max_sample_cov=12.0, min_anchor_cov=0)
    assert ((tight["win_state"] & ref.MA_S_CAPPED) != 0).astype(int).tolist() == host[:, 6].tolist() and 0 < host[:, 6].sum()
    # the listed records of an uncapped, active, covered window are what SelectKept keeps: the unfiltered ones, in arrival order
    for w in np.flatnonzero(wide["win_state"] & ref.MA_S_LISTED):
        a, b = int(rec["rec_win_off"][w]), int(rec["rec_win_off"][w + 1])
        assert wide["sel_src"][int(wide["sel_win_off"][w]):int(wide["sel_win_off"][w + 1])].tolist() == [i for i in range(a, b) if keep[i] & 1]
