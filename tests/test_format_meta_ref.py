"""CPU guards of the read-metadata FORMAT statistics: tests/format_meta_ref.py against closed forms and scipy, the fact about
mirror positions that decides how RPCD must be ranked, the case set of tests/meta_stats_cases.py (it cannot pass vacuously) and
the two new boundary structs against a C compiler."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from lancet2_amd import capi

import format_meta_ref as mref
import format_stats_ref as ref
import meta_stats_cases as cases


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_refpos_to_qpos_closed_forms():
    M, I, D, S = 0, 1, 2, 4
    assert mref.refpos_to_qpos([(M, 10)], 0) == 0 and mref.refpos_to_qpos([(M, 10)], 5) == 5
    assert mref.refpos_to_qpos([(M, 3), (I, 2), (M, 3)], 3) == 5      # an insertion shifts the query
    for pos in (3, 4):
        assert mref.refpos_to_qpos([(M, 3), (D, 2), (M, 3)], pos) == 3  # inside a deletion: the query position at its start
    assert mref.refpos_to_qpos([(M, 3), (D, 2), (M, 3)], 5) == 3
    assert mref.refpos_to_qpos([(S, 2), (M, 4)], 0) == 2              # a soft clip advances the query only
    assert mref.refpos_to_qpos([(M, 4)], 10) == 4                     # beyond the CIGAR: the end of the query
    assert mref.refpos_to_qpos([(S, 3), (M, 4), (S, 5)], 9) == 12
    assert mref.folded(0, 150) == 0.0 and mref.folded(150, 150) == 0.0 and mref.folded(75, 150) == 0.5
    assert mref.folded(7, 0) == 0.5


def test_refpos_to_qpos_is_the_oracles():
    from harness import oracle
    rng = np.random.default_rng(5)
    for _ in range(200):
        cig = [(int(rng.choice([0, 0, 1, 2, 4])), int(rng.integers(1, 9))) for _ in range(int(rng.integers(1, 7)))]
        ops = "".join("MID S"[op] for op, _ in cig).encode()
        lens = np.array([ln for _, ln in cig], np.uint32)
        for pos in range(0, 40, 3):
            want = oracle().orc_refpos_to_qpos(ops, lens.ctypes.data_as(C.c_void_p), len(lens), C.c_uint64(pos))
            assert mref.refpos_to_qpos(cig, pos) == want, (cig, pos)


def test_rank_tallies_and_effect_size_are_scipys():
    from scipy import stats
    rng = np.random.default_rng(11)
    for trial in range(60):
        n_ref, n_alt = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        vals = rng.integers(0, 12, n_ref + n_alt) / float(rng.choice([7, 100, 150]))
        a, b = list(vals[:n_ref]), list(vals[n_ref:])
        rank2, tie = mref.rank_tallies(a, b)
        ranks = stats.rankdata(a + b)  # mid-ranks
        assert rank2 == int(round(2 * ranks[n_ref:].sum()))
        _, counts = np.unique(vals, return_counts=True)
        assert tie == int((counts ** 3 - counts).sum())
        u_alt = stats.mannwhitneyu(b, a, alternative="two-sided").statistic
        assert rank2 / 2.0 - n_alt * (n_alt + 1) / 2.0 == u_alt
        got = ref.mann_whitney_effect_size(a, b)
        n = n_ref + n_alt
        var_u = n_ref * n_alt / 12.0 * ((n + 1) - tie / (n * (n - 1.0)))
        want = 0.0 if var_u <= 0 else (u_alt - n_ref * n_alt / 2.0) / math.sqrt(var_u) / math.sqrt(n)
        assert got == pytest.approx(want, rel=1e-12, abs=1e-15)
    assert ref.mann_whitney_effect_size([], [1.0]) is None and ref.mann_whitney_effect_size([0.5, 0.5], [0.5]) == 0.0


def test_closed_forms_of_the_tallied_statistics():
    assert mref.rms([]) == 0.0 and mref.rms([60, 60]) == 60.0 and mref.rms([3, 4]) == math.sqrt(12.5)
    assert mref.soft_clip_asymmetry(1, 4, 3, 4) == 0.5 and mref.soft_clip_asymmetry(0, 0, 2, 4) == 0.5
    assert mref.soft_clip_asymmetry(2, 4, 0, 0) == -0.5
    assert ref.mean_alt_minus_ref([100, -300], [250]) == 350.0 and ref.mean_alt_minus_ref([], [1]) is None
    assert mref.start_entropy([1, 2]) is None
    assert mref.start_entropy([300, 301, 302]) == 0.0                       # one bin
    assert mref.start_entropy([0, 3, 6]) == pytest.approx(1.0)              # three bins of three reads: log2 3 / log2 3
    assert mref.start_entropy(list(range(0, 90, 3))) == pytest.approx(math.log2(30) / math.log2(20))  # capped at 20 bins
    assert mref.start_entropy([0, 0, 3, 3]) == pytest.approx(1.0 / 2.0)


def test_mirror_positions_are_not_ties_as_doubles():
    """1 - fl(100/150) is not fl(50/150): the reference ranks the doubles, so must the engine"""
    pairs = unequal = 0
    for length in (100, 101, 150, 151, 250):
        for q in range(length + 1):
            pairs += 1
            unequal += (1.0 - float(length - q) / float(length)) != float(q) / float(length)
    assert (pairs, unequal) == (757, 305)
    assert mref.folded(50, 150) != mref.folded(100, 150)
    assert mref.folded(75, 150) == mref.folded(50, 100) and mref.folded(45, 150) == mref.folded(30, 100)


# ---- the case set ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def all_cells():
    return {(name, key): cell for name in cases.NAMES for key, cell in cases.reference(name)["cells"].items()}


def test_the_case_set_cannot_pass_vacuously(all_cells):
    finite = {k: 0 for k in mref.MSTAT}
    missing = {k: 0 for k in mref.MSTAT}
    for cell in all_cells.values():
        for key, x in zip(mref.MSTAT, cell["stats"]):
            finite[key] += x is not None
            missing[key] += x is None
    print(finite, missing)
    for key in ("FLD", "RPCD", "MQCD", "FSSE"):
        assert finite[key] >= 10 and missing[key] >= 2, (key, finite[key], missing[key])
    assert missing["SCA"] == 0  # finite in every cell with evidence
    assert any(c["cross_length_tie"] for c in all_cells.values())
    assert any(c["untied_mirror"] for c in all_cells.values())
    kinds = 0
    for c in all_cells.values():
        kinds |= c["kinds"]
    assert kinds == 7  # a variant before the alignment start, one inside a deletion, a soft-clipped winning alignment
    pair_kinds = set().union(*(c["pair_kinds"] for c in all_cells.values()))
    assert {(True, -1), (True, 0), (False, 1), (False, -1), (True, 1)} <= pair_kinds
    assert any(c["n_alt"] == 0 and c["n_ref"] > 0 for c in all_cells.values())
    assert any(c["n_ref"] == 0 and c["n_alt"] > 0 for c in all_cells.values())
    assert any(c["n_alt"] == 2 for c in all_cells.values()) and any(c["n_alt"] == 3 for c in all_cells.values())
    assert any(c["n_alt"] >= 3 and c["stats"][4] == 0.0 for c in all_cells.values())  # all ALT starts in one bin
    assert any(c["bins"] > 20 for c in all_cells.values())
    assert any(c["stats"][3] == 0.0 and c["n_ref"] > 0 and c["n_alt"] > 0 for c in all_cells.values())  # all MAPQ equal
    assert {cases.case(n).params.num_samples for n in cases.NAMES} >= {1, 8}
    assert any(c["k"] == 5 for c in all_cells.values())
    keys = sorted(c["keys"] for (name, _), c in all_cells.items() if name == "sort_fit")
    assert keys == [cases.SORT_CAP, cases.SORT_CAP + 1]  # exact fit of the LDS sort, and one key more


def test_duplicates_do_not_count():
    """dedup: mates share a name and carry different metadata; the tallies are those of the first reads"""
    c, want = cases.case("dedup"), cases.reference("dedup")
    removed = sum(x["removed"] for x in sc_reference("dedup")["cells"].values())
    assert removed >= 6
    total = sum(int(x) for x in want["ev_meta"].reshape(-1, 4)[:, 0])
    every = sum(int(q) ** 2 for q, s in zip(c.meta["read_mapq"], c.arrs["read_sample"]) if s < c.params.num_samples)
    assert 0 < total < every


def sc_reference(name):
    import scoring_cases as sc
    return sc.stats_reference(name)


# ---- the boundary ------------------------------------------------------------------------------------------------------
def test_new_structs_match_the_compiled_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    header = os.path.join(capi.REPO, "include", "microasm.h")
    structs = {"ma_read_meta_t": capi.ReadMeta, "ma_fmt_meta_out_t": capi.FmtMetaOut}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "microasm.h"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  printf("MA_RM_SOFTCLIP %d\\n", (int)MA_RM_SOFTCLIP);', '  printf("MA_RM_PROPER %d\\n", (int)MA_RM_PROPER);',
              '  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.dirname(header), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert int(got["MA_RM_SOFTCLIP"]) == capi.MA_RM_SOFTCLIP and int(got["MA_RM_PROPER"]) == capi.MA_RM_PROPER
    spec = capi.fmt_meta_out_spec(capi.default_params(), 3)
    assert [k for k, _ in capi.FmtMetaOut._fields_] == list(spec) and set(capi.META_DTYPES) == {k for k, _ in capi.ReadMeta._fields_}


def test_library_exports_the_meta_calls():
    lib = capi.load_cdll()
    for name in ("ma_genotype_meta_batch", "ma_process_meta_batch", "ma_prefetch_meta_batch"):
        assert hasattr(lib, name), name


# ---- the host shell ----------------------------------------------------------------------------------------------------
def rewrite_sam_metadata(path, seed):
    """the SAM fixture of tests/test_pipeline_host.py with the fields the read metadata comes from made interesting: signed and
    zero TLEN, flag 0x2 dropped from some records, MAPQ spread over 20 ... 60, and soft clips on one or both ends of clean
    150M records -- 8 clipped bases of 150 (5.3 %: not soft-clipped), 9 (exactly 6 %: soft-clipped) and more.  Returns what
    the TEXT says per (pos0, sequence): (mapq, MA_RM_* bits, tlen, clipped bases)."""
    rng = np.random.default_rng(seed)
    clips = [(0, 0), (8, 0), (0, 8), (4, 4), (9, 0), (0, 9), (5, 4), (12, 0), (3, 20)]
    head, body = [], []
    for line in open(path):
        if line.startswith("@"):
            head.append(line)
            continue
        f = line.rstrip("\n").split("\t")
        flag, pos1, mapq = int(f[1]), int(f[3]), int(f[4])
        if mapq >= 20:
            mapq = int(rng.integers(20, 61))
        if rng.random() < 0.3:
            flag &= ~0x2
        tlen = int(rng.choice([-455, -170, 0, 0, 171, 388, 902]))
        if f[5] == "150M" and f[11] == "MD:Z:150":
            lead, trail = clips[int(rng.integers(0, len(clips)))]
            if lead or trail:
                f[5] = (f"{lead}S" if lead else "") + f"{150 - lead - trail}M" + (f"{trail}S" if trail else "")
                f[11] = f"MD:Z:{150 - lead - trail}"
                pos1 += lead
        f[1], f[3], f[4], f[8] = str(flag), str(pos1), str(mapq), str(tlen)
        body.append((pos1, "\t".join(f) + "\n"))
    body.sort(key=lambda x: x[0])
    with open(path, "w") as out:
        out.writelines(head + [x[1] for x in body])
    want = {}
    for _, line in body:  # ... and read back from the text alone
        f = line.rstrip("\n").split("\t")
        clipped = sum(int(n) for n, op in __import__("re").findall(r"(\d+)([MIDNSHP=X])", f[5]) if op == "S")
        bits = (mref.MA_RM_SOFTCLIP if clipped / len(f[9]) >= 0.06 else 0) | (mref.MA_RM_PROPER if int(f[1]) & 0x2 else 0)
        want.setdefault((int(f[3]) - 1, f[9]), set()).add((int(f[4]), bits, int(f[8]), clipped))
    return want


def test_the_dumps_read_metadata_is_what_the_sam_text_says(tmp_path):
    """pipeline_driver --extract-only --dump (no device needed): FlatBatch's read_mapq / read_mflags / read_isize / read_start
    of every collected read are MAPQ, (all S operations / sequence length >= 0.06) | flag 0x2, TLEN and POS - 1 of its record"""
    import test_pipeline_host as host
    exe = host.driver(tmp_path)
    host.write_fixture(str(tmp_path))
    want = {}
    for i, name in enumerate(("normal", "tumor")):
        for key, vals in rewrite_sam_metadata(str(tmp_path / (name + ".sam")), 50 + i).items():
            want.setdefault(key, set()).update(vals)
    # (pos, sequence) names a record -- but for error-free reads of one haplotype that happen to start on the same base
    assert sum(len(v) == 1 for v in want.values()) >= 0.9 * len(want)
    dump = tmp_path / "dump"
    dump.mkdir()
    r = subprocess.run([exe, "--reference", str(tmp_path / "ref.fa"), "--normal", str(tmp_path / "normal.sam"),
                        "--tumor", str(tmp_path / "tumor.sam"), "--region", "chr1:1-6000", "--batch-windows", "4",
                        "--dump", str(dump), "--extract-only"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    seen = {"reads": 0, "clipped": 0, "below": 0, "proper": 0, "improper": 0, "neg": 0, "zero": 0, "pos": 0}
    for b in sorted(os.listdir(dump)):
        load = lambda f, dt: np.fromfile(str(dump / b / f), dtype=dt)  # noqa: E731
        off, bases = load("read_off.u64", np.uint64), load("read_bases.u8", np.uint8)
        meta = {k: load(f"{k}.{'u8' if dt == np.uint8 else 'i32'}", dt) for k, dt in capi.META_DTYPES.items()}
        nr = len(off) - 1
        assert nr > 0 and all(len(v) == nr for v in meta.values())
        for i in range(nr):
            seq = bytes(bases[int(off[i]):int(off[i + 1])]).decode()
            got = (int(meta["read_mapq"][i]), int(meta["read_mflags"][i]), int(meta["read_isize"][i]))
            key = (int(meta["read_start"][i]), seq)
            assert key in want and got in {v[:3] for v in want[key]}, (b, i, key[0], got, want.get(key))
            seen["reads"] += 1
            if len(want[key]) == 1:  # the boundary of the 6 % rule: 8 of 150 clipped bases are below it, 9 of 150 are on it
                clipped = next(iter(want[key]))[3]
                seen["below"] += clipped == 8 and not got[1] & mref.MA_RM_SOFTCLIP
                seen["on"] = seen.get("on", 0) + (clipped == 9 and bool(got[1] & mref.MA_RM_SOFTCLIP))
            seen["clipped"] += bool(got[1] & mref.MA_RM_SOFTCLIP)
            seen["proper" if got[1] & mref.MA_RM_PROPER else "improper"] += 1
            seen["neg" if got[2] < 0 else "zero" if got[2] == 0 else "pos"] += 1
    print(seen)
    assert seen["reads"] >= 1000, seen
    assert min(seen[k] for k in ("clipped", "proper", "improper", "neg", "zero", "pos", "below", "on")) >= 20, seen
    assert 8 / 150 < 0.06 <= 9 / 150
