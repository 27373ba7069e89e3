"""The read-level FORMAT statistics of ma_genotype_stats_batch / ma_process_stats_batch (k_assign<true> + k_evid_stats)
against tests/format_stats_ref.py computed from the ORACLE's run of the same batch (tests/format_stats_cases.py; the reference
itself is pinned by tests/test_format_stats_ref.py).  ev_sums exact, NaN positions identical, f64 within 1e-9 max(1, |want|)
-- the engine sums over quality bins where the reference sums over reads, DESIGN.md section 2."""
import ctypes as C

import numpy as np
import pytest

from lancet2_amd import capi

import format_stats_cases as cases

pytestmark = pytest.mark.gpu

FIELDS = ("ev_sums", "fmt_npbq", "fmt_cmlod", "fmt_stat")
# what the genotype stage launches without the statistics (ma_last_kernel_times names)
GENOTYPE_KERNELS = {"k_read_planes", "k_plan", "k_vote", "k_dp_scatter", "k_align_reg", "k_align_tb", "k_align_wave",
                    "k_align_gen", "k_tap_records", "k_assign", "k_evidence", "k_qual"}


def _engine(params, **kw):
    from lancet2_amd.engine import Engine
    return Engine(params, **kw)


@pytest.mark.parametrize("name", cases.GENOTYPE_CASES)
def test_genotype_stats_match_the_reference(name):
    params, arrs, n, nr, asm, var, want = cases.genotype_case(name)
    eng = _engine(params)
    try:
        geno, fmt = eng.genotype_stats(arrs, n, nr, asm, var)
        names = {k for k, _ in eng.kernel_times()}
    finally:
        eng.close()
    assert np.array_equal(geno["allele_counts"], want["allele_counts"])
    assert "k_evid_stats" in names
    bad = cases.compare_fmt(fmt, want, name)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("field", FIELDS)
def test_each_array_asked_for_alone(field):
    params, arrs, n, nr, asm, var, want = cases.genotype_case("c2_dense_variants")
    eng = _engine(params)
    try:
        _, fmt = eng.genotype_stats(arrs, n, nr, asm, var, fields=(field,))
    finally:
        eng.close()
    assert set(fmt) == {field}
    bad = cases.compare_fmt(fmt, want, field)
    assert not bad, "\n".join(bad)


def test_without_statistics_the_stage_is_what_it_was():
    """fmt NULL, or all four members NULL: the kernels the stage launched before, and every output of the call with the
    statistics on is bit-identical to the call without them"""
    params, arrs, n, nr, asm, var, want = cases.genotype_case("c2_dense_variants")
    eng = _engine(params)
    try:
        plain = eng.genotype(arrs, n, nr, asm, var, debug=True)
        plain_names = {k for k, _ in eng.kernel_times()}
        with_stats, _ = eng.genotype_stats(arrs, n, nr, asm, var, debug=True)
        stats_names = {k for k, _ in eng.kernel_times()}
        empty, fmt = eng.genotype_stats(arrs, n, nr, asm, var, debug=True, fields=())
        empty_names = {k for k, _ in eng.kernel_times()}
        # ... and a null pointer for the struct itself
        out = capi.alloc_host(capi.geno_out_spec(params, n, nr, True))
        b = capi.make_batch_struct(arrs, n, nr)
        rc = eng.lib.ma_genotype_stats_batch(eng.h, C.byref(b), C.byref(capi.fill_struct(capi.AsmOut, asm)),
                                             C.byref(capi.fill_struct(capi.VarOut, var)),
                                             C.byref(capi.fill_struct(capi.GenoOut, out)), None)
        assert rc == 0
        null_names = {k for k, _ in eng.kernel_times()}
    finally:
        eng.close()
    assert fmt == {}
    assert plain_names <= GENOTYPE_KERNELS and {"k_assign", "k_evidence", "k_qual"} <= plain_names
    assert empty_names == plain_names and null_names == plain_names
    assert stats_names == plain_names | {"k_evid_stats"}
    for other in (with_stats, empty, out):
        for key, val in plain.items():
            assert np.array_equal(val.view(np.uint8), other[key].view(np.uint8)), key


def _process_want():
    params, arrs, n, nr, want = cases.process_case()
    assert n == cases.PROCESS_WINDOWS
    return params, arrs, n, nr, want


@pytest.mark.parametrize("streams", [2, 1])
def test_process_stats_on_the_device_route(streams):
    """MA_MEM_DEVICE: the caller's device arrays, sliced per lane"""
    from harness import DeviceArena
    params, arrs, n, nr, want = _process_want()
    specs = [capi.gate_out_spec(n), capi.asm_out_spec(params, n), capi.var_out_spec(params, n),
             capi.geno_out_spec(params, n, nr, debug=False), capi.fmt_out_spec(params, n)]
    eng = _engine(params, memspace=capi.MA_MEM_DEVICE)
    arena = DeviceArena()
    try:
        b = capi.make_batch_struct({k: arena.upload(v) for k, v in arrs.items()}, n, nr)
        ptrs = [{k: arena.alloc(int(sz) * np.dtype(dt).itemsize) for k, (dt, sz) in spec.items()} for spec in specs]
        eng.set_streams(streams)
        eng.process_stats_device(b, capi.fill_struct(capi.GateOut, ptrs[0]), capi.fill_struct(capi.AsmOut, ptrs[1]),
                                 capi.fill_struct(capi.VarOut, ptrs[2]), capi.fill_struct(capi.GenoOut, ptrs[3]),
                                 capi.fill_struct(capi.FmtOut, ptrs[4]))
        eng.synchronize()
        counts = arena.download(ptrs[3]["allele_counts"], *specs[3]["allele_counts"])
        fmt = {k: arena.download(ptrs[4][k], dt, sz) for k, (dt, sz) in specs[4].items()}
    finally:
        eng.close()
        arena.close()
    assert np.array_equal(counts, want["allele_counts"])
    bad = cases.compare_fmt(fmt, want, f"device route, {streams} lanes")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("streams", [2, 1])
def test_process_stats_on_the_host_route(streams):
    """MA_MEM_HOST: packed records; plain, after ma_prefetch_batch (queued ahead with the statistics), and a batch queued
    ahead WITHOUT them that the call then asks them for (dropped and computed again)"""
    params, arrs, n, nr, want = _process_want()
    eng = _engine(params)
    try:
        eng.set_streams(streams)
        b = capi.make_batch_struct(arrs, n, nr)
        *_, q0, f0 = eng.process_stats(arrs, n, nr)
        eng.prefetch(b)  # (the last call asked for the statistics: so does the job queued here)
        outs = [capi.alloc_host(s) for s in (capi.gate_out_spec(n), capi.asm_out_spec(params, n), capi.var_out_spec(params, n),
                                             capi.geno_out_spec(params, n, nr, False), capi.fmt_out_spec(params, n))]
        outs[4]["fmt_stat"][:] = 7.0  # whatever the caller's array held: unused slots must come back NaN
        structs = [capi.fill_struct(cls, o) for cls, o in zip((capi.GateOut, capi.AsmOut, capi.VarOut, capi.GenoOut, capi.FmtOut), outs)]
        eng.process_stats_device(b, *structs)
        eng.process_device(b, *structs[:4])
        eng.prefetch(b)  # queued without the statistics ...
        outs2 = capi.alloc_host(capi.fmt_out_spec(params, n))
        eng.process_stats_device(b, *structs[:4], capi.fill_struct(capi.FmtOut, outs2))  # ... that this call wants
    finally:
        eng.close()
    for what, counts, fmt in (("plain", q0["allele_counts"], f0), ("prefetched", outs[3]["allele_counts"], outs[4]),
                              ("recomputed", outs[3]["allele_counts"], outs2)):
        assert np.array_equal(counts, want["allele_counts"]), what
        bad = cases.compare_fmt(fmt, want, f"host route, {streams} lanes, {what}")
        assert not bad, "\n".join(bad)


def test_vcf_carries_the_statistics(tmp_path):
    """pipeline_driver --out-vcf on the small genome of tests/test_pipeline_host.py: NPBQ, CMLOD, BQCD, ASMD, AHDD, HSE and
    PDCV are printed, and missing exactly where the AD column of the same line says they must be"""
    import subprocess
    import test_pipeline_host as host
    exe = host.driver(tmp_path)
    host.write_fixture(str(tmp_path))
    vcf = tmp_path / "calls.vcf"
    r = subprocess.run([exe, "--reference", str(tmp_path / "ref.fa"), "--normal", str(tmp_path / "normal.sam"),
                        "--tumor", str(tmp_path / "tumor.sam"), "--region", "chr1:1-6000", "--min-kmer", "25", "--max-kmer", "25",
                        "--batch-windows", "3", "--out-vcf", str(vcf)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    body = [x.split("\t") for x in open(vcf).read().splitlines() if not x.startswith("#")]
    assert len(body) >= 6
    seen = dict(samples=0, bqcd=0, hse=0, missing_bqcd=0, missing_hse=0, pdcv=0)
    for f in body:
        key = f[8].split(":")
        for col in f[9:]:
            vals = dict(zip(key, col.split(":")))
            if vals["GT"] == "./.":
                continue
            seen["samples"] += 1
            ad = [int(x) for x in vals["AD"].split(",")]
            npbq = vals["NPBQ"].split(",")
            assert len(npbq) == len(ad), (vals["NPBQ"], ad)
            for x, d in zip(npbq, ad):
                assert (float(x) > 0.0) if d > 0 else (float(x) == 0.0), (vals["NPBQ"], ad)
            cmlod = vals["CMLOD"].split(",")
            assert len(cmlod) == len(ad) - 1 and all(float(x) >= 0.0 for x in cmlod)
            both = ad[0] > 0 and sum(ad[1:]) > 0
            for name in ("BQCD", "ASMD", "AHDD"):
                assert (vals[name] != ".") == both, (name, vals[name], ad)
                if both:
                    float(vals[name])
            assert (vals["HSE"] != ".") == (sum(ad[1:]) >= 3), (vals["HSE"], ad)
            if vals["HSE"] != ".":
                assert 0.0 <= float(vals["HSE"]) <= 1.0
            if vals["PDCV"] != ".":
                assert float(vals["PDCV"]) >= 0.0
                seen["pdcv"] += 1
            for name in ("RMQ", "SCA", "FLD", "RPCD", "MQCD", "FSSE"):  # still a host's work
                assert vals[name] == "."
            seen["bqcd"] += both
            seen["missing_bqcd"] += not both
            seen["hse"] += vals["HSE"] != "."
            seen["missing_hse"] += vals["HSE"] == "."
    assert seen["samples"] >= 8 and seen["bqcd"] >= 3 and seen["missing_bqcd"] >= 1 and seen["hse"] >= 3, seen
