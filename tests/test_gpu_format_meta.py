"""RMQ, MQCD, SCA, FLD, RPCD and FSSE of ma_genotype_meta_batch / ma_process_meta_batch (k_assign<true> + k_evid_stats<true>)
against tests/format_meta_ref.py computed from the ORACLE's run of the same batch (tests/meta_stats_cases.py; the reference
itself is pinned by tests/test_format_meta_ref.py).  Integer tallies exact, NaN positions identical, f64 within 1e-9
max(1, |want|), as for the seven statistics of ma_fmt_out_t."""
import ctypes as C
import functools

import numpy as np
import pytest

from lancet2_amd import capi, synth

import format_meta_ref as mref
import meta_stats_cases as cases

pytestmark = pytest.mark.gpu

OUT_CLASSES = (capi.GateOut, capi.AsmOut, capi.VarOut, capi.GenoOut, capi.FmtOut, capi.FmtMetaOut)


def _engine(params, **kw):
    from lancet2_amd.engine import Engine
    return Engine(params, **kw)


@pytest.mark.parametrize("name", cases.NAMES)
def test_genotype_meta_matches_the_reference(name):
    c, want = cases.case(name), cases.reference(name)
    eng = _engine(c.params)
    try:
        geno0, fmt0 = eng.genotype_stats(c.arrs, c.n, c.nr, c.asm, c.var)
        geno, fmt, fmeta = eng.genotype_meta(c.arrs, c.meta, c.n, c.nr, c.asm, c.var)
        names = {k for k, _ in eng.kernel_times()}
    finally:
        eng.close()
    assert "k_evid_stats" in names
    assert np.array_equal(geno["allele_counts"], want["allele_counts"])
    bad = cases.compare_meta(fmeta, want, name)
    assert not bad, "\n".join(bad)
    # ma_fmt_out_t's arrays and the genotype outputs are those of ma_genotype_stats_batch, bit for bit
    for key, val in fmt0.items():
        assert np.array_equal(val.view(np.uint8), fmt[key].view(np.uint8)), key
    for key, val in geno0.items():
        assert np.array_equal(val.view(np.uint8), geno[key].view(np.uint8)), key


@pytest.mark.parametrize("field", list(capi.fmt_meta_out_spec(capi.default_params(), 1)))
def test_each_array_asked_for_alone(field):
    c, want = cases.case("positions"), cases.reference("positions")
    eng = _engine(c.params)
    try:
        _, fmt, fmeta = eng.genotype_meta(c.arrs, c.meta, c.n, c.nr, c.asm, c.var, fields=(), meta_fields=(field,))
    finally:
        eng.close()
    assert fmt == {} and set(fmeta) == {field}
    bad = cases.compare_meta(fmeta, want, field)
    assert not bad, "\n".join(bad)


# ---- the whole chain ---------------------------------------------------------------------------------------------------
PROCESS_WINDOWS = 6


@functools.lru_cache(maxsize=None)
def _process_case():
    """a synthetic batch with seeded metadata -> (params, arrs, meta, n, nr, want): the oracle's chain feeding the reference"""
    from harness import OracleEngine
    params = capi.default_params(min_k=25, max_k=25)
    arrs, n, nr = synth.make_config_batch("C1", PROCESS_WINDOWS, first_index=900)
    meta = cases.random_meta(4242, nr)
    orc = OracleEngine(params)
    asm = orc.assemble(arrs, n, nr)
    var = orc.msa(arrs, n, nr, asm)
    taps = orc.genotype(arrs, n, nr, asm, var)
    want = mref.meta_stats(params, arrs, n, asm, var, taps["aln_rec"], taps["aln_cigar"], meta)
    assert np.array_equal(want["allele_counts"], taps["allele_counts"])
    assert sum(1 for c in want["cells"].values() if c["n_ref"] and c["n_alt"]) >= 4
    return params, arrs, meta, n, nr, want, asm, var


def _check(what, counts, fmeta, want):
    assert np.array_equal(counts, want["allele_counts"]), what
    bad = cases.compare_meta(fmeta, want, what)
    assert not bad, "\n".join(bad)


def _host_outs(params, n, nr):
    outs = [capi.alloc_host(s) for s in (capi.gate_out_spec(n), capi.asm_out_spec(params, n), capi.var_out_spec(params, n),
                                         capi.geno_out_spec(params, n, nr, False), capi.fmt_out_spec(params, n),
                                         capi.fmt_meta_out_spec(params, n))]
    outs[5]["fmt_mstat"][:] = 7.0  # whatever the caller's arrays held: unused slots must come back NaN / zero
    outs[5]["ev_meta"][:] = -3
    return outs, [capi.fill_struct(cls, o) for cls, o in zip(OUT_CLASSES, outs)]


@pytest.mark.parametrize("streams", [2, 1])
def test_process_meta_on_the_host_route(streams):
    """MA_MEM_HOST: ASCII and packed; then after ma_prefetch_meta_batch (queued ahead with the statistics), and a batch queued
    by plain ma_prefetch_batch -- without the metadata -- that the call then brings with them (dropped and computed again)"""
    params, arrs, meta, n, nr, want, _, _ = _process_case()
    packed, twin = capi.pack_reads(arrs)
    assert all(np.array_equal(twin[k], arrs[k]) for k in ("read_bases", "read_quals"))  # (ACGT only: the same batch)
    eng = _engine(params)
    try:
        eng.set_streams(streams)
        *_, q0, _, m0 = eng.process_meta(arrs, meta, n, nr)
        *_, q1, _, m1 = eng.process_meta(arrs, meta, n, nr, packed=packed)
        b = capi.make_batch_struct(arrs, n, nr)
        ms = capi.fill_struct(capi.ReadMeta, meta)
        eng.prefetch_meta(b, None, ms)  # (the last call asked for the statistics: so does the job queued here)
        outs2, structs2 = _host_outs(params, n, nr)
        eng.process_meta_device(b, None, ms, *structs2)
        eng.prefetch(b)  # queued without the metadata ...
        outs3, structs3 = _host_outs(params, n, nr)
        eng.process_meta_device(b, None, ms, *structs3)  # ... that this call brings
    finally:
        eng.close()
    _check(f"host route, {streams} lanes, ascii", q0["allele_counts"], m0, want)
    _check(f"host route, {streams} lanes, packed", q1["allele_counts"], m1, want)
    _check(f"host route, {streams} lanes, prefetched", outs2[3]["allele_counts"], outs2[5], want)
    _check(f"host route, {streams} lanes, recomputed", outs3[3]["allele_counts"], outs3[5], want)


@pytest.mark.parametrize("streams", [2, 1])
def test_process_meta_on_the_device_route(streams):
    """MA_MEM_DEVICE: the caller's device arrays, the four metadata arrays among them, sliced per lane"""
    from harness import DeviceArena
    params, arrs, meta, n, nr, want, _, _ = _process_case()
    specs = [capi.gate_out_spec(n), capi.asm_out_spec(params, n), capi.var_out_spec(params, n),
             capi.geno_out_spec(params, n, nr, debug=False), capi.fmt_out_spec(params, n), capi.fmt_meta_out_spec(params, n)]
    eng = _engine(params, memspace=capi.MA_MEM_DEVICE)
    arena = DeviceArena()
    try:
        b = capi.make_batch_struct({k: arena.upload(v) for k, v in arrs.items()}, n, nr)
        ms = capi.fill_struct(capi.ReadMeta, {k: arena.upload(v) for k, v in meta.items()})
        ptrs = [{k: arena.alloc(int(sz) * np.dtype(dt).itemsize) for k, (dt, sz) in spec.items()} for spec in specs]
        eng.set_streams(streams)
        eng.process_meta_device(b, None, ms, *[capi.fill_struct(cls, p) for cls, p in zip(OUT_CLASSES, ptrs)])
        eng.synchronize()
        counts = arena.download(ptrs[3]["allele_counts"], *specs[3]["allele_counts"])
        fmeta = {k: arena.download(ptrs[5][k], dt, sz) for k, (dt, sz) in specs[5].items()}
    finally:
        eng.close()
        arena.close()
    _check(f"device route, {streams} lanes", counts, fmeta, want)


def test_process_meta_is_genotype_meta():
    """the chain's statistics are those of the genotype stage alone over the chain's own assembly and variants"""
    params, arrs, meta, n, nr, _, _, _ = _process_case()
    eng = _engine(params)
    try:
        _, a, v, q, f, m = eng.process_meta(arrs, meta, n, nr)
        q2, f2, m2 = eng.genotype_meta(arrs, meta, n, nr, a, v)
    finally:
        eng.close()
    for got, again in ((q, q2), (f, f2), (m, m2)):
        for key, val in again.items():
            assert np.array_equal(val.view(np.uint8), got[key].view(np.uint8)), key


def test_without_the_new_outputs_the_calls_are_what_they_were():
    """fmeta NULL, or its four members NULL: every output is byte-identical to ma_process_stats_batch's and the same kernels
    are launched; meta is then not read (a NULL pointer, and a struct of NULL members, are accepted)"""
    params, arrs, meta, n, nr, _, _, _ = _process_case()
    eng = _engine(params)
    try:
        b = capi.make_batch_struct(arrs, n, nr)
        plain = eng.process_stats(arrs, n, nr)
        plain_names = sorted(k for k, _ in eng.kernel_times())
        runs = []
        for meta_struct, fmeta_struct in ((None, None), (capi.ReadMeta(), capi.FmtMetaOut()),
                                          (capi.fill_struct(capi.ReadMeta, meta), capi.FmtMetaOut())):
            outs, structs = _host_outs(params, n, nr)
            eng.process_meta_device(b, None, meta_struct, *structs[:5], fmeta_struct)
            runs.append((outs, sorted(k for k, _ in eng.kernel_times())))
        with_meta = eng.process_meta(arrs, meta, n, nr)
        meta_names = sorted(k for k, _ in eng.kernel_times())
    finally:
        eng.close()
    for outs, names in runs:
        assert names == plain_names
        for got, ref in zip(outs[:5], plain):
            for key, val in ref.items():
                assert np.array_equal(val.view(np.uint8), got[key].view(np.uint8)), key
        assert (outs[5]["fmt_mstat"] == 7.0).all()  # not touched
    assert meta_names == plain_names  # (k_evid_stats either way: the new statistics ride in the same launch)
    for got, ref in zip(with_meta[:5], plain):
        for key, val in ref.items():
            assert np.array_equal(val.view(np.uint8), got[key].view(np.uint8)), key


def test_argument_errors():
    """a member of fmeta set with meta NULL, or with a NULL member of meta: MA_ERR_ARG, from every entry point"""
    c = cases.case("positions")
    eng = _engine(c.params)
    try:
        b = capi.make_batch_struct(c.arrs, c.n, c.nr)
        asm, var = capi.fill_struct(capi.AsmOut, c.asm), capi.fill_struct(capi.VarOut, c.var)
        geno = capi.alloc_host(capi.geno_out_spec(c.params, c.n, c.nr, False))
        fmeta = capi.alloc_host(capi.fmt_meta_out_spec(c.params, c.n))
        outs, structs = _host_outs(c.params, c.n, c.nr)
        only_rmq = capi.fill_struct(capi.FmtMetaOut, dict(fmt_rmq=fmeta["fmt_rmq"]))
        bad_metas = [None] + [capi.fill_struct(capi.ReadMeta, {k: v for k, v in c.meta.items() if k != drop}) for drop in c.meta]
        for m in bad_metas:
            ref = C.byref(m) if m is not None else None
            rc = eng.lib.ma_genotype_meta_batch(eng.h, C.byref(b), ref, C.byref(asm), C.byref(var),
                                                C.byref(capi.fill_struct(capi.GenoOut, geno)), None, C.byref(only_rmq))
            assert rc == -1
            rc = eng.lib.ma_process_meta_batch(eng.h, C.byref(b), None, ref, *[C.byref(s) for s in structs[:4]], None,
                                               C.byref(only_rmq))
            assert rc == -1
        for m in bad_metas[1:]:
            assert eng.lib.ma_prefetch_meta_batch(eng.h, C.byref(b), None, C.byref(m)) == -1
        good = capi.fill_struct(capi.ReadMeta, c.meta)
        pk = capi.PackedReads()  # an ASCII batch brought as packed, and a packed struct without arrays
        assert eng.lib.ma_process_meta_batch(eng.h, C.byref(b), C.byref(pk), C.byref(good), *[C.byref(s) for s in structs[:4]],
                                             None, C.byref(only_rmq)) == -1
        # ... and the engine still works
        _, _, got = eng.genotype_meta(c.arrs, c.meta, c.n, c.nr, c.asm, c.var, meta_fields=("fmt_rmq",))
    finally:
        eng.close()
    bad = cases.compare_meta(got, cases.reference("positions"), "after the errors")
    assert not bad, "\n".join(bad)


def test_vcf_carries_all_24_format_values(tmp_path):
    """pipeline_driver --out-vcf --read-meta on the small genome of tests/test_pipeline_host.py (its SAM metadata made
    interesting): the six values are printed with the reference's formats and are missing exactly where the AD column says
    they must be; the other 18 columns are those of the run without --read-meta, where the six are "."; --packed-reads gives
    the same file"""
    import subprocess
    import test_pipeline_host as host
    from test_format_meta_ref import rewrite_sam_metadata
    exe = host.driver(tmp_path)
    host.write_fixture(str(tmp_path))
    for i, name in enumerate(("normal", "tumor")):
        rewrite_sam_metadata(str(tmp_path / (name + ".sam")), 50 + i)
    six = ("RMQ", "SCA", "FLD", "RPCD", "MQCD", "FSSE")

    def run(tag, *flags):
        vcf = tmp_path / f"calls_{tag}.vcf"
        r = subprocess.run([exe, "--reference", str(tmp_path / "ref.fa"), "--normal", str(tmp_path / "normal.sam"),
                            "--tumor", str(tmp_path / "tumor.sam"), "--region", "chr1:1-6000", "--min-kmer", "25", "--max-kmer", "25",
                            "--batch-windows", "3", "--out-vcf", str(vcf), *flags], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return [x.split("\t") for x in open(vcf).read().splitlines() if not x.startswith("#")]

    plain, meta, packed = run("plain"), run("meta", "--read-meta"), run("packed", "--read-meta", "--packed-reads")
    assert meta == packed and len(meta) == len(plain) >= 6
    seen = dict(samples=0, fld=0, rpcd=0, fsse=0, missing_rpcd=0, missing_fsse=0)
    for f, g in zip(meta, plain):
        assert f[:9] == g[:9]
        key = f[8].split(":")
        for col, col0 in zip(f[9:], g[9:]):
            vals, vals0 = dict(zip(key, col.split(":"))), dict(zip(key, col0.split(":")))
            for name in key:
                if name in six:
                    assert vals0[name] == "."
                else:
                    assert vals[name] == vals0[name], name
            if vals["GT"] == "./.":
                assert all(vals[name] == "." for name in six)
                continue
            seen["samples"] += 1
            ad = [int(x) for x in vals["AD"].split(",")]
            rmq = vals["RMQ"].split(",")
            assert len(rmq) == len(ad)
            for x, d in zip(rmq, ad):
                assert len(x.split(".")[1]) == 1  # {:.1f}
                assert (0.0 < float(x) <= 60.0) if d > 0 else (float(x) == 0.0), (vals["RMQ"], ad)  # (MAPQ 7 ... 60 in the fixture)
            both = ad[0] > 0 and sum(ad[1:]) > 0
            assert -1.0 <= float(vals["SCA"]) <= 1.0 and len(vals["SCA"].split(".")[1]) == 4
            for name in ("RPCD", "MQCD"):
                assert (vals[name] != ".") == both, (name, vals[name], ad)
                if both:
                    assert len(vals[name].split(".")[1]) == 4 and abs(float(vals[name])) <= 1.0
            assert (vals["FSSE"] != ".") == (sum(ad[1:]) >= 3), (vals["FSSE"], ad)
            if vals["FSSE"] != ".":
                # entropy <= log2(ALT reads), normalised by log2(min(ALT reads, 20)): above 1 only with more than 20 bins
                n_alt = sum(ad[1:])
                assert 0.0 <= float(vals["FSSE"]) <= max(1.0, np.log2(n_alt) / np.log2(20.0)) + 5e-5, (vals["FSSE"], ad)
            if vals["FLD"] != ".":
                assert both and len(vals["FLD"].split(".")[1]) == 1 and abs(float(vals["FLD"])) <= 902 + 455
                seen["fld"] += 1
            seen["rpcd"] += both
            seen["missing_rpcd"] += not both
            seen["fsse"] += vals["FSSE"] != "."
            seen["missing_fsse"] += vals["FSSE"] == "."
    assert seen["samples"] >= 8 and seen["rpcd"] >= 3 and seen["missing_rpcd"] >= 1 and seen["fsse"] >= 3 and seen["fld"] >= 3, seen
