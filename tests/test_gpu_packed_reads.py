"""ma_process_packed_batch / ma_prefetch_packed_batch on the GPU (tests/packed_reads_cases.py): k_unpack_reads expands the
4-bit bases (and qualities) into the arrays a plain call copies, so every output is byte-identical to ma_process_stats_batch
on the decoded twin -- both memory spaces, one and two lanes, prefetched or not -- and the twin's results are the oracle's."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

from lancet2_amd import capi

import packed_reads_cases as cases

pytestmark = pytest.mark.gpu

STRUCTS = (capi.GateOut, capi.AsmOut, capi.VarOut, capi.GenoOut, capi.FmtOut)
NAMES = ("gate", "asm", "var", "geno", "fmt")


def _engine(params, **kw):
    from lancet2_amd.engine import Engine
    return Engine(params, **kw)


def _specs(params, n, nr):
    return [capi.gate_out_spec(n), capi.asm_out_spec(params, n), capi.var_out_spec(params, n),
            capi.geno_out_spec(params, n, nr, debug=False), capi.fmt_out_spec(params, n)]


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert set(g) == set(w), (what, name)
        for key in w:
            assert np.array_equal(g[key].view(np.uint8), w[key].view(np.uint8)), (what, name, key)


def _run_device(cfg, bits, streams, packed_call):
    """MA_MEM_DEVICE: every array of the call in device memory; the nibble arrays at an odd address inside their allocation"""
    from harness import DeviceArena
    arrs, n, nr, packed, twin = cases.batch(cfg, bits)
    params = cases.params(cfg)
    specs = _specs(params, n, nr)
    eng = _engine(params, memspace=capi.MA_MEM_DEVICE)
    arena = DeviceArena()
    try:
        eng.set_streams(streams)
        ptrs = [{k: arena.alloc(int(sz) * np.dtype(dt).itemsize) for k, (dt, sz) in spec.items()} for spec in specs]
        outs = [capi.fill_struct(cls, p) for cls, p in zip(STRUCTS, ptrs)]
        if packed_call:
            b = capi.make_batch_struct({k: arena.upload(v) for k, v in capi.packed_batch_arrays(arrs).items()}, n, nr)
            dev = dict(packed, bases4=arena.upload_unaligned(packed["bases4"], shift=1),
                       quals=arena.upload_unaligned(packed["quals"], shift=3))
            eng.process_packed_device(b, capi.make_packed_struct(dev), *outs)
        else:
            b = capi.make_batch_struct({k: arena.upload(v) for k, v in twin.items()}, n, nr)
            eng.process_stats_device(b, *outs)
        eng.synchronize()
        names = {k for k, _ in eng.kernel_times()}
        got = [{k: arena.download(p[k], dt, sz) for k, (dt, sz) in spec.items()} for spec, p in zip(specs, ptrs)]
    finally:
        eng.close()
        arena.close()
    return got, names


@functools.lru_cache(maxsize=None)
def _device_reference(cfg, bits):
    """the plain call on the decoded twin, device arrays, computed once per case (results do not depend on the lanes; the
    caller's output arrays start zeroed, so every byte of them is defined)"""
    got, names = _run_device(cfg, bits, 1, packed_call=False)
    assert "k_unpack_reads" not in names
    return got


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("cfg", sorted(cases.CASES))
def test_packed_call_is_the_ascii_call_host_arrays(cfg, bits, streams):
    """The plain call runs on the SAME engine and lanes right before the packed one: the host route brings whole variant
    records home, and the ALT slots a variant does not use hold whatever the lane's device buffer held before -- bytes no
    call defines, equal between two calls only when they go through the same buffers."""
    arrs, n, nr, packed, twin = cases.batch(cfg, bits)
    eng = _engine(cases.params(cfg))
    try:
        eng.set_streams(streams)
        want = eng.process_stats(twin, n, nr)
        got = eng.process_packed(arrs, n, nr, packed)
        names = {k for k, _ in eng.kernel_times()}
    finally:
        eng.close()
    assert int(want[2]["win_nvars"].sum()) > 0  # (the comparison is of calls that found something)
    assert "k_unpack_reads" in names
    _same(got, want, f"{cfg}, {bits}-bit qualities, host arrays, {streams} lanes")


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("cfg", sorted(cases.CASES))
def test_packed_call_is_the_ascii_call_device_arrays(cfg, bits, streams):
    want = _device_reference(cfg, bits)
    got, names = _run_device(cfg, bits, streams, packed_call=True)
    assert "k_unpack_reads" in names
    _same(got, want, f"{cfg}, {bits}-bit qualities, device arrays, {streams} lanes")


def test_packed_call_through_the_legacy_host_staging(monkeypatch):
    """MA_HOST_LEGACY: host arrays staged whole on the caller's stream, the stages on the fixed-stride outputs"""
    arrs, n, nr, packed, twin = cases.batch("C2", 4)
    monkeypatch.setenv("MA_HOST_LEGACY", "1")
    eng = _engine(cases.params("C2"))
    try:
        eng.set_streams(1)
        want = eng.process_stats(twin, n, nr)
        got = eng.process_packed(arrs, n, nr, packed)
        names = {k for k, _ in eng.kernel_times()}
    finally:
        eng.close()
    assert "k_unpack_reads" in names
    _same(got, want, "legacy host staging")


def test_decoded_twin_against_the_oracle():
    """a packer and an unpacker that agree with each other but not with the letters would pass the identity tests"""
    from harness import OracleEngine, compare_asm, compare_geno, compare_vars
    arrs, n, nr, packed, twin = cases.batch("C2", 4)
    params = cases.params("C2")
    eng = _engine(params)
    try:
        g, a, v, q, _ = eng.process_packed(arrs, n, nr, packed, debug=True)
    finally:
        eng.close()
    orc = OracleEngine(params)
    wg = orc.gate(twin, n, nr)
    wa = orc.assemble(twin, n, nr)
    wv = orc.msa(twin, n, nr, wa)
    wq = orc.genotype(twin, n, nr, wa, wv)
    assert np.array_equal(g["max_approx"], wg["max_approx"])
    bad = compare_asm(params, a, wa, n) + compare_vars(params, v, wv, n) + \
        compare_geno(params, q, wq, n, nr, wv["win_nvars"], twin["read_win_off"])
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("streams", [1, 2])
def test_prefetched_or_not_the_result_is_the_same(streams):
    """packed queued and brought packed; ASCII queued and brought packed (same struct address: dropped, computed in the
    call); packed queued and brought ASCII"""
    arrs, n, nr, packed, twin = cases.batch("C2", 4)
    params = cases.params("C2")
    specs = _specs(params, n, nr)
    eng = _engine(params)
    try:
        eng.set_streams(streams)
        want = eng.process_packed(arrs, n, nr, packed)
        pk = capi.make_packed_struct(packed)
        b = capi.make_batch_struct(capi.packed_batch_arrays(arrs), n, nr)
        ascii_ptrs = (twin["read_bases"].ctypes.data, twin["read_quals"].ctypes.data)

        def call(as_packed):
            outs = [capi.alloc_host(s) for s in specs]
            structs = [capi.fill_struct(cls, o) for cls, o in zip(STRUCTS, outs)]
            if as_packed:
                eng.process_packed_device(b, pk, *structs)
            else:
                eng.process_stats_device(b, *structs)
            return outs

        eng.prefetch_packed(b, pk)
        both_packed = call(True)
        b.read_bases, b.read_quals = ascii_ptrs
        eng.prefetch(b)
        b.read_bases, b.read_quals = None, None
        ascii_then_packed = call(True)
        eng.prefetch_packed(b, pk)
        b.read_bases, b.read_quals = ascii_ptrs
        packed_then_ascii = call(False)
        names_ascii = {k for k, _ in eng.kernel_times()}
    finally:
        eng.close()
    assert "k_unpack_reads" not in names_ascii
    for what, got in (("packed, packed", both_packed), ("ASCII, packed", ascii_then_packed), ("packed, ASCII", packed_then_ascii)):
        _same(got, want, f"{streams} lanes, queued and brought as {what}")


def test_unpack_kernel_runs_in_packed_calls_only():
    arrs, n, nr, packed, twin = cases.batch("C5", 4)
    eng = _engine(cases.params("C5"))
    try:
        eng.process_packed(arrs, n, nr, packed, fields=())
        packed_names = [k for k, _ in eng.kernel_times()]
        eng.process(twin, n, nr)
        plain_names = [k for k, _ in eng.kernel_times()]
    finally:
        eng.close()
    assert "k_unpack_reads" in packed_names and "k_unpack_reads" not in plain_names
    assert set(packed_names) - {"k_unpack_reads"} == set(plain_names)


@pytest.mark.parametrize("memspace", [capi.MA_MEM_HOST, capi.MA_MEM_DEVICE])
def test_argument_errors_and_the_empty_batch(memspace):
    arrs, n, nr, packed, twin = cases.batch("C5", 4)
    params = cases.params("C5")
    outs = [capi.alloc_host(s) for s in _specs(params, n, nr)]
    structs = [capi.fill_struct(cls, o) for cls, o in zip(STRUCTS, outs)]
    eng = _engine(params, memspace=memspace)
    try:
        def rc(b, pk):
            return eng.lib.ma_process_packed_batch(eng.h, C.byref(b), C.byref(pk) if pk is not None else None,
                                                   *[C.byref(s) for s in structs])
        pk = capi.make_packed_struct(packed)
        ascii_too = capi.make_batch_struct(twin, n, nr)  # read_bases / read_quals beside pk
        assert rc(ascii_too, pk) == -1
        assert eng.lib.ma_prefetch_packed_batch(eng.h, C.byref(ascii_too), C.byref(pk)) == -1
        b = capi.make_batch_struct(capi.packed_batch_arrays(arrs), n, nr)
        assert rc(b, None) == -1
        five = capi.make_packed_struct(dict(packed, qual_bits=5))
        assert rc(b, five) == -1
        no_bases = capi.make_packed_struct(packed)
        no_bases.bases4 = None
        assert rc(b, no_bases) == -1
        empty = capi.make_batch_struct(capi.packed_batch_arrays(arrs), 0, 0)
        assert rc(empty, pk) == 0
    finally:
        eng.close()


def test_driver_writes_the_same_vcf_from_packed_reads(tmp_path):
    import test_pipeline_host as host
    exe = host.driver(tmp_path)
    host.write_fixture(str(tmp_path))
    texts = []
    for tag, extra in (("ascii", []), ("packed", ["--packed-reads"])):
        vcf = tmp_path / f"calls_{tag}.vcf"
        r = subprocess.run([exe, "--reference", str(tmp_path / "ref.fa"), "--normal", str(tmp_path / "normal.sam"),
                            "--tumor", str(tmp_path / "tumor.sam"), "--region", "chr1:1-6000", "--min-kmer", "25", "--max-kmer", "25",
                            "--batch-windows", "3", "--out-vcf", str(vcf)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = open(vcf, "rb").read().split(b"\n")
        assert sum(x.startswith(b"##commandLine=") for x in lines) == 1
        # (every byte but the header line that quotes the command itself: the flag and the output path are in it)
        texts.append(b"\n".join(x for x in lines if not x.startswith(b"##commandLine=")))
    assert texts[0] == texts[1] and texts[0].count(b"\n") > 20
    assert sum(not x.startswith(b"#") for x in texts[1].split(b"\n") if x) >= 6
