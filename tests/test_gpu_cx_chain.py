"""ma_process_cx_batch: the annotation (SEQ_CX / GRAPH_CX) as a stage of the chained call, on every route -- the host route's
lanes with packed records, prefetched jobs, the device route with and without lanes, the legacy host staging -- against
ma_annotate_batch over the call's own assembly and variant arrays (byte for byte in the used variant slots) and against the
oracle's chain (tests/cx_chain_cases.py, guarded by tests/test_cx_chain_cases.py); and k_hap_lq over a hand-made table of
haplotype shapes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lancet2_amd import capi

import cx_chain_cases as cases
from harness import SEQCX_FLOAT_TOL, DeviceArena, compare_cx

pytestmark = pytest.mark.gpu

OUT_CLASSES = (capi.GateOut, capi.AsmOut, capi.VarOut, capi.GenoOut, capi.FmtOut, capi.FmtMetaOut)
CX_KERNELS = ["k_hap_lq", "k_seqcx"]
SENTINEL = 0x5A


def _engine(params, **kw):
    from lancet2_amd.engine import Engine
    return Engine(params, **kw)


def _used_bytes(params, cx, win_nvars):
    """the bytes of the four arrays in the variant slots the windows use"""
    used = cases.used_slots(params, win_nvars)
    return {k: v.view(np.uint8).reshape(len(used), -1)[used] for k, v in cx.items()}


def _assert_same_used(params, got, want, win_nvars, what):
    g, w = _used_bytes(params, got, win_nvars), _used_bytes(params, want, win_nvars)
    for key in w:
        assert np.array_equal(g[key], w[key]), f"{what}: {key}"


def _host_outs(params, n, nr, with_meta=True):
    specs = [capi.gate_out_spec(n), capi.asm_out_spec(params, n), capi.var_out_spec(params, n),
             capi.geno_out_spec(params, n, nr, False), capi.fmt_out_spec(params, n), capi.fmt_meta_out_spec(params, n)]
    outs = [capi.alloc_host(s) for s in specs]
    structs = [capi.fill_struct(cls, o) for cls, o in zip(OUT_CLASSES, outs)]
    if not with_meta:
        structs[5] = None
    cx = capi.alloc_host(capi.cx_out_spec(params, n))
    for v in cx.values():
        v.view(np.uint8)[:] = SENTINEL  # whatever the caller's arrays held: only the used slots are compared
    return outs, structs, cx, capi.fill_struct(capi.CxOut, cx)


@pytest.mark.parametrize("streams", [2, 1])
def test_chain_annotation_is_the_stage_call(streams):
    """host route: ASCII and packed input, with and without the read metadata, at two GC fractions in one engine (the second
    rebuilds the tables inside a lane)"""
    c = cases.chain_case()
    eng = _engine(c.params)
    runs = []
    try:
        eng.set_streams(streams)
        for gc in cases.GC_FRACS:
            for packed in (None, c.packed):
                for meta in (c.meta, None):
                    out = eng.process_cx(c.arrs, c.n, c.nr, meta=meta, packed=packed, gc_frac=gc)
                    names = sorted(k for k, _ in eng.kernel_times())
                    stage = eng.annotate(c.arrs, c.n, c.nr, out[1], out[2], gc_frac=gc)
                    runs.append((f"gc {gc} packed {packed is not None} meta {meta is not None}", gc, out, stage, names))
    finally:
        eng.close()
    for what, gc, out, stage, names in runs:
        assert np.array_equal(out[2]["win_nvars"], c.var["win_nvars"]), what
        _assert_same_used(c.params, out[6], stage, out[2]["win_nvars"], what)
        assert compare_cx(c.params, out[6], c.cx[gc], c.var["win_nvars"]) == int(c.var["win_nvars"].sum())
        assert all(k in names for k in CX_KERNELS), what
        assert (out[5] == {}) == ("meta False" in what)


def test_chain_annotation_prefetched():
    """a job queued ahead carries the annotation of the previous call; one queued under other assumptions (no annotation, another
    GC fraction) is dropped and computed in the call"""
    c = cases.chain_case()
    eng = _engine(c.params)
    got = {}
    try:
        eng.set_streams(2)
        b = capi.make_batch_struct(c.arrs, c.n, c.nr)
        ms = capi.fill_struct(capi.ReadMeta, c.meta)
        first = eng.process_cx(c.arrs, c.n, c.nr, meta=c.meta, gc_frac=0.41)
        for name, queue in (("prefetch_meta", lambda: eng.prefetch_meta(b, None, ms)), ("prefetch", lambda: eng.prefetch(b))):
            queue()  # (the last call asked for the annotation at 0.41: so does the job queued here)
            outs, structs, cx, cxs = _host_outs(c.params, c.n, c.nr, with_meta=name == "prefetch_meta")
            eng.process_cx_device(b, None, ms if name == "prefetch_meta" else None, *structs, cxs, gc_frac=0.41)
            got[name] = (outs, cx, 0.41)
        # queued after a call WITHOUT the annotation, brought with it
        outs, structs, _, _ = _host_outs(c.params, c.n, c.nr)
        eng.process_meta_device(b, None, ms, *structs)
        eng.prefetch_meta(b, None, ms)
        outs, structs, cx, cxs = _host_outs(c.params, c.n, c.nr)
        eng.process_cx_device(b, None, ms, *structs, cxs, gc_frac=0.41)
        got["queued without"] = (outs, cx, 0.41)
        # queued with 0.41, brought with 0.30
        eng.prefetch_meta(b, None, ms)
        outs, structs, cx, cxs = _host_outs(c.params, c.n, c.nr)
        eng.process_cx_device(b, None, ms, *structs, cxs, gc_frac=0.30)
        got["queued at another gc"] = (outs, cx, 0.30)
        again = eng.process_cx(c.arrs, c.n, c.nr, meta=c.meta, gc_frac=0.30)
    finally:
        eng.close()
    for what, (outs, cx, gc) in got.items():
        want = first if gc == 0.41 else again
        assert np.array_equal(outs[2]["win_nvars"], c.var["win_nvars"]), what
        _assert_same_used(c.params, cx, want[6], c.var["win_nvars"], what)
        compare_cx(c.params, cx, c.cx[gc], c.var["win_nvars"])
        for key, val in want[3].items():  # ... and the rest of the call is the plain call's
            assert np.array_equal(val.view(np.uint8), outs[3][key].view(np.uint8)), (what, key)


@pytest.mark.parametrize("streams", [2, 1])
def test_chain_annotation_on_the_device_route(streams):
    """MA_MEM_DEVICE: caller-owned device arrays, the four annotation arrays sliced per lane"""
    c = cases.chain_case()
    p, n, nr = c.params, c.n, c.nr
    specs = [capi.gate_out_spec(n), capi.asm_out_spec(p, n), capi.var_out_spec(p, n), capi.geno_out_spec(p, n, nr, debug=False),
             capi.fmt_out_spec(p, n), capi.fmt_meta_out_spec(p, n), capi.cx_out_spec(p, n), capi.cx_out_spec(p, n)]
    eng = _engine(p, memspace=capi.MA_MEM_DEVICE)
    arena = DeviceArena()
    try:
        b = capi.make_batch_struct({k: arena.upload(v) for k, v in c.arrs.items()}, n, nr)
        ms = capi.fill_struct(capi.ReadMeta, {k: arena.upload(v) for k, v in c.meta.items()})
        ptrs = [{k: arena.alloc(int(sz) * np.dtype(dt).itemsize) for k, (dt, sz) in spec.items()} for spec in specs]
        structs = [capi.fill_struct(cls, x) for cls, x in zip(OUT_CLASSES + (capi.CxOut, capi.CxOut), ptrs)]
        eng.set_streams(streams)
        eng.process_cx_device(b, None, ms, *structs[:7], gc_frac=0.41)
        eng.synchronize()
        names = sorted(k for k, _ in eng.kernel_times())
        eng.annotate_device(b, structs[1], structs[2], structs[7], gc_frac=0.41)
        eng.synchronize()
        nv = arena.download(ptrs[2]["win_nvars"], *specs[2]["win_nvars"])
        chain, stage = ({k: arena.download(ptrs[i][k], dt, sz) for k, (dt, sz) in specs[i].items()} for i in (6, 7))
    finally:
        eng.close()
        arena.close()
    assert np.array_equal(nv, c.var["win_nvars"])
    _assert_same_used(p, chain, stage, nv, f"device route, {streams} lanes")
    assert compare_cx(p, chain, c.cx[0.41], nv) == int(nv.sum())
    assert names.count("k_hap_lq") == streams and names.count("k_seqcx") == streams


def test_big_arrays_left_out():
    """host route: the annotation reads the engine's own device arrays, whatever the caller asked to have brought back"""
    c = cases.chain_case()
    eng = _engine(c.params)
    try:
        eng.set_streams(2)
        full = eng.process_cx(c.arrs, c.n, c.nr, meta=c.meta)
        outs, structs, cx, cxs = _host_outs(c.params, c.n, c.nr)
        b = capi.make_batch_struct(c.arrs, c.n, c.nr)
        for key in ("hap_bases", "hap_runs"):
            setattr(structs[1], key, None)
        for key in ("allele_pool", "var_hap_start"):
            setattr(structs[2], key, None)
        eng.process_cx_device(b, None, capi.fill_struct(capi.ReadMeta, c.meta), *structs, cxs, gc_frac=0.41)
    finally:
        eng.close()
    _assert_same_used(c.params, cx, full[6], c.var["win_nvars"], "without the big arrays")
    assert not outs[1]["hap_bases"].any() and not outs[2]["allele_pool"].any()  # not written
    assert np.array_equal(outs[3]["allele_counts"], full[3]["allele_counts"])


def test_without_cx_the_call_is_what_it_was():
    """cx NULL, or its four members NULL, at any gc_frac (NaN included): ma_process_meta_batch, bytes and kernels"""
    c = cases.chain_case()
    eng = _engine(c.params)
    try:
        b = capi.make_batch_struct(c.arrs, c.n, c.nr)
        ms = capi.fill_struct(capi.ReadMeta, c.meta)
        plain = eng.process_meta(c.arrs, c.meta, c.n, c.nr)
        plain_names = sorted(k for k, _ in eng.kernel_times())
        runs = []
        for cxs, gc in ((None, 0.41), (None, float("nan")), (capi.CxOut(), 7.5), (capi.CxOut(), float("nan"))):
            outs, structs, _, _ = _host_outs(c.params, c.n, c.nr)
            eng.process_cx_device(b, None, ms, *structs, cxs, gc_frac=gc)
            runs.append((outs, sorted(k for k, _ in eng.kernel_times())))
        with_cx = eng.process_cx(c.arrs, c.n, c.nr, meta=c.meta)
        cx_names = sorted(k for k, _ in eng.kernel_times())
    finally:
        eng.close()
    assert not any(k in plain_names for k in CX_KERNELS)
    for outs, names in runs:
        assert names == plain_names
        for got, ref in zip(outs, plain):
            for key, val in ref.items():
                assert np.array_equal(val.view(np.uint8), got[key].view(np.uint8)), key
    lanes = cx_names.count("k_seqcx")
    assert lanes >= 1 and cx_names == sorted(plain_names + CX_KERNELS * lanes)  # that list plus exactly the two, per lane
    for got, ref in zip(with_cx[:6], plain):
        for key, val in ref.items():
            assert np.array_equal(val.view(np.uint8), got[key].view(np.uint8)), key


def test_argument_errors():
    c = cases.chain_case()
    eng = _engine(c.params)
    try:
        b = capi.make_batch_struct(c.arrs, c.n, c.nr)
        outs, structs, cx, cxs = _host_outs(c.params, c.n, c.nr, with_meta=False)
        refs = [C.byref(s) for s in structs[:5]]

        def call(cx_struct, gc, pk=None):
            return eng.lib.ma_process_cx_batch(eng.h, C.byref(b), pk, None, *refs, None, C.c_double(gc), C.byref(cx_struct))

        keys = list(cx)
        for subset in (keys[:1], keys[1:2], keys[:2], keys[2:], keys[:3], keys[1:]):  # one, two or three of the four
            assert call(capi.fill_struct(capi.CxOut, {k: cx[k] for k in subset}), 0.41) == -1, subset
        assert call(cxs, float("nan")) == -1
        assert call(cxs, 0.41, C.byref(capi.PackedReads())) == -1  # a packed struct on an ASCII batch
        assert call(cxs, 0.41) == 0
        good = eng.process_cx(c.arrs, c.n, c.nr)  # ... and the engine still works
    finally:
        eng.close()
    _assert_same_used(c.params, cx, good[6], c.var["win_nvars"], "after the errors")
    compare_cx(c.params, good[6], c.cx[0.41], c.var["win_nvars"])


@pytest.mark.parametrize("group", [g.name for g in cases.hap_lq_groups()])
def test_hap_lq_shapes(group):
    g = {x.name: x for x in cases.hap_lq_groups()}[group]
    want = cases.hap_lq_reference()[group]
    eng = _engine(g.params)
    try:
        got = eng.annotate(cases.group_batch(g), g.n, 0, g.asm, g.var)
    finally:
        eng.close()
    nv = g.var["win_nvars"]
    assert compare_cx(g.params, got, want, nv) == int(nv.sum())
    used = cases.used_slots(g.params, nv)
    have, ref = (x["seq_cx_d"].reshape(-1, 3)[used, 1] for x in (got, want))
    for name, a, b in zip(np.repeat(np.array(g.names), nv), have, ref):
        print(f"{group} {name}: ContextHaplotypeLQ {a!r} oracle {b!r}")
    assert np.isfinite(have).all()  # every component that has a variant: present and finite
    assert np.abs(have - ref).max() <= SEQCX_FLOAT_TOL


_LEGACY_CHILD = """
import sys
import numpy as np
sys.path.insert(0, {tests!r})
import cx_chain_cases as cases
from lancet2_amd.engine import Engine
c = cases.chain_case()
eng = Engine(c.params)
try:
    out = eng.process_cx(c.arrs, c.n, c.nr, meta=c.meta, packed=c.packed)
finally:
    eng.close()
np.savez({path!r}, win_nvars=out[2]["win_nvars"], allele_counts=out[3]["allele_counts"], **out[6])
"""


def test_legacy_host_staging(tmp_path):
    """MA_HOST_LEGACY=1 (whole-array staging on the caller's context), in a process of its own: the default route's bytes"""
    c = cases.chain_case()
    eng = _engine(c.params)
    try:
        want = eng.process_cx(c.arrs, c.n, c.nr, meta=c.meta, packed=c.packed)
    finally:
        eng.close()
    path = str(tmp_path / "legacy.npz")
    env = dict(os.environ, MA_HOST_LEGACY="1", PYTHONPATH=os.pathsep.join([capi.REPO] + sys.path))
    r = subprocess.run([sys.executable, "-c", _LEGACY_CHILD.format(tests=os.path.dirname(os.path.abspath(__file__)), path=path)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = dict(np.load(path))
    assert np.array_equal(got["win_nvars"], want[2]["win_nvars"]) and np.array_equal(got["allele_counts"], want[3]["allele_counts"])
    _assert_same_used(c.params, {k: got[k] for k in want[6]}, want[6], want[2]["win_nvars"], "MA_HOST_LEGACY")
