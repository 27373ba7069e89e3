"""The caller's eight output caps at exact fit and one under the need (tests/cap_cases.py; tests/test_cap_cases.py pins the
table and the oracle's side of it on the CPU): for every cap and every tight parameter set -- the roomy caps with that cap
alone set to one of the needs of its batch -- one Engine against the oracle under the same set.

The contract ("Output-format caps are the caller's"):
  * the status word of EVERY window equals the oracle's, bit for bit: a window over the cap carries the cap's flag, a window at
    exact fit does not;
  * every unflagged window is bit-identical in the assembly, the variants and the call-level genotype arrays;
  * a flagged window is compared by status only, but its counts stay inside the caps (they index the caller's arrays).
One chained run per cap (ma_process_batch) on the host route with two lanes, whose packed result copy walks these strides too,
and on MA_MEM_DEVICE with 256 bytes of junk in front of and behind every output array, which must come back unchanged.

Every compared value is an integer, a byte, a status word or the bits of a double (QUAL: within 1e-9, compare_geno_calls)."""
import time

import numpy as np
import pytest

import cap_cases as cc
from harness import compare_asm, compare_geno_calls, compare_vars
from lancet2_amd import capi

pytestmark = pytest.mark.gpu

TIGHT = cc.tight_sets()
GUARD, JUNK = 256, 0x5A


def _check(cap, c, bname, got_asm, got_var, got_geno):
    """engine results of a batch under the tight set (cap, c) against the oracle's under the same set"""
    b = cc.batch(bname)
    p, asm, var, geno = cc.oracle_chain(bname, cap, c)
    status, want_status = got_asm["win_status"], asm["win_status"]
    for w in range(b.n):
        print(f"{cap}={c}: {b.names[w]:20s} status {int(status[w]):3d} (oracle {int(want_status[w]):3d})")
    assert np.array_equal(status, want_status), (cap, c, status.tolist(), want_status.tolist())
    fits = [w for w in range(b.n) if not int(want_status[w]) & cc.CAP_BITS]
    bad = compare_asm(p, got_asm, asm, b.n, windows=fits) + compare_vars(p, got_var, var, b.n, windows=fits) + \
        compare_geno_calls(got_geno, geno, windows=fits, n=b.n)
    assert not bad, "\n".join(bad[:20])
    MC, MH, MV = p.max_comps, p.max_haps, p.max_vars
    for w in range(b.n):  # flagged or not: no count of a window may point past its rows
        nc = int(got_asm["win_ncomp"][w])
        assert nc <= MC, (b.names[w], nc)
        nh = got_asm["comp_nhaps"][w * MC:w * MC + nc].astype(np.int64)
        assert int(nh.sum()) <= MH and all(int(h0) + int(k) <= MH for h0, k in zip(got_asm["comp_hap0"][w * MC:w * MC + nc], nh)), b.names[w]
        used = int(nh.sum())
        assert (got_asm["hap_len"][w * MH:w * MH + used] <= p.max_hap_len).all() and (got_asm["hap_nruns"][w * MH:w * MH + used] <= p.max_runs).all(), b.names[w]
        nv = int(got_var["win_nvars"][w])
        assert nv <= MV and (got_var["var_nalts"][w * MV:w * MV + nv] <= p.max_alts).all(), b.names[w]
    return fits


def _staged(cap, c, lib_path=None):
    from lancet2_amd.engine import Engine
    bname = cc.CAPS[cap][2]
    b = cc.batch(bname)
    p = cc.params(**{cap: c})
    t0 = time.perf_counter()
    eng = Engine(p, lib_path=lib_path)
    try:
        asm = cc.fresh_asm(b, p) if b.asm else eng.assemble(b.arrs, b.n, b.nr)
        var = eng.msa(b.arrs, b.n, b.nr, asm)
        geno = eng.genotype(b.arrs, b.n, b.nr, asm, var, debug=False)
    finally:
        eng.close()
    print(f"{cap}={c}: engine {time.perf_counter() - t0:.2f} s")
    return bname, asm, var, geno


@pytest.mark.parametrize("cap,c", TIGHT, ids=[f"{cap}-{c}" for cap, c in TIGHT])
def test_tight_set(cap, c):
    bname, asm, var, geno = _staged(cap, c)
    fits = _check(cap, c, bname, asm, var, geno)
    assert fits, "every tight set of the table holds windows that fit"


def _exact_fit_case(name, max_haps):
    b = cc.batch("reads")
    w = b.names.index(name)
    assert int(cc.needs("reads")["slots"][w]) == max_haps
    _, asm, var, geno = _staged("max_haps", max_haps)
    p, want_asm, want_var, want_geno = cc.oracle_chain("reads", "max_haps", max_haps)
    assert int(want_asm["win_status"][w]) == 0
    assert int(asm["win_status"][w]) == 0, f"{name}: status {int(asm['win_status'][w])} with max_haps = {max_haps}"
    bad = compare_asm(p, asm, want_asm, b.n, windows=[w]) + compare_vars(p, var, want_var, b.n, windows=[w]) + \
        compare_geno_calls(geno, want_geno, windows=[w], n=b.n)
    assert not bad, "\n".join(bad[:20])
    assert int(asm["comp_nhaps"][w * p.max_comps]) == max_haps


def test_alt_heavier_exact_fit():
    """max_haps = 2, one SNV whose ALT haplotype is deeper than REF: the walks sorted by MinWeight are "kept ALT, then the walk
    that spells the REF anchor" (oracle/graph.cpp, BuildHaplotypes: the stable sort, then the loop that drops walks that repeat
    an earlier one or equal the anchor), 2 haplotypes, and oracle/capi.cpp's orc_assemble_batch flags MA_W_HAP_OVERFLOW only
    when slot + haps.size() > max_haps -- after the drop.  clean.hip (clean_candidates, the loop over the sorted walks) used to
    test slot >= max_haps BEFORE it spelled and compared the walk, and flagged this window."""
    _exact_fit_case("alt_heavier", 2)


def test_two_alt_heavier_exact_fit():
    """the three-haplotype version at max_haps = 3: two ALT haplotypes deeper than REF, the REF-equal walk last (see
    test_alt_heavier_exact_fit for the code lines)"""
    _exact_fit_case("two_alt_heavier", 3)


def _chained_value(cap):
    """the batch a chained run of `cap` takes (read-built batches only) and the value of the cap with the most exact fits there"""
    key, _, bname, (lo, hi) = cc.CAPS[cap]
    if bname == "poa":
        bname = "reads"
    nd = cc.needs(bname)[key]
    vals = sorted({int(v) for v in nd if lo <= int(v) <= hi}) or [lo]  # (no need reaches the smallest admitted value: that one)
    return bname, max(vals, key=lambda c: (int((nd == c).sum()), -c))


@pytest.mark.parametrize("cap", tuple(cc.CAPS))
def test_chained_host_route_two_lanes(cap):
    from lancet2_amd.engine import Engine
    bname, c = _chained_value(cap)
    b = cc.batch(bname)
    eng = Engine(cc.params(**{cap: c}))
    try:
        eng.set_streams(2)
        _, asm, var, geno = eng.process(b.arrs, b.n, b.nr, debug=False)
    finally:
        eng.close()
    _check(cap, c, bname, asm, var, geno)


@pytest.mark.parametrize("cap", tuple(cc.CAPS))
def test_chained_device_route_keeps_its_guards(cap):
    from harness import DeviceArena
    from lancet2_amd.engine import Engine
    bname, c = _chained_value(cap)
    b = cc.batch(bname)
    p = cc.params(**{cap: c})
    specs = [capi.gate_out_spec(b.n), capi.asm_out_spec(p, b.n), capi.var_out_spec(p, b.n), capi.geno_out_spec(p, b.n, b.nr, debug=False)]
    eng = Engine(p, memspace=capi.MA_MEM_DEVICE)
    arena = DeviceArena()
    try:
        bs = capi.make_batch_struct({k: arena.upload(v) for k, v in b.arrs.items()}, b.n, b.nr)
        # every output array exactly sized, junk in front of it and behind it
        ptrs = [{k: arena.upload_unaligned(np.zeros(int(sz), dt), shift=0, guard=GUARD, junk=JUNK) for k, (dt, sz) in spec.items()} for spec in specs]
        eng.process_device(bs, capi.fill_struct(capi.GateOut, ptrs[0]), capi.fill_struct(capi.AsmOut, ptrs[1]),
                           capi.fill_struct(capi.VarOut, ptrs[2]), capi.fill_struct(capi.GenoOut, ptrs[3]))
        eng.synchronize()
        outs = [{k: arena.download(pt[k], dt, sz) for k, (dt, sz) in spec.items()} for spec, pt in zip(specs, ptrs)]
        for spec, pt in zip(specs, ptrs):
            for k, (dt, sz) in spec.items():
                nbytes = int(sz) * np.dtype(dt).itemsize
                front, behind = arena.download(pt[k] - GUARD, np.uint8, GUARD), arena.download(pt[k] + nbytes, np.uint8, GUARD)
                assert (front == JUNK).all() and (behind == JUNK).all(), f"{cap}={c}: the guard of {k} changed"
    finally:
        eng.close()
        arena.close()
    _check(cap, c, bname, outs[1], outs[2], outs[3])
