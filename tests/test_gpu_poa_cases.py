"""The POA stage (k_poa / msa_window, poa.hip) on the hand-made components of tests/poa_cases.py, against the oracle, whose POA
has none of the engine's widths.  tests/test_poa_cases.py checks on the CPU what every case is for.

The contract:
  * a window that is not may_flag equals the oracle in every variant array and stays unflagged;
  * a may_flag window EITHER equals the oracle with status 0 OR carries exactly MA_W_VAR_OVERFLOW (a long case:
    MA_W_LEN_OVERFLOW) and is compared by status only -- never an unflagged result that differs;
  * the call returns MA_OK and the flagged window's batch neighbours equal the oracle.
Which may_flag windows ARE flagged is pinned in FLAGGED: the "over" and long cases by construction (kPE = 4, the node
capacity pn <= longest haplotype + 263, the LDS block), the headroom cases as the stage sizes pn today (DESIGN section 9:
lifting kPE, a retry with a larger pn and a pn that does not depend on batch mates are open).

Every compared value is an integer, a byte or a status word: no tolerance anywhere."""
import numpy as np
import pytest

import poa_cases as pc
from harness import compare_vars
from lancet2_amd import capi

pytestmark = pytest.mark.gpu

# may_flag windows that come back flagged, per route ("*": every route).  The others come back called, equal to the oracle.
FLAGGED = {
    "*": {"out_degree_5", "out_degree_6", "in_degree_5", "in_degree_6", "ring_6", "ins_8x60", "over_between_two_fitting",
          "length_3072", "length_3073", "length_4096", "length_2552", "narrow_2400_then_17_haplotypes"},
    # every window through the LAB32 kernels: no 2400-base haplotype fits their LDS block (poa_cases.LAB32_LEN_CEILING), the
    # three are left out, pn follows the 1060 bases that remain and the eight insertions are over again
    "lab32": {"snv_20_on_2400", "snv_20_on_2400_b", "snv_80_on_2400", "ins_8x60_beside_2400", "length_2551", "length_2256"},
}


def _run(group, route, monkeypatch):
    from lancet2_amd.engine import Engine
    for k, v in pc.ROUTES[route].items():
        monkeypatch.setenv(k, v)
    g = pc.groups()[group]
    p = g.params
    arrs, n, nr, asm = pc.build(group)
    want, want_status = pc.oracle_msa(group)
    eng = Engine(p)
    try:
        got = eng.msa(arrs, n, nr, asm)  # (raises on a return code other than MA_OK)
    finally:
        eng.close()
    status = asm["win_status"]
    masked = {k: np.array(v, copy=True) for k, v in got.items()}
    flagged = set()
    for wi, w in enumerate(g.windows):
        may, bit = pc.may_flag_on(route, w)
        st = int(status[wi])
        print(f"{group}/{route}: {w.name:28s} status {st:3d} variants {int(got['win_nvars'][wi]):3d} (oracle {int(want['win_nvars'][wi])})")
        if may and st != 0:
            assert st == bit, (w.name, st, bit)
            if bit == capi.MA_W_LEN_OVERFLOW:  # left out whole: no component of it ran
                assert int(got["win_nvars"][wi]) == 0, w.name
            flagged.add(w.name)
            for k in masked:  # compared by status only
                stride = len(masked[k]) // n
                masked[k][wi * stride:(wi + 1) * stride] = want[k][wi * stride:(wi + 1) * stride]
        else:
            assert st == int(want_status[wi]) == 0, (w.name, st)
    bad = compare_vars(p, masked, want, n)
    assert not bad, "\n".join(bad[:20])
    names = {w.name for w in g.windows}
    assert flagged == (FLAGGED["*"] | FLAGGED.get(route, set())) & names, sorted(flagged)


@pytest.mark.parametrize("group", tuple(g for g in pc.groups() if g not in ("length_edge", "wide_long")))
def test_default_route(group, monkeypatch):
    _run(group, "default", monkeypatch)


@pytest.mark.parametrize("route", ["default", "lab32"])
def test_longest_haplotype_that_fits_and_one_more(route, monkeypatch):
    """2551 / 2552 bases in the common kernels, 2255 / 2256 in the LAB32 kernels: the window at the edge is called from the
    largest LDS block the stage ever launches with, the one beyond it is flagged MA_W_LEN_OVERFLOW and the batch goes on"""
    _run("length_edge", route, monkeypatch)


@pytest.mark.parametrize("route", ["default", "host_rounds", "lab32"])
def test_wide_window_whose_narrow_component_is_the_longest_of_the_batch(route, monkeypatch):
    """a 2400-base haplotype in a window that takes the LAB32 kernels (a 17-haplotype component behind it): longer than those
    kernels hold (2255), shorter than the common kernels' bound (2551), and the longest of the batch.  The window is flagged
    MA_W_LEN_OVERFLOW alone, has no variant, and no pass runs it -- the passes are sized from its neighbours, which equal
    the oracle"""
    _run("wide_long", route, monkeypatch)


def test_alt_slots_a_variant_does_not_fill_read_zero():
    """MA_MEM_DEVICE, the caller's variant arrays filled with junk before the call: of a used variant's max_alts slots in
    alt_off / alt_len / alt_type / alt_length those from var_nalts on are 0 afterwards (the host route delivers whole rows of
    used variants from device buffers nobody clears: two runs of one batch differed there), the used ones are the oracle's"""
    import ctypes as C
    from harness import DeviceArena
    from lancet2_amd.engine import Engine
    g = pc.groups()["degree"]
    p = g.params
    arrs, n, nr, asm = pc.build("degree")
    want, _ = pc.oracle_msa("degree")
    spec = capi.var_out_spec(p, n)
    eng = Engine(p, memspace=capi.MA_MEM_DEVICE)
    arena = DeviceArena()
    try:
        b = capi.make_batch_struct({k: arena.upload(v) for k, v in arrs.items()}, n, nr)
        a = capi.fill_struct(capi.AsmOut, {k: arena.upload(v) for k, v in asm.items()})
        ptrs = {k: arena.upload(np.full(int(sz) * np.dtype(dt).itemsize, 0x5A, np.uint8)) for k, (dt, sz) in spec.items()}
        o = capi.fill_struct(capi.VarOut, ptrs)
        eng._check(eng.lib.ma_msa_batch(eng.h, C.byref(b), C.byref(a), C.byref(o)), "ma_msa_batch")
        eng.synchronize()
        got = {k: arena.download(ptrs[k], *spec[k]) for k in ("win_nvars", "var_nalts", "alt_off", "alt_len", "alt_type", "alt_length")}
    finally:
        eng.close()
        arena.close()
    MV, MA = p.max_vars, p.max_alts
    checked = 0
    for w in range(n):
        for v in range(int(got["win_nvars"][w])):
            vi = w * MV + v
            na = int(got["var_nalts"][vi])
            for key in ("alt_off", "alt_len", "alt_type", "alt_length"):
                row = got[key][vi * MA:(vi + 1) * MA]
                assert not row[na:].any(), (w, v, key, row.tolist())
                if int(want["win_nvars"][w]) == int(got["win_nvars"][w]):
                    assert np.array_equal(row[:na], want[key][vi * MA:vi * MA + na]), (w, v, key)
            checked += MA - na
    assert checked >= 20  # (max_alts = 8, one to four ALT alleles per site)


@pytest.mark.parametrize("group", pc.ROUTE_GROUPS)
@pytest.mark.parametrize("route", [r for r in pc.ROUTES if r != "default"])
def test_other_routes(route, group, monkeypatch):
    """host-counted rounds (MA_POA_SCHED=0), full fill only (MA_POA_BAND=0), no closed-form alignments (MA_POA_NO_DIRECT=1),
    32-bit label masks for every window (MA_POA_FORCE_LAB32=1), the bubble walk's HBM scratch (MA_POA_RAW_CAP=4)"""
    _run(group, route, monkeypatch)
