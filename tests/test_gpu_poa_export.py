"""ma_msa_graph_batch (Engine.msa_graph): the SPOA graph and the MSA rows of every component, against tests/poa_graph_ref.py --
which builds the graph from the oracle's alignment pairs alone -- node for node, edge for edge, rank for rank, row for row.
The variant arrays and win_status of the exporting call are compared with Engine.msa on the same input.

Everything is an integer or a byte: no tolerance anywhere.  Inputs are hand-made components (harness.handmade_poa_case)
unless a test says otherwise; tests/poa_export_cases.py draws them, tests/test_poa_graph_ref.py checks the restatement."""
import ctypes as C
import re
from functools import lru_cache

import numpy as np
import pytest

import poa_cases as pc
import poa_export_cases as pxc
import poa_graph_ref as ref
from harness import handmade_poa_case
from lancet2_amd import capi, synth
from pin_cases import rand_dna

pytestmark = pytest.mark.gpu

SMALL = dict(min_k=25, max_k=25, max_haps=32, max_vars=128, max_alts=8, max_allele_bytes=4096)
ANCHOR = 17
CMP_KEYS = ("base", "rank", "col", "haps", "edges", "seq_first", "ncols", "rows", "paths")
VAR_KEYS = tuple(capi.var_out_spec(capi.default_params(), 1))
SWITCHES = {"full_fill": {"MA_POA_BAND": "0"}, "band_in_kernel": {"MA_POA_BAND": "1"}, "no_direct": {"MA_POA_NO_DIRECT": "1"},
            "raw_cap": {"MA_POA_RAW_CAP": "4"}, "lab32": {"MA_POA_FORCE_LAB32": "1"}}


@lru_cache(maxsize=None)
def want_component(haps):
    return ref.component(list(haps))


def want_windows(windows):
    return [[want_component(tuple(h)) for h, _ in comps] for comps in windows]


def needs(windows):
    """(nodes, edges, columns) every window needs, from the restatement"""
    ws = want_windows(windows)
    return [(sum(len(d["base"]) for d in w), sum(len(d["edges"]) for d in w), max(d["ncols"] for d in w)) for w in ws]


# ---- batches ----
@lru_cache(maxsize=None)
def batch_fill():
    """batch 1, the in-kernel fill route: 12 windows of 1 .. 3 components, 2 .. 8 haplotypes of 30 .. 380 bases (below the 400
    bases of the banded route); window 3 holds one-base haplotypes, window 5 an ALT that is the REF but for its last base"""
    rng = np.random.default_rng(8101)
    windows = []
    for w in range(12):
        comps = []
        for c in range(1 + w % 3):
            haps = pxc.random_component(rng, lo=30, hi=380, min_haps=2, max_haps=8)
            comps.append((haps, ANCHOR + 1000 * c))
        windows.append(comps)
    ref40 = rand_dna(rng, 40)
    windows[3] = [([b"A", b"C"], ANCHOR), ([ref40, b"T"], ANCHOR + 1000), ([b"G", b"G", ref40[:7]], ANCHOR + 2000)]
    r = rand_dna(rng, 211)
    windows[5] = [([r, r[:-1] + bytes([pc.other_base(r[-1])]), r[:100] + r[103:]], ANCHOR)] + windows[5][1:]
    return windows


@lru_cache(maxsize=None)
def batch_band():
    """batch 2, the coroutine route (haplotypes of 400 .. 700 bases: the image is saved and restored between the k_msa
    launches): a 60-base insertion and a 60-base deletion (they start at the 256-column tier), and in window 1 a third
    haplotype of the REF's length with an 80-base insertion at 120 and an 80-base deletion 300 bases on -- it starts at the
    128-column tier and walks 80 columns off the backbone in between: the tier fails and the alignment is redone at 256"""
    rng = np.random.default_rng(8102)
    windows = []
    for w in range(4):
        n = 460 + 60 * w
        r = rand_dna(rng, n)
        haps = [r, r[:150] + rand_dna(rng, 60) + r[150:], r[:250] + r[310:], pxc.mutated(rng, r, 3, 0, 0)]
        if w == 1:
            haps[2] = r[:120] + rand_dna(rng, 80) + r[120:340] + r[420:]
        haps = [h[:700] for h in haps]
        comps = [(haps, ANCHOR)]
        if w == 2:
            comps.append((pxc.random_component(rng, lo=430, hi=640, min_haps=3, max_haps=4), ANCHOR + 2000))
        windows.append(comps)
    return windows


def run(windows, monkeypatch=None, env=None, retry=0, caps=None, params=None, export=True):
    """-> (asm, var, px) of Engine.msa_graph on the hand-made windows (export=False: Engine.msa, px None)"""
    from lancet2_amd.engine import Engine
    p = params or capi.default_params(**SMALL)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    n = len(windows)
    asm = handmade_poa_case(p, [list(c) for c in windows])
    arrs, n2, nr = synth.make_config_batch("C1", n, first_index=77)
    assert n2 == n
    if caps is None:
        nd = needs(windows)
        caps = tuple(max(x[i] for x in nd) for i in range(3))
    eng = Engine(p)
    try:
        if retry:
            eng.set_poa_retry(1)
        if not export:
            return asm, eng.msa(arrs, n, nr, asm), None
        var, px = eng.msa_graph(arrs, n, nr, asm, max_pnodes=caps[0], max_pedges=caps[1], max_cols=caps[2])
        px["last"] = eng.last_poa_export()
    finally:
        eng.close()
    return asm, var, px


def same_vars(got, want, asm_got, asm_want, p=None):
    """the variant arrays of two calls are equal byte for byte in everything a call defines: win_nvars, the whole rows of the
    variants a window reports (unused ALT slots included: they read 0) and the allele bytes those rows point at"""
    p = p or capi.default_params(**SMALL)
    n = len(want["win_nvars"])
    assert np.array_equal(asm_got["win_status"], asm_want["win_status"])
    assert np.array_equal(got["win_nvars"], want["win_nvars"])
    MV, MP = p.max_vars, p.max_allele_bytes
    for w in range(n):
        nv = int(want["win_nvars"][w])
        used = 0
        for k in VAR_KEYS:
            if k in ("win_nvars", "allele_pool"):
                continue
            width = len(want[k]) // (n * MV)
            g, x = got[k][w * MV * width:(w * MV + nv) * width], want[k][w * MV * width:(w * MV + nv) * width]
            assert np.array_equal(g, x), (w, k)
        for v in range(w * MV, w * MV + nv):
            used = max(used, int(want["var_ref_off"][v]) + int(want["var_ref_len"][v]))
            for a in range(int(want["var_nalts"][v])):
                used = max(used, int(want["alt_off"][v * p.max_alts + a]) + int(want["alt_len"][v * p.max_alts + a]))
        assert np.array_equal(got["allele_pool"][w * MP:w * MP + used], want["allele_pool"][w * MP:w * MP + used]), w


def check_window(p, px, asm, w, want):
    """window w of the export equals the restatement's components `want`"""
    MC = p.max_comps
    assert int(px["win_pstatus"][w]) == 0 and not int(asm["win_status"][w]) & capi.MA_W_VAR_OVERFLOW, w
    n0 = e0 = 0
    for c, d in enumerate(want):
        ci = w * MC + c
        got = ref.from_export(px, p, w, c, asm)
        assert (int(px["comp_pnode0"][ci]), int(px["comp_npnodes"][ci])) == (n0, len(d["base"])), (w, c)
        assert (int(px["comp_pedge0"][ci]), int(px["comp_npedges"][ci])) == (e0, len(d["edges"])), (w, c)
        for k in CMP_KEYS:
            assert got[k] == d[k], (w, c, k)
        n0 += len(d["base"])
        e0 += len(d["edges"])
    for c in range(len(want), MC):
        assert not any(int(px[k][w * MC + c]) for k in ("comp_pnode0", "comp_npnodes", "comp_pedge0", "comp_npedges", "comp_ncols")), (w, c)
    assert (int(px["win_npnodes"][w]), int(px["win_npedges"][w]), int(px["win_ncols"][w])) == (n0, e0, max(d["ncols"] for d in want)), w


def check_all(p, px, asm, windows, skip=()):
    want = want_windows(windows)
    for w in range(len(windows)):
        if w not in skip:
            check_window(p, px, asm, w, want[w])


COUNT_KEYS = ("win_pstatus", "win_npnodes", "win_npedges", "win_ncols", "comp_pnode0", "comp_npnodes", "comp_pedge0", "comp_npedges",
              "comp_ncols")


def same_export(p, a, b, asm):
    """two exports of one batch hold the same counts and, for every component of every unflagged window, the same rows (what
    lies beyond a window's rows is not defined)"""
    for k in COUNT_KEYS:
        assert np.array_equal(a[k], b[k]), k
    for w in range(len(a["win_pstatus"])):
        if int(a["win_pstatus"][w]) or int(asm["win_status"][w]) & capi.MA_W_VAR_OVERFLOW:
            continue
        for c in range(int(asm["win_ncomp"][w])):
            assert ref.from_export(a, p, w, c, asm) == ref.from_export(b, p, w, c, asm), (w, c)


@lru_cache(maxsize=None)
def default_run(which):
    """the exporting call on batch 1 / 2 with no switch set, computed once; callers do not write to it"""
    windows = batch_fill() if which == "fill" else batch_band()
    asm, var, px = run(windows)
    for d in (asm, var, px):
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return windows, asm, var, px


# ---- 1, 2: the two fill routes ----
def test_in_kernel_fill_route():
    windows, asm, var, px = default_run("fill")
    p = capi.default_params(**SMALL)
    assert len(windows) == 12 and all(1 <= len(c) <= 3 for c in windows)
    assert all(len(h) < 400 for comps in windows for haps, _ in comps for h in haps)
    check_all(p, px, asm, windows)
    asm2, var2, _ = run(windows, export=False)
    same_vars(var, var2, asm, asm2)
    assert px["last"] == dict(first=12, lab32=0, retry_width=0, retry_capacity=0)
    # the one-base components: a ring of two letters in one column, and paths of one node that only sequences() knows
    d = ref.from_export(px, p, 3, 0, asm)
    assert d["rows"] == [b"A", b"C"] and d["edges"] == [] and d["seq_first"] == [0, 1] and d["haps"] == [1, 2]


def test_coroutine_route(monkeypatch, capfd):
    windows = batch_band()
    assert all(400 <= len(h) <= 700 for comps in windows for haps, _ in comps for h in haps)
    # (MA_POA_MIN_PENDING=1: every banded fill goes through k_msa_band, however few windows wait for one)
    asm, var, px = run(windows, monkeypatch, {"MA_VERBOSE": "1", "MA_POA_MIN_PENDING": "1"})
    err = capfd.readouterr().err
    failed = [tuple(map(int, m)) for m in re.findall(r"failed certificates = (\d+)/(\d+)/(\d+)", err)]
    fills = [tuple(map(int, m)) for m in re.findall(r"fills 64/128/256 = (\d+)/(\d+)/(\d+)", err)]
    print(err)
    assert sum(f[2] for f in fills) >= 8, "the insertions and deletions start at the 256-column tier, in k_msa_band"
    assert sum(f[1] for f in failed) >= 1, "window 1's third haplotype fails the 128-column tier"
    p = capi.default_params(**SMALL)
    check_all(p, px, asm, windows)
    _, asm0, var0, px0 = default_run("band")
    check_all(p, px0, asm0, windows)
    same_export(p, px, px0, asm)
    asm2, var2, _ = run(windows, export=False)
    same_vars(var, var2, asm, asm2)
    same_vars(var0, var2, asm0, asm2)


# ---- 3: route switches ----
@pytest.mark.parametrize("switch", tuple(SWITCHES))
def test_route_switches_give_an_identical_export(switch, monkeypatch):
    for which in ("fill", "band"):
        windows, asm0, var0, px0 = default_run(which)
        asm, var, px = run(windows, monkeypatch, SWITCHES[switch])
        same_export(capi.default_params(**SMALL), px, px0, asm)
        same_vars(var, var0, asm, asm0)
        if switch == "lab32":
            assert px["last"]["lab32"] == len(windows) and px["last"]["first"] == 0


# ---- 4: the LAB32 pass beside 16-bit windows ----
def test_wide_components_take_the_lab32_pass():
    rng = np.random.default_rng(8104)
    r = rand_dna(rng, 200)
    wide = [r] + [pxc.mutated(rng, r, 2, i % 2, (i + 1) % 2, max_indel=5)[:200] for i in range(16)]
    r2 = rand_dna(rng, 200)
    wide2 = [r2] + [pxc.mutated(rng, r2, 1 + i % 3, 0, i % 2, max_indel=4) for i in range(16)]
    narrow = pxc.random_component(rng, lo=100, hi=200, min_haps=3, max_haps=3)
    assert len(wide) == len(wide2) == 17
    windows = [batch_fill()[0], [(wide, ANCHOR)], batch_fill()[1], [(narrow, ANCHOR), (wide2, ANCHOR + 1000)], batch_fill()[2]]
    asm, var, px = run(windows)
    p = capi.default_params(**SMALL)
    check_all(p, px, asm, windows)
    assert px["last"] == dict(first=3, lab32=2, retry_width=0, retry_capacity=0)
    d = ref.from_export(px, p, 3, 1, asm)
    assert max(d["haps"]) >> 16, "labels beyond bit 15 are exported"
    asm2, var2, _ = run(windows, export=False)
    same_vars(var, var2, asm, asm2)


# ---- 5: retry passes ----
@lru_cache(maxsize=None)
def retry_windows():
    """tests/poa_retry_cases.py's inputs between ordinary windows: deletion fans of 1 .. 4 and 1 .. 5 bases from one base (five
    and six edges out of one node: the width pass) and eight 60-base insertions on 1000 bases (480 new nodes: the capacity pass)"""
    import poa_retry_cases as prc
    ws = [prc._plain("retry_plain_a", 8500), prc._out_degree(4, 6004), prc._plain("retry_plain_b", 8501), prc._out_degree(5, 6005),
          prc._plain("retry_plain_c", 8502), prc._insertions("ins_8x60", 8, 6202), prc._plain("retry_plain_d", 8503, 900)]
    return [[(c.haps(), c.anchor) for c in w.comps] for w in ws]


RETRIED = (1, 3, 5)
RETRY_PARAMS = dict(SMALL, max_haps=16)


def test_retried_windows_export_the_graph_of_the_retry_pass():
    windows = retry_windows()
    p = capi.default_params(**RETRY_PARAMS)
    asm, var, px = run(windows, retry=1, params=p)
    assert not asm["win_status"].any()
    check_all(p, px, asm, windows)
    assert px["last"] == dict(first=7, lab32=0, retry_width=2, retry_capacity=1)
    fan = ref.from_export(px, p, 1, 0, asm)
    assert max(sum(1 for t, _, _ in fan["edges"] if t == v) for v in range(len(fan["base"]))) == 5
    fan = ref.from_export(px, p, 3, 0, asm)
    assert max(sum(1 for t, _, _ in fan["edges"] if t == v) for v in range(len(fan["base"]))) == 6
    assert int(px["comp_npnodes"][5 * p.max_comps]) == 1000 + 480
    asm2, var2, _ = run(windows, retry=1, params=p, export=False)
    same_vars(var, var2, asm, asm2, p)


def test_without_the_retry_the_flagged_windows_stay_inside_the_caps():
    windows = retry_windows()
    p = capi.default_params(**RETRY_PARAMS)
    nd = needs(windows)
    caps = tuple(max(x[i] for w, x in enumerate(nd) if w not in RETRIED) for i in range(3))
    asm, var, px = run(windows, retry=0, params=p, caps=caps)
    for w in range(len(windows)):
        assert int(asm["win_status"][w]) == (capi.MA_W_VAR_OVERFLOW if w in RETRIED else 0), w
    check_all(p, px, asm, windows, skip=RETRIED)
    asm2, var2, _ = run(windows, retry=0, params=p, export=False)
    same_vars(var, var2, asm, asm2, p)


# ---- 6: caps ----
CAP_NAMES = ("max_pnodes", "max_pedges", "max_cols")
CAP_BITS = (capi.MA_P_NODE_OVERFLOW, capi.MA_P_EDGE_OVERFLOW, capi.MA_P_COL_OVERFLOW)
CAP_NEEDS = ("win_npnodes", "win_npedges", "win_ncols")


@pytest.mark.parametrize("which", range(3))
def test_cap_at_exact_fit_and_one_under(which):
    windows, asm0, var0, px0 = default_run("fill")
    p = capi.default_params(**SMALL)
    nd = needs(windows)
    top = max(x[which] for x in nd)
    neediest = [w for w, x in enumerate(nd) if x[which] == top]
    assert len(neediest) == 1
    roomy = [2 * max(x[i] for x in nd) for i in range(3)]
    # exact fit: everything is written
    caps = list(roomy)
    caps[which] = top
    asm, var, px = run(windows, caps=tuple(caps))
    assert not px["win_pstatus"].any()
    check_all(p, px, asm, windows)
    # one under: that window alone is flagged and reports its need
    caps[which] = top - 1
    asm, var, px = run(windows, caps=tuple(caps))
    for w in range(len(windows)):
        assert int(px["win_pstatus"][w]) == (CAP_BITS[which] if w == neediest[0] else 0), w
        for i in range(3):
            assert int(px[CAP_NEEDS[i]][w]) == nd[w][i], (w, i)
    check_all(p, px, asm, windows, skip=neediest)
    same_vars(var, var0, asm, asm0)


def test_device_arrays_keep_their_guards():
    """MA_MEM_DEVICE, every export array exactly sized at the batch's exact-fit caps with 256 bytes of junk in front of it and
    behind it: the junk comes back untouched and the arrays are those of the host call"""
    from harness import DeviceArena
    from lancet2_amd.engine import Engine
    GUARD, JUNK = 256, 0x5A
    windows, asm0, var0, px0 = default_run("fill")
    p = capi.default_params(**SMALL)
    n = len(windows)
    caps = tuple(px0[k] for k in CAP_NAMES)
    asm = handmade_poa_case(p, [list(c) for c in windows])
    arrs, _, nr = synth.make_config_batch("C1", n, first_index=77)
    xspec, vspec = capi.poa_out_spec(p, n, *caps), capi.var_out_spec(p, n)
    eng = Engine(p, memspace=capi.MA_MEM_DEVICE)
    arena = DeviceArena()
    try:
        b = capi.make_batch_struct({k: arena.upload(v) for k, v in arrs.items()}, n, nr)
        a = capi.fill_struct(capi.AsmOut, {k: arena.upload(v) for k, v in asm.items()})
        vp = {k: arena.upload(np.zeros(int(sz), dt)) for k, (dt, sz) in vspec.items()}
        xp = {k: arena.upload_unaligned(np.full(int(sz), JUNK, dt), shift=0, guard=GUARD, junk=JUNK) for k, (dt, sz) in xspec.items()}
        eng.msa_graph_device(b, a, capi.fill_struct(capi.VarOut, vp), capi.make_poa_struct(xp, *caps))
        eng.synchronize()
        got = {k: arena.download(xp[k], dt, sz) for k, (dt, sz) in xspec.items()}
        gotv = {k: arena.download(vp[k], dt, sz) for k, (dt, sz) in vspec.items()}
        for k, (dt, sz) in xspec.items():
            nbytes = int(sz) * np.dtype(dt).itemsize
            front, behind = arena.download(xp[k] - GUARD, np.uint8, GUARD), arena.download(xp[k] + nbytes, np.uint8, GUARD)
            assert (front == JUNK).all() and (behind == JUNK).all(), f"the guard of {k} changed"
    finally:
        eng.close()
        arena.close()
    got.update(zip(CAP_NAMES, caps))
    check_all(p, got, asm0, windows)
    same_vars(gotv, var0, asm0, asm0)


def test_argument_errors_and_the_plain_call():
    from lancet2_amd.engine import Engine
    windows = batch_fill()[:2]
    p = capi.default_params(**SMALL)
    n = len(windows)
    asm = handmade_poa_case(p, [list(c) for c in windows])
    arrs, _, nr = synth.make_config_batch("C1", n, first_index=77)
    eng = Engine(p)
    try:
        b = capi.make_batch_struct(arrs, n, nr)
        a = capi.fill_struct(capi.AsmOut, asm)
        var = capi.alloc_host(capi.var_out_spec(p, n))
        v = capi.fill_struct(capi.VarOut, var)
        px = capi.alloc_host(capi.poa_out_spec(p, n, 4096, 8192, 1024))
        for missing in px:
            x = capi.make_poa_struct({k: v2 for k, v2 in px.items() if k != missing}, 4096, 8192, 1024)
            assert eng.lib.ma_msa_graph_batch(eng.h, C.byref(b), C.byref(a), C.byref(v), C.byref(x)) == -1, missing
        for i in range(3):
            caps = [4096, 8192, 1024]
            caps[i] = 0
            x = capi.make_poa_struct(px, *caps)
            assert eng.lib.ma_msa_graph_batch(eng.h, C.byref(b), C.byref(a), C.byref(v), C.byref(x)) == -5, i
        eng.msa_graph_device(b, a, v, capi.make_poa_struct(px, 4096, 8192, 1024))
        assert eng.last_poa_export()["first"] == n
        first = {k: np.array(x, copy=True) for k, x in var.items()}
        eng.msa_graph_device(b, a, v, None)
        assert eng.last_poa_export() == dict(first=0, lab32=0, retry_width=0, retry_capacity=0)
        same_vars(var, first, asm, asm)
    finally:
        eng.close()


# ---- 7: from real assembly ----
def test_export_from_the_engines_own_assembly():
    from lancet2_amd.engine import Engine
    p = capi.default_params(min_k=25, max_k=25)
    arrs, n, nr = synth.make_config_batch("C2", 12, first_index=300)
    eng = Engine(p)
    try:
        asm = eng.assemble(arrs, n, nr)
        asm_plain = {k: np.array(v, copy=True) for k, v in asm.items()}
        want_var = eng.msa(arrs, n, nr, asm_plain)  # the default route: k_poa
        MC, MH, ML = p.max_comps, p.max_haps, p.max_hap_len
        windows = []
        for w in range(n):
            comps = []
            for c in range(int(asm["win_ncomp"][w])):
                ci = w * MC + c
                h0, nh = int(asm["comp_hap0"][ci]), int(asm["comp_nhaps"][ci])
                comps.append(([bytes(asm["hap_bases"][(w * MH + h0 + h) * ML:(w * MH + h0 + h) * ML + int(asm["hap_len"][w * MH + h0 + h])])
                               for h in range(nh)], int(asm["comp_anchor"][ci])))
            windows.append(comps)
        live = [w for w in range(n) if windows[w] and not int(asm["win_status"][w]) & (capi.MA_W_NO_HAPLOTYPE | capi.MA_W_LEN_OVERFLOW)]
        assert len(live) >= 6
        nd = needs([windows[w] for w in live])
        caps = tuple(max(x[i] for x in nd) for i in range(3))
        var, px = eng.msa_graph(arrs, n, nr, asm, max_pnodes=caps[0], max_pedges=caps[1], max_cols=caps[2])
        assert eng.last_poa_export()["first"] == len(live)
        same_vars(var, want_var, asm, asm_plain, p)
        want = want_windows([windows[w] for w in live])
        for i, w in enumerate(live):
            check_window(p, px, asm, w, want[i])
        for w in set(range(n)) - set(live):
            assert not any(int(px[k][w]) for k in ("win_pstatus", "win_npnodes", "win_npedges", "win_ncols")), w
        # px = NULL through the new entry point is ma_msa_batch
        asm_null = {k: np.array(v, copy=True) for k, v in asm_plain.items()}
        var_null = capi.alloc_host(capi.var_out_spec(p, n))
        eng.msa_graph_device(capi.make_batch_struct(arrs, n, nr), capi.fill_struct(capi.AsmOut, asm_null),
                             capi.fill_struct(capi.VarOut, var_null), None)
        same_vars(var_null, want_var, asm_null, asm_plain, p)
        assert not any(eng.last_poa_export().values())
    finally:
        eng.close()


# ---- 8: more than one chunk ----
def test_export_is_indexed_by_the_global_window_over_several_chunks(monkeypatch, capfd):
    """25 windows -- batch 1 twice and one window with a 2400-base haplotype -- under MA_WS_GB=1: on the host-counted route a
    window's areas take about 54 MB at that length, so the 1 GB budget holds 19 windows per chunk and the batch runs as two
    chunks (19 + 6).  The export equals that of the same batch in one chunk."""
    rng = np.random.default_rng(8108)
    r = rand_dna(rng, 2400)
    long_w = [([r, pxc.mutated(rng, r, 4, 0, 0), r[:1200] + r[1230:]], ANCHOR)]
    windows = batch_fill() + [long_w] + batch_fill()
    p = capi.default_params(**dict(SMALL, max_hap_len=4096))
    asm1, var1, px1 = run(windows, params=p)
    capfd.readouterr()
    asm, var, px = run(windows, monkeypatch, {"MA_WS_GB": "1", "MA_VERBOSE": "1"}, params=p)
    err = capfd.readouterr().err
    chunks = [int(x) for x in re.findall(r"msa: 25 windows.*chunks of (\d+)", err)]
    assert chunks and max(chunks) < 25, err
    same_export(p, px, px1, asm)
    same_vars(var, var1, asm, asm1, p)
    check_all(p, px, asm, windows)


# ---- 9: the driver ----
def test_driver_writes_a_gfa_and_a_fasta_per_component(tmp_path):
    """--out-msa-dir on the fixture of tests/test_pipeline_host.py: the VCF is the one of a run without the flag; every
    component of every assembled window has its .gfa and its .fasta, and each is the text the restatement renders from the
    haplotypes Engine.assemble returns for the batches the driver flattened (--dump); --out-graphs-dir alone still writes
    nothing but .dot files."""
    import os
    import subprocess
    from lancet2_amd.engine import Engine
    from test_pipeline_host import driver, write_fixture
    exe = driver(tmp_path)
    write_fixture(str(tmp_path))
    for d in ("msa", "graphs", "dump"):
        (tmp_path / d).mkdir()
    common = [exe, "--reference", str(tmp_path / "ref.fa"), "--normal", str(tmp_path / "normal.sam"), "--tumor", str(tmp_path / "tumor.sam"),
              "--region", "chr1:1-6000", "--min-kmer", "25", "--max-kmer", "25", "--batch-windows", "3"]
    r0 = subprocess.run(common + ["--out-vcf", str(tmp_path / "plain.vcf"), "--out-graphs-dir", str(tmp_path / "graphs")],
                        capture_output=True, text=True)
    assert r0.returncode == 0, r0.stderr
    assert os.listdir(tmp_path / "graphs") and all(f.endswith(".dot") for f in os.listdir(tmp_path / "graphs"))
    assert "MSA files" not in r0.stderr
    r1 = subprocess.run(common + ["--out-vcf", str(tmp_path / "msa.vcf"), "--out-msa-dir", str(tmp_path / "msa"), "--dump", str(tmp_path / "dump")],
                        capture_output=True, text=True)
    assert r1.returncode == 0, r1.stderr
    body = lambda path: [ln for ln in open(path).read().splitlines() if not ln.startswith("##commandLine=")]  # noqa: E731
    assert body(tmp_path / "plain.vcf") == body(tmp_path / "msa.vcf")
    r2 = subprocess.run(common + ["--packed-reads", "--out-msa-dir", str(tmp_path / "msa")], capture_output=True, text=True)
    assert r2.returncode == 2 and "--out-msa-dir" in r2.stderr
    p = capi.default_params(min_k=25, max_k=25)
    dt = {"u8": np.uint8, "u32": np.uint32, "u64": np.uint64, "i32": np.int32}
    want = {}
    eng = Engine(p)
    try:
        for b in sorted(os.listdir(tmp_path / "dump")):
            arrs = {f.rsplit(".", 1)[0]: np.fromfile(str(tmp_path / "dump" / b / f), dtype=dt[f.rsplit(".", 1)[1]]) for f in os.listdir(tmp_path / "dump" / b)}
            wins = arrs.pop("windows").reshape(-1, 4)
            n, nr = len(wins), len(arrs["read_qname_id"])
            asm = eng.assemble(arrs, n, nr)
            MC, MH, ML = p.max_comps, p.max_haps, p.max_hap_len
            for w in range(n):
                for c in range(int(asm["win_ncomp"][w])):
                    h0, nh = int(asm["comp_hap0"][w * MC + c]), int(asm["comp_nhaps"][w * MC + c])
                    haps = [bytes(asm["hap_bases"][(w * MH + h0 + h) * ML:(w * MH + h0 + h) * ML + int(asm["hap_len"][w * MH + h0 + h])]) for h in range(nh)]
                    d = want_component(tuple(haps))
                    stem = f"msa__chr1_{int(wins[w, 1])}_{int(wins[w, 2])}__c{c}"
                    want[stem + ".gfa"] = ref.gfa_text(d)
                    want[stem + ".fasta"] = ref.fasta_text(d)
    finally:
        eng.close()
    files = sorted(os.listdir(tmp_path / "msa"))
    assert files == sorted(want) and len(files) >= 2 * int(re.search(r"(\d+) assembled", r1.stderr).group(1))
    for f in files:
        assert open(tmp_path / "msa" / f).read() == want[f], f
    assert f"{len(files)} MSA files written" in r1.stderr, r1.stderr
