"""ma_assemble_graph_batch: the pruned graph of every reported component, checked by the independent restatement of
tests/graph_export_ref.py -- comp_cx, comp_cxf, hap_runs and hap_stats recomputed from the exported nodes and edges alone and
compared with the engine's assembly arrays AND with the oracle's -- on every clean route, up the k ladder, with three
samples, at the caps, and through the driver."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import graph_export_ref as ref
from harness import OracleEngine
from lancet2_amd import capi, synth
from lancet2_amd.engine import Engine

pytestmark = pytest.mark.gpu

ROUTE_ENVS = (("compact", {}), ("raw", {"MA_NO_CHAINS": "1"}), ("large classes", {"MA_CHAINS_CAP": "64"}))
UNSPECIFIED = capi.MA_W_TABLE_OVERFLOW | capi.MA_W_HAP_OVERFLOW | capi.MA_W_LEN_OVERFLOW
ASM_KEYS = tuple(capi.asm_out_spec(capi.default_params(), 1))
# what ma_last_kernel_times names after a plain ma_assemble_batch of case 1, taken with the library of the commit before the
# export existed
PLAIN_ASSEMBLE_KERNELS = {"gate_kernel", "k_classify", "k_clean", "k_clean_chains", "k_clean_tail", "k_graph", "k_graph_gen",
                          "k_insert", "k_mm_hbm", "k_mm_q", "k_support"}


def assert_same_assembly(p, a, b, n):
    """Every assembly array equal byte for byte in what the call defines: the staging buffers of the host route are not
    cleared, so hap_bases behind hap_len and hap_runs behind hap_nruns hold whatever the allocation held (the device-route
    test, whose arrays start from zeros, compares every byte)."""
    for k in ASM_KEYS:
        if k not in ("hap_bases", "hap_runs"):
            assert a[k].tobytes() == b[k].tobytes(), k
    ML, MR = p.max_hap_len, p.max_runs
    for h in range(n * p.max_haps):
        ln, nr_ = int(a["hap_len"][h]), int(a["hap_nruns"][h])
        assert a["hap_bases"][h * ML:h * ML + ln].tobytes() == b["hap_bases"][h * ML:h * ML + ln].tobytes(), ("hap_bases", h)
        assert a["hap_runs"][h * MR * 2:(h * MR + nr_) * 2].tobytes() == b["hap_runs"][h * MR * 2:(h * MR + nr_) * 2].tobytes(), ("hap_runs", h)


def _set_env(monkeypatch, env):
    for k in ("MA_NO_CHAINS", "MA_CHAINS_CAP", "MA_NO_SPEC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def run_export(params, arrs, n, nr, caps=(512, 2048, 32768), names=None):
    eng = Engine(params)
    try:
        asm, gr = eng.assemble_graph(arrs, n, nr, *caps)
        routes = eng.last_graph_export()
        if names is not None:
            names.update(k for k, _ in eng.kernel_times())
        return asm, gr, routes
    finally:
        eng.close()


def verify(params, arrs, n, nr, asm, gr, want, min_windows=1):
    """every check of the restatement on every window with a result, against the engine's rows and the oracle's"""
    checked = 0
    for w in range(n):
        if int(asm["win_ncomp"][w]) == 0:
            assert (int(gr["win_nnodes"][w]), int(gr["win_nedges"][w]), int(gr["win_nseq"][w]), int(gr["win_gstatus"][w])) == (0, 0, 0, 0), w
            continue
        if int(asm["win_status"][w]) & UNSPECIFIED:
            continue
        assert int(gr["win_gstatus"][w]) == 0, (w, int(gr["win_nnodes"][w]), int(gr["win_nedges"][w]), int(gr["win_nseq"][w]))
        refb = arrs["ref_bases"][int(arrs["ref_off"][w]):int(arrs["ref_off"][w + 1])]
        k = int(asm["win_k"][w])
        for name, rows in (("engine", asm), ("oracle", want)):
            assert int(rows["win_k"][w]) == k and int(rows["win_ncomp"][w]) == int(asm["win_ncomp"][w]), (name, w)
            bad = ref.check_window(gr, w, rows, params, refb, k)
            assert not bad, f"{name}: " + "\n".join(bad[:10])
        checked += 1
    assert checked >= min_windows, checked
    return checked


@functools.lru_cache(maxsize=None)
def case1():
    params = capi.default_params(min_k=25, max_k=25)
    arrs, n, nr = synth.make_config_batch("C2", 8, first_index=40_000)
    want = OracleEngine(params).assemble(arrs, n, nr)
    return params, arrs, n, nr, want


@functools.lru_cache(maxsize=None)
def case1_roomy():
    params, arrs, n, nr, _ = case1()
    return run_export(params, arrs, n, nr)


def test_compact_route_single_k(monkeypatch):
    _set_env(monkeypatch, {})
    params, arrs, n, nr, want = case1()
    asm, gr, routes = case1_roomy()
    verify(params, arrs, n, nr, asm, gr, want)
    assert routes["tail_small"] > 0, routes
    assert sum(routes.values()) == int((asm["win_ncomp"] > 0).sum()), routes


def test_three_routes_export_the_same_graphs(monkeypatch):
    params = capi.default_params(min_k=25, max_k=25)
    a1, n1, r1 = synth.make_config_batch("C2", 8, first_index=40_000)
    a2, n2, r2 = synth.make_config_batch("C3", 6, first_index=41_000, error_scale=4.0)
    keys = {}
    for arrs, n, nr in ((a1, n1, r1), (a2, n2, r2)):
        want = OracleEngine(params).assemble(arrs, n, nr)
        for route, env in ROUTE_ENVS:
            _set_env(monkeypatch, env)
            asm, gr, routes = run_export(params, arrs, n, nr)
            verify(params, arrs, n, nr, asm, gr, want)
            if route == "raw":
                assert routes["clean"] > 0 and routes["clean"] == sum(routes.values()), routes
            done = [w for w in range(n) if int(asm["win_ncomp"][w]) > 0 and not int(asm["win_status"][w]) & UNSPECIFIED]
            keys.setdefault(id(arrs), {})[route] = {w: ref.graph_key(gr, w, params.num_samples) for w in done}
    for per_route in keys.values():
        assert per_route["compact"] == per_route["raw"] == per_route["large classes"]
        assert per_route["compact"]


def test_large_image_and_long_windows(monkeypatch):
    _set_env(monkeypatch, {})
    params = capi.default_params(min_k=25, max_k=25, max_hap_len=4096)
    arrs, n, nr = synth.make_config_batch("C2", 4, first_index=45_000, W=2501)
    want = OracleEngine(params).assemble(arrs, n, nr)
    asm, gr, routes = run_export(params, arrs, n, nr)
    verify(params, arrs, n, nr, asm, gr, want)
    assert routes["tail_large"] + routes["tail_hbm"] > 0, routes


def test_hbm_tail(monkeypatch):
    """One deep-panel window (500x / 500x): a compact graph of 276 nodes, beyond both LDS images.  Window 91 002: 91 000 and
    91 001 yield no haplotype at k = 25 (nothing is reported, nothing exported), 91 002 is the first that takes this route."""
    _set_env(monkeypatch, {})
    params = capi.default_params(min_k=25, max_k=25)
    arrs, n, nr = synth.make_config_batch("C4", 1, first_index=91_002)
    want = OracleEngine(params).assemble(arrs, n, nr)
    asm, gr, routes = run_export(params, arrs, n, nr, caps=(4096, 16384, 262144))
    print("routes", routes, "needs", int(gr["win_nnodes"][0]), int(gr["win_nedges"][0]), int(gr["win_nseq"][0]))
    verify(params, arrs, n, nr, asm, gr, want)
    assert routes["tail_hbm"] == 1, routes


def test_the_ladder_exports_the_rung_that_reported(monkeypatch):
    _set_env(monkeypatch, {})
    params = capi.default_params()
    arrs, n, nr = synth.make_config_batch("C3", 6, first_index=43_000, tandem_dup=40, softclip_frac=0.03)
    want = OracleEngine(params).assemble(arrs, n, nr)
    asm, gr, routes = run_export(params, arrs, n, nr)
    assert (asm["win_k"] > params.min_k).any()
    verify(params, arrs, n, nr, asm, gr, want)  # (with each window's own win_k; windows without a result export nothing)
    for w in range(n):
        if int(asm["win_status"][w]) & capi.MA_W_NO_HAPLOTYPE and int(asm["win_ncomp"][w]) == 0:
            assert int(gr["win_nnodes"][w]) == 0 and int(gr["win_nedges"][w]) == 0 and int(gr["win_nseq"][w]) == 0
    # the assembly rows are those of the plain call, which takes the last rungs six at a time
    eng = Engine(params)
    try:
        plain = eng.assemble(arrs, n, nr)
    finally:
        eng.close()
    assert_same_assembly(params, plain, asm, n)


def render_window(tmp_path, params, asm, gr, w, comp):
    """RenderComponentDot on window w of an export: its rows written to files, tests/host/graph_dot_render.cpp built with g++
    (as tests/test_pipeline_host.py builds its host programs) and run.  Returns the DOT text."""
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    MN, ME, MS, S = gr["max_nodes"], gr["max_edges"], gr["max_seq_bytes"], params.num_samples
    MC, MH, ML = params.max_comps, params.max_haps, params.max_hap_len
    d = tmp_path / f"rows_w{w}"
    d.mkdir(exist_ok=True)
    per_window = dict(win_gstatus=1, win_nnodes=1, win_nedges=1, win_nseq=1, node_comp=MN, node_seq_off=MN, node_len=MN, node_cnt=MN * S,
                      node_sign=MN, node_label=MN, node_flags=MN, edge_src=ME, edge_dst=ME, edge_kind=ME, seq_pool=MS)
    for k, stride in per_window.items():
        gr[k][w * stride:(w + 1) * stride].tofile(str(d / k))
    for k, stride in dict(comp_hap0=MC, comp_nhaps=MC, hap_len=MH, hap_bases=MH * ML).items():
        asm[k][w * stride:(w + 1) * stride].tofile(str(d / k))
    exe = str(tmp_path / "graph_dot_render")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(capi.REPO, "tests/host/graph_dot_render.cpp"), "-I",
                               os.path.join(capi.REPO, "include"), "-lpthread", "-o", exe])
    r = subprocess.run([exe, str(d), str(comp), str(int(asm["win_k"][w])), str(S), str(MC), str(MH), str(ML), str(MN), str(ME), str(MS)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_three_samples(monkeypatch, tmp_path):
    """node_cnt has three columns, and they sum to the coverage the DOT prints for the node"""
    import re
    _set_env(monkeypatch, {})
    params = capi.default_params(min_k=25, max_k=25, num_samples=3)
    arrs, n, nr = synth.make_config_batch("C5", 4, first_index=44_000)
    want = OracleEngine(params).assemble(arrs, n, nr)
    asm, gr, routes = run_export(params, arrs, n, nr)
    verify(params, arrs, n, nr, asm, gr, want)
    MN = gr["max_nodes"]
    rendered = three_in_use = 0
    for w in range(n):
        nodes = ref.window_nodes(gr, w, 3) if int(asm["win_ncomp"][w]) else {}
        for c in range(int(asm["win_ncomp"][w])):
            dot = render_window(tmp_path, params, asm, gr, w, c)
            printed = {int(m.group(1)): (m.group(2), int(m.group(3)), int(m.group(4)))
                       for m in re.finditer(r"^  n(\d+) \[label=\"[^\"]*\\n\d+:([+-]) len=(\d+) cov=(\d+)\"", dot, re.M)}
            mine = [s for s, nd in nodes.items() if nd.comp == c]
            assert sorted(printed) == sorted(mine) and mine, (w, c)
            for s in mine:
                cols = gr["node_cnt"][(w * MN + s) * 3:(w * MN + s) * 3 + 3]  # the three columns of the node's row, straight from the array
                assert len(cols) == 3 and printed[s] == ("+" if gr["node_sign"][w * MN + s] else "-", len(nodes[s].seq), int(cols.sum())), (w, c, s)
                three_in_use += int((cols > 0).all())
            rendered += 1
    assert rendered > 0 and three_in_use > 0  # (a wrong sample stride would show: nodes with support in all three columns)


def _kernel_names(eng):
    return {k for k, _ in eng.kernel_times()}


def test_identity_host(monkeypatch):
    _set_env(monkeypatch, {})
    params, arrs, n, nr, _ = case1()
    asm, gr, _ = case1_roomy()
    eng = Engine(params)
    try:
        plain = eng.assemble(arrs, n, nr)
        plain_names = _kernel_names(eng)
        asm2, _ = eng.assemble_graph(arrs, n, nr)
        export_names = _kernel_names(eng)
    finally:
        eng.close()
    for k in ASM_KEYS:  # the two calls of ONE engine go through the same staging buffers: every byte
        assert plain[k].tobytes() == asm2[k].tobytes(), k
    assert_same_assembly(params, plain, asm, n)  # (another engine's run: what the call defines, see there)
    assert plain_names == PLAIN_ASSEMBLE_KERNELS
    assert export_names == PLAIN_ASSEMBLE_KERNELS | {"k_graph_export"}


def test_identity_device_route_keeps_its_guards(monkeypatch):
    from harness import DeviceArena
    _set_env(monkeypatch, {})
    params, arrs, n, nr, _ = case1()
    asm, gr, _ = case1_roomy()
    caps = (512, 2048, 32768)
    GUARD, JUNK = 256, 0x5A
    specs = [capi.asm_out_spec(params, n), capi.graph_out_spec(params, n, *caps)]
    eng = Engine(params, memspace=capi.MA_MEM_DEVICE)
    arena = DeviceArena()
    try:
        bs = capi.make_batch_struct({k: arena.upload(v) for k, v in arrs.items()}, n, nr)
        ptrs = [{k: arena.upload_unaligned(np.zeros(int(sz), dt), shift=0, guard=GUARD, junk=JUNK) for k, (dt, sz) in spec.items()} for spec in specs]
        eng.assemble_graph_device(bs, capi.fill_struct(capi.AsmOut, ptrs[0]), capi.make_graph_struct(ptrs[1], *caps))
        eng.synchronize()
        for spec, pt in zip(specs, ptrs):
            for k, (dt, sz) in spec.items():
                nbytes = int(sz) * np.dtype(dt).itemsize
                front, behind = arena.download(pt[k] - GUARD, np.uint8, GUARD), arena.download(pt[k] + nbytes, np.uint8, GUARD)
                assert (front == JUNK).all() and (behind == JUNK).all(), f"the guard of {k} changed"
        dev_asm = {k: arena.download(ptrs[0][k], dt, sz) for k, (dt, sz) in specs[0].items()}
        dev_gr = {k: arena.download(ptrs[1][k], dt, sz) for k, (dt, sz) in specs[1].items()}
        # ... and the plain call on the same device batch
        plain_ptrs = {k: arena.upload(np.zeros(int(sz), dt)) for k, (dt, sz) in specs[0].items()}
        eng.assemble_graph_device(bs, capi.fill_struct(capi.AsmOut, plain_ptrs), None)
        eng.synchronize()
        assert "k_graph_export" not in _kernel_names(eng)
        dev_plain = {k: arena.download(plain_ptrs[k], dt, sz) for k, (dt, sz) in specs[0].items()}
    finally:
        eng.close()
        arena.close()
    for k in ASM_KEYS:  # both device calls wrote into zeroed arrays: every byte
        assert dev_asm[k].tobytes() == dev_plain[k].tobytes(), k
    assert_same_assembly(params, asm, dev_asm, n)  # (the host route's rows: what the call defines, see there)
    dev_gr.update(max_nodes=caps[0], max_edges=caps[1], max_seq_bytes=caps[2])
    for w in range(n):
        assert [int(dev_gr[k][w]) for k in ("win_gstatus", "win_nnodes", "win_nedges", "win_nseq")] == \
               [int(gr[k][w]) for k in ("win_gstatus", "win_nnodes", "win_nedges", "win_nseq")]
        if int(gr["win_nnodes"][w]):
            assert ref.graph_key(dev_gr, w, params.num_samples) == ref.graph_key(gr, w, params.num_samples)


def _rows(gr, w, S, caps):
    """the defined rows of window w, as bytes"""
    MN, ME, MS = caps
    nn, ne, ns = int(gr["win_nnodes"][w]), int(gr["win_nedges"][w]), int(gr["win_nseq"][w])
    out = []
    for k in ("node_comp", "node_seq_off", "node_len", "node_sign", "node_label", "node_flags"):
        out.append(gr[k][w * MN:w * MN + nn].tobytes())
    out.append(gr["node_cnt"][w * MN * S:(w * MN + nn) * S].tobytes())
    for k in ("edge_src", "edge_dst", "edge_kind"):
        out.append(gr[k][w * ME:w * ME + ne].tobytes())
    out.append(gr["seq_pool"][w * MS:w * MS + ns].tobytes())
    return out


@pytest.mark.parametrize("which", (0, 1, 2))
def test_caps_at_the_need_and_one_under(which, monkeypatch):
    _set_env(monkeypatch, {})
    params, arrs, n, nr, _ = case1()
    asm, gr, _ = case1_roomy()
    roomy = (512, 2048, 32768)
    S = params.num_samples
    w0 = next(w for w in range(n) if int(asm["win_ncomp"][w]) > 0)
    needs = (int(gr["win_nnodes"][w0]), int(gr["win_nedges"][w0]), int(gr["win_nseq"][w0]))
    assert min(needs) > 1
    count_keys = ("win_nnodes", "win_nedges", "win_nseq")
    # exact fit of ONE cap: windows that need more of it are flagged, w0 and everything that fits is as in the roomy run
    caps = tuple(needs[i] if i == which else roomy[i] for i in range(3))
    a1, g1, _ = run_export(params, arrs, n, nr, caps)
    assert int(g1["win_gstatus"][w0]) == 0
    for w in range(n):
        assert [int(g1[k][w]) for k in count_keys] == [int(gr[k][w]) for k in count_keys], w
        over = int(gr[count_keys[which]][w]) > needs[which]
        assert int(g1["win_gstatus"][w]) == ((1 << which) if over else 0), w
        if not over:
            assert _rows(g1, w, S, caps) == _rows(gr, w, S, roomy), w
    # one under: exactly that bit on w0, the counts still the need, the others as before
    caps = tuple(needs[i] - 1 if i == which else roomy[i] for i in range(3))
    a2, g2, r2 = run_export(params, arrs, n, nr, caps)
    assert int(g2["win_gstatus"][w0]) == 1 << which
    flagged2 = int((g2["win_gstatus"] != 0).sum())
    assert sum(r2.values()) == int((asm["win_ncomp"] > 0).sum()) - flagged2, r2  # flagged windows are not counted as exported
    for w in range(n):
        assert [int(g2[k][w]) for k in count_keys] == [int(gr[k][w]) for k in count_keys], w
        if int(gr[count_keys[which]][w]) < needs[which]:
            assert int(g2["win_gstatus"][w]) == 0 and _rows(g2, w, S, caps) == _rows(gr, w, S, roomy), w
    assert np.array_equal(a1["win_status"], asm["win_status"]) and np.array_equal(a2["win_status"], asm["win_status"])


def test_arguments(monkeypatch):
    _set_env(monkeypatch, {})
    params, arrs, n, nr, _ = case1()
    asm, _, _ = case1_roomy()
    caps = (512, 2048, 32768)
    eng = Engine(params)
    try:
        out = capi.alloc_host(capi.asm_out_spec(params, n))
        gra = capi.alloc_host(capi.graph_out_spec(params, n, *caps))
        b = capi.make_batch_struct(arrs, n, nr)
        o = capi.fill_struct(capi.AsmOut, out)
        for missing in gra:
            g = capi.make_graph_struct({k: v for k, v in gra.items() if k != missing}, *caps)
            assert eng.lib.ma_assemble_graph_batch(eng.h, C.byref(b), C.byref(o), C.byref(g)) == -1, missing
        for i in range(3):
            g = capi.make_graph_struct(gra, *[0 if j == i else caps[j] for j in range(3)])
            assert eng.lib.ma_assemble_graph_batch(eng.h, C.byref(b), C.byref(o), C.byref(g)) == -5, i
        assert eng.lib.ma_assemble_graph_batch(eng.h, C.byref(b), C.byref(o), None) == 0
        assert_same_assembly(params, out, asm, n)
        empty = capi.make_batch_struct(arrs, 0, 0)
        g = capi.make_graph_struct(gra, *caps)
        assert eng.lib.ma_assemble_graph_batch(eng.h, C.byref(empty), C.byref(o), C.byref(g)) == 0
        assert sum(eng.last_graph_export().values()) == 0
    finally:
        eng.close()


def test_driver_writes_one_dot_file_per_component(tmp_path):
    """--out-graphs-dir on the fixture of tests/test_pipeline_host.py: the VCF is the one of a run without the flag, and every
    record lies in a window that has a graph file."""
    import re
    from test_pipeline_host import driver, write_fixture
    exe = driver(tmp_path)
    write_fixture(str(tmp_path))
    graphs = tmp_path / "graphs"
    graphs.mkdir()
    common = [exe, "--reference", str(tmp_path / "ref.fa"), "--normal", str(tmp_path / "normal.sam"), "--tumor", str(tmp_path / "tumor.sam"),
              "--region", "chr1:1-6000", "--min-kmer", "25", "--max-kmer", "25", "--batch-windows", "3"]
    r0 = subprocess.run(common + ["--out-vcf", str(tmp_path / "plain.vcf")], capture_output=True, text=True)
    assert r0.returncode == 0, r0.stderr
    r1 = subprocess.run(common + ["--out-vcf", str(tmp_path / "graphs.vcf"), "--out-graphs-dir", str(graphs)], capture_output=True, text=True)
    assert r1.returncode == 0, r1.stderr
    body = lambda path: [ln for ln in open(path).read().splitlines() if not ln.startswith("##commandLine=")]  # noqa: E731
    assert body(tmp_path / "plain.vcf") == body(tmp_path / "graphs.vcf")
    files = sorted(os.listdir(graphs))
    spans = []
    for f in files:
        m = re.fullmatch(r"(chr1)_(\d+)_(\d+)__c(\d+)__k25\.dot", f)
        assert m, f
        spans.append((int(m.group(2)), int(m.group(3))))
        text = open(graphs / f).read()
        assert text.startswith('digraph "' + f[:-4] + '" {') and text.rstrip().endswith("}")
        assert text.count('xlabel="source"') == 1 and text.count('xlabel="sink"') == 1 and " -> " in text
    assert f"{len(files)} component graphs written" in r1.stderr, r1.stderr
    assert len(set(files)) == len(files) and len(set(spans)) >= int(re.search(r"(\d+) assembled", r1.stderr).group(1))
    records = [ln.split("\t") for ln in body(tmp_path / "graphs.vcf") if not ln.startswith("#")]
    assert records
    for rec in records:
        assert any(a <= int(rec[1]) <= b for a, b in spans), rec[:2]
    assert "component graphs" not in r0.stderr


def test_a_capacity_retry_pass_takes_the_export_with_it(monkeypatch):
    """A search arena forced too small (MA_ARENA_CAP, as tests/test_gpu_crafted.py forces it): the first pass reports windows
    WITH rows and MA_W_TABLE_OVERFLOW -- walks were found before the arena filled up -- and exports them; the retry passes
    assemble those windows again from scratch.  Their first export is cleared before that, and what the call returns is the
    graph of the pass that reported the window: every window checks out against the oracle's rows, which know no arena."""
    params = capi.default_params(min_k=25, max_k=25)
    arrs, n, nr = synth.make_config_batch("C2", 12, first_index=77_000, snv_rate=1e-2, indel_rate=2e-3)
    want = OracleEngine(params).assemble(arrs, n, nr)
    # (256 records: the arena at which window 9 of this batch finds walks before it runs out; smaller ones leave it without rows)
    _set_env(monkeypatch, {"MA_ARENA_CAP": "256", "MA_NO_CAP_RETRY": "1"})
    a1, g1, r1 = run_export(params, arrs, n, nr)
    first = [w for w in range(n) if int(a1["win_status"][w]) & capi.MA_W_TABLE_OVERFLOW and int(a1["win_ncomp"][w]) > 0
             and int(g1["win_nnodes"][w]) > 0]
    print("flagged with rows after one pass:", first, "routes", r1)
    assert first, "no window is reported with rows and a capacity flag: the test does not reach the retry's clearing"
    monkeypatch.delenv("MA_NO_CAP_RETRY")
    asm, gr, routes = run_export(params, arrs, n, nr)
    assert not (asm["win_status"] & capi.MA_W_TABLE_OVERFLOW).any()
    assert verify(params, arrs, n, nr, asm, gr, want) >= len(first)
    # every pass that exported a window counted it: the windows above twice
    assert sum(routes.values()) >= int((asm["win_ncomp"] > 0).sum()) + len(first), routes
    monkeypatch.delenv("MA_ARENA_CAP")
    _, roomy, _ = run_export(params, arrs, n, nr)
    for w in range(n):
        if int(gr["win_nnodes"][w]):
            assert ref.graph_key(gr, w, params.num_samples) == ref.graph_key(roomy, w, params.num_samples), w
