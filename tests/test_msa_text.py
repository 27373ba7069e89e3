"""The host shell's GFA and FASTA renderers (lancet2_amd/host/pipeline_host.hpp: RenderComponentGfa, RenderComponentFasta) on
the arrays of ma_poa_out_t, against the texts tests/poa_graph_ref.py renders; and poa_graph_ref's own array layout
(to_export) read back (from_export).  No GPU: the arrays come from the restatement."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import poa_export_cases
import poa_graph_ref as ref
from lancet2_amd import capi

REPO = capi.REPO
KEYS = ("base", "rank", "col", "haps", "edges", "order", "seq_first", "ncols", "rows", "paths")


def windows():
    rng = np.random.default_rng(4242)
    small = [poa_export_cases.random_component(rng, lo=30, hi=90, min_haps=2, max_haps=5) for _ in range(5)]
    return [[small[0]], [small[1], [b"A", b"C"], small[2]], [[b"ATCG", b"AAAAG"], small[3]], [small[4], [b"ACGT", b"AGT", b"T"]]]


def test_array_layout_reads_back():
    p = capi.default_params(max_haps=16)
    ws = windows()
    asm, px = ref.to_export(p, ws, (400, 500, 120))
    for w, comps in enumerate(ws):
        for c, haps in enumerate(comps):
            want, got = ref.component(haps), ref.from_export(px, p, w, c, asm)
            for k in KEYS:
                assert got[k] == want[k], (w, c, k)
    assert px["win_npnodes"].tolist() == [sum(len(ref.component(h)["base"]) for h in comps) for comps in ws]


def test_host_renderers_print_the_restatements_texts(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "msa_text_render")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(REPO, "tests/host/msa_text_render.cpp"), "-I",
                           os.path.join(REPO, "include"), "-lpthread", "-o", exe])
    p = capi.default_params(max_haps=16)
    ws = windows()
    caps = (400, 500, 120)
    asm, px = ref.to_export(p, ws, caps)
    px["win_pstatus"][3] = capi.MA_P_COL_OVERFLOW  # a flagged window renders as nothing
    d = tmp_path / "arrays"
    d.mkdir()
    for k, v in list(asm.items()) + list(px.items()):
        if isinstance(v, np.ndarray):
            v.tofile(str(d / k))
    for w, comps in enumerate(ws):
        for c, haps in enumerate(comps):
            r = subprocess.run([exe, str(d), str(w), str(c), str(p.max_comps), str(p.max_haps), *map(str, caps)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            want = ref.component(haps)
            text = "==\n" if w == 3 else ref.gfa_text(want) + "==\n" + ref.fasta_text(want)
            assert r.stdout == text, (w, c)
