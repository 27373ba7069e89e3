"""The boundary of the POA export (ma_msa_graph_batch, ma_last_poa_export, ma_poa_out_t): the built library exports the two
entry points, the ctypes mirror of the struct sits where a C compiler puts it, and the Python constants are the header's."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from lancet2_amd import capi

HEADER = os.path.join(capi.REPO, "include", "microasm.h")


def test_library_exports_the_poa_export_entry_points():
    assert os.path.exists(capi.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = capi.load_cdll()
    for s in ("ma_msa_graph_batch", "ma_last_poa_export"):
        assert hasattr(lib, s), f"libmicroasm.so does not export {s}"
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+ma_msa_graph_batch\s*\(", txt) and re.search(r"\bint\s+ma_last_poa_export\s*\(", txt)


def test_poa_out_offsets_match_the_compiled_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = capi.PoaOut
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "microasm.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(ma_poa_out_t));']
    for fname, _ in cls._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(ma_poa_out_t, {fname}));')
    lines += ['  printf("bits %u %u %u\\n", (unsigned)MA_P_NODE_OVERFLOW, (unsigned)MA_P_EDGE_OVERFLOW, (unsigned)MA_P_COL_OVERFLOW);',
              '  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    got = [line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    offs = {k: int(v[0]) for k, *v in got if k != "bits"}
    assert offs["size"] == C.sizeof(cls)
    assert len(cls._fields_) == 3 + 18
    for fname, _ in cls._fields_:
        assert offs[fname] == getattr(cls, fname).offset, fname
    bits = [int(x) for x in next(v for k, *v in got if k == "bits")]
    assert bits == [capi.MA_P_NODE_OVERFLOW, capi.MA_P_EDGE_OVERFLOW, capi.MA_P_COL_OVERFLOW] == [1, 2, 4]


def test_poa_out_spec_names_every_array_of_the_struct():
    p = capi.default_params()
    spec = capi.poa_out_spec(p, 3, 10, 20, 30)
    assert list(spec) == [n for n, _ in capi.PoaOut._fields_ if n not in capi.POA_OUT_CAPS]
    assert spec["msa"][1] == 3 * p.max_haps * 30 and spec["pnode_base"][1] == 30 and spec["pedge_haps"][1] == 60
    assert spec["comp_ncols"][1] == 3 * p.max_comps and spec["hap_first"][1] == 3 * p.max_haps
    arrs = capi.alloc_host(spec)
    s = capi.make_poa_struct(arrs, 10, 20, 30)
    assert (s.max_pnodes, s.max_pedges, s.max_cols) == (10, 20, 30)
    for name in spec:
        assert getattr(s, name) == arrs[name].ctypes.data, name
