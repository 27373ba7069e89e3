"""ma_inflate_blocks_batch / ma_index_records_batch without a GPU: the library exports both, the header declares them and the
state bits capi.py names, and the four structs of capi.py lie as gcc lays out the header's."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from lancet2_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "microasm.h")
STRUCTS = (("ma_bgzf_t", "Bgzf"), ("ma_inflate_out_t", "InflateOut"), ("ma_record_streams_t", "RecordStreams"), ("ma_index_out_t", "IndexOut"))


def test_library_exports_both_calls():
    lib = capi.load_cdll()
    for name in ("ma_inflate_blocks_batch", "ma_index_records_batch"):
        assert getattr(lib, name) is not None


def test_header_declares_the_calls_and_the_bits():
    text = open(HEADER).read()
    assert "int ma_inflate_blocks_batch(ma_ctx_t* ctx, const ma_bgzf_t* in, const ma_inflate_out_t* out);" in text
    assert "int ma_index_records_batch(ma_ctx_t* ctx, const ma_record_streams_t* in, const ma_index_out_t* out);" in text
    for name in ("MA_Z_HEADER", "MA_Z_ISIZE", "MA_Z_DATA", "MA_Z_SHORT", "MA_Z_CRC", "MA_X_BAD_RECORD"):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == getattr(capi, name)
    for kernel in ("k_inf_header", "k_inf_scan", "k_inf_decode", "k_idx_count", "k_idx_scan", "k_idx_fill", "k_idx_fields"):
        assert kernel in text


def test_struct_sizes_and_offsets_match_the_compiled_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "microasm.h"', 'int main(void) {']
    for cname, pyname in STRUCTS:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in getattr(capi, pyname)._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, pyname in STRUCTS:
        cls = getattr(capi, pyname)
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)


def test_out_specs_name_every_array_of_the_structs():
    assert list(capi.inflate_out_spec(3, 10)) == [n for n, _ in capi.InflateOut._fields_ if n != "raw_cap"]
    assert list(capi.index_out_spec(3, 10)) == [n for n, _ in capi.IndexOut._fields_ if n != "rec_cap"]
