"""RenderComponentDot (lancet2_amd/host/pipeline_host.hpp): the DOT rendering of an exported component, on the hand-written
bubble -- tests/host/graph_dot_units.cpp, built with g++ like tests/test_pipeline_host.py builds host_units.cpp."""
import os
import shutil
import subprocess

import pytest

from lancet2_amd import capi

REPO = capi.REPO


def test_graph_dot_units(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "graph_dot_units")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(REPO, "tests/host/graph_dot_units.cpp"), "-I",
                           os.path.join(REPO, "include"), "-lpthread", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "graph dot units ok" in r.stdout, r.stderr
