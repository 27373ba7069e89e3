"""bench.py's plain run and --dump-outputs: the headline line alone (the rest of the figures are --full's), and the arrays of
the last timed step written as float32 / float64 .npy files -- a fixed seeded sample of windows, at most 64 MB in all,
identical from run to run for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_sample_is_exact_seeded_and_capped(tmp_path):
    import torch
    import bench
    from lancet2_amd import capi
    n = 1000
    lp = capi.default_params(min_k=25, max_k=25)
    specs = (capi.gate_out_spec(n), capi.asm_out_spec(lp, n), capi.var_out_spec(lp, n), capi.geno_out_spec(lp, n, 0, debug=False))
    rng = np.random.default_rng(7)
    out = []
    for spec in specs:
        d = {}
        for key, (dt, sz) in spec.items():
            host = rng.integers(0, 1 << 20, sz).astype(dt) if np.dtype(dt).kind in "iu" else rng.random(sz).astype(dt)
            d[key] = torch.from_numpy(host.view(np.uint8).copy())
        out.append(d)
    ids = [10_000 + 3 * j for j in range(n)]
    written = bench.dump_outputs(str(tmp_path / "a"), lp, n, out, ids)
    bench.dump_outputs(str(tmp_path / "b"), lp, n, out, ids)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted([k + ".npy" for spec in specs for k in spec] + ["window_id.npy"])
    assert written <= bench.DUMP_BYTES and sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 2**20
    wid = np.load(tmp_path / "a" / "window_id.npy")
    rows = (wid - 10_000).astype(np.int64) // 3
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0)  # a sample of distinct windows, in batch order
    for spec, d in zip(specs, out):
        for key, (dt, sz) in spec.items():
            got = np.load(tmp_path / "a" / (key + ".npy"))
            assert got.dtype in (np.float32, np.float64), (key, got.dtype)
            want = d[key].numpy().view(dt).reshape(n, sz // n)[rows]
            assert np.array_equal(got, want.astype(got.dtype)) and np.array_equal(got.astype(dt), want), key
            assert np.array_equal(got, np.load(tmp_path / "b" / (key + ".npy")))


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120, cwd=REPO)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    lines, dirs = [], []
    for rep in range(2):
        d = tmp_path / f"dump{rep}"
        cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
               "--windows", "512", "--distinct", "512", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=REPO)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
        dirs.append(d)
    for out in lines:
        assert out["metric"] == "microassembly windows/sec (whole node)" and out["unit"] == "windows/s"
        assert out["higher_is_better"] is True and out["dtype"] == "u8/i32 (f64 statistics)"
        assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
        assert out["config"]["windows_per_step_per_gpu"] == 512
        assert "roofline" not in out and "cpu_baseline" not in out and "also" not in out  # --full's figures
    assert lines[0]["config"]["assembled_fraction"] == lines[1]["config"]["assembled_fraction"]
    files = sorted(os.listdir(dirs[0]))
    assert "window_id.npy" in files and "var_qual.npy" in files and "hap_bases.npy" in files
    assert files == sorted(os.listdir(dirs[1]))
    assert sum(os.path.getsize(dirs[0] / f) for f in files) <= 64 * 2**20
    for f in files:
        x, y = np.load(dirs[0] / f), np.load(dirs[1] / f)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape
        assert np.array_equal(x, y, equal_nan=True), f
