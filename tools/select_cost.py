"""Developer tool: what ma_select_records_batch costs, beside ma_flatten_records_batch on the same bytes.
C3 workload (60x tumour / 30x normal), 8192 windows; timing mode 2, the median of three runs each: the kernels of the call one
by one, the whole call with host arrays and with device arrays; then the flatten call on the same records (its 7.5 ms are the
yardstick) and on the lists the select call made.
The reads of 64 synthesised windows are encoded as BAM records with NM and MD fields (tests/select_cases.py: the MD string of
the read laid on its window without gaps) and tiled, blob included, to the window count: every window reads its own bytes.
usage: python tools/select_cost.py [windows]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import select_cases  # noqa: E402
import select_ref  # noqa: E402
from harness import DeviceArena  # noqa: E402
from lancet2_amd import capi, synth  # noqa: E402
from lancet2_amd.engine import Engine  # noqa: E402

n_want = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
params = capi.default_params(min_k=25, max_k=25)
arrs, nw, nr = synth.make_config_batch("C3", 64, first_index=0)
one, nw, n_one, win_len = select_cases.records_of_synth(arrs, nw, nr, synth.CONFIGS["C3"]["roles"], np.random.default_rng(1), extras=False)
want = select_ref.select(one, nw, n_one, 2, win_len, max_sample_cov=1000.0, min_anchor_cov=5)
times = max(1, n_want // nw)
n, n_rec = nw * times, n_one * times
blob = one["blob"]
rec = dict(one, blob=np.tile(blob, times),
           rec_off=np.concatenate([one["rec_off"] + np.uint64(t * blob.size) for t in range(times)]),
           rec_len=np.tile(one["rec_len"], times), rec_sample=np.tile(one["rec_sample"], times),
           rec_win_off=np.concatenate([[0]] + [one["rec_win_off"][1:].astype(np.uint64) + t * n_one for t in range(times)]).astype(np.uint32),
           win_chrom=np.tile(one["win_chrom"], times), win_start0=np.tile(one["win_start0"], times))
win_len = np.tile(win_len, times)
total = int(arrs["read_off"][nr]) * times
sel_params = dict(max_sample_cov=1000.0, min_anchor_cov=5, skip_active_region=False)
med = statistics.median
eng = Engine(params)
print(f"library {capi.LIB_PATH}: windows {n} candidates {n_rec} bases {total} blob {rec['blob'].size} bytes; "
      f"of 64 windows {int((want['win_state'] & select_ref.MA_S_LISTED != 0).sum())} listed, "
      f"{int((want['win_state'] & select_ref.MA_S_HOST_BITS != 0).sum())} with a host bit")
try:
    def timed(fn):
        eng.timing_control(2)
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        t = {}
        for k, v in eng.kernel_times():
            t[k] = t.get(k, 0.0) + v
        return t, wall, out

    def report(what, fn):
        timed(fn)  # warm-up: workspaces
        runs = [timed(fn) for _ in range(3)]
        print(f"{what}, host arrays: kernels {med([sum(t.values()) for t, _, _ in runs]):.3f} ms, whole call {med([w for _, w, _ in runs]):.1f} ms")
        for k in sorted({k for t, _, _ in runs for k in t}):
            print(f"    {k}: {med([t.get(k, 0.0) for t, _, _ in runs]):.3f} ms")
        return runs[0][2]

    sel = report("ma_select_records_batch", lambda: eng.select_records(rec, n, n_rec, win_len, **sel_params))
    n_sel = int(sel["n_selected"][0])
    state = sel["win_state"]
    print(f"    selected {n_sel} of {n_rec}; windows listed {int((state & capi.MA_S_LISTED != 0).sum())}, with a host bit "
          f"{int((state & capi.MA_S_HOST_BITS != 0).sum())}, inactive {int((state & capi.MA_S_ACTIVE == 0).sum())}")
    report("ma_flatten_records_batch on the candidates", lambda: eng.flatten_records(rec, n, n_rec, bases_cap=total, n_refs=1))
    lists = dict(rec, rec_off=sel["sel_off"], rec_len=sel["sel_len"], rec_sample=sel["sel_sample"], rec_win_off=sel["sel_win_off"])
    report("ma_flatten_records_batch on the selected lists", lambda: eng.flatten_records(lists, n, n_sel, bases_cap=total, n_refs=1))
    dev = Engine(params, memspace=capi.MA_MEM_DEVICE)
    arena = DeviceArena()
    try:
        ins = {k: arena.upload(np.ascontiguousarray(rec[k], dtype=capi.RECORDS_DTYPES[k])) for k in capi.SELECT_IN_KEYS}
        ins["win_len"] = arena.upload(win_len)
        rs = capi.make_records_struct(dict(ins, n_samples_in=2), n, n_rec, blob_bytes=rec["blob"].size)
        sp = capi.make_select_params(ins["win_len"], **sel_params)
        so = capi.fill_struct(capi.SelectOut, {k: arena.alloc(int(sz) * np.dtype(dt).itemsize + 64) for k, (dt, sz) in capi.select_out_spec(n, n_rec, 2).items()})
        walls = []
        for i in range(4):
            t0 = time.perf_counter()
            dev.select_records_device(rs, sp, so)
            walls.append((time.perf_counter() - t0) * 1e3)
        print(f"ma_select_records_batch, device arrays: whole call {med(walls[1:]):.2f} ms (runs {[round(x, 2) for x in walls[1:]]})")
    finally:
        dev.close()
        arena.close()
finally:
    eng.close()
