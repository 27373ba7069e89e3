"""Developer tool: what the annotation costs as a stage of the chained call (ma_process_cx_batch) against the separate
ma_annotate_batch call that a caller had to make before.
C3 workload (60x tumour / 30x normal), k = 25, 8192 windows.  One process, the routes alternating, the median of five rounds:
  1. host route (MA_MEM_HOST, page-locked inputs, the next batch prefetched before every call): submitted windows/s of
     process_stats + annotate (two calls) against process_cx (one call), ASCII and packed reads, and of the call without the
     annotation; host-to-device and device-to-host bytes per window of both, counted from the array sizes
  2. device route (MA_MEM_DEVICE): ms per step of process + annotate against process_cx, and of process alone
  3. k_hap_lq per launch (ma_annotate_batch on the device arrays of 2.), and whether the four annotation arrays of the two
     libraries are byte-identical in the used variant slots
--baseline-lib PATH: another build of the library (the parent commit's) in the same alternation; it has no one-call route.
usage: python tools/annotate_chain_cost.py [windows] [--baseline-lib PATH] [--calls N]"""
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from lancet2_amd import capi, synth  # noqa: E402
from lancet2_amd.engine import Engine  # noqa: E402
from harness import DeviceArena  # noqa: E402  (hipMalloc / hipMemcpy through ctypes)

args = sys.argv[1:]
baseline = args[args.index("--baseline-lib") + 1] if "--baseline-lib" in args else None
calls = int(args[args.index("--calls") + 1]) if "--calls" in args else 6
n_want = int(args[0]) if args and args[0].isdigit() else 8192
ROUNDS = 5
GC = 0.41
OUT_CLASSES = (capi.GateOut, capi.AsmOut, capi.VarOut, capi.GenoOut, capi.FmtOut)

params = capi.default_params(min_k=25, max_k=25)
arrs64, nw64, nr64 = synth.make_config_batch("C3", 64, first_index=0)
arrs64["read_quals"] = (np.minimum(arrs64["read_quals"], 41) // 6 * 6).astype(np.uint8)
reps = max(1, n_want // 64)
arrs, nw, nr = synth.tile_batch(arrs64, nw64, nr64, reps)
total64, total = int(arrs64["read_off"][-1]), int(arrs["read_off"][-1])
packed64, _ = capi.pack_reads(arrs64)
assert packed64["qual_bits"] == 4
if (total64 + nr64) % 2 == 0:  # every copy of the 64 windows starts on a byte boundary of the nibble arrays: they tile too
    half = (total64 + nr64) // 2
    packed = dict(packed64, bases4=np.tile(packed64["bases4"][:half], reps), quals=np.tile(packed64["quals"][:half], reps))
else:
    packed, _ = capi.pack_reads(arrs)
assert len(packed["bases4"]) == (total + nr + 1) // 2

hip_arena = DeviceArena()
hip_arena.hip.hipHostRegister.argtypes = [hip_arena.C.c_void_p, hip_arena.C.c_size_t, hip_arena.C.c_uint]


def pin(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray) and a.nbytes:
            rc = hip_arena.hip.hipHostRegister(a.ctypes.data, a.nbytes, 0)
            assert rc == 0, f"hipHostRegister: {rc}"


batches = []
for _ in range(2):  # two batches in distinct memory: one is uploaded while the other computes
    a = {k: v.copy() for k, v in arrs.items()}
    pk = dict(packed, bases4=packed["bases4"].copy(), quals=packed["quals"].copy())
    pin(list(a.values()) + [pk["bases4"], pk["quals"]])
    batches.append(dict(arrs=a, packed=pk, b=capi.make_batch_struct(a, nw, nr),
                        bp=capi.make_batch_struct(capi.packed_batch_arrays(a), nw, nr), pk=capi.make_packed_struct(pk)))

specs = [capi.gate_out_spec(nw), capi.asm_out_spec(params, nw), capi.var_out_spec(params, nw),
         capi.geno_out_spec(params, nw, nr, False), capi.fmt_out_spec(params, nw)]
cx_spec = capi.cx_out_spec(params, nw)
outs = [capi.alloc_host(s) for s in specs]
structs = [capi.fill_struct(cls, o) for cls, o in zip(OUT_CLASSES, outs)]
cx_host = capi.alloc_host(cx_spec)
cx_struct = capi.fill_struct(capi.CxOut, cx_host)

other = sum(arrs[k].nbytes for k in ("ref_off", "read_win_off", "read_off", "read_qname_id", "read_sample", "read_flags", "read_hint"))
other += int(arrs["ref_off"][-1])
in_ascii, in_packed = other + 2 * total, other + len(packed["bases4"]) + len(packed["quals"])
asm_var_bytes = sum(np.dtype(dt).itemsize * int(sz) for spec in specs[1:3] for dt, sz in spec.values())
cx_bytes = sum(np.dtype(dt).itemsize * int(sz) for dt, sz in cx_spec.values())


# ---- 1. host route --------------------------------------------------------------------------------------------------------
def run_host(eng, is_packed, mode, n_calls):
    """mode: 'two' = process_stats + annotate, 'one' = process_cx, 'none' = process_stats alone -> windows/s"""
    def prefetch(bt):
        if is_packed:
            eng.prefetch_packed(bt["bp"], bt["pk"])
        else:
            eng.prefetch(bt["b"])

    prefetch(batches[0])
    t0 = time.perf_counter()
    for i in range(n_calls):
        bt = batches[i % 2]
        if i + 1 < n_calls:
            prefetch(batches[(i + 1) % 2])
        b, pk = (bt["bp"], bt["pk"]) if is_packed else (bt["b"], None)
        if mode == "one":
            eng.process_cx_device(b, pk, None, *structs, None, cx_struct, gc_frac=GC)
        else:
            if is_packed:
                eng.process_packed_device(b, pk, *structs)
            else:
                eng.process_stats_device(b, *structs)
            if mode == "two":
                eng.annotate_device(bt["b"], structs[1], structs[2], cx_struct, gc_frac=GC)
    return n_calls * nw / (time.perf_counter() - t0)


host_routes = {}
for form in ("ascii", "packed"):
    for mode, label in (("two", "process_stats + annotate"), ("one", "process_cx"), ("none", "process_stats alone")):
        host_routes[f"{form}: {label}"] = (None, form == "packed", mode)
        if baseline and mode != "one":
            host_routes[f"parent {form}: {label}"] = (baseline, form == "packed", mode)
res = {r: [] for r in host_routes}
for _ in range(ROUNDS):
    for route, (lib, is_packed, mode) in host_routes.items():
        eng = Engine(params, lib_path=lib)  # one engine at a time: an idle context's streams would keep hardware queues
        try:
            run_host(eng, is_packed, mode, 3)  # warm-up: workspaces, staging buffers, worker threads
            res[route].append(run_host(eng, is_packed, mode, calls))
        finally:
            eng.close()
used_vars = int(np.minimum(outs[2]["win_nvars"], params.max_vars).sum())
print(f"windows {nw} reads {nr} read bases {total} variants {used_vars}; {calls} calls per round, {ROUNDS} rounds, alternating")
print(f"host route, bytes per window: in ASCII {in_ascii / nw:.0f}, packed {in_packed / nw:.0f}; the separate annotate call "
      f"uploads {asm_var_bytes / nw:.0f} more (assembly + variant arrays at full stride) and downloads {cx_bytes / nw:.0f}; "
      f"the stage of the chain uploads 0 and downloads {80.0 * used_vars / nw:.0f} (80 per used variant slot)")
for route, rs in res.items():
    print(f"host route, {route}: median {statistics.median(rs) / 1e3:.1f} k windows/s  (rounds {[round(x / 1e3, 1) for x in rs]})")

# ---- 2. and 3. device route -----------------------------------------------------------------------------------------------
arena = DeviceArena()
d_batch = capi.make_batch_struct({k: arena.upload(v) for k, v in arrs.items()}, nw, nr)
d_ptrs = [{k: arena.alloc(int(sz) * np.dtype(dt).itemsize) for k, (dt, sz) in spec.items()} for spec in specs[:4]]
d_structs = [capi.fill_struct(cls, p) for cls, p in zip(OUT_CLASSES[:4], d_ptrs)]
d_cx = {name: {k: arena.alloc(int(sz) * np.dtype(dt).itemsize) for k, (dt, sz) in cx_spec.items()} for name in ("this", "parent")}


def run_device(eng, mode, n_calls, cx):
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_calls):
        if mode == "one":
            eng.process_cx_device(d_batch, None, None, *d_structs, None, None, cx, gc_frac=GC)
        else:
            eng.process_device(d_batch, *d_structs)
            if mode == "two":
                eng.annotate_device(d_batch, d_structs[1], d_structs[2], cx, gc_frac=GC)
        eng.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n_calls


dev_routes = {}
for mode, label in (("two", "process + annotate"), ("one", "process_cx"), ("none", "process alone")):
    dev_routes[label] = (None, mode)
    if baseline and mode != "one":
        dev_routes[f"parent {label}"] = (baseline, mode)
dres = {r: [] for r in dev_routes}
hap_lq = {"this": [], "parent": []}
for _ in range(ROUNDS):
    for route, (lib, mode) in dev_routes.items():
        who = "parent" if lib else "this"
        cx = capi.fill_struct(capi.CxOut, d_cx[who])
        eng = Engine(params, memspace=capi.MA_MEM_DEVICE, lib_path=lib)
        try:
            run_device(eng, mode, 3, cx)
            dres[route].append(run_device(eng, mode, calls, cx))
            if mode == "two":  # 3.: the stage call alone on the arrays the chain just wrote, timed by the library's events
                eng.annotate_device(d_batch, d_structs[1], d_structs[2], cx, gc_frac=GC)
                eng.synchronize()
                t = dict(eng.kernel_times())
                hap_lq[who].append((t["k_hap_lq"], t["k_seqcx"]))
        finally:
            eng.close()
for route, rs in dres.items():
    print(f"device route, {route}: median {statistics.median(rs):.2f} ms per step  (rounds {[round(x, 2) for x in rs]})")
for who, ts in hap_lq.items():
    if ts:
        print(f"k_hap_lq, {who} library: median {statistics.median(t[0] for t in ts):.3f} ms per launch of {nw} windows "
              f"(rounds {[round(t[0], 3) for t in ts]}); k_seqcx {statistics.median(t[1] for t in ts):.3f} ms")
if baseline:
    nv = arena.download(d_ptrs[2]["win_nvars"], *specs[2]["win_nvars"])
    used = (np.arange(params.max_vars)[None, :] < nv[:, None]).reshape(-1)
    same = True
    for k, (dt, sz) in cx_spec.items():
        a, b = (arena.download(d_cx[who][k], dt, sz).view(np.uint8).reshape(len(used), -1)[used] for who in ("this", "parent"))
        same = same and np.array_equal(a, b)
    print(f"annotation arrays of the two libraries over {int(used.sum())} used variant slots: identical: {same}")
arena.close()
