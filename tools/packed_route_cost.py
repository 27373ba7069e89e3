"""Developer tool: what packed read input buys the host route.
C3 workload (60x tumour / 30x normal), k = 25, MA_MEM_HOST, page-locked input arrays, ma_prefetch_*_batch of the next batch
before every call; two batches in turn.  One process, the routes alternating, the median of five rounds each: submitted
windows/s of the ASCII call and of the packed call (4-bit bases, 4-bit qualities binned to 8 levels; the ASCII call gets
the same binned qualities), host-to-device bytes per window of both counted from the array sizes, and k_unpack_reads' time.
--baseline-lib PATH: the ASCII route of another build of the library (the parent commit's) in the same alternation.
usage: python tools/packed_route_cost.py [windows] [--baseline-lib PATH] [--calls N]"""
import ctypes as C
import importlib.util
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lancet2_amd import capi, synth  # noqa: E402
from lancet2_amd.engine import Engine  # noqa: E402

args = sys.argv[1:]
baseline = args[args.index("--baseline-lib") + 1] if "--baseline-lib" in args else None
calls = int(args[args.index("--calls") + 1]) if "--calls" in args else 6
n_want = int(args[0]) if args and args[0].isdigit() else 8192
STRUCTS = (capi.GateOut, capi.AsmOut, capi.VarOut, capi.GenoOut)


def hip_runtime():
    path = "libamdhip64.so"
    spec = importlib.util.find_spec("torch")
    if spec is not None and spec.submodule_search_locations:
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            path = cand
    hip = C.CDLL(path, mode=C.RTLD_GLOBAL)
    hip.hipHostRegister.argtypes = [C.c_void_p, C.c_size_t, C.c_uint]
    return hip


def pin(hip, arrays):
    for a in arrays:
        if isinstance(a, np.ndarray) and a.nbytes:
            rc = hip.hipHostRegister(a.ctypes.data, a.nbytes, 0)
            assert rc == 0, f"hipHostRegister: {rc}"


params = capi.default_params(min_k=25, max_k=25)
arrs, nw, nr = synth.make_config_batch("C3", 64, first_index=0)
arrs, nw, nr = synth.tile_batch(arrs, nw, nr, max(1, n_want // 64))
arrs["read_quals"] = (np.minimum(arrs["read_quals"], 41) // 6 * 6).astype(np.uint8)
total = int(arrs["read_off"][-1])
batches = []
for _ in range(2):  # two batches in distinct memory: one is uploaded while the other computes
    a = {k: v.copy() for k, v in arrs.items()}
    packed, twin = capi.pack_reads(a)
    assert packed["qual_bits"] == 4 and np.array_equal(twin["read_bases"], a["read_bases"])
    batches.append(dict(arrs=a, packed=packed, b=capi.make_batch_struct(a, nw, nr),
                        bp=capi.make_batch_struct(capi.packed_batch_arrays(a), nw, nr), pk=capi.make_packed_struct(packed)))

other = sum(arrs[k].nbytes for k in ("ref_off", "read_win_off", "read_off", "read_qname_id", "read_sample", "read_flags", "read_hint"))
other += int(arrs["ref_off"][-1])
ascii_bytes = other + 2 * total
packed_bytes = other + len(batches[0]["packed"]["bases4"]) + len(batches[0]["packed"]["quals"])

# one engine at a time: an idle context's streams would keep hardware queues from the one that is measured
routes = {"ascii": None, "packed": None}
if baseline:
    routes["parent ascii"] = baseline
hip = hip_runtime()
for bt in batches:
    pin(hip, list(bt["arrs"].values()) + [bt["packed"]["bases4"], bt["packed"]["quals"]])
outs = [capi.alloc_host(s) for s in (capi.gate_out_spec(nw), capi.asm_out_spec(params, nw), capi.var_out_spec(params, nw),
                                     capi.geno_out_spec(params, nw, nr, False))]
structs = [capi.fill_struct(cls, o) for cls, o in zip(STRUCTS, outs)]


def run(eng, route, n_calls):
    """n_calls batches with the next one prefetched -> (windows/s, ms of k_unpack_reads per call, ms of all kernels per call)"""
    eng.timing_control(2)
    is_packed = route == "packed"

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
        if is_packed:
            eng.process_packed_device(bt["bp"], bt["pk"], *structs)
        else:
            eng.process_device(bt["b"], *structs)
    dt = time.perf_counter() - t0
    t = {}
    for k, v in eng.kernel_times():
        t[k] = t.get(k, 0.0) + v
    eng.timing_control(1)
    return n_calls * nw / dt, t.get("k_unpack_reads", 0.0) / n_calls, sum(t.values()) / n_calls


res = {route: [] for route in routes}
for _ in range(5):
    for route, lib_path in routes.items():
        eng = Engine(params, lib_path=lib_path)
        try:
            run(eng, route, 3)  # warm-up: workspaces, staging buffers, worker threads
            res[route].append(run(eng, route, calls))
        finally:
            eng.close()

print(f"windows {nw} reads {nr} read bases {total}; {calls} calls per round, 5 rounds, alternating")
print(f"host-to-device bytes per window: ASCII {ascii_bytes / nw:.0f}, packed {packed_bytes / nw:.0f}")
for route, rs in res.items():
    rates = [r[0] for r in rs]
    print(f"{route}: median {statistics.median(rates) / 1e3:.1f} k windows/s  (rounds {[round(x / 1e3, 1) for x in rates]})")
unpack = statistics.median(r[1] for r in res["packed"])
kernels = statistics.median(r[2] for r in res["packed"])
print(f"k_unpack_reads: {unpack:.3f} ms per call of {nw} windows, summed over the lanes = {100 * unpack / kernels:.2f} % of the "
      f"lanes' kernel time ({kernels:.2f} ms)")
