"""Developer tool: what ma_set_poa_retry costs the POA stage when no window is marked (ma_msa_batch on engine-assembled C3
windows, setting off and on in turn on one context): wall time of the call, median of `reps` calls each, and the counts.
usage: python tools/poa_retry_cost.py [windows=8192] [distinct=256] [reps=7]   (env: MA_LIB)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lancet2_amd import capi, synth  # noqa: E402
from lancet2_amd import engine as E  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
distinct = int(sys.argv[2]) if len(sys.argv) > 2 else 256
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
arrs, nw, nr = synth.make_config_batch("C3", distinct, first_index=10_000)
arrs, nw, nr = synth.tile_batch(arrs, nw, nr, max(1, n // distinct))
eng = E.Engine(capi.default_params(min_k=25, max_k=25))
asm = eng.assemble(arrs, nw, nr)
eng.timing_control(0)
for on in (0, 1):  # warm both settings: workspaces, the cause buffer
    eng.set_poa_retry(on)
    eng.msa(arrs, nw, nr, asm)
times = {0: [], 1: []}
counts = {}
for _ in range(reps):  # alternated, so that drift hits both alike
    for on in (0, 1):
        eng.set_poa_retry(on)
        t0 = time.perf_counter()
        eng.msa(arrs, nw, nr, asm)
        times[on].append((time.perf_counter() - t0) * 1e3)
        counts[on] = eng.last_poa_retry()
eng.close()
med = {on: statistics.median(v) for on, v in times.items()}
print(f"{nw} windows, {reps} calls each, ma_msa_batch wall ms (host arrays in and out included)")
for on in (0, 1):
    print(f"  retry {on}: median {med[on]:.2f}  min {min(times[on]):.2f}  max {max(times[on]):.2f}  counts {counts[on]}")
print(f"  on - off: {med[1] - med[0]:+.2f} ms ({100.0 * (med[1] - med[0]) / med[0]:+.2f} %)")
