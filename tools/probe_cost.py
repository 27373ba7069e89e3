"""Developer tool: what ma_assemble_probe_batch costs beside ma_assemble_batch.
C3 workload (60x tumour / 30x normal), 8192 windows, k = 25, host arrays; timing mode 2, the median of three runs each: the
kernels of the stage and the whole call, for the plain call, the probe call with no probe at all and with one probe per window
(an SNV at offset 500).  MA_LIB=<another build's libmicroasm.so> times the plain call of that build (the parent commit's).
usage: python tools/probe_cost.py [windows]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lancet2_amd import capi, synth  # noqa: E402
from lancet2_amd.engine import Engine  # noqa: E402

n_want = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
params = capi.default_params(min_k=25, max_k=25)
arrs, nw, nr = synth.make_config_batch("C3", 64, first_index=0)
arrs, nw, nr = synth.tile_batch(arrs, nw, nr, max(1, n_want // 64))
one = capi.pack_probes([[(500, 1, b"ACGT"[(b"ACGT".index(bytes(arrs["ref_bases"][int(arrs["ref_off"][w]) + 500:][:1])) + 1) % 4:][:1])]
                        for w in range(nw)])
none = capi.pack_probes([[] for _ in range(nw)])
eng = Engine(params)
has_probes = hasattr(eng.lib, "ma_assemble_probe_batch")
try:
    def run(probes):
        eng.timing_control(2)
        t0 = time.perf_counter()
        if probes is None:
            eng.assemble(arrs, nw, nr)
        else:
            eng.assemble_probes(arrs, nw, nr, probes)
        wall = (time.perf_counter() - t0) * 1e3
        t = {}
        for k, v in eng.kernel_times():
            t[k] = t.get(k, 0.0) + v
        return t, wall

    legs = [("ma_assemble_batch", None)] + ([("probe call, no probes", none), ("probe call, one probe per window", one)] if has_probes else [])
    for _, p in legs:
        run(p)  # warm-up: workspaces
    res = {name: [run(p) for _ in range(3)] for name, p in legs}
finally:
    eng.close()
med = statistics.median
print(f"library {capi.LIB_PATH}: windows {nw} reads {nr}")
for name, runs in res.items():
    ks = [sum(t.values()) for t, _ in runs]
    print(f"{name}: kernels {med(ks):.3f} ms (runs {[round(x, 3) for x in ks]}), whole call {med([w for _, w in runs]):.1f} ms")
    for k in ("k_probe_raw", "k_probe_nodes", "k_probe_reads"):
        if any(k in t for t, _ in runs):
            print(f"    {k}: {med([t.get(k, 0.0) for t, _ in runs]):.3f} ms")
