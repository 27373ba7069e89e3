"""Developer tool: what the POA export costs the POA stage.
C3 workload (60x tumour / 30x normal), 8192 windows, k = 25 -- the workload of tools/fmt_stats_cost.py; timing mode 2, the
median of three runs each: ma_msa_batch as it runs by default (k_poa), ma_msa_batch as host-counted rounds (MA_POA_SCHED=0:
the route the exporting call takes) and ma_msa_graph_batch.  Per leg the stage's kernel time and the call's wall time.
--lib PATH: another build of the library (an A/B of the default ma_msa_batch against a build without the export; the
export leg is left out when that build has no ma_msa_graph_batch).
usage: python tools/poa_export_cost.py [windows] [--lib PATH]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lancet2_amd import capi, synth  # noqa: E402
from lancet2_amd.engine import Engine  # noqa: E402

POA = {"k_poa", "k_msa", "k_msa_band"}

args = sys.argv[1:]
lib_path = None
if "--lib" in args:
    i = args.index("--lib")
    lib_path = args[i + 1]
    del args[i:i + 2]
n_want = int(args[0]) if args else 8192
params = capi.default_params(min_k=25, max_k=25)
arrs, nw, nr = synth.make_config_batch("C3", 64, first_index=0)
arrs, nw, nr = synth.tile_batch(arrs, nw, nr, max(1, n_want // 64))
eng = Engine(params, lib_path=lib_path)
try:
    asm = eng.assemble(arrs, nw, nr)
    can_export = hasattr(eng.lib, "ma_msa_graph_batch")
    caps = (2048, 4096, 2048)

    def run(leg):
        if leg == "rounds":
            os.environ["MA_POA_SCHED"] = "0"
        else:
            os.environ.pop("MA_POA_SCHED", None)
        eng.timing_control(2)
        eng.synchronize()
        t0 = time.perf_counter()
        if leg == "export":
            _, px = eng.msa_graph(arrs, nw, nr, asm, max_pnodes=caps[0], max_pedges=caps[1], max_cols=caps[2])
            assert not px["win_pstatus"].any(), "caps too small for this workload"
        else:
            eng.msa(arrs, nw, nr, asm)
        wall = (time.perf_counter() - t0) * 1e3
        os.environ.pop("MA_POA_SCHED", None)
        return sum(v for k, v in eng.kernel_times() if k in POA), wall

    legs = ["default", "rounds"] + (["export"] if can_export else [])
    for leg in legs:
        run(leg)  # warm-up: workspaces, staging
    res = {leg: [run(leg) for _ in range(3)] for leg in legs}
    exported = eng.last_poa_export() if can_export else {}
finally:
    eng.close()
print(f"windows {nw} components {int(asm['win_ncomp'].sum())} library {lib_path or capi.LIB_PATH}")
names = {"default": "ma_msa_batch (default, k_poa)", "rounds": "ma_msa_batch (MA_POA_SCHED=0)", "export": "ma_msa_graph_batch"}
for leg in legs:
    ks, ws = [r[0] for r in res[leg]], [r[1] for r in res[leg]]
    print(f"{names[leg]:32s} kernels {statistics.median(ks):8.3f} ms (runs {[round(x, 3) for x in ks]})  "
          f"call {statistics.median(ws):8.2f} ms (runs {[round(x, 2) for x in ws]})")
if exported:
    print("windows exported per pass:", exported)
