"""Developer tool: what the read-level FORMAT statistics cost the genotype stage.
C3 workload (60x tumour / 30x normal), 8192 windows, k = 25; timing mode 2, the median of three runs each:
the stage's kernel time without and with the statistics, k_evid_stats's own time and the bytes of the per-read record array.
--meta: a third leg with the six statistics over the read metadata as well (ma_genotype_meta_batch; metadata from a fixed seed).
usage: python tools/fmt_stats_cost.py [windows] [--meta]"""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lancet2_amd import capi, synth  # noqa: E402
from lancet2_amd.engine import Engine  # noqa: E402

GENOTYPE = {"k_read_planes", "k_plan", "k_vote", "k_dp_scatter", "k_align_reg", "k_align_tb", "k_align_wave", "k_align_gen",
            "k_tap_records", "k_assign", "k_evidence", "k_qual", "k_evid_stats"}

with_meta = "--meta" in sys.argv[1:]
args = [a for a in sys.argv[1:] if a != "--meta"]
n_want = int(args[0]) if args else 8192
params = capi.default_params(min_k=25, max_k=25)
arrs, nw, nr = synth.make_config_batch("C3", 64, first_index=0)
arrs, nw, nr = synth.tile_batch(arrs, nw, nr, max(1, n_want // 64))
eng = Engine(params)
try:
    _, asm, var, _ = eng.process(arrs, nw, nr)

    rng = np.random.default_rng(1)
    meta = dict(read_mapq=rng.integers(0, 61, nr).astype(np.uint8), read_mflags=rng.integers(0, 4, nr).astype(np.uint8),
                read_isize=rng.integers(-600, 600, nr).astype(np.int32), read_start=rng.integers(0, 1 << 20, nr).astype(np.int32))

    def run(stats):
        eng.timing_control(2)
        if stats == "meta":
            eng.genotype_meta(arrs, meta, nw, nr, asm, var, debug=False)
        elif stats:
            eng.genotype_stats(arrs, nw, nr, asm, var, debug=False)
        else:
            eng.genotype(arrs, nw, nr, asm, var, debug=False)
        t = {}
        for k, v in eng.kernel_times():
            t[k] = t.get(k, 0.0) + v
        return t

    run(True)  # warm-up: workspaces
    off = [run(False) for _ in range(3)]
    on = [run(True) for _ in range(3)]
    if with_meta:
        run("meta")
    both = [run("meta") for _ in range(3)] if with_meta else []
finally:
    eng.close()
stage = lambda t: sum(v for k, v in t.items() if k in GENOTYPE)  # noqa: E731
med = lambda xs: statistics.median(xs)  # noqa: E731
print(f"windows {nw} reads {nr} variants {int(var['win_nvars'].sum())}")
print(f"genotype stage, statistics off: {med([stage(t) for t in off]):.3f} ms  (runs {[round(stage(t), 3) for t in off]})")
print(f"genotype stage, statistics on:  {med([stage(t) for t in on]):.3f} ms  (runs {[round(stage(t), 3) for t in on]})")
if both:
    print(f"genotype stage, fmt + fmeta:    {med([stage(t) for t in both]):.3f} ms  (runs {[round(stage(t), 3) for t in both]})")
for k in ("k_assign", "k_evid_stats"):
    print(f"{k}: off {med([t.get(k, 0.0) for t in off]):.3f} ms, on {med([t.get(k, 0.0) for t in on]):.3f} ms" +
          (f", fmt + fmeta {med([t.get(k, 0.0) for t in both]):.3f} ms" if both else ""))
print(f"per-read record array: {8 * nr * params.max_vars} bytes ({8 * nr * params.max_vars / nw:.0f} per window)")
