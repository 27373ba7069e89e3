#!/bin/bash
# usage: bash tools/measure_profiles.sh   -- run from the repository root on the GPU machine, on a built tree (__graft_entry__.build()).
# Re-takes the stamped round-6 measurement set (profiles/README.md) in ONE run on one box and writes it into profiles/ under
# the r6_* names bench.py and tests/test_profiles_fresh.py read.  Scratch goes to build/measure_profiles/ (git ignores
# build/), and a copy of every file written into profiles/ to build/measure_profiles/profiles/ (to bring home from a remote
# checkout).
# Stops at the first failure or time limit: every GPU step has a limit of its own, nothing is retried.
set -euo pipefail
R=$PWD
O=$R/build/measure_profiles
P=$O/profiles
T=r6_final
rm -rf "$O" && mkdir -p "$P"
export TMPDIR=/tmp
# the windows are synthesised ONCE and kept (outside the scratch directory: it is large): every profiler pass below loads them
export MA_BENCH_CACHE=$(mktemp -d)
trap 'rm -rf "$MA_BENCH_CACHE"' EXIT
B="python3 $R/bench.py --full --steps 2 --no-cpu --no-also --gen-workers 1"
keep() { cp "$1" "$P/$2"; cp "$1" "$R/profiles/$2"; }  # into profiles/ (and its copy)
last_line() { grep -h '^{"metric"' "$1" | tail -1; }

timeout -k 10 600 python3 bench.py --no-cpu --no-also --gen-only > "$O/gen.log" 2>&1
# PMC passes: one counter group each, --kernel-trace the only other tracing (the counters go into the kernel records)
for c in FETCH_SIZE WRITE_SIZE SQ_INSTS_VALU; do
  timeout -k 10 600 rocprofv3 --pmc $c --kernel-trace --output-format csv -d "$O/pmc_$c" -- $B > "$O/pmc_$c.log" 2>&1
done
python3 tools/pmc_per_kernel.py "$O/pmc_FETCH_SIZE" "$O/pmc_WRITE_SIZE" "$O/pmc_SQ_INSTS_VALU" "$O/${T}_pmc_per_kernel.json" \
  "$O/pmc_SQ_INSTS_VALU.log" > "$O/${T}_pmc_per_kernel.txt"
# bench.py prices its kernels with this file: it is in place before any later run
keep "$O/${T}_pmc_per_kernel.json" r6_pmc_per_kernel.json
keep "$O/${T}_pmc_per_kernel.json" ${T}_pmc_per_kernel.json
keep "$O/${T}_pmc_per_kernel.txt" ${T}_pmc_per_kernel.txt
last_line "$O/pmc_SQ_INSTS_VALU.log" > "$O/${T}_pmc_bench_under_rocprof.json"
keep "$O/${T}_pmc_bench_under_rocprof.json" ${T}_pmc_bench_under_rocprof.json

timeout -k 10 600 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU SQ_BUSY_CYCLES SQ_WAVES \
  --kernel-trace --output-format csv -d "$O/pmc_sq" -- $B > "$O/pmc_sq.log" 2>&1
python3 tools/pmc_generic.py "$O/pmc_sq" - "$O/${T}_pmc_sq_per_kernel.json" > "$O/${T}_pmc_sq_per_kernel.txt"
keep "$O/${T}_pmc_sq_per_kernel.json" r6_pmc_sq_per_kernel.json
keep "$O/${T}_pmc_sq_per_kernel.json" ${T}_pmc_sq_per_kernel.json
keep "$O/${T}_pmc_sq_per_kernel.txt" ${T}_pmc_sq_per_kernel.txt

# achieved occupancy and L2 hit rate, each in a pass of its own (a pass that asks for too much aborts the profiler)
timeout -k 10 600 rocprofv3 --pmc SQ_BUSY_CU_CYCLES --kernel-trace --output-format csv -d "$O/pmc_occ" -- $B > "$O/pmc_occ.log" 2>&1
python3 tools/pmc_generic.py "$O/pmc_occ" > "$O/${T}_pmc_occupancy_per_kernel.txt"
keep "$O/${T}_pmc_occupancy_per_kernel.txt" ${T}_pmc_occupancy_per_kernel.txt
timeout -k 10 600 rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --kernel-trace --output-format csv -d "$O/pmc_l2" -- $B > "$O/pmc_l2.log" 2>&1
python3 tools/pmc_generic.py "$O/pmc_l2" > "$O/${T}_pmc_l2_per_kernel.txt"
keep "$O/${T}_pmc_l2_per_kernel.txt" ${T}_pmc_l2_per_kernel.txt

timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/ktrace" -- \
  python3 "$R/bench.py" --full --no-cpu --no-also --gen-workers 1 > "$O/ktrace.log" 2>&1
last_line "$O/ktrace.log" > "$O/${T}_bench_under_rocprof.json"
keep "$O/${T}_bench_under_rocprof.json" ${T}_bench_under_rocprof.json
keep "$(find "$O/ktrace" -name '*kernel_stats.csv' | head -1)" ${T}_kernel_stats.csv

MA_STREAMS=1 timeout -k 10 300 python3 bench.py --full --no-cpu --no-also > "$O/single_lane.log" 2>&1
last_line "$O/single_lane.log" > "$O/${T}_bench_single_lane.json"
keep "$O/${T}_bench_single_lane.json" ${T}_bench_single_lane.json

# the plain --full line: its parity sample and GCUPS are what tests/test_profiles_fresh.py checks (so: with the CPU side)
timeout -k 10 1200 python3 bench.py --full > "$O/bench.log" 2>&1
last_line "$O/bench.log" > "$O/${T}_bench.json"
keep "$O/${T}_bench.json" ${T}_bench.json

python3 tools/kernel_resources.py > "$O/r6_kernel_resources.txt"
keep "$O/r6_kernel_resources.txt" r6_kernel_resources.txt
rm -rf "$O/pmc_FETCH_SIZE" "$O/pmc_WRITE_SIZE" "$O/pmc_SQ_INSTS_VALU" "$O/pmc_sq" "$O/pmc_occ" "$O/pmc_l2" "$O/ktrace"
python3 -c "
import json
from lancet2_amd.stamp import csrc_sha16
p = json.load(open('profiles/r6_pmc_per_kernel.json'))['_stamp']['csrc_sha16']
print('profiles/r6_pmc_per_kernel.json stamp', p, 'sources', csrc_sha16(), 'FRESH' if p == csrc_sha16() else 'STALE')
"
