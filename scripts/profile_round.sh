#!/bin/bash
# Profiling pass of one round on the GPU box:  bash scripts/profile_round.sh <tag>   (run through gpurun)
# Per bench leg (f64 = the headline, f32 = the fixed-point leg): one --stats pass and five --pmc passes (counters in passes of
# their own, never combined with other trace domains), on a shorter run of the same workload (512 rounds per step).
set -e
TAG=${1:-r01_x}
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=$REPO/gpurun_out/prof_$TAG
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
export NLMC_BENCH_ROUNDS_PER_STEP=512
# One profiler pass of the bench: prof <output directory> <file prefix> <rocprofv3 options...>.  A process that made cooperative
# launches (k_rounds_fused, the headline leg's default route) ends with a segmentation fault inside exit() under rocprofv3, AFTER
# the tool has written its tables and its "tool finalization" line (the same with bench.py --persistent before the route became
# the default: the profiler's teardown, not the kernel).  Such a pass counts when the bench line and the tables are there.
prof() {
  local dir=$1 pre=$2; shift 2
  timeout -k 10 300 rocprofv3 --output-format csv --kernel-trace "$@" -d "$dir" -o "$pre" -- $B > "$dir.log" 2>&1 && return 0
  grep -q '"ms_per_step"' "$dir.log" && grep -q 'tool finalization' "$dir.log" && [ -n "$(find "$dir" -name "${pre}_*.csv" -size +0 | head -1)" ] || return 1
  echo "  ($(basename "$dir"): the profiler's process crashed in exit() after writing its tables)"
}
for LEG in f64 f32; do
  B="python3 $REPO/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-second-leg --headline $LEG"
  prof "$OUT/stats_$LEG" s --stats
  prof "$OUT/fetch_$LEG" f --pmc FETCH_SIZE
  prof "$OUT/write_$LEG" w --pmc WRITE_SIZE
  prof "$OUT/sq1_$LEG" q --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD
  prof "$OUT/sq2_$LEG" q --pmc SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY SQ_BUSY_CYCLES
  prof "$OUT/sq3_$LEG" q --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_ANY SQ_WAVE_CYCLES
  python3 "$REPO/scripts/summarize_prof.py" "$TAG" "$LEG" "$OUT/stats_$LEG" "$OUT/fetch_$LEG" "$OUT/write_$LEG" "$OUT/sq1_$LEG" "$OUT/sq2_$LEG" "$OUT/sq3_$LEG"
  echo "leg $LEG profiled"
done
unset NLMC_BENCH_ROUNDS_PER_STEP
if [ -z "$SKIP_SECONDARY" ]; then
# secondary kernels: backbone inference (k_lbp) and the APT + iso-cluster round (C5)
timeout -k 10 300 rocprofv3 --output-format csv --kernel-trace --stats -d "$OUT/lbp" -o s -- python3 $REPO/scripts/lbp_throughput.py > "$OUT/lbp.log" 2>&1
timeout -k 10 300 rocprofv3 --output-format csv --kernel-trace --stats -d "$OUT/c5" -o s -- python3 $REPO/scripts/c5_only.py > "$OUT/c5.log" 2>&1
RESTARTS=8 timeout -k 10 300 rocprofv3 --output-format csv --kernel-trace --stats -d "$OUT/c3nmc" -o s -- python3 $REPO/scripts/npt_nmc_throughput.py > "$OUT/c3nmc.log" 2>&1
cp "$OUT/c3nmc/s_kernel_stats.csv" "$REPO/profiles/${TAG}_c3nmc_kernel_stats.csv"
cp "$OUT/lbp/s_kernel_stats.csv" "$REPO/profiles/${TAG}_lbp_kernel_stats.csv"
cp "$OUT/c5/s_kernel_stats.csv" "$REPO/profiles/${TAG}_c5_kernel_stats.csv"
fi
cp "$REPO"/profiles/${TAG}_* "$REPO"/profiles/current_sweep_pmc.json "$OUT"/
python3 "$REPO/bench.py" --full > "$OUT/bench.json" 2> "$OUT/bench.err"
cp "$OUT/bench.json" "$REPO/profiles/${TAG}_bench_n1.json"
cp "$REPO/profiles/${TAG}_bench_n1.json" "$OUT"/
tail -1 "$OUT/bench.json"
