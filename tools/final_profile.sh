#!/bin/bash
# final evidence of the round: default bench line + rocprofv3 kernel stats of the same command
export TMPDIR=/tmp
root=$(pwd)
out=${PROFILE_OUT:-$root/profile_out}   # outputs (kept out of git)
mkdir -p "$out"
python3 bench.py --full > "$out/r04f_bench_full.json" 2> "$out/r04f_bench_full.err"; echo "bench rc=$?"
export HK_NO_FIRST_PROCESS_PROBE=1
rm -rf "$out/r04f_stats"
(cd "$TMPDIR" && rocprofv3 --kernel-trace --stats -d "$out/r04f_stats" -o run --output-format csv -- python3 "$root/bench.py" --full --no-cpu-baseline > "$out/r04f_stats.log" 2>&1)
python3 tools/kstat_by_grid.py "$out/r04f_stats/run_kernel_trace.csv" 3 > "$out/r04f_kernel_stats_by_grid.csv"
head -3 "$out/r04f_kernel_stats_by_grid.csv" | cut -c1-200
