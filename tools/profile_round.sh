#!/bin/bash
# The profile set of a round, on the GPU box, from the repo root:  tools/profile_round.sh <tag> [<out dir, default profile_out>]
# 1. rocprofv3 --kernel-trace --stats of the bench with --full (its roofline launches on their own symbols) -> <out>/<tag>_stats/
# 2. kernel trace of a few steps                            -> <out>/<tag>_trace/  (tools/trace_csv.py)
# 3. PMC passes of the bench with --full, one counter set per pass (never together with trace domains other than --kernel-trace)
tag=${1:-r04}
R=$(pwd)
O=$(realpath -m "${2:-profile_out}")
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/${tag}_stats -- python3 $R/bench.py --steps 20 --warmup 3 --full --no-cpu-baseline > $O/${tag}_stats.json 2> $O/${tag}_stats.err || exit 1
rocprofv3 --kernel-trace --output-format csv -d $O/${tag}_trace -- python3 $R/bench.py --steps 12 --warmup 3 > $O/${tag}_trace.json 2> $O/${tag}_trace.err || exit 1
for set in "pmc_fetch:FETCH_SIZE" "pmc_write:WRITE_SIZE" "pmc_clk:GRBM_GUI_ACTIVE" "pmc_sq:SQ_BUSY_CYCLES SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES"; do
  name=${set%%:*}; ctrs=${set#*:}
  rocprofv3 --pmc $ctrs --kernel-trace --output-format csv -d $O/${tag}_pmc/$name -- python3 $R/bench.py --steps 3 --warmup 2 --full --no-cpu-baseline > $O/${tag}_$name.log 2>&1 || exit 1
done
cd $R
f=$(ls -t $O/${tag}_trace/*/*kernel_trace.csv | head -1)
python tools/trace_csv.py $f 8 > $O/${tag}_step_timeline.txt
python tools/trace_csv.py $f 8 --sum > $O/${tag}_step_anatomy.txt
STEP_TIMELINE=$O/${tag}_step_timeline.txt python tools/pmc_summary.py --dominant $O/${tag}_pmc_dominant.json $O/${tag}_pmc/pmc_fetch $O/${tag}_pmc/pmc_write $O/${tag}_pmc/pmc_clk $O/${tag}_pmc/pmc_sq > $O/${tag}_pmc_summary.txt
cp $(ls -t $O/${tag}_stats/*/*kernel_stats.csv | head -1) $O/${tag}_bench_kernel_stats.csv
