#!/bin/bash
# Round-end evidence in one GPU call (run on the GPU box from the repo root):  bash tools/finalize_profiles.sh r02
#   1. HBM traffic of the step's kernels (two counter passes)   -> gpurun_out/traffic_<tag>/summary.json
#   2. rocprofv3 --kernel-trace --stats of the default bench     -> gpurun_out/stats_<tag>/.../kernel_stats.csv
#   3. the default bench line                                    -> bench_<tag>.json in the same directory
set -e
tag=${1:-r02}
root=$GRAFT_REPO_ROOT
bash $root/tools/pmc_traffic.sh $tag > /dev/null
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $root/gpurun_out/stats_$tag --output-format csv -- python3 $root/bench.py --steps 25 --warmup 3 --no-cpu-baseline > $root/gpurun_out/stats_$tag.log 2>&1
cd $root
f=$(find gpurun_out/stats_$tag -name "*kernel_stats.csv" | head -1)
cp $f gpurun_out/kernel_stats_$tag.csv
python3 tools/kernel_stats_summary.py gpurun_out/kernel_stats_$tag.csv 12
