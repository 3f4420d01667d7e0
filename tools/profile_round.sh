#!/bin/bash
# On the GPU box: bench line and rocprofv3 kernel stats of the same bench command (-> <dir>, default bench_out), and the PMC passes.
# Usage: bash tools/profile_round.sh v10 [dir]
V=${1:-vX}
R=$GRAFT_REPO_ROOT
O=$R/${2:-bench_out}
cd $R
mkdir -p $O
python bench.py --full > $O/bench_line_$V.json 2> $O/bench_$V.err
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_$V -o bench -- python3 $R/bench.py --full --no-cpu-baseline > $O/bench_prof_$V.log 2>&1
cd $R
bash tools/pmc_passes.sh
python tools/pmc_report.py gpurun_out gpurun_out/pmc_summary_$V.json > gpurun_out/pmc_table_$V.txt
tail -c 400 $O/bench_line_$V.json
