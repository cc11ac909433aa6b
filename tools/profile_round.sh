#!/bin/bash
# Round evidence, on a GPU machine from the repo root:  tools/profile_round.sh rNN [OUT]   (OUT: default profile_out)
#   OUT/<tag>_bench_c2.json        full bench line (bench.py --full: roofline + cpu_baseline)
#   OUT/<tag>_stats/               rocprofv3 --kernel-trace --stats of the same command
#   OUT/<tag>_pmc_{fetch,write}/   separate --pmc passes (one outer iteration, kernels serialised)
set -e
tag=$1
R=$PWD
O=$(realpath -m "${2:-profile_out}")
mkdir -p $O
python bench.py --full > $O/${tag}_bench_c2.json 2> $O/${tag}_bench_c2.err
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/${tag}_stats -o run -- python3 $R/bench.py --full --no-cpu-baseline --no-selfcheck > $O/${tag}_bench_under_rocprof.json 2> $O/${tag}_stats.log
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/${tag}_pmc_fetch -o run -- python3 $R/bench.py --steps 1 --warmup 0 --no-roofline --no-cpu-baseline --no-selfcheck > /dev/null 2> $O/${tag}_pmc_fetch.log
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/${tag}_pmc_write -o run -- python3 $R/bench.py --steps 1 --warmup 0 --no-roofline --no-cpu-baseline --no-selfcheck > /dev/null 2> $O/${tag}_pmc_write.log
cd $R
# summaries (the raw per-dispatch csv files are tens of MB: only the summaries are kept)
cp $(find $O/${tag}_stats -name "*kernel_stats.csv" | head -1) $O/${tag}_kernel_stats.csv
python3 tools/pmc_traffic.py $(find $O/${tag}_pmc_fetch -name "*counter_collection.csv" | head -1) \
    $(find $O/${tag}_pmc_write -name "*counter_collection.csv" | head -1) \
    $O/traffic_${tag}.json $O/${tag}_pmc_traffic_summary.csv
rm -rf $O/${tag}_stats $O/${tag}_pmc_fetch $O/${tag}_pmc_write
ls $O | grep ${tag}
