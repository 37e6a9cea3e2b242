#!/bin/bash
# Run on the GPU box: rocprofv3 passes + the two bench lines (default, the driver's setting) + the forced-sharded line.
# usage: tools/final_profiles.sh <tag>
set +e
TAG=${1:-r02d}
cd $GRAFT_REPO_ROOT
bash tools/collect_profiles.sh $TAG || exit $?
O=${BENCH_OUT:?BENCH_OUT: the directory collect_profiles.sh wrote to}
python bench.py --full > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err
python bench.py --full --steps 20 --warmup 5 > $O/${TAG}_bench_s20w5.json 2> $O/${TAG}_bench_s20w5.err
MS_BENCH_FORCE_SHARDED=1 python bench.py --full --no-large > $O/${TAG}_bench_forced_sharded.json 2> $O/${TAG}_bench_forced_sharded.err
echo finished
