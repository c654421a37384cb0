#!/bin/bash
# Collect the committed profile set on the GPU box: kernel stats of the default bench command + two PMC passes.
# Usage (on the GPU machine): PROFILE_OUT=<dir> bash scratch/profile_round.sh <tag>
set -e
tag=${1:-r01}
R=$GRAFT_REPO_ROOT
O=${PROFILE_OUT:?set PROFILE_OUT to the directory the profiles go to}
cd /tmp && export TMPDIR=/tmp
[ -n "$SKIP_STATS" ] || rocprofv3 --kernel-trace --stats --output-format csv -d $O/${tag}_stats -- python $R/bench.py --full > $O/${tag}_bench_under_rocprof.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/${tag}_pmc_fetch -- python $R/bench.py --full --steps 4 --warmup 2 --no-cpu-baseline --prof-steps 0 > $O/${tag}_pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/${tag}_pmc_write -- python $R/bench.py --full --steps 4 --warmup 2 --no-cpu-baseline --prof-steps 0 > $O/${tag}_pmc_write.log 2>&1
echo done
