#!/bin/bash
# One session on a GPU machine: GPU tests, smoke, the full bench line, rocprofv3 kernel stats of a plain bench run.
# Every GPU step has its own time limit and the chain stops at the first failure.
# Usage: tools/gpu_round.sh [TAG]; the logs go to $NANOPOW_OUT (default bench_out/).
set -o pipefail
TAG=${1:-r01}
O=${NANOPOW_OUT:-bench_out}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 900 python3 -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $O/pytest_gpu_$TAG.log 2>&1 &&
timeout -k 10 180 python3 -c "import __graft_entry__ as g; g.smoke()" > $O/smoke_$TAG.log 2>&1 &&
timeout -k 10 600 python3 bench.py --full > $O/bench_$TAG.json 2> $O/bench_$TAG.err &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$TAG -o run -- python3 bench.py --steps 200 > $O/bench_prof_$TAG.json 2> $O/prof_$TAG.err
rc=$?
tail -3 $O/pytest_gpu_$TAG.log; cat $O/smoke_$TAG.log $O/bench_$TAG.json 2>/dev/null
exit $rc
