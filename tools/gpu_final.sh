#!/bin/bash
# A checkpoint without profile passes (kernels.hip unchanged since the stored
# PMC summaries): the whole GPU suite, smoke, and the bench run with --full.
# Usage: gpu_final.sh TAG
set -o pipefail
TAG=${1:-x}
R=$GRAFT_REPO_ROOT
O=${KWOK_OUT:-$R/out}  # where the run's files go
mkdir -p $O
timeout -k 10 960 python -u -m pytest tests -x -v -m gpu --timeout 300 --timeout-method thread > $O/tests_$TAG.log 2>&1
trc=$?
tail -4 $O/tests_$TAG.log
[ $trc -eq 0 ] || { grep -E "FAILED|Error" $O/tests_$TAG.log | head -20; exit $trc; }
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke_$TAG.log 2>&1 || { tail -20 $O/smoke_$TAG.log; exit 5; }
timeout -k 10 600 python bench.py --full > $O/bench_$TAG.json 2> $O/bench_$TAG.err || { tail -20 $O/bench_$TAG.err; exit 3; }
cut -c1-600 $O/bench_$TAG.json
