#!/bin/bash
# everything under profiles/r02_* : PMC traffic and rocprofv3 kernel stats first, then -- with the fresh PMC summaries copied
# into profiles/ so that bench.py finds them for `roofline.traffic` -- the bench lines of the three workloads and the default line
cd $GRAFT_REPO_ROOT
ROUND=r02 bash tools/exp/bench_pmc.sh resnet18 | tail -3
ROUND=r02 bash tools/exp/bench_pmc.sh conv3x3 | tail -2
cd $GRAFT_REPO_ROOT
cp gpurun_out/r02_resnet18_pmc.json gpurun_out/r02_conv3x3_pmc.json profiles/
NAME=resnet18 bash tools/exp/bench_trace.sh | head -3
NAME=conv3x3 BENCH_ARGS="--workload conv3x3" bash tools/exp/bench_trace.sh | head -3
NAME=mobilenet BENCH_ARGS="--workload mobilenet" bash tools/exp/bench_trace.sh | head -3
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p "$OUT"   # where the bench lines below go
for wl in resnet18 conv3x3 mobilenet; do
  python3 bench.py --full --workload $wl --steps 20 --warmup 5 --no-side-workloads > $OUT/r02_bench_$wl.json 2> $OUT/r02_bench_$wl.err
  tail -c 200 $OUT/r02_bench_$wl.json; echo
done
python3 bench.py --full > $OUT/r02_bench_default_line.json 2> $OUT/r02_bench_default_line.err
tail -c 200 $OUT/r02_bench_default_line.json; echo
