#!/bin/bash
# On the GPU box: per-shape kernel durations of one bench run (rocprofv3 kernel trace).
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
export OUT="${OUT:?set OUT to the directory the results go to}" && mkdir -p "$OUT"
TAG=${1:-shapes}
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_kt -- python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_kt.err
python profiles/summarize.py $OUT/${TAG}_sum $OUT/${TAG}_kt > /dev/null
head -12 $OUT/${TAG}_sum/per_shape.csv
