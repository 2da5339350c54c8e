#!/bin/bash
# Runs on the GPU box (through gpurun): kernel trace + PMC passes of the bench workload.
# Counters are collected in their own passes, with --kernel-trace only (gpurun refuses --pmc
# together with sys/hip/hsa traces).  Usage: OUT=<dir> profiles/collect.sh <tag>   -> $OUT/<tag>_*
set -e
TAG=${1:-prof}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
export OUT="${OUT:?set OUT to the directory the results go to}" && mkdir -p "$OUT"
B="python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-extras --profile-legs"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_kt -- python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extras --profile-legs > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_kt.err
timeout -k 10 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --kernel-trace --output-format csv -d $OUT/${TAG}_sq -- $B > /dev/null 2> $OUT/${TAG}_sq.err
timeout -k 10 300 rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum --kernel-trace --output-format csv -d $OUT/${TAG}_tcc -- $B > /dev/null 2> $OUT/${TAG}_tcc.err
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/${TAG}_fetch -- $B > /dev/null 2> $OUT/${TAG}_fetch.err
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/${TAG}_write -- $B > /dev/null 2> $OUT/${TAG}_write.err
echo collected $TAG
