#!/bin/bash
# A/B of prebuilt library variants inside ONE GPU call (boxes differ by ~1 %: never compare across calls):
# tools/ab_so.sh build/libofx_a.so build/libofx_b.so ...   each is timed twice, interleaved; restores the default build
# AB_ARGS: the bench arguments (default "--steps 40 --warmup 10"; the acceptance form is "--steps 200 --warmup 40", and
# "--policy-ships 1 --steps 300 --warmup 50" for the one-policy-ship line).  Stops at the first run that fails.
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
cp ofighters_amd/libofx.so /tmp/libofx_keep.so
trap 'cp /tmp/libofx_keep.so ofighters_amd/libofx.so' EXIT   # an interrupted run must not leave a variant installed
for rep in 1 2; do
  for so in "$@"; do
    cp "$so" ofighters_amd/libofx.so
    timeout -k 10 240 python bench.py --gpus 1 ${AB_ARGS:---steps 40 --warmup 10} --no-cpu-baseline --no-extra 2>/dev/null > /tmp/ab_so_line.json || { echo "[$so] failed"; exit 1; }
    python -c "
import json,sys
d=json.loads(open('/tmp/ab_so_line.json').read().strip().splitlines()[-1]); print('[$so]', 'run $rep', 'head ms', round(d['roofline']['avg_kernel_ms'],4), 'tick ms', round(d['ms_per_step'],4))"
  done
done
