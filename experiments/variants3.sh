#!/bin/bash
# usage: variants3.sh <outdir> "<wpw> <exp> <budget> <config> [extra bench args]" ...
cd $GRAFT_REPO_ROOT
O=gpurun_out/$1; shift; mkdir -p $O
for spec in "$@"; do
  set -- $spec; w=$1; ex=$2; bud=$3; cfg=$4; shift 4
  tag=${cfg}_w${w}_e${ex}_b${bud}$(echo "$*" | tr -d ' -')
  PB_WPW=$w PB_EXP=$ex timeout -k 10 200 python bench.py --full --config $cfg --budget $bud --steps 120 --warmup 10 --no-cpu-baseline "$@" > $O/$tag.json 2> $O/$tag.err || echo "FAILED $tag"
  python3 - <<PY
import json
try:
    d=json.loads(open('$O/$tag.json').read().strip().splitlines()[-1]); r=d['roofline']; p=r['plan']
    print('%-34s us/frame %7.2f  p10 %7.2f p90 %7.2f  frac %.4f  lean %5d direct %5d' % ('$tag', r['kernel_ms_per_frame']*1e3, r['kernel_ms_p10']*1e3/d['config']['frames_per_launch'], r['kernel_ms_p90']*1e3/d['config']['frames_per_launch'], r['frac'], p['lean_tiles'], p['direct_tiles']))
except Exception as e: print('$tag ERR', e)
PY
done | tee $O/summary.txt
