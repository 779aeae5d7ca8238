#!/bin/bash
# The CLIPSeg CLI (loader + prefetcher, through tools/clipseg_cli_probe.py with the power knob) against bench.py's resident-batch line on the SAME box, alternating, with the board's power / shader clock sampled in both (round 6).
root=$(cd "$(dirname "$0")/.." && pwd); cd $root
run() { d=$(mktemp -d); ( cd $d && timeout -k 10 120 python $root/tools/clipseg_cli_probe.py power --dataset BUSI --synthetic --synthetic_train 7680 --synthetic_val 128 --synthetic_test 128 --batch_size 128 --epochs 3 --dtype bf16 --exp ab --stats_json $d/s.json > $d/log 2>&1 ); python -c "
import json,sys
try:
    p=json.loads([l for l in open('$d/log') if l.startswith('PROBE ')][-1][6:]); print('cli  ', p['ms_per_iter'], p['power'])
except Exception as ex: print('cli failed', ex, open('$d/log').read()[-600:])"; rm -rf $d; }
bench() { python bench.py --config clipseg --no-cpu-baseline --no-entry-point --steps 120 --warmup 30 2>/dev/null | python -c "import sys,json; o=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('bench', o['ms_per_step'], o.get('power'))"; }
run; bench; run; bench
