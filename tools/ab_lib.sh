#!/bin/bash
# A/B timing of the C3 bench: the in-tree library against build/ab/lib_head.so, alternating
# (TESTS=1 runs the GPU suite on the in-tree library first); PAIRS pairs, STEPS steps each
O=${OUT:-bench_out}/ab
mkdir -p $O
if [ -n "$TESTS" ]; then
  timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/t.log 2>&1 || { tail -n 30 $O/t.log; exit 1; }
  tail -n 1 $O/t.log
fi
for i in $(seq ${PAIRS:-2}); do
for v in new head; do
  if [ $v = head ]; then export RMIMO_LIB=$PWD/build/ab/lib_head.so; else unset RMIMO_LIB; fi
  timeout -k 10 200 python bench.py --full --cpu-baseline 0 --sc16-steps 0 --steps ${STEPS:-20} $BENCH_ARGS > $O/b_$v.json 2>$O/b_$v.err || { tail $O/b_$v.err; exit 1; }
  python -c "
import json; d=json.load(open('$O/b_$v.json')); st=d['stages_ms_per_step']; print('$v', round(d['ms_per_step'],4), ' '.join('%s %.4f'%(k,st[k]) for k in ('sc','search','decode')), 'roof', round(d['roofline']['frac'],3), d['frames_ok'])"
done
done
