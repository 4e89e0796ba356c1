#!/bin/bash
# run bench c3 (fc32 and sc16) with each build/abl/*.so and print the decode stage time
set -o pipefail
O=${OUT:-bench_out}/abl
mkdir -p $O
for v in ${VARIANTS:-base nostore nodma nofft nostore_nodma}; do
  for fmt in fc32 sc16; do
    RMIMO_LIB=build/abl/$v.so timeout -k 10 120 python bench.py --full --workload ${WL:-c3} --cpu-baseline 0 --sc16-steps 0 --sample-format $fmt > $O/$v.$fmt.json 2> $O/$v.$fmt.err || { echo "$v $fmt failed"; tail -5 $O/$v.$fmt.err; exit 1; }
    python -c "
import json; d=json.load(open('$O/$v.$fmt.json'))
s=d['stages_ms_per_step']; print('%-14s %s decode %.4f step %.4f'%('$v','$fmt',s['decode'],d['ms_per_step']))"
  done
done
