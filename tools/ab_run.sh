#!/bin/bash
# on the GPU box: bench.py (headline step only) once per library variant in build/variants, alternating, $AB_ROUNDS rounds (default 2); extra bench
# args via $AB_ARGS (later arguments win: AB_ARGS="--steps 20 --warmup 3")
O=$(mktemp -d); trap 'rm -rf "$O"' EXIT
for rep in $(seq ${AB_ROUNDS:-2}); do
for lib in build/variants/*.so; do
  PWN_HIP_LIB=$PWD/$lib timeout -k 10 300 python bench.py --steps 6 --warmup 2 --full --no-cpu-baseline --no-latency --no-extras $AB_ARGS > $O/b.json 2>$O/b.err || { echo "$lib FAILED"; tail -3 $O/b.err; exit 1; }
  python -c "
import json; d=json.load(open('$O/b.json')); s=d['stage_ms_per_step']; print('$lib', round(d['value']), 'ms/step', round(d['ms_per_step'],2), {k: round(v,2) for k,v in s.items() if v}, 'chi2', round(d['counters_mean']['chi2_final'],3))"
done
done
