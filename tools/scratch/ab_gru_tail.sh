#!/bin/bash
# the GRU's layer-0 weight-gradient products and bias sums on the side stream, under the encoder's backward (shipped) against the
# immediate form (CPC_NO_GRAD_TAIL=1); alternating pairs on one box
mkdir -p bench_out
OUT=bench_out/ab_gru_tail.txt
: > $OUT
for cfg in small large; do
for rep in 1 2 3; do
  for v in immediate deferred; do
    unset CPC_NO_GRAD_TAIL
    [ $v = immediate ] && export CPC_NO_GRAD_TAIL=1
    timeout -k 10 200 python bench.py --full --config $cfg --cpu-seconds 0 --also "" --steps 40 --warmup 8 > bench_out/ab_x_$v.json 2>bench_out/ab_x_$v.err || tail -5 bench_out/ab_x_$v.err >> $OUT
    python - >> $OUT <<PY
import json
d=json.loads(open("bench_out/ab_x_$v.json").read().strip().splitlines()[-1])
print("$cfg $v rep $rep: %.3f ms/step" % d["ms_per_step"], "frac", d["roofline"]["frac"], "loss", d["config"]["final_losses"][:2])
PY
  done
done
done
cat $OUT
