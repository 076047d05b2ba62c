#!/bin/bash
# throughput of the judged workload against the number of utterances in flight
O=${OUT_DIR:-/tmp/sweep_inflight}; mkdir -p $O
for n in ${NS:-1 2 3 4}; do
  python bench.py --full --steps 8 --warmup 3 --no-cpu-baseline --no-rooflines --inflight $n > $O/n$n.json 2> $O/n$n.err
  python - <<PY
import json
l = json.loads([x for x in open("$O/n$n.json") if x.startswith("{")][-1])
print("inflight $n:", l["ms_per_step"], "ms/utt;", "host_io", l["host_io"]["ms_per_step"])
PY
done
