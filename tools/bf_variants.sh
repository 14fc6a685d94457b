#!/bin/bash
# timing experiments for the brute-force select kernel (results are wrong for dbg&3 != 0)
for d in ${@:-0 4 260 516 772 1028 2052}; do
  echo -n "dbg=$d "; NMSLIB_GPU_DEBUG=$d python bench.py --workload bruteforce --full --steps 20 --warmup 3 --no-cpu-baseline 2>/dev/null | python -c "import sys,json; j=json.loads(sys.stdin.read()); print(j['roofline']['kernel_ms'], j['roofline']['achieved'], j['ms_per_step'], j['recall_at_k'])"
done
