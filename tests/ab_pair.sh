#!/bin/bash
# experiment helper (GPU box): rows of the corner + surf target in one launch sequence (default) against the side stream of rounds 4-5 (LISREG_CROW_PAIR=0)
R=${GRAFT_REPO_ROOT:-$(pwd)}; cd $R; export LISREG_BENCH_NO_EXACT=1 LISREG_BENCH_NO_OVERLAP=1
for rep in 1 2 3; do for r in 0 1; do
  LISREG_CROW_PAIR=$r python bench.py --full --steps 20 --warmup 5 --cpu-regs 0 --no-pcie 2>/dev/null | tail -1 | python -c "
import sys,json; d=json.loads(sys.stdin.read()); print('crow_pair $r value', d['value'], 'ms/step', d['ms_per_step'], 'step_frac', d['roofline'].get('step_frac'))"
done; done
bash tests/timeline.sh | head -24
