#!/bin/bash
# regenerates the bench lines / kernel tables kept under profiles/ (on the GPU box): tests/final_profiles.sh <tag>
TAG=${1:-r03}; R=$(pwd); O=$R/gpurun_out/final_$TAG; rm -rf $O; mkdir -p $O
for w in cfg1 cfg3 odom cfg4 cfg5 cfg4_icp; do timeout 300 python bench.py --full --workload $w 2>/dev/null | tail -1 > $O/${TAG}_bench_$w.json; done
timeout 300 python bench.py --full --workload cfg5 --batch 32 2>/dev/null | tail -1 > $O/${TAG}_bench_cfg5_b32.json        # "B >= 8" — both ends reported
timeout 300 python bench.py --full 2>/dev/null | tail -1 > $O/${TAG}_bench.json
LISREG_BENCH_FORCE_DIST=1 timeout 300 python bench.py --full --steps 10 --warmup 2 --cpu-regs 0 --no-pcie 2>/dev/null | tail -1 > $O/${TAG}_bench_force_dist_1rank.json
( D=$(mktemp -d); cd $D; export TMPDIR=$D; rocprofv3 --output-format csv --kernel-trace --stats -d $O/icp_trace -o trace -- python $R/bench.py --full --workload cfg4_icp --steps 2 --warmup 1 --cpu-regs 0 > $O/icp_trace.log 2>&1 )
python - "$O" "$TAG" <<'PY'
import csv, glob, sys
O, TAG = sys.argv[1], sys.argv[2]
f = glob.glob(f"{O}/icp_trace/**/*kernel_stats.csv", recursive=True)
if f:
    rows = [r for r in csv.DictReader(open(f[0])) if "lisreg" in r["Name"]]
    with open(f"{O}/{TAG}_cfg4_icp_kernel_stats.csv", "w") as o:
        w = csv.DictWriter(o, fieldnames=list(rows[0].keys())); w.writeheader(); w.writerows(rows)
PY
rm -rf $O/icp_trace
timeout 120 python tests/replay_probe.py 2>/dev/null > $O/${TAG}_replay_stage_times.txt
( timeout 120 tests/ktrace.sh cfg3 30; timeout 120 tests/ktrace.sh odom 30 ) 2>&1 | grep -v "^W2026" > $O/${TAG}_replay_kernel_times.txt
timeout 900 bash tests/prof.sh $TAG > $O/prof.log 2>&1
cp gpurun_out/prof_$TAG/summary.txt $O/${TAG}_rocprofv3_summary.txt 2>/dev/null
cp gpurun_out/prof_$TAG/kernel_stats.csv $O/${TAG}_kernel_stats.csv 2>/dev/null
cp gpurun_out/prof_$TAG/traffic.json $O/traffic.json 2>/dev/null
# per-GN-iteration k_assoc durations (rocprofv3 --kernel-trace) of configs[1], configs[3] (own targets) and configs[4] (30 iterations)
{ echo "configs[1]:"; AB_ITERS=10 timeout 400 bash tests/ab.sh base 2>/dev/null | tail -2
  echo "configs[3] (cfg4):"; AB_ITERS=10 BENCH_ARGS="--workload cfg4" timeout 400 bash tests/ab.sh base 2>/dev/null | tail -2
  echo "configs[4] (cfg5):"; AB_ITERS=30 BENCH_ARGS="--workload cfg5" timeout 400 bash tests/ab.sh base 2>/dev/null | tail -2; } > $O/${TAG}_per_iteration.txt
# per-kernel tables of configs[3] / configs[4] restricted to the STEPS: everything after the batch was prepared (the last k_count_jumps — the
# source-order probe of lisreg_batch_prepare; the 512 lisreg_set_target calls of configs[3] in front of it are set-up, outside the timed region:
# round 5's table had their 514 x k_target_keys / k_bbox_* / k_scan_* launches next to the steps' kernels)
for w in cfg4 cfg5 cfg5b32; do
  a="--workload $w"; [ $w = cfg5b32 ] && a="--workload cfg5 --batch 32"
  ( cd /tmp; export TMPDIR=/tmp LISREG_BENCH_NO_EXACT=1 LISREG_BENCH_NO_OVERLAP=1; rocprofv3 --output-format csv --kernel-trace -d $O/tr_$w -o trace -- python $R/bench.py $a --steps 3 --warmup 1 --cpu-regs 0 --no-profile --no-pcie --min-seconds 0 > $O/tr_$w.log 2>&1 )
  python - "$O" "$TAG" "$w" <<'PY'
import csv, glob, sys, re, collections
O, TAG, W = sys.argv[1:4]
f = glob.glob(f"{O}/tr_{W}/**/*kernel_trace.csv", recursive=True)
if f:
    rows = sorted([r for r in csv.DictReader(open(f[0])) if "lisreg" in r["Kernel_Name"]], key=lambda r: int(r["Start_Timestamp"]))
    last = max([i for i, r in enumerate(rows) if "k_count_jumps" in r["Kernel_Name"]] or [-1])
    rows = rows[last + 1:]
    agg = collections.OrderedDict()
    for r in rows:
        n = re.sub(r"\(.*", "", r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("lisreg::", "").replace("fast_arith::", "")).replace("void ", "")
        d = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        a = agg.setdefault(n, [0, 0, 1 << 62, 0]); a[0] += 1; a[1] += d; a[2] = min(a[2], d); a[3] = max(a[3], d)
    tot = sum(a[1] for a in agg.values())
    with open(f"{O}/{TAG}_{W}_kernel_stats.csv", "w") as o:
        o.write("kernel,calls,total_ns,avg_ns,min_ns,max_ns,pct_of_step_kernel_time\n")
        for n, a in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            o.write(f"\"{n}\",{a[0]},{a[1]},{a[1] / a[0]:.1f},{a[2]},{a[3]},{100.0 * a[1] / max(tot, 1):.2f}\n")
PY
  rm -rf $O/tr_$w
done
timeout 300 bash tests/timeline.sh > $O/${TAG}_step_timeline.txt 2>&1                  # the kernels of one configs[1] step in order
timeout 600 python -m pytest tests/test_fit_device.py tests/test_round6_edges.py tests/test_configs.py -m gpu -q -s 2>&1 | grep -E "^\[|\|p\||unit normal|planes through|passed|failed" > $O/${TAG}_new_tests_output.txt
LISREG_BENCH_OVERSUBSCRIBE=1 timeout 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 2 --steps 10 --warmup 2 --full 2>/dev/null | tail -1 > $O/${TAG}_bench_2ranks_one_gpu.json
ls $O
