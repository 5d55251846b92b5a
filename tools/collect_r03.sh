#!/bin/bash
# Round-3 evidence: the driver's bench command, the rocprofv3 kernel stats of the same command, MFMA-busy counters of the epoch's
# kernels, the optimizer launch's workgroup stamps, the accuracy sweep.   bash tools/collect_r03.sh <out_dir>
out=${1:-gpurun_out/r03_p}
mkdir -p $out
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
python3 bench.py --gpus 1 --steps 20 --warmup 5 --full > $out/bench_default.json 2> $out/bench_default.err
echo "bench rc=$?"
rocprofv3 --kernel-trace --stats --output-format csv -d $out/trace -- python3 bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-e2e > $out/trace_bench.json 2> $out/trace.err
cp $out/trace/*/*kernel_stats.csv $out/bench_kernel_stats.csv
python3 - $out <<'PY'
import csv, sys
out = sys.argv[1]
rows = list(csv.DictReader(open(out + "/bench_kernel_stats.csv")))
tot = 0; lines = ["== per-step kernels of `python3 bench.py --steps 5 --warmup 2` (rocprofv3 --kernel-trace --stats), us per launch"]
for r in rows:
    if int(r["Calls"]) >= 2000:
        tot += float(r["AverageNs"]); lines.append(f"   {r['Name'][:86]:86s} {int(r['Calls']):6d} x {float(r['AverageNs'])/1000:7.2f}")
lines.append(f"   sum of the per-step kernels {tot/1000:.1f} us")
for r in rows:
    if any(k in r["Name"] for k in ("vectorise", "mimic", "col_stats", "stats")) and int(r["Calls"]) < 2000:
        lines.append(f"   {r['Name'][:86]:86s} {int(r['Calls']):6d} x {float(r['AverageNs'])/1000:7.2f}")
open(out + "/step_kernels.txt", "w").write("\n".join(lines) + "\n"); print("\n".join(lines))
PY
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $out/pmc_mfma -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-e2e > $out/pmc_mfma.json 2> $out/pmc_mfma.err
python3 - $out <<'PY'
import csv, glob, json, sys, collections
out = sys.argv[1]
f = glob.glob(out + "/pmc_mfma/**/*counter_collection.csv", recursive=True)[0]
acc = collections.defaultdict(lambda: collections.defaultdict(float)); seen = collections.defaultdict(set)
def key(n):
    for k, v in (("Cijk_", "hipBLASLt/rocBLAS GEMMs (Cijk_*)"), ("wgrad_rmsprop_kernel", "wgrad_rmsprop_kernel (dW1 tiles + optimizer)"), ("mid_fwd", "mid_fwd_kernel"),
                 ("mid_bwd", "mid_bwd_kernel"), ("nce_pass1", "nce_pass1_kernel"), ("nce_pass2", "nce_pass2_kernel"), ("vectorise3", "vectorise3_kernel")):
        if k in n: return v
    return None
for r in csv.DictReader(open(f)):
    k = key(r["Kernel_Name"])
    if k is None: continue
    acc[k][r["Counter_Name"]] += float(r["Counter_Value"]); seen[k].add(r["Dispatch_Id"])
res = {}
for k, c in acc.items():
    n = len(seen[k]); d = {x: v / n for x, v in c.items()}; d["dispatches"] = n
    if d.get("GRBM_GUI_ACTIVE"): d["mfma_busy_fraction_of_kernel"] = d.get("SQ_VALU_MFMA_BUSY_CYCLES", 0) / 1024 / (d["GRBM_GUI_ACTIVE"] / 8)
    res[k] = d
json.dump({"source": "rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE -- python3 bench.py --steps 2 --warmup 1 (cfg2); means per dispatch; "
                     "mfma_busy_fraction = busy cycles / 1024 SIMDs / (GRBM_GUI_ACTIVE / 8 XCDs)", "kernels": res}, open(out + "/epoch_pmc_mfma.json", "w"), indent=1)
print(json.dumps({k: round(v.get("mfma_busy_fraction_of_kernel", 0), 3) for k, v in res.items()}))
PY
python3 tools/stamps_step.py > $out/stamps_optimizer_launch.txt 2>&1
SEEDS=16 python3 tools/acc_sweep.py > $out/acc_sweep.txt 2>&1
tail -2 $out/acc_sweep.txt
