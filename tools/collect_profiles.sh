# One GPU-box session: full GPU test suite, smoke, the default bench line, and for ONE arithmetic mode the rocprofv3 kernel
# stats + per-op trace table + three PMC passes.
# usage: bash tools/collect_profiles.sh <tag> [precision: f16x3 | f16] [skip-tests]
# (outputs under results/; copy what should be judged into profiles/)
TAG=${1:-r06}
PREC=${2:-f16x3}
mkdir -p results
if [ "$3" != "skip-tests" ]; then
  timeout -k 5 2700 python -m pytest tests -m gpu -q --durations=25 > results/pytest_gpu_$TAG.log 2>&1; echo "pytest rc=$?"; tail -3 results/pytest_gpu_$TAG.log
  python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -3
  timeout -k 5 900 python bench.py --full --steps 20 --warmup 5 > results/bench_$TAG.log 2>&1; tail -1 results/bench_$TAG.log > results/bench_$TAG.json
  python - <<PY
import json
d=json.load(open("results/bench_$TAG.json"))
print("BENCH", d["dtype"], d["value"], d["unit"], d["ms_per_step"], "ms/step; roofline", d["roofline"]["kernel"], d["roofline"]["frac"], d["roofline"].get("frac_issued"))
print("  modes", (d.get("roofline") or {}).get("modes"))
print("  extras", d.get("extras")); print("  cpu", d["cpu_baseline"]["value"] if d.get("cpu_baseline") else None)
PY
fi
ARGS="--full --precision $PREC --no-cpu-baseline --no-second-mode --no-extras"
SBBSEG_BENCH_OPS=results/ops_${TAG}_$PREC.json timeout -k 5 600 python bench.py --steps 5 --warmup 2 $ARGS > results/bench_${TAG}_$PREC.log 2>&1
REPO=$(pwd)
(cd /tmp && export TMPDIR=/tmp && timeout -k 5 600 rocprofv3 --kernel-trace --stats --output-format csv -d $REPO/results/prof_$TAG -o prof -- python $REPO/bench.py --steps 5 --warmup 2 $ARGS > $REPO/results/rocprof_$TAG.log 2>&1)
F=$(find results/prof_$TAG -name "*kernel_stats.csv" | head -1); [ -n "$F" ] && cp "$F" results/kernel_stats_${TAG}_$PREC.csv && head -8 "$F"
T=$(find results/prof_$TAG -name "*kernel_trace.csv" | head -1); [ -n "$T" ] && python tools/trace_per_op.py "$T" results/ops_${TAG}_$PREC.json > results/kernel_trace_per_op_${TAG}_$PREC.md 2>&1; tail -5 results/kernel_trace_per_op_${TAG}_$PREC.md
rm -rf results/prof_$TAG
BENCH_ARGS="$ARGS" bash tools/pmc_run.sh pmc_$TAG > results/pmc_run_$TAG.log 2>&1
python tools/pmc_report.py pmc_$TAG results/ops_${TAG}_$PREC.json results/pmc_summary_${TAG}_$PREC.json $PREC 140 > results/pmc_per_op_${TAG}_$PREC.txt 2>&1; tail -12 results/pmc_per_op_${TAG}_$PREC.txt
rm -rf results/pmc_${TAG}_sq results/pmc_${TAG}_fetch results/pmc_${TAG}_write
