#!/bin/bash
# Full end-of-round measurement: tests, bench, kernel trace, PMC passes.
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/r1g; mkdir -p $O
cd $R
timeout 900 python -m pytest tests -m gpu -x -q 2>&1 | tail -3 > $O/pytest.log
timeout 600 python bench.py --full > $O/bench.json 2> $O/bench.err
cd /tmp && export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $O/trace -o r1g -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $O/trace.log 2>&1
python $R/tools/rocpd_summary.py $(find $O/trace -name '*.db' | head -1) > $O/trace_summary.md 2>&1
timeout 600 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_f -o f -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --mesh-iters 1000 > $O/pmc_f.log 2>&1
timeout 600 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_w -o w -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --mesh-iters 1000 > $O/pmc_w.log 2>&1
python $R/tools/pmc_summary.py $(find $O/pmc_f -name '*counter_collection.csv' | head -1) $(find $O/pmc_w -name '*counter_collection.csv' | head -1) $O/pmc_traffic.json > $O/pmc_summary.log 2>&1
timeout 600 rocprofv3 --pmc SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_sq -o sq -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --mesh-iters 10 > $O/pmc_sq.log 2>&1
python - <<PY > $O/pmc_sq_summary.txt 2>&1
import csv, collections, glob
f = glob.glob('$O/pmc_sq/**/*counter_collection.csv', recursive=True)[0]
agg = collections.defaultdict(lambda: collections.defaultdict(lambda: [0, 0.0]))
for r in csv.DictReader(open(f)):
  a = agg[r['Kernel_Name'][:60]][r['Counter_Name']]; a[0] += 1; a[1] += float(r['Counter_Value'])
for k, v in agg.items():
  print(k, {c: (n, s / n) for c, (n, s) in v.items()})
PY
rm -rf $O/trace/*/*.db.tmp; find $O -name '*.db' -size +20M -delete
cat $O/pytest.log $O/bench.json; tail -3 $O/bench.err
