#!/bin/bash
# End-of-round measurement (round 3): tests, bench, kernel trace, PMC passes.
# Run on the GPU box:  gpurun -- bash tools/measure/profile_round3.sh
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/r3; mkdir -p $O
cd $R
SHA=$(python -c "from sofima_amd import _build; print(_build.source_hash())")
timeout 2400 python -m pytest tests -m gpu -q -rf --tb=line 2>&1 | grep -E "^FAILED|passed|failed|error" | tail -12 > $O/pytest.log
timeout 900 python bench.py --full --steps 20 --warmup 2 > $O/bench.json 2> $O/bench.err
timeout 600 python bench.py --full --steps 5 --warmup 1 --pair exact --no-cpu-baseline > $O/bench_exact.json 2> /dev/null
timeout 600 python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-legs --sustain 1 --mesh-sharded 2 > $O/bench_sharded2.json 2> /dev/null
timeout 600 python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-legs --sustain 1 --mesh-sharded 4 > $O/bench_sharded4.json 2> /dev/null
cd /tmp && export TMPDIR=/tmp
# production launches only in the traced / counted runs: no un-pruned legs, no sustained loop
B="python $R/bench.py --no-cpu-baseline --no-legs --sustain 0"
timeout 600 rocprofv3 --kernel-trace --stats -d $O/trace -o r3 -- $B --steps 3 --warmup 1 > $O/trace.log 2>&1
python $R/tools/rocpd_summary.py $(find $O/trace -name '*.db' | head -1) > $O/trace_summary.md 2>&1
# the same with the roofline legs on (un-pruned pair, other pair, aux_rooflines: FFT form, volumetric / large meshes)
timeout 600 rocprofv3 --kernel-trace --stats -d $O/trace_aux -o r3 -- python $R/bench.py --full --no-cpu-baseline --sustain 0 --steps 1 --warmup 1 > $O/trace_aux.log 2>&1
python $R/tools/rocpd_summary.py $(find $O/trace_aux -name '*.db' | head -1) > $O/trace_aux_summary.md 2>&1
timeout 600 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_f -o f -- $B --steps 1 --warmup 1 > $O/pmc_f.log 2>&1
timeout 600 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_w -o w -- $B --steps 1 --warmup 1 > $O/pmc_w.log 2>&1
python $R/tools/pmc_summary.py $(find $O/pmc_f -name '*counter_collection.csv' | head -1) $(find $O/pmc_w -name '*counter_collection.csv' | head -1) $O/pmc_traffic.json $SHA 40401 > $O/pmc_summary.log 2>&1
python - <<PY
import json
p = '$O/pmc_traffic.json'
d = json.load(open(p)); d['_meta']['pair'] = 'warped'; json.dump(d, open(p, 'w'), indent=1)
PY
timeout 600 rocprofv3 --pmc SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_sq -o sq -- $B --steps 1 --warmup 1 --mesh-iters 10 > $O/pmc_sq.log 2>&1
python - <<PY > $O/pmc_sq_summary.txt 2>&1
import csv, collections, glob
f = glob.glob('$O/pmc_sq/**/*counter_collection.csv', recursive=True)[0]
agg = collections.defaultdict(lambda: collections.defaultdict(lambda: [0, 0.0]))
for r in csv.DictReader(open(f)):
  a = agg[r['Kernel_Name'][:60]][r['Counter_Name']]; a[0] += 1; a[1] += float(r['Counter_Value'])
for k, v in agg.items():
  print(k, {c: (n, s / n) for c, (n, s) in v.items()})
PY
SFM_MFMA_PRUNE=0 timeout 600 rocprofv3 --pmc SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_sq_full -o sq -- $B --steps 1 --warmup 1 --mesh-iters 10 > $O/pmc_sq_full.log 2>&1
python - <<PY > $O/pmc_sq_full_summary.txt 2>&1
import csv, collections, glob
f = glob.glob('$O/pmc_sq_full/**/*counter_collection.csv', recursive=True)[0]
agg = collections.defaultdict(lambda: collections.defaultdict(lambda: [0, 0.0]))
for r in csv.DictReader(open(f)):
  a = agg[r['Kernel_Name'][:60]][r['Counter_Name']]; a[0] += 1; a[1] += float(r['Counter_Value'])
for k, v in agg.items():
  print(k, {c: (n, s / n) for c, (n, s) in v.items()})
PY
cd $R
python $R/tools/measure/montage_time.py > $O/montage_time.log 2>&1
python $R/tools/measure/mesh3d_time.py > $O/mesh3d_time.log 2>&1
python $R/tools/measure/mesh_big.py > $O/mesh_big.log 2>&1
python $R/tools/measure/masked_time.py > $O/masked_time.log 2>&1
python $R/tools/measure/configs_time.py > $O/configs_time.log 2>&1
python $R/tools/measure/banded_c_loop.py > $O/banded.log 2>&1
bash $R/tools/measure/pmc_mesh2d.sh > $O/pmc_mesh2d.txt 2>&1
python $R/tools/measure/mesh2d_xcd.py 2>&1 | grep -v amdgpu > $O/mesh2d_xcd.log
python $R/tools/measure/patch_size_rates.py 2>&1 | grep -v amdgpu > $O/patch_size_rates.log
python $R/tools/measure/montage3d_time.py 2>&1 | grep volumetric > $O/montage3d_time.log
DRIFT=0 python $R/tools/measure/montage3d_time.py 2>&1 | grep volumetric >> $O/montage3d_time.log
rm -rf $O/trace/*/*.db.tmp; find $O -name '*.db' -size +20M -delete; find $O -name '*.csv' -size +5M -delete
cat $O/pytest.log $O/bench.json; tail -3 $O/bench.err
