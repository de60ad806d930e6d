#!/bin/bash
# One gpurun call that regenerates the r02_* evidence under gpurun_out/r02/ (copied into profiles/ afterwards).
cd $GRAFT_REPO_ROOT
O=gpurun_out/r02; mkdir -p $O
timeout 600 python bench.py --full > $O/bench_cfg2.json 2> $O/bench_cfg2.err; tail -1 $O/bench_cfg2.json | cut -c1-200
for c in cfg3 cfg4 cfg5; do timeout 400 python bench.py --full --config $c --no-cpu-baseline --no-extras > $O/bench_$c.json 2>/dev/null; tail -1 $O/bench_$c.json | cut -c1-160; done
BENCH="python $GRAFT_REPO_ROOT/bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-roofline --no-extras"
cd /tmp && export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $GRAFT_REPO_ROOT/$O/prof -- $BENCH > /dev/null 2>&1
BENCH1="python $GRAFT_REPO_ROOT/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-roofline --no-extras"
timeout 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $GRAFT_REPO_ROOT/$O/pmc_fetch -- $BENCH1 > /dev/null 2>&1
timeout 600 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $GRAFT_REPO_ROOT/$O/pmc_write -- $BENCH1 > /dev/null 2>&1
timeout 600 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d $GRAFT_REPO_ROOT/$O/pmc_sq -- $BENCH1 > /dev/null 2>&1
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OLDPWD/$O/prof_default -- python $OLDPWD/bench.py --full --no-cpu-baseline --no-extras > $OLDPWD/$O/default_bench_under_rocprof.json 2>/dev/null
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $GRAFT_REPO_ROOT/$O/prof_cfg5 -- python $GRAFT_REPO_ROOT/bench.py --config cfg5 --steps 2 --warmup 1 --no-cpu-baseline --no-roofline --no-extras > /dev/null 2>&1
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $GRAFT_REPO_ROOT/$O/prof_train -- python -c "
import sys; sys.path.insert(0, '$GRAFT_REPO_ROOT')
import bench
print(bench.training_leg(steps=40, baseline=False))
" > /dev/null 2>&1
cd $GRAFT_REPO_ROOT
cp $(find $O/prof_cfg5 -name "*kernel_stats.csv" | head -1) $O/cfg5_kernel_stats.csv
cp $(find $O/prof_train -name "*kernel_stats.csv" | head -1) $O/train_kernel_stats.csv
rm -rf $O/prof_cfg5 $O/prof_train
timeout 900 python -c "
import json, bench
print(json.dumps({'batch32_D4': bench.training_leg(), 'batch128_D14': bench.training_leg(B=128, D=14)}, indent=1))
" 2>/dev/null > $O/training.json
cp $(find $O/prof -name "*kernel_stats.csv" | head -1) $O/cfg2_kernel_stats.csv
cp $(find $O/prof_default -name "*kernel_stats.csv" | head -1) $O/default_cmd_kernel_stats.csv
python tools/pmc_traffic.py $O/pmc_fetch $O/pmc_write 100 > $O/pmc_traffic.json
python tools/pmc_summary.py $O/pmc_sq > $O/pmc_sq_summary.json
rm -rf $O/prof $O/prof_default $O/pmc_fetch $O/pmc_write $O/pmc_sq
timeout 300 python tools/fused_trace.py 100 2>&1 | grep -v amdgpu > $O/fused_trace.txt
timeout 300 python tools/layer_trace.py 100 2>&1 | grep -v amdgpu > $O/layer_trace.txt
MPDX_BENCH_TABLE=1 timeout 300 python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extras 2>&1 >/dev/null | grep "^#" > $O/launch_table.txt
head -4 $O/cfg2_kernel_stats.csv | cut -c1-160
