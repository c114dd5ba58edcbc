#!/bin/bash
# End-of-session validation on the GPU box (one gpurun call, ~35 min): GPU tests, the bench lines of every config, the rocprofv3
# kernel trace of the default bench, per-kernel-class microbenchmarks and the PMC passes at the timed batch.
#   bash tools/final_validation.sh OUT_DIR      (outputs under OUT_DIR; copy into profiles/)
export TMPDIR=/tmp
o=${1:?usage: bash tools/final_validation.sh OUT_DIR}; mkdir -p "$o"
python -m pytest tests -m gpu -q 2>&1 | tail -8 | tee $o/gpu_tests_final.log
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | grep -v amdgpu.ids | tee $o/smoke_final.log
python bench.py --full --steps 2 --warmup 1 > $o/bench_cfg2.json 2> $o/bench_cfg2.err
python bench.py --full --config cfg1 --steps 20 --warmup 5 > $o/bench_cfg1.json 2> $o/bench_cfg1.err
python bench.py --full --config cfg3 --steps 1 --warmup 1 > $o/bench_cfg3.json 2> $o/bench_cfg3.err
python bench.py --full --config cfg4 --steps 1 --warmup 1 > $o/bench_cfg4.json 2> $o/bench_cfg4.err
python bench.py --full --config cfg5 --steps 1 --warmup 0 > $o/bench_cfg5.json 2> $o/bench_cfg5.err
bash tools/r03_profile.sh > $o/r03_profile.log 2>&1
python bench.py --batch 128 --steps 1 --warmup 1 --no-cpu-baseline --no-batch256 > $o/bench_cfg2_b128.json 2> $o/bench_cfg2_b128.err  # what a rank holds at N = 8 (strong scaling)
DDPM_PROF_SHAPES=1 python tools/microbench.py --batch 1024 2>&1 | grep -v amdgpu.ids > $o/r03_microbench_small_b1024_per_shape.log
python tools/microbench.py --batch 128 2>&1 | grep -v amdgpu.ids > $o/r03_microbench_small_b128.log
PMC_CMD="python tools/vqvae_bench.py 1" bash tools/pmc_collect.sh $o/pmc_vqvae > $o/pmc_vqvae_collect.log 2>&1
python tools/pmc_summary.py $o/pmc_vqvae $o/r03_pmc_per_kernel_vqvae.csv $o/pmc_traffic_vqvae_scratch.json > $o/pmc_vqvae_summary.log 2>&1
rm -rf $o/pmc_vqvae/*/pmc_counter_collection.csv
python tools/up_ab.py 1024 2>&1 | grep -v amdgpu.ids > $o/up_ab_final.log
python tools/wino_ab.py 256 2>&1 | grep -v amdgpu.ids > $o/wino_ab_final.log
python tools/wino_ab.py 1024 2>&1 | grep -v amdgpu.ids >> $o/wino_ab_final.log
DDPM_WINO44_F16X3=0 python tools/wino_ab.py 1024 2>&1 | grep -v amdgpu.ids >> $o/wino_ab_final.log
python tools/vqvae_bench.py 2 2>&1 | grep -v amdgpu.ids > $o/vqvae_bench_final.log
python tools/attn_ab.py 2>&1 | grep -v amdgpu.ids > $o/attn_ab_final.log
python tests/parity_report.py --n 64 --skip 500 2>&1 | grep -v amdgpu.ids | tail -12 > $o/parity_report_final.log
for c in 1 2 3 4 5; do python -c "
import json; d=json.load(open('$o/bench_cfg$c.json')); print('cfg$c', d['value'], d.get('value_batch256'), d['roofline']['profile_key'], d['roofline']['frac'])"; done
tail -3 $o/gpu_tests_final.log; tail -4 $o/parity_report_final.log
