#!/bin/bash
# Short end-of-session check on the GPU box: the whole -m gpu suite, smoke, the default bench line and cfg4.
export TMPDIR=/tmp
o=${1:?usage: bash tools/final_check.sh OUT_DIR}; mkdir -p "$o"
python -m pytest tests -m gpu -q 2>&1 | tail -8 | tee $o/gpu_tests_final.log
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | grep -v amdgpu.ids | tee $o/smoke_final.log
python bench.py --full --steps 2 --warmup 1 > $o/bench_cfg2.json 2> $o/bench_cfg2.err
python bench.py --full --config cfg4 --steps 1 --warmup 1 > $o/bench_cfg4.json 2> $o/bench_cfg4.err
for c in 2 4; do python -c "
import json; d=json.load(open('$o/bench_cfg$c.json')); print('cfg$c', d['value'], d.get('value_batch256'), d['roofline']['profile_key'], d['roofline']['frac'], d['roofline'].get('traffic'))"; done
