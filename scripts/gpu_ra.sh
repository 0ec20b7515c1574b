#!/bin/bash
# Regime A checks: the RCCL / two-graph tests, the Regime A suite, then the bench's Regime A line with its
# data-parallel world-1 RCCL sub-record
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 2
OUT=${OUT:-bench_out}/ra; mkdir -p "$OUT"
TESTS="tests/test_gpu_rccl.py tests/test_gpu_regime_a.py" NAME=ra_tests TLIM=600 bash scripts/gpu_check.sh || exit 1
timeout -k 10 300 python3 bench.py --full --regime hensman --no-cpu-baseline > "$OUT/ra.json" 2> "$OUT/ra.err" || { tail -20 "$OUT/ra.err"; exit 1; }
python3 -c "
import json; d = json.load(open('$OUT/ra.json'))
print('regime A', round(d['ms_per_step'], 3), 'ms; dp world-1 RCCL', d.get('dp_world1_rccl'))"
