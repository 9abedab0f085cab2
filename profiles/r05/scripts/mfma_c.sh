#!/bin/bash
# MFMA Gram slabs + single-wavefront feature / triangulation workgroups: parity, driver command, contended timeline
set -o pipefail
O=$PWD/gpurun_out/r05q; mkdir -p $O
timeout -k 10 900 python -m pytest tests/test_gpu_msckf.py -x -q -m gpu > $O/pytest_msckf.txt 2>&1 || { tail -30 $O/pytest_msckf.txt; exit 1; }
tail -3 $O/pytest_msckf.txt
for v in "" "AV_FEAT_WG=256"; do
env $v python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-regimes > $O/bench_c.json 2> $O/e1.txt || { tail -5 $O/e1.txt; exit 1; }
python3 - $O/bench_c.json "$v" <<'PY'
import json,sys
d=json.load(open(sys.argv[1])); m=d.get('roofline_msckf') or {}
print(sys.argv[2], 'value %.0f ms/step %.2f  msckf chain %.2f excl %s' % (d['value'], d['ms_per_step'], m.get('chain_ms_per_step'), (m.get('exclusive') or {}).get('chain_ms_per_step')))
PY
done
bash profiles/r05/scripts/contended_timeline.sh && cat gpurun_out/r05y/contended_timeline.txt
