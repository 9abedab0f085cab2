"""summarize_pmc.py COUNTER_COLLECTION.csv OUT.json -- per-kernel means of one `rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES` pass
(--output-format csv): dispatches, SQ_INSTS_VALU and SQ_WAVES per launch, and their quotient.  The layout is that of
profiles/lk_diet/pmc_frontend_s512_*.json (kernel names cut at 160 characters)."""
import csv
import json
import sys
from collections import defaultdict

per = defaultdict(lambda: defaultdict(float))          # (kernel, dispatch) -> counter -> value, summed over the rows of one dispatch
with open(sys.argv[1]) as f:
    for row in csv.DictReader(f):
        per[(row['Kernel_Name'][:160], row['Dispatch_Id'])][row['Counter_Name']] += float(row['Counter_Value'])
acc = defaultdict(lambda: defaultdict(list))
for (k, _d), cs in per.items():
    for c, v in cs.items():
        acc[k][c].append(v)
out = {}
for k, cs in acc.items():
    valu, waves = cs.get('SQ_INSTS_VALU', []), cs.get('SQ_WAVES', [])
    if not valu or not waves:
        continue
    e = {'dispatches': len(valu), 'SQ_INSTS_VALU_per_launch': sum(valu) / len(valu), 'SQ_WAVES_per_launch': sum(waves) / len(waves)}
    e['SQ_INSTS_VALU_per_wave'] = sum(valu) / sum(waves) if sum(waves) else None
    out[k] = e
json.dump(dict(sorted(out.items(), key=lambda kv: -kv[1]['SQ_INSTS_VALU_per_launch'] * kv[1]['dispatches'])), open(sys.argv[2], 'w'), indent=1)
lk = [e for k, e in out.items() if 'lk_track_g16_kernel' in k]
print(json.dumps(lk))
