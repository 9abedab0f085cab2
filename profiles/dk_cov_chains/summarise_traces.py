#!/usr/bin/env python3
"""summarise_traces.py OUTDIR -- reads what measure.sh traces left in OUTDIR (trace_{exclusive,shared}_{parent,this}/**/*kernel_stats.csv
of rocprofv3 --kernel-trace --stats, bench_{exclusive,shared}_traced_{parent,this}.jsonl) and prints, per run, calls / mean / min / max
of dk_cov<64> and lk_track_g16_kernel<15> in microseconds, the ten kernels with the largest total time, and the bench line's
kernel_ms_per_step.  Writes the same as OUTDIR/trace_summary.json.  Needs no GPU."""
import csv
import glob
import json
import os
import re
import sys

WATCH = ('dk_cov<64>', 'lk_track_g16_kernel<15>')


def short(name):
    name = re.sub(r'\(anonymous namespace\)::', '', name).replace('void ', '')
    return re.sub(r'\(.*$', '', name)


def stats(path):
    rows = {}
    for r in csv.DictReader(open(path)):
        calls, mean = int(r['Calls']), float(r['AverageNs'])
        rows[short(r['Name'])] = dict(calls=calls, mean_us=mean / 1e3, min_us=float(r.get('MinNs') or 'nan') / 1e3, max_us=float(r.get('MaxNs') or 'nan') / 1e3,
                                      total_ms=float(r.get('TotalDurationNs') or calls * mean) / 1e6)
    return rows


def main():
    out, summary = sys.argv[1], {}
    for run in ('exclusive', 'shared'):
        for tag in ('parent', 'this'):
            found = glob.glob(os.path.join(out, 'trace_%s_%s' % (run, tag), '**', '*kernel_stats.csv'), recursive=True)
            if not found:
                continue
            rows = stats(found[0])
            line = open(os.path.join(out, 'bench_%s_traced_%s.jsonl' % (run, tag))).read().strip()
            bench = json.loads(line) if line else {}
            top = sorted(rows.items(), key=lambda kv: -kv[1]['total_ms'])[:10]
            summary['%s_%s' % (run, tag)] = dict(watch={k: rows.get(k) for k in WATCH}, top10={k: v for k, v in top},
                                                 value=bench.get('value'), kernel_ms_per_step=bench.get('kernel_ms_per_step'))
            print('== %s, %s library: %s stereo frames/s under the tracer' % (run, tag, bench.get('value')))
            for k in WATCH:
                v = rows.get(k)
                if v:
                    print('  %-28s calls %5d  mean %9.1f us  min %9.1f  max %9.1f' % (k, v['calls'], v['mean_us'], v['min_us'], v['max_us']))
            for k, v in top:
                print('    top %-40s calls %5d  mean %9.1f us  total %9.2f ms' % (k[:40], v['calls'], v['mean_us'], v['total_ms']))
            print('  kernel_ms_per_step %s' % json.dumps(bench.get('kernel_ms_per_step')))
    json.dump(summary, open(os.path.join(out, 'trace_summary.json'), 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
