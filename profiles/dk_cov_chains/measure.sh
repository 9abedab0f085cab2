#!/bin/bash
# measure.sh PARENT.so THIS.so OUTDIR traces|pairs
# One MI355X.  PARENT.so is the parent commit's library built whole with the flags of uav_airvision_amd/build.py, THIS.so this commit's.
# The library under test is copied over uav_airvision_amd/libairvision_hip.so for each run (the binding has no other way to pick one);
# this commit's is put back at the end.  Every GPU step runs under its own time limit and the script stops at the first that fails.
#   traces: rocprofv3 --kernel-trace --stats (tracing only) around the exclusive run (AV_BENCH_SERIAL=1 AV_MSCKF_GROUPS=1,
#           --steps 10 --warmup 3) and around the default run (--steps 20 --warmup 5), parent then this; tables by summarise_traces.py
#   pairs:  five interleaved pairs, the parent first in each, of `bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR`;
#           bench_parent.jsonl / bench_this.jsonl, cmp of every dumped array against the first parent run, bench_dump_md5.txt
set -euo pipefail
parent=$(realpath "$1"); this=$(realpath "$2"); mkdir -p "$3"; out=$(realpath "$3"); what=$4
here=$(cd "$(dirname "$0")" && pwd); root=$(cd "$here/../.." && pwd); lib=$root/uav_airvision_amd/libairvision_hip.so
cp "$this" "$out/this.so"; cp "$parent" "$out/parent.so"
trap 'cp "$out/this.so" "$lib"; rm -f "$out/this.so" "$out/parent.so"' EXIT
cd "$root"
if [ "$what" = traces ]; then
    for tag in parent this; do
        cp "$out/$tag.so" "$lib"
        AV_BENCH_SERIAL=1 AV_MSCKF_GROUPS=1 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/trace_exclusive_$tag" -o t -- \
            python3 bench.py --steps 10 --warmup 3 | tail -n 1 > "$out/bench_exclusive_traced_$tag.jsonl"
        echo "exclusive $tag done"
        timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/trace_shared_$tag" -o t -- \
            python3 bench.py --steps 20 --warmup 5 | tail -n 1 > "$out/bench_shared_traced_$tag.jsonl"
        echo "shared $tag done"
    done
    python3 "$here/summarise_traces.py" "$out" | tee "$out/trace_tables.txt" || echo "summarise_traces.py failed: the raw files are in $out"
    find "$out" -name '*kernel_trace.csv' -delete          # (tens of MB each; the per-kernel statistics stay)
else
    : > "$out/bench_parent.jsonl"; : > "$out/bench_this.jsonl"
    for i in 1 2 3 4 5; do
        for tag in parent this; do
            cp "$out/$tag.so" "$lib"
            timeout -k 10 300 python3 bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs "$out/dump_${tag}_$i" | tail -n 1 >> "$out/bench_$tag.jsonl"
            echo "pair $i $tag: $(tail -n 1 "$out/bench_$tag.jsonl" | python3 -c 'import json,sys; d=json.loads(sys.stdin.read()); print(d["value"], d.get("kernel_ms_per_step", {}).get("lk"))')"
        done
    done
    bad=0
    for d in "$out"/dump_*; do
        for f in "$out"/dump_parent_1/*.npy; do cmp "$f" "$d/$(basename "$f")" || bad=$((bad + 1)); done
    done
    (cd "$out/dump_parent_1" && md5sum *.npy) > "$out/bench_dump_md5.txt"
    echo "dumped arrays that differ from the first parent run: $bad" | tee -a "$out/bench_dump_md5.txt"
    rm -rf "$out"/dump_*
    [ "$bad" -eq 0 ]
fi
