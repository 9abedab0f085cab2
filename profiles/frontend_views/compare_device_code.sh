#!/bin/bash
# compare_device_code.sh PARENT.so THIS.so OUTDIR
# Extracts every gfx950 code object of the two libraries (one per translation unit), disassembles it and lists its kernels'
# resource descriptors (llvm-readelf --notes: registers, LDS, scratch, kernarg size), then diffs parent against this commit.
# Exit status 0 = no difference.  Needs no GPU.
set -euo pipefail
LLVM=${LLVM:-/opt/rocm/llvm/bin}
out=$3; mkdir -p "$out"
dump() {      # library, tag
    "$LLVM/llvm-objcopy" --dump-section .hip_fatbin="$out/$2.fatbin" "$1" /dev/null
    # the section is a sequence of offload bundles, one per translation unit; split at the magic string and unbundle each
    python3 - "$out/$2.fatbin" "$out/$2" <<'EOF'
import sys
data, stem, magic = open(sys.argv[1], 'rb').read(), sys.argv[2], b'__CLANG_OFFLOAD_BUNDLE__'
starts = [i for i in range(len(data)) if data.startswith(magic, i)]
for k, (a, b) in enumerate(zip(starts, starts[1:] + [len(data)])):
    open('%s.%02d.bundle' % (stem, k), 'wb').write(data[a:b])
EOF
    : > "$out/$2.txt"
    for b in "$out/$2".*.bundle; do
        "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$b" --output="${b%.bundle}.co"
        { "$LLVM/llvm-objdump" -d --no-show-raw-insn --no-leading-addr "${b%.bundle}.co" | grep -v 'file format'
          "$LLVM/llvm-readelf" --notes "${b%.bundle}.co"; } >> "$out/$2.txt"
    done
}
dump "$1" parent
dump "$2" this
grep -c '^ *\.name: ' "$out/this.txt" | sed 's/^/kernels: /'
wc -l "$out/parent.txt" "$out/this.txt"
diff "$out/parent.txt" "$out/this.txt" > "$out/device_code.diff" && echo "device code identical"
