#!/usr/bin/env python3
"""compare_instances.py PARENT.txt THIS.txt -- reads the two listings that profiles/frontend_views/compare_device_code.sh writes
(disassembly and resource notes of every gfx950 code object of a build) and compares, instruction by instruction, the three photometric
kernels of the parent, PhOp<response, gain>, with the instances of this build that have the same two switches and HAS_EXPOSURE off.
The third template parameter is part of the mangled name and PhArgs is two pointers longer, so the plain diff of the script cannot be
empty: here the symbol names, the addresses and the encodings in the trailing comments are dropped and what is left -- mnemonics and
operands, and the registers / LDS / scratch of the notes -- has to be equal.  Every other kernel of the build is compared the same way.
Exit status 0 = equal.  Needs no GPU."""
import re
import sys


def kernels(path):
    """{symbol: [instruction lines]} and {symbol: {note key: value}} of one listing."""
    code, notes, cur, rec = {}, {}, None, {}
    for line in open(path):
        m = re.match(r'^<(\S+)>:$', line.strip())
        if m:
            cur = m.group(1)
            code[cur] = []
            continue
        if cur is not None and line.startswith('\t'):
            text = line.split('//')[0].strip()
            text = re.sub(r'<[^>]*>', '', text).strip()      # branch targets name the symbol
            if text:
                code[cur].append(text)
            continue
        if line.strip() == '' or line.startswith('Disassembly'):
            cur = None if line.startswith('Disassembly') else cur
        m = re.match(r'^\s*-?\s*\.(\w+):\s+(\S+)$', line)
        if m:                                          # a kernel's record starts at .agpr_count (the keys are in alphabetical order)
            k, v = m.groups()
            if k == 'agpr_count':
                rec = {}
            if k == 'name' and v.startswith('_Z'):
                notes[v] = rec
            elif k in ('group_segment_fixed_size', 'private_segment_fixed_size', 'sgpr_count', 'vgpr_count', 'sgpr_spill_count',
                       'vgpr_spill_count', 'agpr_count', 'wavefront_size', 'max_flat_workgroup_size'):
                rec[k] = v
    return code, notes


def main():
    pc, pn = kernels(sys.argv[1])
    tc, tn = kernels(sys.argv[2])
    bad = 0
    pair = {}
    for name in pc:
        twin = name.replace('4PhOpILb1ELb1EEE', '4PhOpILb1ELb1ELb0EEE').replace('4PhOpILb1ELb0EEE', '4PhOpILb1ELb0ELb0EEE').replace('4PhOpILb0ELb1EEE', '4PhOpILb0ELb1ELb0EEE')
        pair[name] = twin
    for name, twin in sorted(pair.items()):
        if not name.startswith('_Z'):
            continue
        if twin not in tc:
            print('MISSING in this build: %s' % twin)
            bad += 1
            continue
        same_code = pc[name] == tc[twin]
        # (notes are listed under the kernel's own name, without the .kd suffix)
        same_notes = pn.get(name) == tn.get(twin)
        if 'PhOp' in name:
            print('%s\n  -> %s\n  %d instructions, code %s, resources %s %s' % (name, twin, len(pc[name]), 'equal' if same_code else 'DIFFERENT',
                                                                                'equal' if same_notes else 'DIFFERENT', pn.get(name)))
        if not (same_code and same_notes):
            if 'PhOp' not in name:
                print('DIFFERENT: %s' % name)
            bad += 1
    new = sorted(k for k in tc if k.startswith('_Z') and k not in pair.values())
    print('kernels only in this build:')
    for k in new:
        print('  %s  %d instructions %s' % (k, len(tc[k]), tn.get(k)))
    print('compared %d kernels of the parent: %s' % (sum(1 for k in pair if k.startswith('_Z')), 'all equal' if not bad else '%d differ' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
