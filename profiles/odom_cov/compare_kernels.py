#!/usr/bin/env python3
"""compare_kernels.py PARENT.txt THIS.txt -- reads the two listings that profiles/frontend_views/compare_device_code.sh writes
(disassembly and resource notes of every gfx950 code object of a build) and compares every kernel of the parent with the kernel of
the same name in this build: instruction by instruction (mnemonics and operands; addresses, encodings and branch-target symbols
dropped, since a kernel added to a code object moves everything behind it) and by its resource notes (registers, LDS, scratch,
workgroup size).  Kernels that only this build has are listed with their instruction count and resources.
Exit status 0 = every kernel of the parent is unchanged.  Needs no GPU."""
import re
import sys

KEYS = ('group_segment_fixed_size', 'private_segment_fixed_size', 'sgpr_count', 'vgpr_count', 'sgpr_spill_count', 'vgpr_spill_count',
        'agpr_count', 'wavefront_size', 'max_flat_workgroup_size', 'kernarg_segment_size')


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
            text = re.sub(r'<[^>]*>', '', text).strip()
            if text:
                code[cur].append(text)
            continue
        if line.startswith('Disassembly'):
            cur = None
        m = re.match(r'^\s*-?\s*\.(\w+):\s+(\S+)$', line)
        if m:                                          # a kernel's record starts at .agpr_count (the keys are in alphabetical order)
            k, v = m.groups()
            if k == 'agpr_count':
                rec = {}
            if k == 'name' and v.startswith('_Z'):
                notes[v] = rec
            elif k in KEYS:
                rec[k] = v
    return code, notes


def main():
    pc, pn = kernels(sys.argv[1])
    tc, tn = kernels(sys.argv[2])
    bad, n = 0, 0
    for name in sorted(pc):
        if not name.startswith('_Z'):
            continue
        n += 1
        if name not in tc:
            print('MISSING in this build: %s' % name)
            bad += 1
        elif pc[name] != tc[name] or pn.get(name) != tn.get(name):
            print('DIFFERENT: %s (code %s, resources %s)' % (name, 'equal' if pc[name] == tc[name] else 'differs',
                                                             'equal' if pn.get(name) == tn.get(name) else 'differ'))
            bad += 1
        elif 'dk_' in name:
            print('equal: %s  %d instructions %s' % (name, len(pc[name]), pn.get(name)))
    print('kernels only in this build:')
    for k in sorted(k for k in tc if k.startswith('_Z') and k not in pc):
        print('  %s  %d instructions %s' % (k, len(tc[k]), tn.get(k)))
    print('compared %d kernels of the parent: %s' % (n, 'all equal' if not bad else '%d differ' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
