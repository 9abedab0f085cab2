"""compare_kernels.py PARENT.txt THIS.txt -- per-kernel comparison of two device-code listings.

The listings are what profiles/frontend_views/compare_device_code.sh writes (OUT/parent.txt, OUT/this.txt: disassembly and
resource notes of every gfx950 code object of a library).  Its whole-file diff is of no use once a translation unit gains a kernel:
every later address moves, and the listing prints addresses.  This compares kernel by kernel instead: the instruction text with the
addresses (the trailing comment, the absolute part of a branch target) removed, and the kernel's resource notes.  Exit status 0 =
every kernel of the parent is in this build with the same instructions and the same resources.  Needs no GPU."""
import re
import sys


def load(path):
    code, notes, cur, note = {}, {}, None, None
    for line in open(path, errors='replace'):
        m = re.match(r'^(?:[0-9a-f]+ )?<(\S+)>:\s*$', line)
        if m:
            cur = m.group(1)
            code[cur] = []
            continue
        if line.startswith('Displaying notes') or line.startswith('Disassembly of section'):
            cur = None
        m = re.match(r'^\s*-?\s*\.(\w+):\s*(\S.*)$', line)
        if m and cur is None:           # a kernel's entry runs from .agpr_count to .wavefront_size (keys in alphabetical order)
            key, val = m.group(1), m.group(2)
            if key == 'agpr_count':
                note = {}
            if note is not None and key in ('agpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size', 'kernarg_segment_size', 'sgpr_count',
                                            'sgpr_spill_count', 'vgpr_count', 'vgpr_spill_count', 'max_flat_workgroup_size', 'wavefront_size', 'symbol'):
                note[key] = val
            if note is not None and key == 'wavefront_size':
                notes[note.pop('symbol').strip("'").replace('.kd', '')] = note
                note = None
            continue
        if cur is not None:
            t = re.sub(r'\s*//.*$', '', line.rstrip())
            t = re.sub(r'<[^>]*\+0x[0-9a-f]+>', '<T>', t)
            if t.strip():
                code[cur].append(t)
    return code, notes


(ca, na), (cb, nb) = load(sys.argv[1]), load(sys.argv[2])
same = [k for k in ca if k in cb and ca[k] == cb[k]]
print('functions in the parent: %d, in this build: %d, with identical instructions: %d' % (len(ca), len(cb), len(same)))
print('resource notes in the parent: %d, in this build: %d, identical: %d' % (len(na), len(nb), sum(1 for k in na if nb.get(k) == na[k])))
bad = 0
for k in ca:
    if k not in cb:
        print('ONLY IN THE PARENT', k)
        bad += 1
    elif ca[k] != cb[k]:
        print('DIFFERENT', k, '(%d / %d instructions)' % (len(ca[k]), len(cb[k])))
        bad += 1
for k in na:
    if k in nb and na[k] != nb[k]:
        print('RESOURCES DIFFER', k, na[k], nb[k])
        bad += 1
for k in cb:
    if k not in ca:
        print('only in this build:', k, '%d instructions' % len(cb[k]), nb.get(k, ''))
sys.exit(1 if bad else 0)
