"""Static instruction census of the fused pyramid kernels from gfx950 assembly.

    hipcc <FLAGS of uav_airvision_amd/build.py> -S --cuda-device-only uav_airvision_amd/csrc/pyramid.hip -o pyramid.s
    python profiles/pyramid_diet/census.py pyramid.s

Per kernel: VALU / LDS / VMEM / SALU instructions in all, then one line per loop: the instructions of all blocks the compiler
marks as belonging to it ("Loop Header" / "in Loop: Header=..."), in source order.  A loop the compiler emitted twice (a flat index
split by multiplication or, for a launch beyond the bound of that, by division) has all its instructions on one line.
"""
import re
import sys


def kind(op):
    if op.startswith('v_'):
        return 'valu'
    if op.startswith('ds_'):
        return 'lds'
    if op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
        return 'vmem'
    if op.startswith('s_'):
        return 'salu'
    return None


def census(path, want=('pyr_l0l1_kernel', 'pyr_l2l3_kernel')):
    lines = open(path).read().split('\n')
    out = []
    i = 0
    while i < len(lines):
        m = re.match(r'^(_Z\w+):', lines[i])
        if not m or not any(w in m.group(1) for w in want):
            i += 1
            continue
        name = m.group(1)
        body = []
        i += 1
        while i < len(lines) and not lines[i].startswith('\t.end_amdhsa_kernel') and not re.match(r'^\s*s_endpgm', lines[i]):
            body.append(lines[i])
            i += 1
        # the kernel may have several s_endpgm (early exit): keep reading until the size directive
        while i < len(lines) and not lines[i].startswith('\t.size') and not re.match(r'^\.Lfunc_end', lines[i]):
            body.append(lines[i])
            i += 1
        # the compiler marks every block of a loop: "=>This Inner Loop Header" on the header, "in Loop: Header=BBn_m" on the others
        tot = {'valu': 0, 'lds': 0, 'vmem': 0, 'salu': 0}
        per, order, cur = {}, [], None
        for l in body:
            lm = re.match(r'^\.L(BB\w+):(.*)$', l)
            if lm:
                hm = re.search(r'Header=(BB\w+)', lm.group(2))
                cur = lm.group(1) if 'Loop Header' in lm.group(2) else (hm.group(1) if hm else None)
                if cur and cur not in per:
                    per[cur] = {'valu': 0, 'lds': 0, 'vmem': 0, 'salu': 0}
                    order.append(cur)
                continue
            t = l.strip().split()
            if t and kind(t[0]):
                tot[kind(t[0])] += 1
                if cur:
                    per[cur][kind(t[0])] += 1
        loops = [(h, k, per[h]) for k, h in enumerate(order)]
        out.append((name, tot, loops))
    return out


if __name__ == '__main__':
    for name, tot, loops in census(sys.argv[1]):
        print('%s: VALU %d  LDS %d  VMEM %d  SALU %d' % (name, tot['valu'], tot['lds'], tot['vmem'], tot['salu']))
        for lab, at, c in sorted(loops, key=lambda x: x[1]):
            print('    loop %-12s VALU %4d  LDS %3d  VMEM %3d' % (lab, c['valu'], c['lds'], c['vmem']))
