"""Static instruction census of fast_kernel per phase, from gfx950 assembly.

    hipcc <FLAGS of uav_airvision_amd/build.py> -S --cuda-device-only uav_airvision_amd/csrc/fast.hip -o fast.s
    python profiles/fast_diet/census.py fast.s

The kernel's workgroup barriers separate its stages: staging | phase 1 and phase 2 | (the survivor counter is zeroed) | phase 3 |
write-out.  Phase 2 is the one loop between the first two barriers; phase 1 is what remains there (its four iterations are unrolled,
so its count is that of four quads with every path).  All paths are counted: the clamped staging of border tiles beside the plain
one, the byte path of unaligned rows, the mask branches.  What a wavefront executes is what the counters say (README.md).
"""
import re
import sys

KINDS = ('valu', 'lds', 'vmem', 'salu')


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


def body_of(path, want='fast_kernel'):
    lines = open(path).read().split('\n')
    for i, l in enumerate(lines):
        m = re.match(r'^(_Z\w+):', l)
        if m and want in m.group(1):
            j = i + 1
            while j < len(lines) and not re.match(r'^\.Lfunc_end', lines[j]):
                j += 1
            return lines[i + 1:j], lines
    raise SystemExit('no %s in %s' % (want, path))


def count(lines):
    c = dict.fromkeys(KINDS, 0)
    ops = {}
    for l in lines:
        t = l.strip().split()
        if t and kind(t[0]):
            c[kind(t[0])] += 1
            ops[t[0]] = ops.get(t[0], 0) + 1
    return c, ops


def loops_of(lines):
    """[(header label, lines)] for the blocks the compiler marks as one loop, in source order."""
    per, order, cur = {}, [], None
    for l in lines:
        lm = re.match(r'^\.L(BB\w+):(.*)$', l)
        if lm:
            hm = re.search(r'Header=(BB\w+)', lm.group(2))
            cur = lm.group(1) if 'Loop Header' in lm.group(2) else (hm.group(1) if hm else None)
            if cur and cur not in per:
                per[cur] = []
                order.append(cur)
            continue
        if cur:
            per[cur].append(l)
    return [(h, per[h]) for h in order]


def census(path):
    body, whole = body_of(path)
    cuts = [i for i, l in enumerate(body) if re.match(r'^\s*s_barrier', l)]
    assert len(cuts) >= 4, 'expected the four barriers of the three phases'
    sec = {'staging': body[:cuts[0]], 'phase 1 + 2': body[cuts[0]:cuts[1]], 'phase 3': body[cuts[2]:cuts[3]], 'write-out': body[cuts[3]:]}
    out = [('whole kernel', count(body))]
    out.append(('staging (all paths)', count(sec['staging'])))
    for h, ll in loops_of(sec['staging']):
        out.append(('  of which loop %s (byte path)' % h, count(ll)))
    p12 = count(sec['phase 1 + 2'])
    loops = loops_of(sec['phase 1 + 2'])
    p2 = max(loops, key=lambda x: count(x[1])[0]['lds'])[1] if loops else []
    c2 = count(p2)
    c1 = ({k: p12[0][k] - c2[0][k] for k in KINDS}, {o: n - c2[1].get(o, 0) for o, n in p12[1].items() if n - c2[1].get(o, 0)})
    out.append(('phase 1 (four unrolled iterations, four quad positions each)', c1))
    out.append(('phase 2 (loop body, 64 candidates)', c2))
    out.append(('phase 3 (three unrolled iterations, all mask paths)', count(sec['phase 3'])))
    out.append(('write-out', count(sec['write-out'])))
    meta = {}
    for l in whole:
        m = re.match(r'^\s*\.(sgpr_count|vgpr_count|sgpr_spill_count|vgpr_spill_count|group_segment_fixed_size|private_segment_fixed_size):\s*(\d+)', l)
        if m:
            meta[m.group(1)] = int(m.group(2))
    return out, meta


if __name__ == '__main__':
    rows, meta = census(sys.argv[1])
    for name, (c, ops) in rows:
        print('%-66s VALU %4d  LDS %3d  VMEM %3d  SALU %3d' % (name, c['valu'], c['lds'], c['vmem'], c['salu']))
        if '-v' in sys.argv and not name.startswith('whole'):
            print('      ' + '  '.join('%s %d' % (o, n) for o, n in sorted(ops.items(), key=lambda x: -x[1]) if kind(o) in ('valu', 'lds'))[:900])
    print('resources: ' + '  '.join('%s %d' % kv for kv in sorted(meta.items())))
