"""Static instruction census of lk_track_g16_kernel<15> from gfx950 assembly: one Newton trip and one level set-up.

    hipcc <FLAGS of uav_airvision_amd/build.py> -S --cuda-device-only uav_airvision_amd/csrc/lk.hip -o lk.s
    python profiles/lk_diet/census.py lk.s [-v]

Block boundaries (the compiler's labels differ between builds; the script finds them by what the blocks contain):

  Newton trip  = the depth-2 loop that holds the "; fp64 step test" marker.  The census WALKS the path a trip takes when no lane
                 leaves the loop, no lane restages and the fp64 test is not needed, from the loop header back to it:
                   * a conditional branch to a block of the loop is TAKEN when the basic block it jumps over (the fall-through up to
                     the next label or branch) opens the J restaging ("; wave barrier"), is the fp64 test (its marker), or holds
                     nothing but register moves and scalar instructions (an exit block: it only copies state for lanes that leave);
                   * every other conditional branch falls through (the lanes are in the image, the step has not converged, no
                     lane leaves the loop);
                   * s_branch is followed.
                 Every decision is printed with -v.
  Level set-up = the text from the header of the depth-1 loop (the levels) to the first block of the Newton loop, cut at the two
                 "; wave barrier" marks of the I staging: head | I staging (all paths: pyramid, in-place image, border) | patch
                 set-up.  From the patch set-up the border-mask block is taken out: the fall-through of the first s_cbranch_vccz
                 after the staging (the ballot over !inside).

Rates: "full" = mnemonics that profiles/r05/valu_issue_microbench.json prices at <= 2 ticks per wave-instruction and SIMD with
four waves (v_add/sub_u32, shifts, v_and/or/xor, v_mov_b32, float add / mul / fma); "half" = priced at about 3 (conversions,
compares, v_perm, v_dot2*, DPP adds, v_cndmask, v_add3, v_floor, ...); "n/m" = not in that table (v_pk_*_f32, v_mov_b64, fp32 division
steps).
"""
import re
import sys

FULL = ('v_add_u32', 'v_sub_u32', 'v_subrev_u32', 'v_ashrrev_i32', 'v_lshlrev_b32', 'v_lshrrev_b32', 'v_and_b32', 'v_or_b32', 'v_xor_b32',
        'v_mov_b32', 'v_add_f32', 'v_sub_f32', 'v_subrev_f32', 'v_mul_f32', 'v_fma_f32', 'v_fmac_f32')
NOT_MEASURED = ('v_pk_add_f32', 'v_pk_mul_f32', 'v_pk_fma_f32', 'v_mov_b64', 'v_div_scale_f32', 'v_div_fmas_f32', 'v_div_fixup_f32',
                'v_lshl_add_u64', 'v_mad_i64_i32', 'v_cmp_class_f32')
KERNEL = 'lk_track_g16_kernelILi15'


def base(op):
    op = re.sub(r'_(e32|e64|dpp|sdwa|e64_dpp)$', '', op)
    return op


def rate(op):
    b = base(op)
    if op.endswith('_dpp') and b == 'v_add_u32':
        return 'half'
    if b in FULL:
        return 'full'
    if b in NOT_MEASURED:
        return 'n/m'
    return 'half'


def kernel_lines(path):
    lines = open(path).read().split('\n')
    for i, l in enumerate(lines):
        m = re.match(r'^(_Z\w+):', l)
        if m and KERNEL in m.group(1):
            j = i + 1
            while j < len(lines) and not re.match(r'^\.Lfunc_end', lines[j]):
                j += 1
            return lines[i + 1:j], lines
    raise SystemExit('no %s in %s' % (KERNEL, path))


def ops_of(lines):
    out = []
    for l in lines:
        t = l.strip().split()
        if t and re.match(r'^[vs]_|^ds_|^global_|^buffer_|^flat_', t[0]):
            out.append(t[0])
    return out


def tally(ops):
    c = {'valu': 0, 'full': 0, 'half': 0, 'n/m': 0, 'salu': 0, 's_nop': 0, 'lds': 0, 'vmem': 0}
    by = {}
    for o in ops:
        if o.startswith('v_'):
            c['valu'] += 1
            c[rate(o)] += 1
            b = base(o) + ('_dpp' if o.endswith('dpp') else '')
            by[b] = by.get(b, 0) + 1
        elif o == 's_nop':
            c['s_nop'] += 1
        elif o.startswith('s_'):
            c['salu'] += 1
        elif o.startswith('ds_'):
            c['lds'] += 1
        else:
            c['vmem'] += 1
    return c, by


def find_loops(body):
    """label -> (line index, depth) of loop headers; the header comment may continue on the following lines"""
    heads = {}
    for i, l in enumerate(body):
        m = re.match(r'^\.L(BB\d+_\d+):', l)
        if not m:
            continue
        txt = l
        k = i + 1
        while k < len(body) and body[k].strip().startswith(';') and not body[k].strip().startswith('; %bb'):
            txt += body[k]
            k += 1
        hm = re.search(r'This (?:Inner )?Loop Header: Depth=(\d+)', txt)
        if hm:
            heads[m.group(1)] = (i, int(hm.group(1)))
    return heads


def label_index(body):
    return {m.group(1): i for i, l in enumerate(body) for m in [re.match(r'^\.L(BB\d+_\d+):', l)] if m}


def loop_members(body, header):
    """labels of the blocks of a loop: the header, and every label whose comment names it (blocks, child loops)"""
    mem = {header}
    for i, l in enumerate(body):
        m = re.match(r'^\.L(BB\d+_\d+):', l)
        if not m:
            continue
        txt, k = l, i + 1
        while k < len(body) and body[k].strip().startswith(';') and not body[k].strip().startswith('; %bb'):
            txt += body[k]
            k += 1
        if re.search(r'(Header=|Parent Loop )%s ' % header, txt):
            mem.add(m.group(1))
    return mem


def only_moves(region):
    ops = ops_of(region)
    return bool(ops) and all(o.startswith('s_') or base(o) in ('v_mov_b32', 'v_mov_b64') for o in ops)


def walk_trip(body, verbose):
    heads, where = find_loops(body), label_index(body)
    mark = next(i for i, l in enumerate(body) if 'fp64 step test' in l)
    # the Newton loop: the depth-2 header whose blocks (marked "Header=<label>") include the one with the marker
    k = mark
    while not re.search(r'Header=(BB\d+_\d+)', body[k]) and not re.match(r'^\.L(BB\d+_\d+):', body[k]):
        k -= 1
    newton = re.search(r'Header=(BB\d+_\d+)', body[k]).group(1)
    assert heads[newton][1] == 2, 'the marker is expected in the depth-2 loop'
    start = heads[newton][0]
    members = loop_members(body, newton)
    path, i, steps, notes = [], start + 1, 0, []
    while steps < 5000:
        steps += 1
        l = body[i]
        if i != start + 1 and re.match(r'^\.L%s:' % newton, l):
            break
        t = l.strip().split()
        if t and t[0] == 's_branch':
            path.append(t[0])
            i = where[t[1].lstrip('.L')]
            continue
        if t and t[0].startswith('s_cbranch'):
            path.append(t[0])
            tgt = where[t[1].lstrip('.L')]
            if tgt == start:      # the back edge itself (a loop that closes with a conditional branch to its header)
                break
            e = i + 1             # the fall-through basic block: up to the next label or branch
            while not re.match(r'^\.LBB', body[e]) and not body[e].strip().startswith(('s_cbranch', 's_branch')):
                e += 1
            region = body[i + 1:e + 1]
            txt = '\n'.join(region)
            inside = t[1].lstrip('.L') in members
            take = inside and ('wave barrier' in txt or 'fp64 step test' in txt or only_moves(region))
            notes.append('    line +%d %s %s: %s' % (i, t[0], t[1], 'taken' if take else 'falls through'))
            i = tgt if take else i + 1
            continue
        if t and re.match(r'^[vs]_|^ds_|^global_', t[0]):
            path.append(t[0])
        i += 1
    if verbose:
        print('\n'.join(notes))
    first = min([start] + [j for j, l in enumerate(body) if re.search(r'in Loop: Header=%s ' % newton, l)])
    return path, first


def setup_parts(body, newton_first):
    heads = find_loops(body)
    lvl = min(i for (i, d) in heads.values() if d == 1)
    seg = body[lvl:newton_first]
    wb = [i for i, l in enumerate(seg) if 'wave barrier' in l]
    assert len(wb) >= 2
    head, stage, patch = seg[:wb[0]], seg[wb[0]:wb[1] + 1], seg[wb[1] + 1:]
    where = label_index(patch)
    b = next(i for i, l in enumerate(patch) if l.strip().startswith('s_cbranch_vccz'))
    tgt = where[patch[b].split()[1].lstrip('.L')]
    return head, stage, patch[:b + 1] + patch[tgt:], patch[b + 1:tgt]


def show(name, ops, verbose=True):
    c, by = tally(ops)
    print('%-44s VALU %4d (full %3d, half %3d, n/m %3d)  SALU %3d  s_nop %2d  LDS %2d  VMEM %2d' %
          (name, c['valu'], c['full'], c['half'], c['n/m'], c['salu'], c['s_nop'], c['lds'], c['vmem']))
    if verbose:
        print('      ' + '  '.join('%s %d' % kv for kv in sorted(by.items(), key=lambda x: (-x[1], x[0]))))


if __name__ == '__main__':
    body, whole = kernel_lines(sys.argv[1])
    v = '-v' in sys.argv
    trip, first = walk_trip(body, v)
    show('Newton trip, common path', trip)
    head, stage, patch, mask = setup_parts(body, first)
    show('level set-up: head', ops_of(head))
    show('level set-up: I staging, all paths', ops_of(stage), False)
    show('level set-up: patches, sums, tests', ops_of(patch))
    show('  (border-mask block, not counted above)', ops_of(mask), False)
    show('whole kernel', ops_of(body), False)
    txt = '\n'.join(whole)
    blk = txt[txt.index('.amdhsa_kernel _ZN12_GLOBAL__N_119' + KERNEL):]
    res = {k: re.search(r'\.amdhsa_%s (\d+)' % k, blk).group(1) for k in ('next_free_vgpr', 'next_free_sgpr', 'group_segment_fixed_size', 'private_segment_fixed_size')}
    print('resources: ' + '  '.join('%s %s' % kv for kv in res.items()))
