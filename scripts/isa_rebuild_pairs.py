#!/usr/bin/env python3
"""Flag-rebuild pairs of one kernel in a `hipcc -S` listing, per s_setprio region (companion of isa_prio_regions.py).

usage: isa_rebuild_pairs.py file.s [kernel-substring] [-v]
A wave vote on a per-lane `bool` that is carried through a loop or a branch compiles to
    v_cndmask_b32 vN, 0, 1, <mask>      ; the flag rebuilt in a VGPR from the lane mask the compiler holds
    v_cmp_ne_u32  <dst>, 0, vN          ; ... and compared, which intersects the mask with exec
Counts them per region (the regions of isa_prio_regions.py: cut at the s_setprio markers, in listing order); -v lists them.
"""
import re
import sys


def main():
    args = [a for a in sys.argv[1:] if a != '-v']
    verbose = '-v' in sys.argv[1:]
    path = args[0]
    kern = args[1] if len(args) > 1 else 'rtow_trace_fastILi3ELb1ELb0ELi5ELb0E'
    lines = open(path).read().split('\n')
    start = next((i for i, l in enumerate(lines)
                  if kern in l and (l.rstrip().endswith(':') or (l.startswith('_Z') and ': ' in l))), None)
    if start is None:
        sys.exit('kernel not found')
    names, counts, found = ['entry'], [0], []
    rebuilt = None  # (line number, text, register) of the last v_cndmask 0, 1 not yet matched
    for n, l in enumerate(lines[start + 1:], start + 2):
        t = l.strip()
        if not t or t.startswith(';') or t.startswith('.'):
            continue
        op = t.split()[0]
        if op == 's_endpgm':
            break
        if op == 's_setprio':
            names.append('prio ' + t.split()[1])
            counts.append(0)
            continue
        m = re.match(r'v_cndmask_b32\S*\s+(v\d+), 0, 1, ', t)
        if m:
            rebuilt = (n, t, m.group(1))
        elif rebuilt and op.startswith('v_cmp_ne_u32') and re.search(r', 0, %s$' % rebuilt[2], t) and n - rebuilt[0] <= 6:
            counts[-1] += 1
            found.append((len(counts) - 1, rebuilt[0], rebuilt[1], t))
            rebuilt = None
    print('%-3s %-8s %6s' % ('#', 'region', 'pairs'))
    for i, (name, c) in enumerate(zip(names, counts)):
        print('%-3d %-8s %6d' % (i, name, c))
    print('total    %9d' % sum(counts))
    if verbose:
        for f in found:
            print('region %d line %d: %s ; %s' % f)


main()
