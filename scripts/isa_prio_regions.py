#!/usr/bin/env python3
"""Vector work of one kernel in a `hipcc -S` listing, cut at its s_setprio markers (companion of isa_blocks.py).

usage: isa_prio_regions.py file.s [kernel-substring]
The trace kernels change their issue priority at the borders of their stages (stage_prio, rtow_trace_math.h), so the
markers cut the listing into the stages in program order: for the GRID kernels the new-ray window, the walk's entry (the
always-test list, up to kPrioSetup), the walk's set-up, the DDA loop, the leaf phase, and the shading up to the next
trip's window.  Per region: the priority it runs at, VALU instructions (v_*), LDS instructions (ds_*), scalar loads,
lgkmcnt waits.  Static counts in listing order: a region holds every block laid out between two markers, taken or not.
"""
import sys


def main():
    path = sys.argv[1]
    kern = sys.argv[2] if len(sys.argv) > 2 else 'rtow_trace_fastILi3ELb1ELb0ELi5ELb0E'
    lines = open(path).read().split('\n')
    start = next((i for i, l in enumerate(lines)
                  if kern in l and (l.rstrip().endswith(':') or (l.startswith('_Z') and ': ' in l))), None)
    if start is None:
        sys.exit('kernel not found')
    regions = [['entry', 0, 0, 0, 0]]
    for l in lines[start + 1:]:
        t = l.strip()
        if not t or t.startswith(';') or t.startswith('.'):
            continue
        op = t.split()[0]
        if op == 's_endpgm':
            break
        if op == 's_setprio':
            regions.append(['prio ' + t.split()[1], 0, 0, 0, 0])
            continue
        r = regions[-1]
        if op.startswith('v_'):
            r[1] += 1
        elif op.startswith('ds_'):
            r[2] += 1
        elif op.startswith('s_load_'):
            r[3] += 1
        elif op == 's_waitcnt' and 'lgkmcnt' in t:
            r[4] += 1
    print('%-3s %-8s %6s %5s %6s %6s' % ('#', 'region', 'valu', 'lds', 'sload', 'lgkm'))
    for i, r in enumerate(regions):
        print('%-3d %-8s %6d %5d %6d %6d' % (i, r[0], r[1], r[2], r[3], r[4]))
    print('total    %9d %5d %6d %6d' % tuple(sum(r[k] for r in regions) for k in (1, 2, 3, 4)))


main()
