#!/usr/bin/env python3
"""Scalar loads and waits of one kernel in a `hipcc -S` listing, block by block (companion of isa_blocks.py).

usage: isa_sloads.py file.s [kernel-substring] [--list]
Prints, for the blocks inside the main loop (Depth >= 1), the number of s_load_* instructions by width and of
s_waitcnt instructions that wait for lgkmcnt, and the totals.  --list prints every scalar load with its block.
"""
import collections
import re
import sys


def main():
    path = sys.argv[1]
    kern = sys.argv[2] if len(sys.argv) > 2 and not sys.argv[2].startswith('--') else 'rtow_trace_fastILi3ELb1ELb0ELi5E'
    show = '--list' in sys.argv
    lines = open(path).read().split('\n')
    start = next((i for i, l in enumerate(lines)
                  if kern in l and (l.rstrip().endswith(':') or (l.startswith('_Z') and ': ' in l))), None)
    if start is None:
        sys.exit('kernel not found')
    label, depth = 'entry', 0
    loads = collections.Counter()   # width -> count, Depth >= 1
    per_block = collections.OrderedDict()
    waits = 0
    for l in lines[start + 1:]:
        t = l.strip()
        if l.startswith('.LBB') or l.startswith('; %bb'):
            m = re.search(r'Depth=(\d+)', l)
            label, depth = l.split(':')[0].lstrip('; '), int(m.group(1)) if m else 0
            continue
        if not t or t.startswith(';') or t.startswith('.'):
            continue
        op = t.split()[0]
        if op == 's_endpgm':
            break
        if depth < 1:
            continue
        if op.startswith('s_load_'):
            loads[op] += 1
            per_block.setdefault(label, []).append(t)
        elif op == 's_waitcnt' and 'lgkmcnt' in t:
            waits += 1
            per_block.setdefault(label, []).append(t)
    for label, ops in per_block.items():
        n = sum(1 for o in ops if o.startswith('s_load_'))
        if n == 0:
            continue
        print('%-12s %2d loads, %2d lgkmcnt waits' % (label, n, len(ops) - n))
        if show:
            for o in ops:
                print('    ' + o.split(';')[0].rstrip())
    print('main loop: %d scalar loads (%s), %d lgkmcnt waits' %
          (sum(loads.values()), ', '.join('%s x%d' % kv for kv in sorted(loads.items())), waits))


main()
