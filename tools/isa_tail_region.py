#!/usr/bin/env python3
"""For the named kernels of an ISA listing: every stretch from an s_barrier to the first global / buffer store behind it with no
other barrier in between (the split-K meeting point of a step-GEMM body and the start of its epilogue), as the scalar loads,
waits, LDS reads, branches and stores in it, with the count of s_load instructions."""
import re, sys
path, names = sys.argv[1], sys.argv[2:]
lines = open(path).read().split('\n')
for nm in names:
    i0 = next(i for i, l in enumerate(lines) if l.startswith(nm + ':'))
    i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith('.Lfunc_end'))
    body = lines[i0:i1]
    bars = [i for i, l in enumerate(body) if re.match(r'\s+s_barrier', l)]
    print('## %s: %d lines, %d barriers' % (nm, len(body), len(bars)))
    for k, b in enumerate(bars):
        end = bars[k + 1] if k + 1 < len(bars) else len(body)
        st = next((i for i in range(b + 1, end) if re.match(r'\s+(global_store|buffer_store)', body[i])), None)
        if st is None:
            continue
        reg = body[b:st + 1]
        if not any('ds_read' in l for l in reg):
            continue  # not a reduction tail
        ninst = len([l for l in reg if l.startswith('\t') and not l.startswith('\t;')])
        sl = [l for l in reg if re.match(r'\s+s_load', l)]
        print('# barrier at line +%d -> first store at +%d: %d instructions, %d s_load' % (b, st, ninst, len(sl)))
        for l in reg:
            if re.match(r'\s+(s_load|s_waitcnt|s_barrier|global_store|buffer_store|s_cbranch|s_branch|ds_read)', l) or re.match(r'\.LBB', l):
                print(l)
