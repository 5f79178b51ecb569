#!/usr/bin/env python3
"""For the named kernels of an ISA listing (hipcc -S --cuda-device-only): the K loops of a step-GEMM body as the sequence of
operand loads, MFMAs, vmcnt waits, branches and labels up to the partial-sum stores (ds_write) and the meeting point's barrier,
runs of one instruction kind collapsed to a count.  What to read from it: every wait inside a loop body is a counted
`vmcnt(N)`, N > 0, and nothing between a loop's exit and the ds_write run waits for loads that no MFMA reads.
    python tools/isa_kloop_waits.py LISTING.s KERNEL [KERNEL ...]"""
import re
import sys

path, names = sys.argv[1], sys.argv[2:]
lines = open(path).read().split('\n')
KINDS = (('load', r'\s+(global_load|buffer_load)_\w+'), ('mfma', r'\s+v_mfma_\w+'), ('ds_write', r'\s+ds_write\w*'),
         ('bpermute', r'\s+ds_bpermute\w*'))
for nm in names:
    i0 = next(i for i, l in enumerate(lines) if l.startswith(nm + ':'))
    i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith('.Lfunc_end'))
    body = lines[i0:i1]
    print('## %s: %d lines' % (nm, len(body)))
    out, run, seen_mfma = [], None, False

    def flush():
        global run
        if run:
            out.append('\t%3d x %s' % (run[1], run[2]))
        run = None

    for l in body:
        kind = next((k for k, pat in KINDS if re.match(pat, l)), None)
        if kind:
            op = l.split()[0]
            if run and run[0] == kind and run[2] == op:
                run[1] += 1
            else:
                flush()
                run = [kind, 1, op]
            continue
        m = re.match(r'\s+s_waitcnt (.*)', l)
        if m and 'vmcnt' in m.group(1):
            flush()
            out.append('\ts_waitcnt ' + m.group(1).split(';')[0].strip())
        elif re.match(r'\s+(s_cbranch|s_branch|s_barrier|s_endpgm)', l) or re.match(r'\.LBB', l):
            flush()
            out.append(l.split(';')[0].rstrip())
    flush()
    # keep the stretch from the first MFMA's enclosing label to the first barrier behind the last MFMA
    first = next(i for i, l in enumerate(out) if 'v_mfma' in l)
    last = max(i for i, l in enumerate(out) if 'v_mfma' in l)
    start = max((i for i in range(first) if out[i].startswith('.LBB')), default=0)
    end = next((i for i in range(last, len(out)) if 's_barrier' in out[i]), len(out) - 1)
    print('\n'.join(out[start:end + 1]))
