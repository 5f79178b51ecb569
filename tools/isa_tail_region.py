#!/usr/bin/env python3
"""For the named kernels of an ISA listing: every stretch from an s_barrier to the first global / buffer store behind it with no
other barrier in between (the split-K meeting point of a step-GEMM body and the start of its epilogue), as the scalar loads,
waits, LDS reads, branches and stores in it, with the count of s_load instructions.  In front of each such barrier: the stretch
from the last MFMA of the listing before it (the K loop's exit path) to the barrier, with its s_load count and its waits.

  isa_tail_region.py LISTING KERNEL [KERNEL ...]           the regions, printed
  isa_tail_region.py --counts LISTING KERNEL [KERNEL ...]  one line per region: kernel, s_load from the last MFMA to the barrier,
                                                           s_load from the barrier to the first store, the waits in front
`regions(lines, name)` gives the same to a caller (tests/test_step_kernel_tail_isa_cpu.py)."""
import re
import sys

SHOWN = r'\s+(s_load|s_waitcnt|s_barrier|global_store|buffer_store|s_cbranch|s_branch|ds_read)'


def kernel_body(lines, nm):
    i0 = next(i for i, l in enumerate(lines) if l.startswith(nm + ':'))
    i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith('.Lfunc_end'))
    return lines[i0:i1]


def regions(lines, nm):
    """The reduction tails of kernel nm: dicts with `barrier` / `store` (line offsets), `head` (last MFMA .. barrier) and `tail`
    (barrier .. first store) as lists of lines, and the s_load counts `head_s_load` / `tail_s_load`."""
    body = kernel_body(lines, nm)
    bars = [i for i, l in enumerate(body) if re.match(r'\s+s_barrier', l)]
    out = []
    for k, b in enumerate(bars):
        end = bars[k + 1] if k + 1 < len(bars) else len(body)
        st = next((i for i in range(b + 1, end) if re.match(r'\s+(global_store|buffer_store)', body[i])), None)
        if st is None:
            continue
        tail = body[b:st + 1]
        if not any('ds_read' in l for l in tail):
            continue  # not a reduction tail
        mf = next((i for i in range(b - 1, -1, -1) if re.match(r'\s+v_mfma', body[i])), 0)
        head = body[mf:b]
        out.append(dict(barrier=b, store=st, head=head, tail=tail,
                        head_s_load=len([l for l in head if re.match(r'\s+s_load', l)]),
                        tail_s_load=len([l for l in tail if re.match(r'\s+s_load', l)]),
                        head_waits=[l.strip() for l in head if re.match(r'\s+s_waitcnt', l)]))
    return len(body), len(bars), out


def main(argv):
    counts = argv[1:2] == ['--counts']
    path, names = (argv[2], argv[3:]) if counts else (argv[1], argv[2:])
    lines = open(path).read().split('\n')
    for nm in names:
        nbody, nbars, regs = regions(lines, nm)
        if counts:
            for r in regs:
                print('%s head_s_load=%d tail_s_load=%d head_waits=[%s]' % (nm, r['head_s_load'], r['tail_s_load'], '; '.join(r['head_waits'])))
            continue
        print('## %s: %d lines, %d barriers' % (nm, nbody, nbars))
        for r in regs:
            ninst = len([l for l in r['tail'] if l.startswith('\t') and not l.startswith('\t;')])
            print('# last MFMA at line +%d -> barrier at +%d: %d s_load' % (r['barrier'] - len(r['head']), r['barrier'], r['head_s_load']))
            for l in r['head']:
                if re.match(SHOWN, l) or re.match(r'\.LBB', l):
                    print(l)
            print('# barrier at line +%d -> first store at +%d: %d instructions, %d s_load' % (r['barrier'], r['store'], ninst, r['tail_s_load']))
            for l in r['tail']:
                if re.match(SHOWN, l) or re.match(r'\.LBB', l):
                    print(l)


if __name__ == '__main__':
    main(sys.argv)
