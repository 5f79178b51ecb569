"""The case table of the column-sum edge tests (`parrot_colsum`) and the shapes of the other reduction / optimiser tests.

A column sum runs on one of two kernels: `colsum4_kernel` (a lane owns four adjacent columns and loads 16 bytes per row:
N and ld multiples of 4, `x` and `out` 16-byte aligned, M >= 64) or `colsum_kernel` (one column per lane; everything
else).  Either may split the rows into `ysplit` slices that write partial sums, which `colsum_finish_kernel` adds in slice
order, eight per round and then one by one.  A case is `(M, N, ld, xoff, ooff, accumulate, vec4, ysplit)` with an id and a
group: the smallest shape at which one branch of those kernels is live, the element offsets of `x` and `out` inside
their parent buffers (what decides their alignment), and the route the call must report (`parrot_colsum_route`).

The model calls the kernel with `accumulate=True` into a slice of the flat gradient buffer, so every shape appears in
both modes and `out` always lies in the middle of a larger buffer.

This module imports no GPU code.  tests/test_reduce_cases_cpu.py checks the premises of the table;
tests/test_gpu_reduce_optim_edges.py runs the cases."""
import zlib
from collections import namedtuple

import torch

Case = namedtuple("Case", "id group M N ld xoff ooff accumulate vec4 ysplit")

CASES = {}
GROUPS = {}
OOFF = 8        # `out` starts 8 floats into its parent buffer unless a case is about its alignment
GUARD = 8       # canary floats on either side of `out`
MAX_ELEMS = 400_000


def _case(group, M, N, vec4, ysplit, ld=None, xoff=0, ooff=OOFF):
    ld = N if ld is None else ld
    assert ld >= N and M * ld <= MAX_ELEMS
    for acc in (0, 1):
        name = "%s-M%d-N%d-ld%d-x%d-o%d-%s" % (group, M, N, ld, xoff, ooff, "acc" if acc else "set")
        assert name not in CASES, name
        CASES[name] = Case(name, group, M, N, ld, xoff, ooff, acc, vec4, ysplit)
        GROUPS.setdefault(group, []).append(name)


# ---- colsum4_kernel -----------------------------------------------------------------------------------------------------
# one slice: whole 32-row rounds (64, 96), then tails in which the four waves hold different row counts; 93 = the last
# round is unrolled for wave 0 alone
for _M in (64, 65, 67, 93, 96, 99):
    _case("v4-rows", _M, 12, 1, 1)
# columns: one lane, one short of a block, a block, a block and one lane
for _N in (4, 252, 256, 260):
    _case("v4-cols", 65, _N, 1, 1)
# padded rows, an aligned offset of x
_case("v4-ld", 67, 8, 1, 1, ld=12)
_case("v4-ld", 67, 8, 1, 1, ld=20, xoff=4)
# row slices: fewer than 8 partials (the finish kernel's one-by-one loop), 8 or more (its rounds of eight)
_case("v4-split", 128, 8, 1, 2)
_case("v4-split", 300, 8, 1, 4, ld=12)
_case("v4-split", 1024, 8, 1, 16)
_case("v4-split", 512, 260, 1, 8)      # two column blocks, the second with one lane
# a last slice shorter than the others (65 + 64; 15 x 65 + 50), and 128 slices of 65 rows over 8193: slice 126 has 3 rows,
# slice 127 none
_case("v4-short", 129, 8, 1, 2)
_case("v4-short", 1025, 12, 1, 16)
_case("v4-short", 8193, 8, 1, 128)

# ---- colsum_kernel, for each of its five reasons ------------------------------------------------------------------------
for _N in (1, 3, 30, 63, 65, 70):
    _case("s-N", 70, _N, 0, 1)
_case("s-N", 70, 30, 0, 1, ld=32)      # N alone: rows of a multiple of 4 floats
_case("s-ld", 64, 8, 0, 1, ld=9)
_case("s-ld", 67, 64, 0, 1, ld=70)
_case("s-xoff", 64, 8, 0, 1, xoff=1)
_case("s-xoff", 99, 256, 0, 1, xoff=3)
_case("s-ooff", 64, 8, 0, 1, ooff=OOFF + 1)
_case("s-ooff", 99, 256, 0, 1, ooff=OOFF + 2)
for _M in (1, 5, 63):
    _case("s-rows", _M, 8, 0, 1)
_case("s-rows", 6, 30, 0, 1)           # a batch of 6, 3 x 10 attention parameters
_case("s-rows", 63, 260, 0, 1)
# row slices of the scalar kernel (at least 256 rows each), a short last slice (257 + 256), a short and an empty one
# (512 slices of 257 rows over 131073: slice 510 has 3 rows, slice 511 none)
_case("s-split", 512, 30, 0, 2)
_case("s-split", 513, 70, 0, 2)
_case("s-split", 2048, 8, 0, 8, xoff=1)
_case("s-split", 4100, 65, 0, 16, ld=67)
_case("s-split", 131073, 3, 0, 512)


def expected_route(M, N, ld, xoff, ooff):
    """The dispatch rule as the table assumes it (the CPU test compares it with the library's)."""
    if N % 4 == 0 and ld % 4 == 0 and xoff % 4 == 0 and ooff % 4 == 0 and M >= 64:
        bx, ys = -(-N // 256), 1
        while bx * ys < 256 and M // (ys * 2) >= 64:
            ys *= 2
        return 1, ys
    bx, ys = -(-N // 64), 1
    while bx * ys < 512 and M // (ys * 2) >= 256:
        ys *= 2
    return 0, ys


def chain_length(M, ysplit):
    """The longest chain of dependent additions behind one column sum on a route: a wave's share of a slice's rows, the
    three additions that join the four waves, one addition per slice (and the old value when accumulating)."""
    per = -(-M // ysplit)
    return -(-per // 4) + 3 + ysplit


def x_extent(case):
    """Floats of the parent buffer of `x`: the offset, M rows of ld, and a tail so that the last row is padded too."""
    return case.xoff + case.M * case.ld + 4


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def integer_data(case):
    """(parent buffer of x, parent buffer of out) as float32 CPU tensors holding small integers: x in [-8, 8] (padding
    included: a kernel that reads it sums something else), out in [-50, 50] (the old values of an accumulating call and
    the canary around them).  Any order of summation is exact in float32."""
    g = _gen("colsum", case.M, case.N, case.ld, case.xoff)
    xbuf = torch.randint(-8, 9, (x_extent(case),), generator=g).float()
    obuf = torch.randint(-50, 51, (case.ooff + case.N + GUARD,), generator=g).float()
    return xbuf, obuf


def x_view(xbuf, case):
    return xbuf.as_strided((case.M, case.N), (case.ld, 1), case.xoff)


# ---- the other kernels' shapes --------------------------------------------------------------------------------------------
SUMSQ_N = (1, 3, 4, 5, 255, 1023, 1024, 1029, 10007)
SUMSQ_BLOCK_CAP = 4 * 256 * 2048          # floats one pass of 2048 blocks covers: past it the grid-stride loop runs
SUMSQ_N_BIG = SUMSQ_BLOCK_CAP + 4 * 300 + 3   # a second pass for 300 threads and three floats of block 0's scalar tail
ADAM_N = (1, 255, 257, 10007)
ADAM_BLOCK_CAP = 256 * 4096
ADAM_N_BIG = ADAM_BLOCK_CAP + 77
ADAM_STEPS = (1, 2, 7, 1000)
NORM_N = (1, 2, 255, 256, 257, 1000)
NORM_R = (1, 3)
BF16_BLOCK_CAP = 8 * 256 * 8192
