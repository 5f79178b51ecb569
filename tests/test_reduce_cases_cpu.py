"""The premises of tests/test_gpu_reduce_optim_edges.py, checked without a GPU: parrot_colsum_route is host arithmetic
over the arguments of a parrot_colsum call (pointers are only looked at for their alignment), so every case of
tests/reduce_cases.py can be asked which kernel it takes and how many row slices it plans, with made-up addresses built
from its offsets.  A later change to the heuristics cannot silently empty a case."""
import ctypes as C

import pytest
import torch

from tests import reduce_cases as RC

BADARG = 10001
X0, O0 = 0x10000, 0x40000000   # 4096-aligned made-up bases


@pytest.fixture(scope="module")
def lib():
    from parrot_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _route(lib, M, N, ld, xoff=0, ooff=0, x0=X0, o0=O0):
    info = (C.c_int * 2)(-1, -1)
    rc = lib.parrot_colsum_route(x0 + 4 * xoff, M, N, ld, None if o0 is None else o0 + 4 * ooff, info)
    return rc, info[0], info[1]


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_case_premise(lib, name):
    c = RC.CASES[name]
    assert _route(lib, c.M, c.N, c.ld, c.xoff, c.ooff) == (0, c.vec4, c.ysplit), name
    assert RC.expected_route(c.M, c.N, c.ld, c.xoff, c.ooff) == (c.vec4, c.ysplit)


def test_table_covers_what_it_claims():
    cs = list(RC.CASES.values())
    v4 = [c for c in cs if c.vec4]
    sc = [c for c in cs if not c.vec4]

    def has(sel, **kw):
        return any(all(getattr(c, k) == v for k, v in kw.items()) for c in sel)

    # the 16-byte kernel: one slice at every row count, the column edges, padded rows
    for M in (64, 65, 67, 99):
        assert has(v4, M=M, ysplit=1)
    for N in (4, 252, 256, 260):
        assert has(v4, N=N)
    assert any(c.ld > c.N and c.ld % 4 == 0 for c in v4)
    # both loops of the finish kernel, a short and an empty last slice
    assert any(1 < c.ysplit < 8 for c in v4) and any(c.ysplit >= 8 for c in v4)
    assert has(v4, M=128, N=8, ysplit=2) and has(v4, M=1024, N=8, ysplit=16) and has(v4, M=129, ysplit=2)
    for sel in (v4, sc):
        short = [c for c in sel if c.ysplit > 1 and c.M % c.ysplit]
        assert short
        assert any((c.ysplit - 1) * -(-c.M // c.ysplit) >= c.M for c in short), "no empty last slice"
    # the scalar kernel for each of its five reasons alone
    ok = dict(N=lambda c: c.N % 4 == 0, ld=lambda c: c.ld % 4 == 0, xoff=lambda c: c.xoff % 4 == 0,
              ooff=lambda c: c.ooff % 4 == 0, M=lambda c: c.M >= 64)
    for reason in ok:
        assert any(not ok[reason](c) and all(ok[o](c) for o in ok if o != reason) for c in sc), reason
    for N in (1, 3, 30, 63, 65, 70):
        assert has(sc, N=N)
    for M in (1, 5, 63):
        assert has(sc, M=M)
    assert any(c.ysplit > 1 and c.M >= 512 for c in sc)
    # every route in both modes, small shapes
    for c in cs:
        twin = c.id[:-3] + ("set" if c.accumulate else "acc")
        assert twin in RC.CASES and RC.CASES[twin].accumulate == 1 - c.accumulate
        assert c.M * c.ld <= RC.MAX_ELEMS and c.ooff >= RC.GUARD
    assert max(len(v) for v in RC.GROUPS.values()) <= 16


def test_route_rule_boundaries(lib):
    """The thresholds themselves, one step either side."""
    assert _route(lib, 64, 8, 8) == (0, 1, 1)
    assert _route(lib, 63, 8, 8) == (0, 0, 1)
    assert _route(lib, 127, 8, 8) == (0, 1, 1)
    assert _route(lib, 128, 8, 8) == (0, 1, 2)
    assert _route(lib, 511, 30, 30) == (0, 0, 1)
    assert _route(lib, 512, 30, 30) == (0, 0, 2)
    # enough column blocks fill the chip by themselves: 256 blocks of 256 columns, 512 blocks of 64
    assert _route(lib, 51200, 2048, 2048) == (0, 1, 32)
    assert _route(lib, 1 << 20, 256 * 256, 256 * 256) == (0, 1, 1)
    assert _route(lib, 1 << 20, 255 * 256, 255 * 256) == (0, 1, 2)
    assert _route(lib, 1 << 20, 512 * 64 + 1, 512 * 64 + 1) == (0, 0, 1)
    assert _route(lib, 1 << 20, 511 * 64 + 1, 511 * 64 + 1, xoff=1) == (0, 0, 1)
    assert _route(lib, 1 << 20, 255 * 64 + 1, 255 * 64 + 1) == (0, 0, 2)
    # each alignment condition; a missing `out` counts as aligned
    assert _route(lib, 64, 8, 8, xoff=2) == (0, 0, 1)
    assert _route(lib, 64, 8, 8, ooff=3) == (0, 0, 1)
    assert _route(lib, 64, 8, 10) == (0, 0, 1)
    assert _route(lib, 64, 8, 8, o0=None) == (0, 1, 1)
    assert _route(lib, 0, 8, 8) == (0, 0, 1)


def test_bad_arguments(lib):
    info = (C.c_int * 2)(-1, -1)
    assert lib.parrot_colsum_route(None, 64, 8, 8, O0, info) == BADARG
    assert lib.parrot_colsum_route(X0, 64, 8, 8, O0, None) == BADARG
    assert lib.parrot_colsum_route(X0, -1, 8, 8, O0, info) == BADARG
    assert lib.parrot_colsum_route(X0, 64, 0, 8, O0, info) == BADARG
    assert tuple(info) == (-1, -1)


def test_chain_length():
    assert RC.chain_length(64, 1) == 16 + 3 + 1
    assert RC.chain_length(129, 2) == 17 + 3 + 2
    assert RC.chain_length(131073, 512) == 65 + 3 + 512


def test_integer_data_is_exact_in_float32():
    """The exact tests' premise: every partial sum of a case is an integer below 2^24."""
    for c in RC.CASES.values():
        assert 8 * c.M + 50 < 2 ** 24
    c = RC.CASES[sorted(RC.CASES)[0]]
    xbuf, obuf = RC.integer_data(c)
    x = RC.x_view(xbuf, c)
    assert x.shape == (c.M, c.N) and float(x.abs().max()) <= 8 and torch.equal(x, x.round())
    assert torch.equal(x[1], xbuf[c.xoff + c.ld:c.xoff + c.ld + c.N])
    xbuf2, obuf2 = RC.integer_data(c)
    assert torch.equal(xbuf, xbuf2) and torch.equal(obuf, obuf2)
    assert obuf.numel() == c.ooff + c.N + RC.GUARD


def test_other_shapes():
    assert RC.SUMSQ_N_BIG > RC.SUMSQ_BLOCK_CAP and RC.SUMSQ_N_BIG % 4 and 4 * RC.SUMSQ_N_BIG < 2 ** 24
    assert RC.ADAM_N_BIG > RC.ADAM_BLOCK_CAP
