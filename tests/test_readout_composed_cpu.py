"""The composed readout -> output entry points (include/parrot_hip.h, ParrotReadoutComposedDesc) without a GPU: the
ctypes mirror has the C layout, bad descriptors are refused before anything is launched, and the host-side slice and
workspace arithmetic (parrot_amd/csrc/readout.h) holds its invariants in a stand-alone program built with the host
sanitizers."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = 10001
FAKE = 0x10000  # a 16-byte aligned non-null address: the calls below are refused before any pointer is followed


@pytest.fixture(scope="module")
def lib():
    from parrot_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _desc(M=130, segs=(32, 32, 16), R=72, O=63, pointers=True):
    from parrot_amd import _lib
    d = _lib.ReadoutComposedDesc()
    d.M, d.nseg, d.R, d.O, d.zero_rows, d.slice_rows, d.nbias = M, len(segs), R, O, 3, 0, len(segs)
    for s, K in enumerate(segs):
        d.K[s], d.ldx[s], d.lddx[s] = K, K, K
    d.ldwr, d.ldwo, d.ldp, d.lddp, d.ldgwr, d.ldgwo = R, O, O, O, R, O
    if pointers:
        for s in range(len(segs)):
            d.x[s], d.dx[s], d.rb[s], d.grb[s] = FAKE, FAKE, FAKE, FAKE
        d.Wr = d.Wo = d.bo = d.pred = d.dp = d.gWr = d.gWo = d.gbo = FAKE
    return d


def _both(lib, d, ws=FAKE):
    return (lib.parrot_readout_composed_fwd(C.byref(d), ws, None), lib.parrot_readout_composed_bwd(C.byref(d), ws, None))


def test_struct_size_matches_header(tmp_path):
    from parrot_amd import _lib
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "parrot_hip.h"\n'
                   'int main(void){printf("%zu\\n", sizeof(ParrotReadoutComposedDesc));return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)])) == C.sizeof(_lib.ReadoutComposedDesc)


def test_workspace_query_reads_sizes_only(lib):
    d = _desc(pointers=False)
    n = lib.parrot_readout_composed_ws_floats(C.byref(d))
    # two fragment-major copies of W', b', the summed bias, dW' (+ the column-sum row), its partial tiles, the gWo slices
    Kt = 80
    assert n >= 2 * Kt * 64 + 64 + 72 + (Kt + 1) * 64 and n % 4 == 0
    d.slice_rows = 64   # 130 rows in slices of 64: three partial tiles
    n3 = lib.parrot_readout_composed_ws_floats(C.byref(d))
    d.slice_rows = 128  # two
    n2 = lib.parrot_readout_composed_ws_floats(C.byref(d))
    assert n3 - n2 == (Kt + 1) * 64
    assert lib.parrot_readout_composed_ws_floats(None) == -BADARG


def test_bad_descriptors_are_refused_without_gpu(lib):
    good = _desc()
    need = lib.parrot_readout_composed_ws_floats(C.byref(good))
    good.ws_floats = need
    # null pointers: the descriptor itself, the workspace, every operand one at a time
    assert lib.parrot_readout_composed_fwd(None, FAKE, None) == BADARG
    assert lib.parrot_readout_composed_bwd(None, FAKE, None) == BADARG
    assert _both(lib, good, ws=None) == (BADARG, BADARG)
    empty = _desc(pointers=False)
    empty.ws_floats = need
    assert _both(lib, empty) == (BADARG, BADARG)
    for name, calls in (('Wr', (0, 1)), ('Wo', (0, 1)), ('bo', (0, 1)), ('pred', (0,)), ('dp', (1,)), ('gWr', (1,)),
                        ('gWo', (1,)), ('gbo', (1,))):
        d = _desc()
        d.ws_floats = need
        setattr(d, name, None)
        rc = _both(lib, d)
        for c in calls:
            assert rc[c] == BADARG, name
    for name, calls in (('x', (0, 1)), ('rb', (0, 1)), ('dx', (1,)), ('grb', (1,))):
        d = _desc()
        d.ws_floats = need
        getattr(d, name)[1] = None
        rc = _both(lib, d)
        for c in calls:
            assert rc[c] == BADARG, name
    # an operand that is not 16-byte aligned
    d = _desc()
    d.ws_floats = need
    d.x[0] = FAKE + 4
    assert _both(lib, d) == (BADARG, BADARG)
    # O > 64
    d = _desc(O=65)
    d.ws_floats = 1 << 40
    assert lib.parrot_readout_composed_ws_floats(C.byref(d)) == -BADARG
    assert _both(lib, d) == (BADARG, BADARG)
    # a segment whose K is not a multiple of 16
    d = _desc(segs=(32, 24))
    d.ws_floats = 1 << 40
    assert lib.parrot_readout_composed_ws_floats(C.byref(d)) == -BADARG
    assert _both(lib, d) == (BADARG, BADARG)
    # more segments than the descriptor holds, a leading dimension below the width
    d = _desc()
    d.ws_floats = need
    d.nseg = 5
    assert _both(lib, d) == (BADARG, BADARG)
    d = _desc()
    d.ws_floats = need
    d.ldx[0] = 16
    assert _both(lib, d) == (BADARG, BADARG)
    # a workspace smaller than the query
    d = _desc()
    d.ws_floats = need - 1
    assert _both(lib, d) == (BADARG, BADARG)


def test_layout_arithmetic_under_host_sanitizers(tmp_path):
    """tools/readout_layout_check.cpp sweeps shapes through csrc/readout.h (slices cover M exactly once, sections are
    aligned, ordered and disjoint) as a stand-alone host program under AddressSanitizer and UBSan."""
    exe = tmp_path / "readout_layout_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "readout_layout_check.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True)
    assert "ok" in out
