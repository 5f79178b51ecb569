"""The premises of tests/test_gpu_gemm_edges.py, checked without a GPU: parrot_gemm_route is host arithmetic over the
arguments of a parrot_gemm call (pointers are only looked at for their alignment), so every case of tests/gemm_cases.py
can be asked which kernel it takes and how many K slices it plans, with made-up addresses built from its frame geometry.
Also pins the three automatic split-K rules."""
import ctypes as C

import pytest

from tests import gemm_cases as G


@pytest.fixture(scope="module")
def lib():
    from parrot_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture
def mode(lib):
    """Sets the precision mode for a test and restores the one it found."""
    prev = lib.parrot_get_gemm_precision()

    def set_mode(m):
        assert lib.parrot_set_gemm_precision(m) == 0
    yield set_mode
    assert lib.parrot_set_gemm_precision(prev) == 0


def _route(lib, *args):
    kernel, slices = C.c_int(-1), C.c_int(-1)
    rc = lib.parrot_gemm_route(*args, C.byref(kernel), C.byref(slices))
    return rc, kernel.value, slices.value


A0, B0 = 0x10000, 0x40000000   # 4096-aligned made-up bases


def _plain(M, N, K, ta=0, tb=0, alpha=1.0, act=0, nbatch=1, split_k=0, gate=0, a=A0, b=B0, lda=None, ldb=None):
    lda = lda if lda is not None else (M if ta else K)
    ldb = ldb if ldb is not None else (K if tb else N)
    return (a, lda, ta, b, ldb, tb, M, N, K, alpha, act, nbatch, 0, 0, split_k, gate)


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_case_premise(lib, mode, name):
    c = G.CASES[name]
    mode(c["mode"])
    rc, kernel, slices = _route(lib, *G.route_args(c))
    if c["raises"] == "split_act":
        assert rc == G.BADARG
        return
    assert rc == 0
    assert (kernel, slices) == (c["route"], c["slices"]), f"{name}: kernel {kernel}, {slices} slices"


def test_table_covers_what_it_claims():
    """The table's own premises: pads are multiples of 4 except where a case is about misalignment, every group is small."""
    odd = {n for n, c in G.CASES.items() for w in "abcg" if c["f" + w].off % 4 or c["f" + w].ldpad % 4 or c["f" + w].bpad % 4}
    assert odd == {"elig-NN-K66", "elig-TN-M130", "elig-A-off1", "elig-lda-K2", "batch-bf16x3-nb8-A-stride-odd",
                   "step-ldc-N3", "step-A-off1", "step-lda-K1", "step-NT-ldb-K2"}
    assert {c["route"] for c in G.CASES.values()} == {G.STEP, G.K_F32, G.K_BF16, G.K_BF16X3}
    assert max(len(v) for v in G.GROUPS.values()) <= 12


def test_mode_is_restored(lib):
    prev = lib.parrot_get_gemm_precision()
    for m in (G.F32, G.BF16, G.BF16X3):
        assert lib.parrot_set_gemm_precision(m) == 0
        assert lib.parrot_get_gemm_precision() == m
    assert lib.parrot_set_gemm_precision(prev) == 0
    assert lib.parrot_get_gemm_precision() == prev


def test_small_m_dispatch_rule(lib, mode):
    """M <= 64, transA = 0, nbatch = 1, split_k <= 1, alpha = 1, no gate -> the step kernel, in every mode; each
    condition alone keeps the product on the batched kernels."""
    for m, big in ((G.F32, G.K_F32), (G.BF16, G.K_BF16), (G.BF16X3, G.K_F32)):   # (M < 128: never the split kernel)
        mode(m)
        assert _route(lib, *_plain(64, 96, 128)) == (0, G.STEP, 1)
        assert _route(lib, *_plain(64, 96, 128, split_k=1)) == (0, G.STEP, 1)
        assert _route(lib, *_plain(64, 96, 128, act=G.TANH)) == (0, G.STEP, 1)
        assert _route(lib, *_plain(1, 16, 16)) == (0, G.STEP, 1)
        assert _route(lib, *_plain(65, 96, 128)) == (0, big, 1)
        assert _route(lib, *_plain(64, 96, 128, ta=1)) == (0, big, 1)
        assert _route(lib, *_plain(64, 96, 128, alpha=0.5)) == (0, big, 1)
        assert _route(lib, *_plain(64, 96, 128, split_k=2)) == (0, big, 2)
        assert _route(lib, *_plain(64, 96, 128, gate=1)) == (0, big, 1)
        assert _route(lib, *_plain(64, 96, 128, nbatch=2)) == (0, big, 1)


def test_auto_split_rules(lib, mode):
    # split kernel (256 x 256 tiles): a multiple of 8 slices of at least 512 K rows, only for tiles < 256 and K >= 4096
    mode(G.BF16X3)
    assert _route(lib, *_plain(136, 136, 4096)) == (0, G.K_BF16X3, 8)
    assert _route(lib, *_plain(136, 136, 4096, ta=1)) == (0, G.K_BF16X3, 8)
    assert _route(lib, *_plain(136, 136, 4095, ta=1)) == (0, G.K_BF16X3, 1)          # (x-contiguous operands: any K is eligible)
    assert _route(lib, *_plain(136, 136, 4095)) == (0, G.K_F32, 15)                  # K % 4: not eligible, the f32 kernel's rule
    assert _route(lib, *_plain(136, 136, 4092)) == (0, G.K_BF16X3, 1)                # eligible, K < 4096
    assert _route(lib, *_plain(136, 136, 4096, act=G.RELU)) == (0, G.K_BF16X3, 1)
    assert _route(lib, *_plain(512, 384, 12000, ta=1)) == (0, G.K_BF16X3, 16)        # 4 tiles: 16 slices of 750 rows
    assert _route(lib, *_plain(4096, 4096, 8192)) == (0, G.K_BF16X3, 1)              # 256 tiles fill the chip
    # f32 / bf16-operand kernels (128 x 128 tiles): ceil(1024 / tiles) slices, at least 256 K rows each, at most 64
    mode(G.F32)
    assert _route(lib, *_plain(96, 200, 5000, ta=1)) == (0, G.K_F32, 19)             # 2 tiles: 512 wanted, 5000 / 256 = 19
    assert _route(lib, *_plain(200, 136, 1024)) == (0, G.K_F32, 4)
    assert _route(lib, *_plain(200, 136, 511)) == (0, G.K_F32, 1)
    assert _route(lib, *_plain(200, 136, 1024, act=G.RELU)) == (0, G.K_F32, 1)
    assert _route(lib, *_plain(128, 128, 100000)) == (0, G.K_F32, 64)
    assert _route(lib, *_plain(3000, 3000, 1024)) == (0, G.K_F32, 1)                 # 576 tiles
    assert _route(lib, *_plain(1024, 1024, 1024)) == (0, G.K_F32, 4)                 # 64 tiles: 16 wanted, 1024 / 256 = 4
    mode(G.BF16)
    assert _route(lib, *_plain(96, 200, 5000, ta=1)) == (0, G.K_BF16, 19)
    # an explicit split_k is taken as it is
    assert _route(lib, *_plain(300, 260, 72, split_k=8)) == (0, G.K_BF16, 8)


def test_bad_arguments(lib, mode):
    mode(G.F32)
    ok = _plain(300, 260, 72)
    assert _route(lib, *ok)[0] == 0
    for i, bad in ((0, None), (3, None), (6, 0), (7, 0), (8, 0), (11, 0)):   # A, B, M, N, K, nbatch
        args = list(ok)
        args[i] = bad
        assert _route(lib, *args)[0] == G.BADARG, i
    assert _route(lib, *_plain(300, 260, 72, gate=1, nbatch=2))[0] == G.BADARG       # the gate is not batched
    assert _route(lib, *_plain(300, 260, 72, act=G.RELU, split_k=2))[0] == G.BADARG  # no activation on a split product
    assert lib.parrot_gemm_route(*ok, None, None) == G.BADARG
    # accumulate with an activation has no one meaning (step kernel: after, batched kernels: before the activation)
    p = C.c_void_p(A0)
    for M in (64, 65):
        assert lib.parrot_gemm(p, 128, 0, p, 96, 0, p, 96, M, 96, 128, None, 1.0, 1, G.TANH, 1, 0, 0, 0, 1, None) == G.BADARG
