"""The case table of the GEMM edge tests: every epilogue, stride and dispatch boundary of `parrot_gemm`.

`parrot_gemm` is a dispatcher over four kernels (the step kernel, the f32-input kernel, the bf16-operand kernel and the
split-bf16 kernel), each with its own epilogue.  A case records a call -- shape, layout, precision mode, keywords -- the
geometry of the frames its operands and its output sit in, and its premise: the kernel the call must take
(`parrot_gemm_route`) and the number of K slices it plans.

Frames.  Every operand is a view into a larger buffer filled with NaN, so a read outside the operand poisons the
result; the output is a view into a larger buffer filled with FRAME_FILL, which must be bit-identical after the call.
A `Frame` is (off, ldpad, tail, bpad, expand): `off` floats before the first element, leading dimension = columns +
`ldpad`, `tail` floats after the last one, batch stride = rows * ld + `bpad` (`expand`: batch stride 0, one matrix).
Pads are multiples of 4 floats unless the case is about a misaligned operand.

tests/test_gemm_route_cpu.py checks the premises without a GPU (made-up addresses built from the frame geometry),
tests/test_gpu_gemm_edges.py runs the calls against the same expression in float64."""
import math
import zlib
from collections import namedtuple

import torch

F32, BF16, BF16X3 = 0, 1, 2                         # ops.PRECISION_*
STEP, K_F32, K_BF16, K_BF16X3 = 0, 1, 2, 3          # ops.ROUTE_* / PARROT_GEMM_ROUTE_*
NONE, RELU, TANH, SIGMOID = 0, 1, 2, 3              # ops.ACT_*
MODE_NAME = {F32: "f32", BF16: "bf16", BF16X3: "bf16x3"}
BADARG = 10001

# The project's norm-wise tolerances (tests.util.assert_close against float64; tests/test_gpu_kernels.py, test_gpu_bf16.py)
TOL_BIG = 3e-6       # f32 and split kernels, unsplit, K <= 1024
TOL_SPLIT = 5e-6     # split-K, tanh, sigmoid, K = 4096
TOL_STEP = 2e-6      # step kernel
TOL_STEP_ACT = 5e-6  # step kernel with tanh or sigmoid
TOL_BF16 = 2e-5      # PRECISION_BF16 against the product of the operands rounded to bf16

FRAME_FILL = 7.25

Frame = namedtuple("Frame", "off ldpad tail bpad expand", defaults=(4, 4, 4, 0, False))
FR = Frame()

LAYOUTS = ((False, False), (False, True), (True, False), (True, True))


def layout_name(ta, tb):
    return "NT"[ta] + "NT"[tb]


def _tol(mode, route, slices, act, K):
    if route == K_BF16:
        return TOL_BF16
    if route == STEP:
        return TOL_STEP_ACT if act in (TANH, SIGMOID) else TOL_STEP
    if slices > 1 or act in (TANH, SIGMOID) or K >= 4096:
        return TOL_SPLIT
    return TOL_BIG


def big_route(mode, act=NONE):
    """Kernel of a product that is eligible for everything its mode offers."""
    if mode == BF16:
        return K_BF16
    if mode == BF16X3 and act <= RELU:
        return K_BF16X3
    return K_F32


CASES = {}


def _case(name, group, M, N, K, ta=False, tb=False, mode=BF16X3, kind="gemm", alpha=1.0, bias=False, accumulate=False,
          act=NONE, split_k=0, nbatch=1, fa=FR, fb=FR, fc=FR, fg=FR, route=None, slices=None, raises=None):
    """kind: "gemm" (ops.gemm), "gated" (ops.gemm_gated), "batched" (ops.gemm_batched), "raw" (parrot_gemm through
    _lib.call with nbatch and split_k together).  raises: None, "split_act" (the library returns PARROT_ERR_BADARG, the
    route query too) or "acc_act" (ops.gemm raises ValueError, the library returns PARROT_ERR_BADARG)."""
    assert name not in CASES, name
    if kind == "batched":
        split_k = 1   # what ops.gemm_batched passes
    if slices is None:
        slices = 1 if route == STEP else max(1, split_k)
    c = dict(name=name, group=group, M=M, N=N, K=K, ta=ta, tb=tb, mode=mode, kind=kind, alpha=alpha, bias=bias,
             accumulate=accumulate, act=act, split_k=split_k, nbatch=nbatch, fa=fa, fb=fb, fc=fc, fg=fg, route=route,
             slices=slices, raises=raises, tol=_tol(mode, route, slices, act, K))
    CASES[name] = c
    return c


# ---- 1. epilogues of the three big kernels: 2 x 2 tiles of 256, 3 x 3 tiles of 128, four and a half K tiles of 16 ----------
EPI_SHAPE = (300, 260, 72)
for _mode in (F32, BF16, BF16X3):
    for _ta, _tb in LAYOUTS:
        _g = f"epi-{MODE_NAME[_mode]}-{layout_name(_ta, _tb)}"
        _kw = dict(ta=_ta, tb=_tb, mode=_mode)
        _r = big_route(_mode)
        _case(_g + "-alpha", _g, *EPI_SHAPE, alpha=-0.5, route=_r, **_kw)
        _case(_g + "-alpha-bias-acc", _g, *EPI_SHAPE, alpha=0.75, bias=True, accumulate=True, route=_r, **_kw)
        _case(_g + "-alpha-bias-acc-split3", _g, *EPI_SHAPE, alpha=0.75, bias=True, accumulate=True, split_k=3, route=_r, **_kw)
        # slices 16 wide (32 on the bf16-operand kernel), the trailing ones empty; BF16X3: Z = 8 takes the 1-d grid
        _case(_g + "-split8", _g, *EPI_SHAPE, split_k=8, route=_r, **_kw)
        _case(_g + "-relu-bias", _g, *EPI_SHAPE, bias=True, act=RELU, route=_r, **_kw)
        _case(_g + "-tanh-bias", _g, *EPI_SHAPE, bias=True, act=TANH, route=big_route(_mode, TANH), **_kw)
        _case(_g + "-sigmoid-bias", _g, *EPI_SHAPE, bias=True, act=SIGMOID, route=big_route(_mode, SIGMOID), **_kw)
        _case(_g + "-split2-relu", _g, *EPI_SHAPE, act=RELU, split_k=2, route=_r, raises="split_act", **_kw)
        _case(_g + "-acc-tanh", _g, *EPI_SHAPE, accumulate=True, act=TANH, route=big_route(_mode, TANH), raises="acc_act", **_kw)
        _case(_g + "-gate", _g, *EPI_SHAPE, kind="gated", route=_r, **_kw)   # ldg = N + 4 (fg = FR)

# ---- 2. the reducer's gate line: gated products with a K long enough for the automatic split ---------------------------
_case("reduce-gate-f32", "reduce-gate", 200, 136, 1024, mode=F32, kind="gated", route=K_F32, slices=4)
_case("reduce-gate-bf16x3", "reduce-gate", 136, 136, 4096, mode=BF16X3, kind="gated", route=K_BF16X3, slices=8)

# ---- 3. eligibility boundary of the split-bf16 kernel (one condition per case; right whichever kernel it takes) -------
_case("elig-base", "elig", 128, 128, 64, route=K_BF16X3)
_case("elig-M124", "elig", 124, 128, 64, route=K_F32)
_case("elig-N124", "elig", 128, 124, 64, route=K_F32)
_case("elig-K60", "elig", 128, 128, 60, route=K_F32)
_case("elig-NN-K66", "elig", 128, 128, 66, fa=FR._replace(ldpad=2), route=K_F32)            # lda = 68: only K % 4 fails
_case("elig-TN-M130", "elig", 130, 128, 64, ta=True, fa=FR._replace(ldpad=2), route=K_F32)  # lda = 132: only M % 4 fails
_case("elig-A-off1", "elig", 128, 128, 64, fa=FR._replace(off=5), route=K_F32)
_case("elig-lda-K2", "elig", 128, 128, 64, fa=FR._replace(ldpad=2), route=K_F32)
_case("elig-lda-K4", "elig", 128, 128, 64, fa=FR._replace(ldpad=4), route=K_BF16X3)

# ---- 4. batched products: nbatch = 3 the 2-d grid, 8 and 16 the 1-d grid that deals slices to XCDs ----------------------
BATCH_SHAPE = (132, 136, 80)
for _mode in (F32, BF16X3):
    _g = f"batch-{MODE_NAME[_mode]}"
    _kw = dict(mode=_mode, kind="batched", route=big_route(_mode))
    for _nb in (3, 8, 16):
        _case(f"{_g}-nb{_nb}", _g, *BATCH_SHAPE, nbatch=_nb, **_kw)
    _case(_g + "-nb8-transA", _g, *BATCH_SHAPE, nbatch=8, ta=True, **_kw)
    _case(_g + "-nb8-transB", _g, *BATCH_SHAPE, nbatch=8, tb=True, **_kw)
    _case(_g + "-nb8-acc", _g, *BATCH_SHAPE, nbatch=8, accumulate=True, **_kw)
    _case(_g + "-nb8-A-stride0", _g, *BATCH_SHAPE, nbatch=8, fa=FR._replace(expand=True), **_kw)
    _case(_g + "-nb8-B-stride0", _g, *BATCH_SHAPE, nbatch=8, fb=FR._replace(expand=True), **_kw)
    _case(_g + "-nb8-C-stride", _g, *BATCH_SHAPE, nbatch=8, fc=FR._replace(bpad=12), **_kw)
    # Z = 24: the 1-d grid with slices and batches together, and the batched reducer (slices 16 wide, 5..7 empty)
    _case(_g + "-nb3-split8", _g, *BATCH_SHAPE, nbatch=3, split_k=8, mode=_mode, kind="raw", route=big_route(_mode))
# batch stride M * K + 2: not a multiple of 4
_case("batch-bf16x3-nb8-A-stride-odd", "batch-bf16x3", *BATCH_SHAPE, nbatch=8, mode=BF16X3, kind="batched",
      fa=FR._replace(ldpad=0, bpad=2), route=K_F32)

# ---- 5. the step kernel's linear path, M <= 64 (SK_NW = 8 waves share K in chunks of 16, ring depth 2) -------------------
for _tb in (False, True):
    _case(f"step-ragged-N30-{layout_name(False, _tb)}", "step-fast", 8, 30, 64, tb=_tb, bias=True, route=STEP)
for _K in (128, 144, 272):   # 8, 9 and 17 chunks: every wave owns 1, then 1 or 2, then 2 or 3
    _case(f"step-K{_K}", "step-fast", 16, 64, _K, bias=True, route=STEP)
_case("step-lda-K4", "step-fast", 16, 48, 64, bias=True, fa=FR._replace(ldpad=4), route=STEP)   # stays on the fast path
_case("step-ldc-N3", "step-fast", 16, 48, 64, bias=True, fc=FR._replace(ldpad=3), route=STEP)
# the generic path, by each condition of sk_finalize_job in turn
_case("step-A-off1", "step-generic", 16, 48, 64, bias=True, fa=FR._replace(off=5), route=STEP)
_case("step-lda-K1", "step-generic", 16, 48, 64, bias=True, fa=FR._replace(ldpad=1), route=STEP)
_case("step-NT-ldb-K2", "step-generic", 16, 48, 64, tb=True, bias=True, fb=FR._replace(ldpad=2), route=STEP)
_case("step-K72", "step-generic", 16, 48, 72, bias=True, route=STEP)
for _act, _n in ((RELU, "relu"), (TANH, "tanh"), (SIGMOID, "sigmoid")):
    _case(f"step-{_n}-bias", "step-epi", 16, 48, 64, bias=True, act=_act, route=STEP)
_case("step-acc-bias", "step-epi", 16, 48, 64, bias=True, accumulate=True, route=STEP)
_case("step-acc-tanh", "step-epi", 16, 48, 64, accumulate=True, act=TANH, route=STEP, raises="acc_act")
# alpha != 1 keeps a small product off the step kernel (M < 128: the f32 kernel in either f32-grade mode)
_case("step-M8-alpha2", "step-epi", 8, 48, 64, alpha=2.0, bias=True, route=K_F32)
# M = 64 against M = 65 on the same data (tests/test_gpu_gemm_edges.py runs both on rows of one operand)
_case("step-M64", "step-boundary", 64, 96, 128, bias=True, route=STEP)
_case("step-M65", "step-boundary", 65, 96, 128, bias=True, route=K_F32)
_case("step-M65-f32", "step-boundary", 65, 96, 128, bias=True, mode=F32, route=K_F32)

# ---- 6. stream capture: a split product runs unsplit inside a capture ---------------------------------------------------
CAPTURE_SHAPE = (96, 200, 2048)   # a.t() @ b with split_k = 4

GROUPS = {}
for _c in CASES.values():
    GROUPS.setdefault(_c["group"], []).append(_c["name"])


# ---- geometry -----------------------------------------------------------------------------------------------------------
def storage_shape(c, which):
    """(rows, cols) of an operand as it lies in memory."""
    M, N, K = c["M"], c["N"], c["K"]
    if which == "a":
        return (K, M) if c["ta"] else (M, K)
    if which == "b":
        return (N, K) if c["tb"] else (K, N)
    return (M, N)   # c, gate


def frame_of(c, which):
    return c["f" + which]


def ld_of(c, which):
    return storage_shape(c, which)[1] + frame_of(c, which).ldpad


def batch_stride(c, which):
    """Element stride between batch entries as the call passes it (0 for a single product)."""
    if c["nbatch"] == 1 or frame_of(c, which).expand:
        return 0
    return storage_shape(c, which)[0] * ld_of(c, which) + frame_of(c, which).bpad


def route_args(c, base_a=0x10000, base_b=0x40000000):
    """Arguments of parrot_gemm_route for the case (up to the two output pointers), with made-up 4096-aligned bases."""
    gated = c["kind"] == "gated"
    return (base_a + 4 * c["fa"].off, ld_of(c, "a"), int(c["ta"]), base_b + 4 * c["fb"].off, ld_of(c, "b"), int(c["tb"]),
            c["M"], c["N"], c["K"], 1.0 if gated else float(c["alpha"]), 0 if gated else c["act"], c["nbatch"],
            batch_stride(c, "a"), batch_stride(c, "b"), 0 if gated else c["split_k"], int(gated))


def place(x, frame, fill):
    """x: [rows, cols] or [nb, rows, cols] values -> (flat buffer filled with `fill` around them, the view of x in it)."""
    batched = x.dim() == 3
    nb = x.shape[0] if batched else 1
    rows, cols = x.shape[-2:]
    ld = cols + frame.ldpad
    one = (rows - 1) * ld + cols
    bs = 0 if frame.expand else rows * ld + frame.bpad
    buf = torch.full((frame.off + (0 if frame.expand else nb - 1) * bs + one + frame.tail,), fill, dtype=x.dtype)
    if batched:
        view = buf.as_strided((nb, rows, cols), (bs, ld, 1), frame.off)
        if frame.expand:
            view[0].copy_(x[0])
        else:
            view.copy_(x)
    else:
        view = buf.as_strided((rows, cols), (ld, 1), frame.off)
        view.copy_(x)
    return buf, view


def view_in(buf, shape, frame):
    """The view `place` made, taken again in a copy of its buffer (on any device)."""
    if len(shape) == 3:
        nb, rows, cols = shape
        ld = cols + frame.ldpad
        return buf.as_strided((nb, rows, cols), (0 if frame.expand else rows * ld + frame.bpad, ld, 1), frame.off)
    rows, cols = shape
    return buf.as_strided((rows, cols), (cols + frame.ldpad, 1), frame.off)


# ---- data and float64 reference -------------------------------------------------------------------------------------------
def data(c):
    """Logical operands of the case in float32 on the CPU: a [nb, M, K] (entries ~ N(0, 1/K)), b [nb, K, N], bias [N],
    c0 [nb, M, N] (the output's prior content), gate [M, N] with zeros and negatives.  nb = 1 is squeezed away; an
    operand with batch stride 0 has the same matrix in every batch."""
    M, N, K, nb = c["M"], c["N"], c["K"], c["nbatch"]
    g = torch.Generator().manual_seed(zlib.crc32(f"{M},{N},{K},{nb}".encode()))
    a = (torch.randn(nb, M, K, generator=g, dtype=torch.float64) / math.sqrt(K)).float()
    b = torch.randn(nb, K, N, generator=g, dtype=torch.float64).float()
    bias = torch.randn(N, generator=g, dtype=torch.float64).float()
    c0 = torch.randn(nb, M, N, generator=g, dtype=torch.float64).float()
    gate = torch.randn(M, N, generator=g, dtype=torch.float64).float()
    gate[torch.rand(M, N, generator=g) < 0.125] = 0.0
    if c["fa"].expand:
        a = a[:1].expand(nb, M, K)
    if c["fb"].expand:
        b = b[:1].expand(nb, K, N)
    if nb == 1:
        a, b, c0 = a[0], b[0], c0[0]
    return dict(a=a, b=b, bias=bias, c0=c0, gate=gate)


def reference(c, d, f32=False):
    """The call's expression in float64 (f32 = True: torch's float32 evaluation of the same expression, for judging a
    bound).  Under PRECISION_BF16 on the bf16-operand kernel the operands are rounded to bf16 first."""
    dt = torch.float32 if f32 else torch.float64
    a, b = d["a"], d["b"]
    if c["route"] == K_BF16:
        a, b = a.to(torch.bfloat16), b.to(torch.bfloat16)
    v = float(c["alpha"]) * (a.to(dt) @ b.to(dt)) if c["kind"] != "gated" else a.to(dt) @ b.to(dt)
    if c["bias"]:
        v = v + d["bias"].to(dt)
    if c["accumulate"]:
        v = v + d["c0"].to(dt)
    if c["act"] == RELU:
        v = torch.relu(v)
    elif c["act"] == TANH:
        v = torch.tanh(v)
    elif c["act"] == SIGMOID:
        v = torch.sigmoid(v)
    if c["kind"] == "gated":
        v = v * (d["gate"] > 0).to(dt)
    return v
