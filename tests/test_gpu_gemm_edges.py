"""Every epilogue, stride and dispatch boundary of parrot_gemm against the same expression in float64 (tests/gemm_cases.py).

Each case first asserts its route (ops.gemm_route: the kernel the call takes and the K slices it plans), then runs with
its operands as views into NaN-filled buffers (a read outside an operand poisons the result) and its output as a view
into a buffer filled with a fixed value, which must be bit-identical afterwards; the output itself is pre-filled with
NaN unless the call accumulates.  Tolerances are the project's own norm-wise ones (gemm_cases.TOL_*).

The float64 reference of a case is computed once per process and shared; nothing in it may be modified."""
import functools

import pytest
import torch

from tests import gemm_cases as G
from tests.util import assert_close

pytestmark = pytest.mark.gpu

NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _data(M, N, K, nb, a_exp, b_exp):
    return G.data(dict(M=M, N=N, K=K, nbatch=nb, fa=G.FR._replace(expand=a_exp), fb=G.FR._replace(expand=b_exp)))


def _case_data(c):
    return _data(c["M"], c["N"], c["K"], c["nbatch"], c["fa"].expand, c["fb"].expand)


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = G.CASES[name]
    return G.reference(c, _case_data(c))


def _stored(c, x, which):
    """A logical operand as it lies in memory: transposed where the call passes a transposed view."""
    t = c["ta"] if which == "a" else c["tb"]
    return x.transpose(-1, -2) if t else x


def _frames(c, d, dev):
    """Device buffers and views of a case: operands in NaN frames, the output in a FRAME_FILL frame."""
    f = {}
    for w in ("a", "b"):
        buf, _ = G.place(_stored(c, d[w], w), c["f" + w], NAN)
        buf = buf.to(dev)
        v = G.view_in(buf, tuple(_stored(c, d[w], w).shape), c["f" + w])
        f[w] = v.transpose(-1, -2) if (c["ta"] if w == "a" else c["tb"]) else v
    if c["bias"]:
        buf, _ = G.place(d["bias"][None, :], G.FR, NAN)
        f["bias"] = G.view_in(buf.to(dev), (1, c["N"]), G.FR)[0]
    if c["kind"] == "gated":
        buf, _ = G.place(d["gate"], c["fg"], NAN)
        f["gate"] = G.view_in(buf.to(dev), tuple(d["gate"].shape), c["fg"])
    interior = d["c0"] if c["accumulate"] else torch.full_like(d["c0"], NAN)
    buf, _ = G.place(interior, c["fc"], G.FRAME_FILL)
    f["cbuf"] = buf.to(dev)
    f["cbuf0"] = f["cbuf"].clone()
    f["out"] = G.view_in(f["cbuf"], tuple(d["c0"].shape), c["fc"])
    return f


def _frame_intact(c, f, whole=False):
    """The output buffer outside the M x N block(s) (whole: all of it) is bit-identical to what it was."""
    after = f["cbuf"].clone()
    if not whole:
        shape = tuple(f["out"].shape)
        G.view_in(after, shape, c["fc"]).copy_(G.view_in(f["cbuf0"], shape, c["fc"]))
    return torch.equal(after.view(torch.int32), f["cbuf0"].view(torch.int32))


def _call(c, f):
    from parrot_amd import _lib, ops
    if c["kind"] == "gated":
        return ops.gemm_gated(f["a"], f["b"], f["gate"], out=f["out"])
    if c["kind"] == "batched":
        return ops.gemm_batched(_unt(c, f, "a"), _unt(c, f, "b"), f["out"], transA=c["ta"], transB=c["tb"],
                                accumulate=c["accumulate"])
    if c["kind"] == "raw":
        a, b, o = _unt(c, f, "a"), _unt(c, f, "b"), f["out"]
        return _lib.call("parrot_gemm", a.data_ptr(), a.stride(1), int(c["ta"]), b.data_ptr(), b.stride(1), int(c["tb"]),
                         o.data_ptr(), o.stride(1), c["M"], c["N"], c["K"], None, float(c["alpha"]), int(c["accumulate"]),
                         c["act"], c["nbatch"], a.stride(0), b.stride(0), o.stride(0), c["split_k"], ops._stream())
    return ops.gemm(f["a"], f["b"], bias=f.get("bias"), out=f["out"], accumulate=c["accumulate"], act=c["act"],
                    alpha=c["alpha"], split_k=c["split_k"])


def _unt(c, f, w):
    """The stored (untransposed) 3-d operand gemm_batched takes."""
    return f[w].transpose(-1, -2) if (c["ta"] if w == "a" else c["tb"]) else f[w]


def _route(c, f):
    from parrot_amd import ops
    if c["kind"] == "gated":
        return ops.gemm_route(f["a"], f["b"], gate=f["gate"])
    if c["kind"] in ("batched", "raw"):
        if c["kind"] == "raw":   # gemm_route's nbatch form asks about gemm_batched's call (one slice): ask the library
            import ctypes as C
            from parrot_amd import _lib
            a, b = _unt(c, f, "a"), _unt(c, f, "b")
            k, s = C.c_int(-1), C.c_int(-1)
            _lib.call("parrot_gemm_route", a.data_ptr(), a.stride(1), int(c["ta"]), b.data_ptr(), b.stride(1), int(c["tb"]),
                      c["M"], c["N"], c["K"], float(c["alpha"]), c["act"], c["nbatch"], a.stride(0), b.stride(0),
                      c["split_k"], 0, C.byref(k), C.byref(s))
            return k.value, s.value
        return ops.gemm_route(_unt(c, f, "a"), _unt(c, f, "b"), nbatch=c["nbatch"], transA=c["ta"], transB=c["tb"])
    return ops.gemm_route(f["a"], f["b"], bias=f.get("bias"), out=f["out"], accumulate=c["accumulate"], act=c["act"],
                          alpha=c["alpha"], split_k=c["split_k"])


def run_case(name, dev):
    from parrot_amd import _lib, ops
    c = G.CASES[name]
    d = _case_data(c)
    f = _frames(c, d, dev)
    # the made-up addresses of the CPU premise test and the real ones agree on what matters: alignment
    assert f["a"].data_ptr() % 16 == (4 * c["fa"].off) % 16 and f["b"].data_ptr() % 16 == (4 * c["fb"].off) % 16
    with ops.gemm_precision(c["mode"]):
        if c["raises"] == "split_act":
            with pytest.raises(_lib.HipCallError):
                _route(c, f)
            with pytest.raises(_lib.HipCallError):
                _call(c, f)
        elif c["raises"] == "acc_act":
            assert _route(c, f) == (c["route"], c["slices"]), name
            with pytest.raises(ValueError):
                _call(c, f)
            o = f["out"]   # and the library itself refuses, whatever M
            rc = _lib.load().parrot_gemm(f["a"].data_ptr(), G.ld_of(c, "a"), int(c["ta"]), f["b"].data_ptr(), G.ld_of(c, "b"),
                                         int(c["tb"]), o.data_ptr(), o.stride(0), c["M"], c["N"], c["K"], None, 1.0, 1,
                                         c["act"], 1, 0, 0, 0, 1, ops._stream())
            assert rc == G.BADARG
        else:
            assert _route(c, f) == (c["route"], c["slices"]), f"{name}: route"
            _call(c, f)
    torch.cuda.synchronize()
    if c["raises"]:
        assert _frame_intact(c, f, whole=True), f"{name}: a refused call wrote to its output"
        return None
    assert _frame_intact(c, f), f"{name}: stored outside the M x N block"
    out = f["out"].cpu().contiguous()
    ref = _reference(name)
    e = assert_close(out, ref, c["tol"], name)
    print(f"{name}: rel err {e:.3e} (bound {c['tol']:.0e})")
    if c["kind"] == "gated":
        closed = ~(d["gate"] > 0)
        assert closed.any() and (d["gate"] == 0).any() and (d["gate"] < 0).any()
        assert bool((out.view(torch.int32)[closed] == 0).all()), f"{name}: a gated element is not exactly 0.0"
    return out


@pytest.mark.parametrize("group", sorted(G.GROUPS))
def test_gemm_edges(dev, group):
    for name in G.GROUPS[group]:
        run_case(name, dev)


def test_step_kernel_boundary_same_data(dev):
    """M = 64 (step kernel) against M = 65 (f32 kernel) on the same data: rows 0..63 agree within the sum of the two
    kernels' tolerances, and each is right against float64."""
    from parrot_amd import ops
    c = G.CASES["step-M65"]
    d = _case_data(c)
    f = _frames(c, d, dev)
    ref = _reference("step-M65")
    with ops.gemm_precision(c["mode"]):
        assert ops.gemm_route(f["a"][:64], f["b"], bias=f["bias"]) == (G.STEP, 1)
        assert ops.gemm_route(f["a"], f["b"], bias=f["bias"])[0] in (G.K_F32, G.K_BF16X3)
        o64 = ops.gemm(f["a"][:64], f["b"], bias=f["bias"])
        o65 = ops.gemm(f["a"], f["b"], bias=f["bias"])
    torch.cuda.synchronize()
    assert_close(o64, ref[:64], G.TOL_STEP, "M = 64")
    assert_close(o65, ref, G.TOL_BIG, "M = 65")
    assert_close(o64, o65[:64].double().cpu(), G.TOL_STEP + G.TOL_BIG, "M = 64 against rows 0..63 of M = 65")


def test_split_runs_unsplit_inside_a_capture(dev):
    """One single-stream capture of a split_k = 4 product: no workspace may be taken inside a capture, so the product
    runs unsplit -- both replays are bit-identical to the eager split_k = 1 result."""
    from parrot_amd import ops
    M, N, K = G.CAPTURE_SHAPE
    g = torch.Generator().manual_seed(61)
    a = torch.randn(K, M, generator=g).to(dev)
    b = torch.randn(K, N, generator=g).to(dev)
    ref = a.double().cpu().t() @ b.double().cpu()
    assert ops.gemm_route(a.t(), b, split_k=4)[1] == 4    # planned; the fallback comes after
    eager1 = ops.gemm(a.t(), b, split_k=1)
    eager4 = ops.gemm(a.t(), b, split_k=4)
    out = torch.full((M, N), NAN, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.gemm(a.t(), b, out=out, split_k=4)
    replays = []
    for _ in range(2):
        out.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        replays.append(out.clone())
    for r in replays:
        assert torch.equal(r.view(torch.int32), eager1.view(torch.int32)), "the captured product did not run unsplit"
        assert_close(r, ref, G.TOL_SPLIT, "captured product")
    assert_close(eager4, ref, G.TOL_SPLIT, "eager split_k = 4")
