"""The kernels that turn gradients into a parameter update, at their edges: parrot_colsum (every case of
tests/reduce_cases.py, exactly), parrot_sumsq, parrot_adam_clip_step and Trainer.step, parrot_simple_norm_fwd/bwd with
real leading dimensions and aliased buffers, the rounding of parrot_to_bf16, and parrot_batch_quantize on one-signed rows.

Two kinds of check.  EXACT: integer-valued float32 data whose every partial sum is an integer below 2^24 (any order of
summation gives the same bits), bit patterns, integer classes: compared with torch.equal, no tolerance.  TOLERANCED
(sumsq on randn, the Adam update, simple_norm): the reference is float64; the allowance is measured, not chosen -- the
same arithmetic restated in torch CPU float32 on the same inputs, its error against float64, times a fixed factor for
fused multiply-adds and the order of operations (`_allow`).  Every toleranced check prints its three figures
(profiles/reduce_optim_errors.md keeps a record of them)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import reduce_cases as RC
from tests.util import make_batch

pytestmark = pytest.mark.gpu

F32 = torch.float32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ulp(x):
    """The spacing of float32 at |x|."""
    return float(np.spacing(np.float32(abs(float(x)))))


def _allow(what, got, ref64, restated32):
    """The Adam / simple_norm rule: the kernel may have 4 times the error of the float32 restatement (fused multiply-adds,
    operation order) plus one ulp of the largest reference value.  Errors are max |. - ref64|."""
    ref64 = ref64.detach().double().cpu()
    err = float((got.detach().double().cpu() - ref64).abs().max())
    err32 = float((restated32.detach().double().cpu() - ref64).abs().max())
    tol = 4.0 * err32 + _ulp(ref64.abs().max())
    print(f"[figures] {what}: kernel {err:.3e}  float32 restatement {err32:.3e}  allowed {tol:.3e}")
    assert err <= tol, f"{what}: error {err:.3e} against float64 > {tol:.3e} (float32 restatement: {err32:.3e})"


# ---- colsum ---------------------------------------------------------------------------------------------------------------
def _colsum_buffers(c, xbuf, obuf, dev):
    xd, od = xbuf.to(dev), obuf.to(dev)
    assert xd.data_ptr() % 16 == 0 and od.data_ptr() % 16 == 0
    return xd, od, RC.x_view(xd, c), od[c.ooff:c.ooff + c.N]


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_colsum_exact(dev, name):
    """Integer data: the column sums (plus the old values when accumulating) bit for bit, whatever the order; the floats on
    either side of `out` -- the neighbouring parameters' gradients in the flat buffer -- and `x` are left alone."""
    from parrot_amd import ops
    c = RC.CASES[name]
    xbuf, obuf = RC.integer_data(c)
    xd, od, x, out = _colsum_buffers(c, xbuf, obuf, dev)
    assert ops.colsum_route(x, out) == (c.vec4, c.ysplit), "the case no longer takes the route it was written for"
    ret = ops.colsum(x, out=out, accumulate=bool(c.accumulate))
    assert ret.data_ptr() == out.data_ptr()
    want = RC.x_view(xbuf, c).long().sum(0)
    if c.accumulate:
        want = want + obuf[c.ooff:c.ooff + c.N].long()
    got = od.cpu()
    assert torch.equal(got[c.ooff:c.ooff + c.N], want.float()), \
        f"{int((got[c.ooff:c.ooff + c.N] != want.float()).sum())} of {c.N} column sums differ"
    assert torch.equal(got[:c.ooff], obuf[:c.ooff]), "a store landed before out[0]"
    assert torch.equal(got[c.ooff + c.N:], obuf[c.ooff + c.N:]), "a store landed past out[N-1]"
    assert torch.equal(xd.cpu(), xbuf), "x was written"


def test_colsum_exact_fresh_output_and_3d(dev):
    """The wrapper's other entries: no `out` (a fresh result, never accumulated into), a 3-d input, no rows."""
    from parrot_amd import ops
    x = torch.randint(-8, 9, (5, 13, 24), generator=torch.Generator().manual_seed(5)).float()
    xd = x.to(dev)
    assert ops.colsum_route(xd) == (1, 1)
    assert torch.equal(ops.colsum(xd, accumulate=True).cpu(), x.long().sum((0, 1)).float())
    old = torch.arange(24.0).to(dev)
    assert torch.equal(ops.colsum(xd[:0].reshape(0, 24), out=old.clone(), accumulate=True), old)
    assert torch.equal(ops.colsum(xd[:0].reshape(0, 24), out=old.clone()), torch.zeros_like(old))


@pytest.mark.parametrize("name", ["v4-rows-M99-N12-ld12-x0-o8-set", "v4-short-M1025-N12-ld12-x0-o8-set",
                                  "s-N-M70-N30-ld32-x0-o8-set", "s-split-M4100-N65-ld67-x0-o8-set"])
def test_colsum_rounding(dev, name):
    """randn against float64, per column: |err| <= L * 2^-24 * sum_m |x[m,n]| with L the longest chain of dependent
    additions the route implies (reduce_cases.chain_length, from the route the library reports): each addition rounds a
    partial sum no larger than sum |x| by at most half an ulp of it."""
    from parrot_amd import ops
    c = RC.CASES[name]
    g = torch.Generator().manual_seed(c.M * 1000 + c.N)
    xbuf = torch.randn(RC.x_extent(c), generator=g)
    obuf = torch.zeros(c.ooff + c.N + RC.GUARD)
    xd, od, x, out = _colsum_buffers(c, xbuf, obuf, dev)
    vec4, ysplit = ops.colsum_route(x, out)
    assert (vec4, ysplit) == (c.vec4, c.ysplit)
    ops.colsum(x, out=out)
    x64 = RC.x_view(xbuf, c).double()
    err = (out.double().cpu() - x64.sum(0)).abs()
    bound = RC.chain_length(c.M, ysplit) * 2.0 ** -24 * x64.abs().sum(0)
    print(f"[figures] colsum {name}: worst error / bound = {float((err / bound).max()):.3f} (L = {RC.chain_length(c.M, ysplit)})")
    assert bool((err <= bound).all()), f"column {int((err / bound).argmax())}: {float((err / bound).max()):.2f} x the bound"


# ---- sumsq ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", RC.SUMSQ_N + (RC.SUMSQ_N_BIG,))
def test_sumsq_exact(dev, n):
    """Values in {-2..2}: every partial sum is an integer below 2^24.  n < 4 and n % 4 are block 0's scalar tail, the largest
    n runs the grid-stride loop past the 2048-block cap as well.  A fresh result, a result buffer holding garbage, two
    runs: the same bits."""
    from parrot_amd import ops
    x = torch.randint(-2, 3, (n,), generator=torch.Generator().manual_seed(n))
    want = torch.tensor([float(int((x * x).sum()))])
    assert float(want) < 2 ** 24
    xd = x.float().to(dev)
    first = ops.sumsq(xd)
    assert first.shape == (1,) and torch.equal(first.cpu(), want), f"{float(first)} != {float(want)}"
    out = torch.full((1,), 12345.0, device=dev)
    assert ops.sumsq(xd, out=out) is out
    assert torch.equal(out.cpu(), want), "a result buffer holding garbage changed the sum"


def test_sumsq_reproducible_and_rounding(dev):
    """randn, n = 65536, against float64: 8 times the larger of torch's own float32 error on the same data and one ulp of
    the result (2^-23 * ref) -- the chains differ in shape, the exact cases carry the structural checks.  Two runs give
    the same bits (fixed-order partials, no atomics)."""
    from parrot_amd import ops
    x = torch.randn(65536, generator=torch.Generator().manual_seed(65536))
    ref = float((x.double() ** 2).sum())
    err32 = abs(float((x * x).sum()) - ref)
    xd = x.to(dev)
    a, b = ops.sumsq(xd), ops.sumsq(xd)
    assert torch.equal(a, b)
    err = abs(float(a) - ref)
    tol = 8.0 * max(err32, 2.0 ** -23 * ref)
    print(f"[figures] sumsq n=65536: kernel {err:.3e}  float32 restatement {err32:.3e}  allowed {tol:.3e}  (ref {ref:.6e})")
    assert err <= tol
    big = torch.randn(RC.SUMSQ_N_BIG, generator=torch.Generator().manual_seed(3)).to(dev)
    assert torch.equal(ops.sumsq(big), ops.sumsq(big)), "two runs past the block cap differ"


# ---- adam_clip_step -------------------------------------------------------------------------------------------------------
ADAM = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8)


def _adam32(p, g, m, v, gnorm_sq, step, clip, grad_scale, lr, b1, b2, eps):
    """The update restated in torch CPU float32, in place.  Every hyper-parameter is the float32 value the C ABI receives,
    the bias correction included: 1 - 0.999f is 1.3e-5 (relative) off 1 - 0.999, so the step size of ANY float32 statement
    of this update sits 6e-6 off the float64 oracle's at step 1 -- that is part of the measured float32 error, and of
    what the kernel (whose host side forms lr_t in double, but from the same float32 b1 and b2) may have."""
    t = lambda s: torch.tensor(s, dtype=F32)  # noqa: E731
    scale = t(grad_scale)
    if clip > 0:
        nrm = gnorm_sq.to(F32).sqrt() * t(grad_scale)
        if bool(nrm > t(clip)):
            scale = scale * (t(clip) / nrm)
    lr_t = t(lr) * (t(1.0) - t(b2) ** step).sqrt() / (t(1.0) - t(b1) ** step)
    gi = g * scale
    m.copy_(t(b1) * m + (t(1.0) - t(b1)) * gi)
    v.copy_(t(b2) * v + (t(1.0) - t(b2)) * gi * gi)
    p.sub_(lr_t * m / (v.sqrt() + t(eps)))


def _with_norm(n, norm, gen):
    g = torch.randn(n, generator=gen)
    return g * (norm / float(g.double().norm()))


def _adam_state(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    m = 0.1 * torch.randn(n, generator=gen)
    v = (0.1 * torch.randn(n, generator=gen)) ** 2 + 1e-4
    return gen, p, m, v


@pytest.mark.parametrize("mode", ["clip", "noclip", "off"])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("n", RC.ADAM_N + (RC.ADAM_N_BIG,))
def test_adam_clip_step_vs_oracle(dev, n, grad_scale, mode):
    """p, m and v after each of four calls (step = 1, 2, 7, 1000: the bias correction from its largest to none) against
    oracle.parrot_ref.clip_adam_step in float64, which gets g * grad_scale.  A new gradient every call, non-zero moments
    at the start.  clip: ||g * grad_scale|| = 30 * grad_scale > 9; noclip: 3 * grad_scale < 9; off: threshold 0 and no norm
    pointer.  The kernel, the float32 restatement and the oracle each carry their own state from the same start."""
    from oracle import parrot_ref as R
    from parrot_amd import ops
    gen, p, m, v = _adam_state(n, n + 17)
    clip = 0.0 if mode == "off" else 9.0
    dp, dm, dv = p.to(dev), m.to(dev), v.to(dev)
    p32, m32, v32 = p.clone(), m.clone(), v.clone()
    rp, rm, rv = {"x": p.double()}, {"x": m.double()}, {"x": v.double()}
    for step in RC.ADAM_STEPS:
        g = _with_norm(n, 30.0 if mode == "clip" else 3.0, gen)
        dg = g.to(dev)
        ops.adam_clip_step(dp, dg, dm, dv, None if mode == "off" else ops.sumsq(dg), step, lr=ADAM["lr"], clip=clip,
                           grad_scale=grad_scale)
        _adam32(p32, g, m32, v32, (g * g).sum(), step, clip, grad_scale, **ADAM)
        tot = R.clip_adam_step(rp, {"x": g.double() * grad_scale}, rm, rv, step, lr=ADAM["lr"],
                               clip=clip if clip > 0 else float("inf"))
        assert (tot > 9.0) == (mode == "clip") or mode == "off"
        assert torch.equal(dg.cpu(), g), "the gradient was written"
        for what, got, ref, re32 in (("p", dp, rp, p32), ("m", dm, rm, m32), ("v", dv, rv, v32)):
            _allow(f"adam n={n} scale={grad_scale} {mode} step={step} {what}", got, ref["x"], re32)


def _one_step(dev, g, clip, gnorm, n_state=None, step=1, grad_scale=1.0):
    """One call from the standard start; returns (p, m, v) on the CPU."""
    from parrot_amd import ops
    n = g.numel()
    _, p, m, v = _adam_state(n, 99)
    dp, dm, dv = p.to(dev), m.to(dev), v.to(dev)
    ops.adam_clip_step(dp, g.to(dev), dm, dv, gnorm, step, lr=ADAM["lr"], clip=clip, grad_scale=grad_scale)
    return (dp.cpu(), dm.cpu(), dv.cpu()), (p, m, v)


def test_adam_clip_boundary_is_strict(dev):
    """81 ones: sumsq == 81 exactly, the norm is exactly 9.0, and `nrm > threshold` is strict: clip = 9.0 must give the bits
    of threshold = 0.  82 ones are scaled by 9 / sqrt(82): with m = v = 0 before, m == (1 - b1) * scale in every element,
    to 3 * 2^-24 relative (square root, quotient and one product, each correctly rounded; every other operation is
    exact)."""
    from parrot_amd import ops
    g = torch.ones(81)
    nrm = ops.sumsq(g.to(dev))
    assert float(nrm) == 81.0
    at, _ = _one_step(dev, g, 9.0, nrm)
    off, _ = _one_step(dev, g, 0.0, None)
    for a, b, what in zip(at, off, "pmv"):
        assert torch.equal(a, b), f"{what}: a norm equal to the threshold was clipped"
    g = torch.ones(82)
    dg = g.to(dev)
    dp, dm, dv = torch.zeros(82, device=dev), torch.zeros(82, device=dev), torch.zeros(82, device=dev)
    ops.adam_clip_step(dp, dg, dm, dv, ops.sumsq(dg), 1, lr=ADAM["lr"], clip=9.0)
    want = (1.0 - float(np.float32(0.9))) * 9.0 / math.sqrt(82.0)
    assert float(dm.max()) == float(dm.min())
    assert abs(float(dm[0]) - want) <= 3.001 * 2.0 ** -24 * want, f"m = {float(dm[0])!r}, (1 - b1) * 9 / sqrt(82) = {want!r}"
    assert float(dm[0]) < float(np.float32(1.0) - np.float32(0.9)) * 0.9999


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_adam_nonfinite_norm_skips_the_step(dev, kind):
    """A NaN in g (the norm is NaN), and finite gradients whose squares overflow (the norm is inf): p, m and v keep their
    bits."""
    from parrot_amd import ops
    n = 10007
    g = torch.randn(n, generator=torch.Generator().manual_seed(4))
    if kind == "nan":
        g[n // 2] = float("nan")
    else:
        g[:8] = 3.0e30
    dg = g.to(dev)
    nrm = ops.sumsq(dg)
    assert math.isnan(float(nrm)) if kind == "nan" else math.isinf(float(nrm))
    got, before = _one_step(dev, g, 9.0, nrm)
    for a, b, what in zip(got, before, "pmv"):
        assert torch.equal(a, b), f"{what} was written on a {kind} norm"


def test_adam_two_buffers_one_norm(dev):
    """The trainer's two parameter groups: gnorm_sq = sumsq(g1) + sumsq(g2), one step on each buffer with it.  ||g1|| =
    ||g2|| = 7: neither alone reaches the threshold of 9, together (9.9) they do.  Against the oracle called with a
    two-entry dict."""
    from oracle import parrot_ref as R
    from parrot_amd import ops
    names, sizes = ("a", "b"), (300, 1001)
    st = {k: _adam_state(n, 7 + n) for k, n in zip(names, sizes)}
    g = {k: _with_norm(n, 7.0, st[k][0]) for k, n in zip(names, sizes)}
    dg = {k: g[k].to(dev) for k in names}
    part = torch.full((1,), -1.0, device=dev)
    nrm = ops.sumsq(dg["a"])
    ops.sumsq(dg["b"], out=part)
    nrm.add_(part)
    assert float(ops.sumsq(dg["a"])) < 81.0 and float(part) < 81.0 < float(nrm)
    dev_state = {k: [t.to(dev) for t in st[k][1:]] for k in names}
    for k in names:
        ops.adam_clip_step(*dev_state[k][:1], dg[k], *dev_state[k][1:], nrm, 2, lr=ADAM["lr"], clip=9.0)
    rp, rm, rv = ({k: st[k][i].double() for k in names} for i in (1, 2, 3))
    tot = R.clip_adam_step(rp, {k: g[k].double() for k in names}, rm, rv, 2, lr=ADAM["lr"], clip=9.0)
    assert tot > 9.0
    n32 = (g["a"] * g["a"]).sum() + (g["b"] * g["b"]).sum()
    for k in names:
        p32, m32, v32 = (t.clone() for t in st[k][1:])
        _adam32(p32, g[k], m32, v32, n32, 2, 9.0, 1.0, **ADAM)
        for what, got, ref, re32 in (("p", dev_state[k][0], rp, p32), ("m", dev_state[k][1], rm, m32),
                                     ("v", dev_state[k][2], rv, v32)):
            _allow(f"adam two buffers {k} {what}", got, ref[k], re32)


# ---- Trainer.step -----------------------------------------------------------------------------------------------------------
KW = dict(num_layers=2, rnn_h_dim=64, readouts_dim=48, encoder_dim=16, input_dim=24, encoder_type='bidirectional',
          weak_feedback=True, encoder_literal=False)   # the small model of tests/test_gpu_dp.py
T, B, U = 9, 6, 7


def test_trainer_step_update_vs_oracle(dev):
    """One process, two steps, then a learning-rate cut and a third: after each step the update is redone in float64 from
    the parameters and moments before it and the gradients the step left in flat_gradients; parameters, both moments
    and the global squared norm are compared under the Adam rule (`_allow`).  cut_learning_rate zeroes both moments
    and the step count, so the step after it is a step-1 update: the oracle is called with step = 1 and zero moments."""
    from oracle import parrot_ref as R
    from parrot_amd.model import Parrot
    from parrot_amd.trainer import Trainer
    cfg = R.default_config(**KW)
    m = Parrot(device=dev, use_graph=True, **KW).allocate()
    m.set_parameter_values(R.init_params(cfg, seed=7, scale_by_fan_in=True))
    tr = Trainer(m, learning_rate=1e-2, grad_clip=0.05)  # threshold 0.5: the clip is active
    feat, fm, lab, lm, _ = make_batch(cfg, T, B, U, seed=3, ragged=True)
    try:
        for s, (a, b, want_step) in enumerate(((0, 5, 1), (4, T, 2), (4, T, 1))):
            if s == 2:
                lr = tr.lr
                tr.cut_learning_rate()
                assert tr.lr == 0.5 * lr and tr.step_count == 0
                assert not bool(tr.ms[0].any()) and not bool(tr.vs[0].any()), "the cut leaves moments behind"
            p0, m0, v0 = m.flat_parameters.detach().cpu().clone(), tr.ms[0].cpu().clone(), tr.vs[0].cpu().clone()
            tr.step(feat[a:b + 1].float().to(dev), fm[a:b + 1].float().to(dev), lab.to(dev), lm.float().to(dev), None,
                    1 if s == 0 else 0)
            assert tr.step_count == want_step
            g = m.flat_gradients.detach().cpu().clone()
            assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
            _allow(f"trainer step {s} gnorm_sq", tr.gnorm_sq, (g.double() ** 2).sum().reshape(1), (g * g).sum().reshape(1))
            rp, rm, rv = {"x": p0.double()}, {"x": m0.double()}, {"x": v0.double()}
            tot = R.clip_adam_step(rp, {"x": g.double()}, rm, rv, want_step, lr=tr.lr, clip=tr.clip)
            assert tot > tr.clip, "the clip is meant to be active"
            p32, m32, v32 = p0.clone(), m0.clone(), v0.clone()
            _adam32(p32, g, m32, v32, (g * g).sum(), want_step, tr.clip, 1.0, tr.lr, tr.beta1, tr.beta2, tr.eps)
            for what, got, rr, re32 in (("p", m.flat_parameters, rp, p32), ("m", tr.ms[0], rm, m32), ("v", tr.vs[0], rv, v32)):
                _allow(f"trainer step {s} {what}", got, rr["x"], re32)
    finally:
        m.close()


# ---- simple_norm ------------------------------------------------------------------------------------------------------------
EPS = 1e-5


class _Wide:
    """An [R, N] matrix as a column slice of a wider [R, ld] one (random padding): the pointer and leading dimension for
    the C ABI, the slice back on the CPU, and whether the padding still holds what it held."""

    def __init__(self, data, ld, off, dev, seed=0):
        R, N = data.shape
        assert off + N <= ld
        self.N, self.ld, self.off = N, ld, off
        self.host = torch.randn(R, ld, generator=torch.Generator().manual_seed(1000 + seed))
        self.host[:, off:off + N] = data
        self.d = self.host.to(dev)
        self.ptr = self.d.data_ptr() + 4 * off

    def get(self):
        return self.d[:, self.off:self.off + self.N].cpu()

    def padding_intact(self):
        now = self.d.cpu()
        keep = torch.ones(self.ld, dtype=torch.bool)
        keep[self.off:self.off + self.N] = False
        return torch.equal(now[:, keep], self.host[:, keep])


def _norm_fwd(x, y, sigma, R, N, add=None):
    from parrot_amd import _lib
    _lib.call("parrot_simple_norm_fwd", x.ptr, x.ld, y.ptr, y.ld, sigma.data_ptr(), R, N, EPS,
              None if add is None else add.ptr, 0 if add is None else add.ld, _stream())


def _norm_bwd(dy, y, sigma, dx, R, N, accumulate=0):
    from parrot_amd import _lib
    _lib.call("parrot_simple_norm_bwd", dy.ptr, dy.ld, y.ptr, y.ld, sigma.data_ptr(), dx.ptr, dx.ld, R, N, EPS,
              int(accumulate), _stream())


def _norm_ref64(x, dy):
    """oracle.parrot_ref.simple_norm and its autograd in float64 -> (y, sigma, dx).  A constant row (N = 1 included) has
    sigma = 0, where autograd differentiates sqrt at 0 and returns NaN; the kernel defines the backward there as the limit
    with the sigma term dropped, dx = (dy - mean(dy)) / eps, and that closed form is the reference for such rows."""
    from oracle import parrot_ref as Rf
    x64 = x.double().requires_grad_()
    y = Rf.simple_norm(x64, EPS)
    y.backward(dy.double())
    sigma = x64.detach().std(-1, unbiased=False)
    dx = x64.grad.clone()
    const = sigma == 0
    if bool(const.any()):
        d64 = dy.double()
        dx[const] = ((d64 - d64.mean(-1, keepdim=True)) / EPS)[const]
    return y.detach(), sigma, dx


def _norm32(x, dy):
    """The two kernels restated in torch CPU float32 -> (y, sigma, dx)."""
    N = x.shape[1]
    n, eps = torch.tensor(float(N), dtype=F32), torch.tensor(EPS, dtype=F32)
    mean = x.sum(-1, keepdim=True) / n
    d = x - mean
    sd = ((d * d).sum(-1, keepdim=True) / n).sqrt()
    inv = 1.0 / (eps + sd)
    y = d * inv
    mdy = dy.sum(-1, keepdim=True) / n
    dot = (dy * y).sum(-1, keepdim=True)
    k = torch.where(sd > 0, dot / (n * sd), torch.zeros_like(sd))
    return y, sd[:, 0], (dy - mdy) * inv - y * k


def _norm_all_paths(dev, x, dy, tag):
    """Forward (out of place with add_dst, then in place), backward (own buffer, dx aliasing dy, dx aliasing y, accumulate
    onto a non-zero dx), every matrix with its own leading dimension > N; the padding columns keep their contents."""
    R, N = x.shape
    gen = torch.Generator().manual_seed(R * 7919 + N)
    add0, acc0 = torch.randn(R, N, generator=gen), torch.randn(R, N, generator=gen)
    y64, s64, dx64 = _norm_ref64(x, dy)
    y32, s32, dx32 = _norm32(x, dy)
    X, Y, ADD = _Wide(x, N + 3, 1, dev, 1), _Wide(torch.zeros(R, N), N + 5, 2, dev, 2), _Wide(add0, N + 2, 1, dev, 3)
    sigma = torch.full((R,), -1.0, device=dev)
    _norm_fwd(X, Y, sigma, R, N, ADD)
    y = Y.get()
    _allow(f"norm {tag} y", y, y64, y32)
    _allow(f"norm {tag} sigma", sigma, s64, s32)
    _allow(f"norm {tag} add_dst", ADD.get(), add0.double() + y64, add0 + y32)
    assert torch.equal(X.get(), x), "the forward wrote its input"
    assert X.padding_intact() and Y.padding_intact() and ADD.padding_intact(), "forward: padding columns written"
    XI = _Wide(x, N + 3, 1, dev, 1)
    sigma_i = torch.full((R,), -1.0, device=dev)
    _norm_fwd(XI, XI, sigma_i, R, N)
    assert torch.equal(XI.get(), y) and torch.equal(sigma_i, sigma), "in place differs from out of place"
    assert XI.padding_intact(), "forward in place: padding columns written"
    # backward, from the kernel's own y and sigma
    DY, DX = _Wide(dy, N + 1, 0, dev, 4), _Wide(torch.zeros(R, N), N + 7, 3, dev, 5)
    _norm_bwd(DY, Y, sigma, DX, R, N)
    dx = DX.get()
    _allow(f"norm {tag} dx", dx, dx64, dx32)
    assert torch.equal(DY.get(), dy) and torch.equal(Y.get(), y), "the backward wrote an input"
    assert DY.padding_intact() and DX.padding_intact(), "backward: padding columns written"
    DY2 = _Wide(dy, N + 1, 0, dev, 4)
    _norm_bwd(DY2, Y, sigma, DY2, R, N)
    assert torch.equal(DY2.get(), dx), "dx aliasing dy differs"
    assert DY2.padding_intact()
    Y2 = _Wide(y, N + 5, 2, dev, 2)
    _norm_bwd(DY, Y2, sigma, Y2, R, N)
    assert torch.equal(Y2.get(), dx), "dx aliasing y differs"
    assert Y2.padding_intact()
    ACC = _Wide(acc0, N + 7, 3, dev, 6)
    _norm_bwd(DY, Y, sigma, ACC, R, N, accumulate=1)
    _allow(f"norm {tag} dx accumulate", ACC.get(), acc0.double() + dx64, acc0 + dx32)
    assert ACC.padding_intact()
    return y, sigma.cpu(), dx


@pytest.mark.parametrize("R", RC.NORM_R)
@pytest.mark.parametrize("N", RC.NORM_N)
def test_simple_norm_strided_aliased(dev, R, N):
    gen = torch.Generator().manual_seed(R * 1000 + N)
    x = torch.randn(R, N, generator=gen) * 2 + 0.5
    dy = torch.randn(R, N, generator=gen)
    _norm_all_paths(dev, x, dy, f"R={R} N={N}")


def test_simple_norm_large_mean_row(dev):
    """Rows of 1000 + 1e-3 * randn: the spread is 1e-6 of the mean, about 16 float32 spacings.  Two passes (mean, then the
    centred second moment) keep the row accurate; E[x^2] - E[x]^2 in float32 has no correct digit here.  Same rule."""
    gen = torch.Generator().manual_seed(11)
    x = 1000.0 + 1e-3 * torch.randn(2, 1000, generator=gen)
    dy = torch.randn(2, 1000, generator=gen)
    y, sigma, _ = _norm_all_paths(dev, x, dy, "large mean")
    one_pass = ((x * x).mean(-1) - x.mean(-1) ** 2)
    print(f"[figures] large mean: sigma {sigma.tolist()}, a one-pass float32 variance gives {one_pass.tolist()}")
    assert float(y.abs().max()) > 1.0


@pytest.mark.parametrize("N", [1, 256, 1000])
def test_simple_norm_constant_row(dev, N):
    """Constant rows (sums of 3.25 and -1.5 are exact in float32, so the mean is the constant itself): y == 0 and
    sigma == 0 exactly.  Autograd gives NaN at sigma = 0 (the derivative of sqrt at 0); the kernel's backward there is
    dx = (dy - mean(dy)) / eps, the closed form with the sigma term dropped, and that is the reference (_norm_ref64)."""
    x = torch.stack([torch.full((N,), 3.25), torch.full((N,), -1.5)])
    dy = torch.randn(2, N, generator=torch.Generator().manual_seed(N))
    y, sigma, dx = _norm_all_paths(dev, x, dy, f"constant N={N}")
    assert not bool(y.any()) and not bool(sigma.any()), "a constant row must normalise to exact zeros with sigma == 0"
    assert bool(torch.isfinite(dx).all())
    if N == 1:
        assert not bool(dx.any())


# ---- to_bf16 ----------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.cpu().contiguous().view(torch.int16)


def _from_bits(words):
    assert len(words) % 8 == 0
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32).view(F32)


def test_to_bf16_rounding_patterns(dev):
    """Bit patterns against torch CPU `x.to(torch.bfloat16)` (round to nearest, ties to even): exact ties on an even and on
    an odd upper half, one ulp either side, both signs; zeros, infinities, the largest finite float (rounds to inf);
    mantissas whose rounding carries into the exponent."""
    from parrot_amd import ops
    pos = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,   # ties and their neighbours
           0x00000000, 0x7F800000, 0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF,               # 0, inf, the largest floats
           0x3FFFFFFF, 0x3FFF8000, 0x3FFF7FFF, 0x407FFFFF, 0x00FF8000, 0x7EFFFFFF,   # carries into the exponent
           0x3F800000, 0x40490FDB, 0x00800000, 0x3F7FFFFF, 0x42FE8000, 0x42FF8000]   # plain values, the smallest normal
    pos += [0x3F800001]
    words = pos + [w | 0x80000000 for w in pos]
    x = _from_bits(words)
    got, want = _bits(ops.to_bf16(x.to(dev))), _bits(x.to(torch.bfloat16))
    bad = [(hex(w), hex(int(g) & 0xFFFF), hex(int(r) & 0xFFFF)) for w, g, r in zip(words, got, want) if g != r]
    assert not bad, f"(input, got, nearest even): {bad}"
    # what nearest-even means, independent of torch, for the two ties
    assert int(got[0]) == 0x3F80 and int(got[1]) == 0x3F82 and int(got[8]) == 0x7F80


def test_to_bf16_nan_and_subnormals(dev):
    """NaN inputs (quiet, signalling, a payload in the low half only, all mantissa bits set) come out NaN; the payload is not
    compared.  float32 subnormals come out as the nearest-even bf16 or as a zero of their sign."""
    from parrot_amd import ops
    nans = [0x7FC00000, 0x7F800001, 0x7F80FFFF, 0x7FFFFFFF, 0xFFC00000, 0xFF800001, 0xFFFFFFFF, 0x7FA00000]
    got = _bits(ops.to_bf16(_from_bits(nans).to(dev))).int() & 0xFFFF
    bad = [(hex(w), hex(int(g))) for w, g in zip(nans, got) if not (int(g) & 0x7FFF) > 0x7F80]
    assert not bad, f"NaN inputs that did not come out NaN (input, got): {bad}"
    subs = [0x00000001, 0x00008000, 0x00008001, 0x00018000, 0x00400000, 0x007FFFFF, 0x007F8000, 0x00010000]
    subs += [w | 0x80000000 for w in subs]
    x = _from_bits(subs)
    got = _bits(ops.to_bf16(x.to(dev))).int() & 0xFFFF
    want = _bits(x.to(torch.bfloat16)).int() & 0xFFFF
    seen = ["nearest" if g == r else "zero" if int(g) == (w >> 16 & 0x8000) else "other" for w, g, r in zip(subs, got, want)]
    table = [(hex(w), hex(int(g)), hex(int(r)), s) for w, g, r, s in zip(subs, got, want, seen)]
    print(f"[figures] to_bf16 subnormals (input, got, nearest even, verdict): {table}")
    assert "other" not in seen, f"subnormal inputs, neither nearest even nor a signed zero: {table}"


@pytest.mark.parametrize("n", [8, 2048, RC.BF16_BLOCK_CAP + 8])
def test_to_bf16_randn(dev, n):
    """One vector, one block, and eight elements past the 8192-block cap (the grid-stride loop).  Several scales so that the
    exponents vary."""
    from parrot_amd import ops
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen) * torch.tensor([1e-20, 1e-3, 1.0, 1e4, 1e30, 3.0, 0.1, 1e-30]).repeat(n // 8)
    out = torch.full((n + 8,), -7.0, device=dev, dtype=torch.bfloat16)
    ops.to_bf16(x.to(dev), out=out[:n])
    assert torch.equal(_bits(out[:n]), _bits(x.to(torch.bfloat16)))
    assert bool((out[n:] == -7.0).all()), "a store landed past the end"


# ---- batch_quantize ---------------------------------------------------------------------------------------------------------
def _quantize_rows():
    """name -> float32 rows [rows, n].  No constant row: the reference divides 0 by 0 there and casts NaN to an integer, so
    its value is not a contract."""
    rng = np.random.RandomState(77)
    pz, nz = np.float32(0.0), np.float32(-0.0)
    rows = {
        "all-positive": np.abs(rng.randn(3, 1000)) + 0.5,
        "all-negative": -np.abs(rng.randn(3, 1000)) - 0.5,
        "tiny-positive": np.abs(rng.randn(2, 70)) * 1e-30 + 1e-32,
        "min-is-zero": np.stack([np.r_[pz, np.abs(rng.randn(99)) + 0.1], np.r_[np.abs(rng.randn(99)) + 0.1, nz],
                                 np.r_[nz, pz, np.abs(rng.randn(98)) + 0.1], np.r_[pz, nz, np.abs(rng.randn(98)) + 0.1]]),
        "max-is-zero": np.stack([np.r_[pz, -np.abs(rng.randn(99)) - 0.1], np.r_[-np.abs(rng.randn(99)) - 0.1, nz],
                                 np.r_[nz, pz, -np.abs(rng.randn(98)) - 0.1], np.r_[pz, nz, -np.abs(rng.randn(98)) - 0.1]]),
        "two-elements": np.array([[0.25, -3.0]]),
        "two-elements-positive": np.array([[7.0, 2.0]]),
        "300-rows": rng.randn(300, 16) + np.where(np.arange(300) % 3 == 0, 5.0, np.where(np.arange(300) % 3 == 1, -5.0, 0.0))[:, None],
        "long-row": rng.randn(1, 300000) * 0.3 + 2.0,
    }
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in rows.items()}


QROWS = _quantize_rows()


def test_quantize_rows_premises():
    assert (QROWS["all-positive"] > 0).all() and (QROWS["all-negative"] < 0).all() and (QROWS["long-row"].min() > 0)
    assert QROWS["300-rows"].shape[0] > 256 and (QROWS["300-rows"][0::3] > 0).all() and (QROWS["300-rows"][1::3] < 0).all()
    assert QROWS["long-row"].shape[1] > 256 * 256 * 4 > 64 * 256 * 8   # past both grid caps
    for k in ("min-is-zero", "max-is-zero"):
        z = QROWS[k][:, :2]
        assert np.signbit(z[1:3]).any() and not np.signbit(z[0, 0])
    assert all((v.max(1) > v.min(1)).all() for v in QROWS.values()), "a constant row"


@pytest.mark.parametrize("q_type", ["mu-law", "linear"])
@pytest.mark.parametrize("name", sorted(QROWS))
def test_quantize_one_signed_rows(dev, name, q_type):
    """Bit-exact against oracle.quantize_ref.batch_quantize.  A row of one sign takes the other branch of the
    order-preserving key (f2key / key2f) for its max or its min; +0 and -0 sit on either side of the key's sign switch."""
    from oracle import quantize_ref as Q
    from parrot_amd import ops
    x = QROWS[name]
    got = ops.batch_quantize(torch.from_numpy(x).to(dev), 256, q_type).cpu().numpy()
    want = Q.batch_quantize(x.copy(), 256, q_type)
    assert got.dtype == want.dtype
    assert np.array_equal(got, want), f"{(got != want).sum()} of {got.size} classes differ, rows {sorted(set(np.nonzero(got != want)[0]))[:8]}"


@pytest.mark.parametrize("mode,dtype", [(0, torch.int16), (1, torch.int32)])
def test_quantize_strided(dev, mode, dtype):
    """ld > n and ldo > n through the C ABI: rows taken from a wider matrix, classes written into a wider one whose padding
    keeps its contents."""
    from oracle import quantize_ref as Q
    from parrot_amd import _lib
    rows, n, ld, ldo = 5, 333, 340, 337
    rng = np.random.RandomState(5)
    wide = rng.randn(rows, ld).astype(np.float32) * 100.0          # padding far outside the rows' range
    wide[:, 3:3 + n] = (rng.randn(rows, n) + np.array([4.0, -4.0, 0.0, 9.0, -9.0])[:, None]).astype(np.float32)
    xd = torch.from_numpy(wide).to(dev)
    out = torch.full((rows, ldo), -7, device=dev, dtype=dtype)
    ws = torch.empty(2 * rows, device=dev, dtype=torch.float64)
    _lib.call("parrot_batch_quantize", xd.data_ptr() + 4 * 3, rows, n, ld, ws.data_ptr(),
              out.data_ptr() + 2 * out.element_size(), ldo, mode, 256, _stream())
    got = out.cpu().numpy()
    want = Q.batch_quantize(wide[:, 3:3 + n].copy(), 256, "linear" if mode else "mu-law")
    assert np.array_equal(got[:, 2:2 + n], want)
    assert (got[:, :2] == -7).all() and (got[:, 2 + n:] == -7).all(), "padding of the output written"
    assert torch.equal(xd.cpu(), torch.from_numpy(wide))
