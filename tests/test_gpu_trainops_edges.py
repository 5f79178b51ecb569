"""Edge tests of the SampleRNN training operators (parrot_amd/csrc/trainops.hip) and the audio quantisers
(parrot_amd/csrc/quantize.hip): every case of tests/trainops_cases.py through the C entries, against the float64
references of that module.

Every output, and every operand with a leading dimension, is a view into a larger allocation (tests/util.py Framed) whose
frame, and whose padding between the rows, holds a NaN with a payload of its own.  After a call the frame and the padding
of an output must be bit-identical and an operand unchanged as a whole; a read of an operand's padding poisons the result
(the quantisers' padding holds +-1e30 instead: a read of it moves the row's range).  Everything a kernel must write
starts as NaN.  The segmented sum's workspace is exactly as long as parrot_gather_sum_bwd_ws_floats says.

Integer cases are compared bit for bit.  Float checks are per row (cross-entropy), per element (dlogits) or per column
(weight-norm) against the bounds derived in tests/trainops_cases.py, and print `ratio <case> <buffer> <error / bound>`.
Largest ratios measured on an MI355X: lse 0.034, ce 0.035, dlogits 0.67 (1.34 against the first derivation of its bound,
which trainops_cases.dlogits_bound corrects and explains); weight-norm norm 0.094, W_eff 0.13, dg 0.042, dW 0.48."""
import warnings

import numpy as np
import pytest
import torch

from tests import trainops_cases as TC
from tests.util import FRAME_BITS, Framed, _bits, assert_close

pytestmark = pytest.mark.gpu

BADARG = 10001
NAN = float("nan")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from parrot_amd import _lib as L
    return L.load()


def _ptr(f):
    """Address of a framed view's first element (a view without elements has no data_ptr of its own)."""
    return f.big.data_ptr() + 4 * f.lo


def _matrix(dev, rows, cols, ld, data=None):
    """A framed [rows, ld] parent and its [rows, cols] view: `data`, or NaN for the kernel to overwrite.  The padding of
    every row (the last one included) keeps the frame's NaN."""
    f = Framed((rows, ld), dev)
    v = f.view[:, :cols]
    if data is None:
        v.fill_(NAN)
    else:
        v.copy_(data)
    return f, v


def _vector(dev, n, data=None):
    f = Framed((n,), dev)
    if data is None:
        f.view.fill_(NAN)
    else:
        f.view.copy_(data)
    return f


def _intact(f, cols=None):
    """The frame, and the padding of every row of a matrix, as they were."""
    pad_ok = cols is None or bool((_bits(f.view[:, cols:]) == FRAME_BITS).all())
    return f.frame_untouched() and pad_ok


def _ratio(case, buf, got, ref, bound):
    """Prints and returns the largest error / bound of a buffer.  An element that is exact passes whatever its bound."""
    got = got.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), "%s: %s has elements that are not finite (not written?)" % (case, buf)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("ratio %s %s %.4f" % (case, buf, worst))
    where = int(ratio.argmax()) if ratio.numel() else -1
    assert worst <= 1.0, "%s: %s is %.2f x its bound at flat index %d" % (case, buf, worst, where)
    return worst


# ---- gather-sum forward -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TC.FWD))
def test_gather_sum_fwd_exact(dev, name):
    c = TC.FWD[name]
    d = TC.fwd_data(c)
    tbl = Framed((c.J, c.Q, c.D), dev)
    tbl.view.copy_(d["tbl"])
    idx = d["idx"].to(torch.int32).to(dev)
    addf, _ = _matrix(dev, c.N, c.D, c.ldadd, d["add"])
    yf, y = _matrix(dev, c.N, c.D, c.ldy)
    want = TC.gather_sum_reference(d["tbl"], d["idx"], d["add"] if c.has_add else None).float()
    for f in (tbl, addf):
        f.snapshot()
    for rep in ("first", "second"):
        y.fill_(NAN)
        yf.snapshot()
        rc = _lib().parrot_gather_sum_fwd(_ptr(tbl), idx.data_ptr(), _ptr(addf) if c.has_add else None, c.ldadd if c.has_add else 0,
                                          _ptr(yf), c.ldy, c.N, c.J, c.Q, c.D, _stream())
        torch.cuda.synchronize()
        assert rc == 0
        got = y.cpu()
        assert torch.equal(got, want), "%s call: %d of %d elements differ" % (rep, int((got != want).sum()), got.numel())
        assert _intact(yf, c.D), "written outside y"
        assert tbl.untouched() and addf.untouched()


def test_gather_sum_fwd_arguments(dev):
    N, J, Q, D = 5, 2, 3, 8
    tbl = _vector(dev, J * Q * D, torch.ones(J * Q * D))
    idx = torch.zeros(N, J, dtype=torch.int32, device=dev)
    yf, y = _matrix(dev, N, D, D + 4)
    yf.snapshot()
    f = _lib().parrot_gather_sum_fwd
    assert f(_ptr(tbl), idx.data_ptr(), None, 0, _ptr(yf), D + 4, 0, J, Q, D, _stream()) == 0          # N = 0: nothing to do
    assert f(_ptr(tbl), idx.data_ptr(), None, 0, _ptr(yf), D + 4, N, J, Q, 6, _stream()) == BADARG     # D % 4
    assert f(_ptr(tbl), idx.data_ptr(), None, 0, _ptr(yf), D + 2, N, J, Q, D, _stream()) == BADARG     # ldy % 4
    assert f(_ptr(tbl), idx.data_ptr(), _ptr(tbl), D + 2, _ptr(yf), D + 4, N, J, Q, D, _stream()) == BADARG   # ldadd % 4
    torch.cuda.synchronize()
    assert yf.untouched(), "a call that returned without work wrote y"


# ---- segmented-sum backward ---------------------------------------------------------------------------------------------
def _bwd_call(c, dyf, perm, offs, dtbl, ws, n_ws, **over):
    a = dict(N=c.N, J=c.J, Q=c.Q, D=c.D, lddy=c.lddy, n_ws=n_ws)
    a.update(over)
    return _lib().parrot_gather_sum_bwd(_ptr(dyf), a["lddy"], perm.data_ptr(), offs.data_ptr(), _ptr(dtbl), _ptr(ws), a["n_ws"],
                                        a["N"], a["J"], a["Q"], a["D"], c.accumulate, _stream())


def _bwd_buffers(dev, c, d):
    n_ws = int(_lib().parrot_gather_sum_bwd_ws_floats(c.N, c.J, c.Q, c.D))
    assert n_ws == c.J * (-(-c.N // TC.GS_CH) + c.Q) * c.D
    dyf, _ = _matrix(dev, c.N, c.D, c.lddy, d["dy"])
    return dyf, d["perm"].to(dev), d["offs"].to(dev), Framed((c.J, c.Q, c.D), dev), Framed((n_ws,), dev), n_ws


@pytest.mark.parametrize("name", sorted(TC.BWD))
def test_gather_sum_bwd_exact(dev, name):
    c = TC.BWD[name]
    d = TC.bwd_data(c)
    dyf, perm, offs, dtbl, ws, n_ws = _bwd_buffers(dev, c, d)
    dyf.snapshot()
    want = TC.segmented_sum_reference(d["idx"], d["dy"], c.Q, d["old"] if c.accumulate else None).float()
    for rep in ("first", "second"):
        ws.view.fill_(NAN)
        if c.accumulate:
            dtbl.view.copy_(d["old"])
        else:
            dtbl.view.fill_(NAN)
        ws.snapshot()
        dtbl.snapshot()
        rc = _bwd_call(c, dyf, perm, offs, dtbl, ws, n_ws)
        torch.cuda.synchronize()
        assert rc == 0
        got = dtbl.view.cpu()
        assert torch.equal(got, want), "%s call: %d of %d elements differ, bins %s" % (
            rep, int((got != want).sum()), got.numel(), sorted(set(torch.nonzero((got != want).any(2))[:, 1].tolist()))[:8])
        assert dtbl.frame_untouched() and ws.frame_untouched(), "written outside dtbl or the workspace"
        assert dyf.untouched()


def test_gather_sum_bwd_arguments(dev):
    """What returns PARROT_ERR_BADARG does so before any launch: dtbl and the workspace keep their NaNs."""
    c = TC.BWD["bwd-runs-a-N109-J2-Q9-D12-set"]
    d = TC.bwd_data(c)
    dyf, perm, offs, dtbl, ws, n_ws = _bwd_buffers(dev, c, d)
    dtbl.view.fill_(NAN)
    ws.view.fill_(NAN)
    dtbl.snapshot()
    ws.snapshot()
    assert _bwd_call(c, dyf, perm, offs, dtbl, ws, n_ws - 1) == BADARG    # a workspace one float short
    assert _bwd_call(c, dyf, perm, offs, dtbl, ws, n_ws, D=10) == BADARG            # D % 4
    assert _bwd_call(c, dyf, perm, offs, dtbl, ws, n_ws, lddy=c.lddy + 2) == BADARG  # lddy % 4
    assert _bwd_call(c, dyf, perm, offs, dtbl, ws, 1 << 40, J=65536) == BADARG       # J is a grid's y extent
    assert _bwd_call(c, dyf, perm, offs, dtbl, ws, n_ws, N=0) == BADARG              # unlike the forward (parrot_hip.h)
    torch.cuda.synchronize()
    assert dtbl.untouched() and ws.untouched()
    assert _bwd_call(c, dyf, perm, offs, dtbl, ws, n_ws) == 0
    torch.cuda.synchronize()
    assert torch.equal(dtbl.view.cpu(), TC.segmented_sum_reference(d["idx"], d["dy"], c.Q).float())


# ---- softmax cross-entropy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TC.CE))
def test_softmax_ce_per_row(dev, name):
    c = TC.CE[name]
    d = TC.ce_data(c)
    x, rs = d["x"], d["rowscale"]
    xf, _ = _matrix(dev, c.rows, c.Q, c.ld, x)
    tgt = d["target"].to(torch.int32).to(dev)
    rsf, lse, ce = _vector(dev, c.rows, rs), _vector(dev, c.rows), _vector(dev, c.rows)
    dlf, dl = _matrix(dev, c.rows, c.Q, c.ldd)
    for f in (xf, rsf, lse, ce, dlf):
        f.snapshot()
    L = _lib()
    assert L.parrot_softmax_ce_fwd(_ptr(xf), c.ld, tgt.data_ptr(), c.rows, c.Q, _ptr(lse), _ptr(ce), _stream()) == 0
    torch.cuda.synchronize()
    assert dlf.untouched()
    lse.snapshot()
    assert L.parrot_softmax_ce_bwd(_ptr(xf), c.ld, tgt.data_ptr(), _ptr(lse), _ptr(rsf), c.rows, c.Q, _ptr(dlf), c.ldd,
                                   _stream()) == 0
    torch.cuda.synchronize()
    assert xf.untouched() and rsf.untouched() and lse.untouched(), "an operand was written"
    assert lse.frame_untouched() and ce.frame_untouched() and _intact(dlf, c.Q), "written outside an output"
    ref = TC.ce_reference(x, d["target"], rs)
    rowb = TC.ce_bound(c, ref)
    _ratio(name, "lse", lse.view, ref["lse"], rowb)
    _ratio(name, "ce", ce.view, ref["ce"], rowb)
    got = dl.cpu()
    _ratio(name, "dlogits", got, ref["dlogits"], TC.dlogits_bound(c, x, rs, ref))
    assert bool((got[torch.isinf(x)] == 0.0).all()), "a class at -inf has a gradient"
    assert bool((got[rs == 0] == 0.0).all()), "a row with rowscale 0 has a gradient"


def test_softmax_ce_arguments(dev):
    rows, Q = 3, 5
    xf, _ = _matrix(dev, rows, Q, Q + 3, torch.zeros(rows, Q))
    tgt = torch.zeros(rows, dtype=torch.int32, device=dev)
    rs, lse, ce = _vector(dev, rows, torch.ones(rows)), _vector(dev, rows), _vector(dev, rows)
    dlf, _ = _matrix(dev, rows, Q, Q + 5)
    for f in (lse, ce, dlf):
        f.snapshot()
    L, s = _lib(), _stream()
    fwd = lambda rows_, Q_, ld: L.parrot_softmax_ce_fwd(_ptr(xf), ld, tgt.data_ptr(), rows_, Q_, _ptr(lse), _ptr(ce), s)
    bwd = lambda rows_, Q_, ld, ldd: L.parrot_softmax_ce_bwd(_ptr(xf), ld, tgt.data_ptr(), _ptr(ce), _ptr(rs), rows_, Q_,
                                                              _ptr(dlf), ldd, s)
    assert fwd(0, Q, Q + 3) == 0 and bwd(0, Q, Q + 3, Q + 5) == 0                   # no rows: nothing to do
    assert fwd(rows, Q, Q - 1) == BADARG and fwd(rows, 0, Q + 3) == BADARG
    assert bwd(rows, Q, Q - 1, Q + 5) == BADARG and bwd(rows, Q, Q + 3, Q - 1) == BADARG and bwd(rows, 0, Q + 3, Q + 5) == BADARG
    torch.cuda.synchronize()
    assert lse.untouched() and ce.untouched() and dlf.untouched()


# ---- ReLU gate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TC.RELU_N)
def test_relu_gate_is_a_select(dev, n):
    """Bit equality with where(gate > 0, dy, +0.0): the smallest denormal opens the gate, -0.0 and NaN do not, and a closed
    gate gives +0.0 whatever dy holds (NaN, inf)."""
    dy, gate = TC.relu_data(n)
    want = torch.from_numpy(TC.relu_reference(dy, gate))
    dyf, gf, out = _vector(dev, n, torch.from_numpy(dy)), _vector(dev, n, torch.from_numpy(gate)), _vector(dev, n)
    assert torch.equal(_bits(gf.view).cpu(), _bits(torch.from_numpy(gate))), "the copy changed the gate's bits"
    for f in (dyf, gf, out):
        f.snapshot()
    assert _lib().parrot_relu_gate(_ptr(dyf), _ptr(gf), _ptr(out), n, _stream()) == 0
    torch.cuda.synchronize()
    got = out.view.cpu()
    diff = _bits(got) != _bits(want)
    assert not bool(diff.any()), "differs at %s: gate %s" % (torch.nonzero(diff)[:8, 0].tolist(), gate[diff.numpy()][:8])
    assert out.frame_untouched() and dyf.untouched() and gf.untouched()


def test_relu_gate_arguments(dev):
    a = _vector(dev, 8, torch.ones(8))
    out = _vector(dev, 8)
    out.snapshot()
    assert _lib().parrot_relu_gate(_ptr(a), _ptr(a), _ptr(out), 6, _stream()) == BADARG
    assert _lib().parrot_relu_gate(_ptr(a), _ptr(a), _ptr(out), -4, _stream()) == BADARG
    torch.cuda.synchronize()
    assert out.untouched()


# ---- weight-norm fold ---------------------------------------------------------------------------------------------------
class _Fold:
    """The buffers of one weight-norm case, framed, and the two calls."""

    def __init__(self, dev, c):
        self.c, self.d = c, TC.wn_data(c)
        d = self.d
        self.ref = TC.wn_reference(d["W"], d["g"], d["dWe"])
        self.Wf, _ = _matrix(dev, c.K, c.N, c.ld, d["W"])
        self.dWef, _ = _matrix(dev, c.K, c.N, c.ldd, d["dWe"])
        self.g = _vector(dev, c.N, d["g"])
        self.outf, self.out = _matrix(dev, c.K, c.N, c.ldo)
        self.dWf, self.dW = _matrix(dev, c.K, c.N, c.lddw)
        self.norm, self.dg = _vector(dev, c.N), _vector(dev, c.N)
        n_ws = int(_lib().samplernn_weightnorm_ws_floats(c.N))
        assert n_ws == TC.WN_KS * c.N
        self.ws = _vector(dev, n_ws)
        for f in (self.Wf, self.dWef, self.g):
            f.snapshot()

    def forward(self, with_norm=True):
        c = self.c
        self.out.fill_(NAN)
        self.ws.view.fill_(NAN)
        if with_norm:
            self.norm.view.fill_(NAN)
        for f in (self.outf, self.norm, self.ws):
            f.snapshot()
        rc = _lib().samplernn_weightnorm_fold(_ptr(self.Wf), c.ld, _ptr(self.g), _ptr(self.outf), c.ldo,
                                              _ptr(self.norm) if with_norm else None, _ptr(self.ws), c.K, c.N, _stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert _intact(self.outf, c.N) and self.norm.frame_untouched() and self.ws.frame_untouched(), "written outside an output"
        assert self.Wf.untouched() and self.g.untouched()
        return self.out.cpu(), self.norm.view.cpu()

    def backward(self, acc_w=0, acc_g=0):
        c, d = self.c, self.d
        self.ws.view.fill_(NAN)
        if acc_w:
            self.dW.copy_(d["old_dW"])
        else:
            self.dW.fill_(NAN)
        if acc_g:
            self.dg.view.copy_(d["old_dg"])
        else:
            self.dg.view.fill_(NAN)
        for f in (self.dWf, self.dg, self.ws, self.norm):
            f.snapshot()
        rc = _lib().samplernn_weightnorm_fold_bwd(_ptr(self.Wf), c.ld, _ptr(self.g), _ptr(self.norm), _ptr(self.dWef), c.ldd,
                                                  _ptr(self.dWf), c.lddw, _ptr(self.dg), _ptr(self.ws), c.K, c.N, acc_w, acc_g,
                                                  _stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert _intact(self.dWf, c.N) and self.dg.frame_untouched() and self.ws.frame_untouched(), "written outside an output"
        assert self.Wf.untouched() and self.g.untouched() and self.dWef.untouched() and self.norm.untouched()
        return self.dW.cpu(), self.dg.view.cpu()

    def check_backward(self, what, dW, dg, acc_w=0, acc_g=0):
        c, d, ref = self.c, self.d, self.ref
        old_dW, old_dg = (d["old_dW"] if acc_w else None), (d["old_dg"] if acc_g else None)
        b = TC.wn_bounds(c, d["W"], d["g"], d["dWe"], ref, old_dW, old_dg)
        _ratio(what, "dg", dg, ref["dg"] + (old_dg.double() if acc_g else 0.0), b["dg"])
        _ratio(what, "dW", dW, ref["dW"] + (old_dW.double() if acc_w else 0.0), b["dW"])


@pytest.mark.parametrize("name", sorted(TC.WN))
def test_weightnorm_fold_per_column(dev, name):
    c = TC.WN[name]
    fold = _Fold(dev, c)
    d, ref = fold.d, fold.ref
    b = TC.wn_bounds(c, d["W"], d["g"], d["dWe"], ref)
    out, norm = fold.forward()
    _ratio(name, "norm", norm, ref["norm"], b["norm"])
    _ratio(name, "W_eff", out, ref["W_eff"], b["W_eff"])
    if c.kind == "int":  # an exact sum of squares with an exact root
        sq = TC.wn_is_square_column(c.N)
        assert torch.equal(norm[sq], ref["norm"][sq].float()), "the norm of a perfect-square column is not exact"
    dW, dg = fold.backward()
    fold.check_backward(name, dW, dg)
    out2, norm2 = fold.forward()
    dW2, dg2 = fold.backward()
    for a, a2, what in ((out, out2, "W_eff"), (norm, norm2, "norm"), (dW, dW2, "dW"), (dg, dg2, "dg")):
        assert torch.equal(a, a2), "the second call gives another " + what
    out3, _ = fold.forward(with_norm=False)     # norm == NULL: the same W_eff, the norm buffer left alone
    assert torch.equal(out3, out) and fold.norm.untouched()


@pytest.mark.parametrize("acc_w,acc_g", [(0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("name", TC.WN_ACC_CASES)
def test_weightnorm_fold_bwd_accumulates(dev, name, acc_w, acc_g):
    fold = _Fold(dev, TC.WN[name])
    fold.forward()
    dW, dg = fold.backward(acc_w, acc_g)
    fold.check_backward("%s-accw%d-accg%d" % (name, acc_w, acc_g), dW, dg, acc_w, acc_g)
    dW0, dg0 = fold.backward(0, 0)
    if not acc_w:
        assert torch.equal(dW, dW0), "accumulate_g changed dW"
    if not acc_g:
        assert torch.equal(dg, dg0), "accumulate_w changed dg"


def test_weightnorm_fold_arguments(dev):
    c = TC.WN["wn-K-K5-N65"]
    fold = _Fold(dev, c)
    for f in (fold.outf, fold.norm, fold.dWf, fold.dg):
        f.snapshot()
    L, s = _lib(), _stream()
    fwd = lambda ld, ldo: L.samplernn_weightnorm_fold(_ptr(fold.Wf), ld, _ptr(fold.g), _ptr(fold.outf), ldo, _ptr(fold.norm),
                                                      _ptr(fold.ws), c.K, c.N, s)
    bwd = lambda ld, ldd, lddw: L.samplernn_weightnorm_fold_bwd(_ptr(fold.Wf), ld, _ptr(fold.g), _ptr(fold.g), _ptr(fold.dWef), ldd,
                                                                 _ptr(fold.dWf), lddw, _ptr(fold.dg), _ptr(fold.ws), c.K, c.N, 0, 0, s)
    assert fwd(c.N - 1, c.ldo) == BADARG and fwd(c.ld, c.N - 1) == BADARG
    assert bwd(c.N - 1, c.ldd, c.lddw) == BADARG and bwd(c.ld, c.N - 1, c.lddw) == BADARG and bwd(c.ld, c.ldd, c.N - 1) == BADARG
    torch.cuda.synchronize()
    assert fold.outf.untouched() and fold.norm.untouched() and fold.dWf.untouched() and fold.dg.untouched()


# ---- quantisers ---------------------------------------------------------------------------------------------------------
def _oracle_classes(x, q_type):
    from oracle import quantize_ref as Q
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")     # a constant row is 0 / 0 in the reference
        return Q.batch_quantize(x.copy(), 256, q_type)


_CLASSES = {}


def _quantize(dev, c, mode):
    """The case through parrot_batch_quantize, once per session: (classes [rows, n] numpy, reference classes)."""
    if (c.id, mode) in _CLASSES:
        return _CLASSES[c.id, mode]
    x = TC.quant_data(c)
    xf, _ = _matrix(dev, c.rows, c.n, c.ld, torch.from_numpy(x))
    npad = c.ld - c.n
    xf.view[:, c.n:] = torch.tensor([1e30, -1e30] * npad)[:npad].to(dev)
    xf.snapshot()
    dtype = torch.int32 if mode else torch.int16
    per = 4 // dtype.itemsize                                  # classes per float of the frame
    of = Framed((-(-c.rows * c.ldo // per),), dev)
    words = of.big.view(dtype)
    region = words[of.lo * per:of.lo * per + c.rows * c.ldo].view(c.rows, c.ldo)
    assert region.data_ptr() == _ptr(of)
    before = words.clone()
    ws = torch.empty(2 * c.rows, device=dev, dtype=torch.float64)
    rc = _lib().parrot_batch_quantize(_ptr(xf), c.rows, c.n, c.ld, ws.data_ptr(), region.data_ptr(), c.ldo, mode, 256, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = region[:, :c.n].cpu().numpy().copy()
    region[:, :c.n] = 0
    before[of.lo * per:of.lo * per + c.rows * c.ldo].view(c.rows, c.ldo)[:, :c.n] = 0
    assert torch.equal(words, before), "written outside the classes: the frame or the padding of a row"
    assert xf.untouched()
    _CLASSES[c.id, mode] = (got, _oracle_classes(x, "linear" if mode else "mu-law"))
    return _CLASSES[c.id, mode]


@pytest.mark.parametrize("mode", [0, 1], ids=["mu-law", "linear"])
@pytest.mark.parametrize("name", sorted(TC.QUANT))
def test_quantize_padded_rows_exact(dev, name, mode):
    c = TC.QUANT[name]
    got, want = _quantize(dev, c, mode)
    assert got.dtype == want.dtype == (np.int32 if mode else np.int16)
    keep = [r for r in range(c.rows) if r not in TC.quant_constant_rows(c)]
    assert 0 <= got[keep].min() and got[keep].max() <= 255, "an element was not written"
    assert np.array_equal(got[keep], want[keep]), "%d classes differ, first at %s" % (
        (got[keep] != want[keep]).sum(), np.argwhere(got[keep] != want[keep])[:4].tolist())
    if c.group in TC.QUANT_CLAMP_GROUPS:
        assert (got[:, -1] == 0).all() and (got[:, -2] == 255).all()


@pytest.mark.parametrize("n", [1, 257, None], ids=["one", "a-block-and-one", "past-the-clamp"])
def test_mu2linear_framed(dev, n):
    from oracle import quantize_ref as Q
    if n is None:
        c = TC.QUANT[[k for k, v in TC.QUANT.items() if v.group == "q-clamp-mu2linear"][0]]
        q = _quantize(dev, c, 0)[0].reshape(-1).astype(np.int32)
        assert q.size > TC.MU2LIN_CLAMP
    else:
        q = (np.arange(n, dtype=np.int32) * 7) % 256
    qd = torch.from_numpy(q).to(dev)
    out = _vector(dev, q.size)
    out.snapshot()
    assert _lib().parrot_mu2linear(qd.data_ptr(), q.size, _ptr(out), _stream()) == 0
    torch.cuda.synchronize()
    assert out.frame_untouched() and torch.equal(qd.cpu(), torch.from_numpy(q))
    np.testing.assert_allclose(out.view.cpu().numpy(), Q.mu2linear(q), rtol=2e-6, atol=1e-8)


# ---- the Python wrappers: strides that reach the kernels ----------------------------------------------------------------
def _embed_operands(N, J, Q, EMB, D, seed):
    g = torch.Generator().manual_seed(seed)
    E = torch.randn(Q, EMB, generator=g, dtype=torch.float64)
    W1 = torch.randn(J * EMB, D, generator=g, dtype=torch.float64) / (J * EMB) ** 0.5
    wide = torch.randn(N, D + 8, generator=g, dtype=torch.float64)
    idx = torch.randint(0, Q, (N, J), generator=g)
    return E, W1, wide, idx, torch.randn(N, D, generator=g, dtype=torch.float64)


def test_embed_sum_with_a_column_slice_as_add(dev):
    """`add` = columns 4..4+D of a wider matrix reaches gs_fwd_kernel with ldadd > D."""
    from parrot_amd import ops
    N, J, Q, EMB, D = 77, 5, 16, 4, 36
    E, W1, wide, idx, dy = _embed_operands(N, J, Q, EMB, D, 11)
    r = [t.clone().requires_grad_() for t in (E, W1, wide)]
    ref = r[0][idx.reshape(-1)].reshape(N, J * EMB) @ r[1] + r[2][:, 4:4 + D]
    ref.backward(dy)
    h = [t.float().to(dev).requires_grad_() for t in (E, W1, wide)]
    add = h[2][:, 4:4 + D]
    assert add.stride(0) == D + 8 and add.data_ptr() % 16 == 0
    y = ops.embed_sum(h[0], h[1], idx.to(dev), add)
    y.backward(dy.float().to(dev))
    assert_close(y, ref, 2e-6, "embed_sum with a strided add")
    for got, want, n in zip(h, r, ("dE", "dW1", "d wide")):
        assert_close(got.grad, want.grad, 2e-5, n)
    assert float(h[2].grad[:, :4].abs().max()) == 0.0 and float(h[2].grad[:, 4 + D:].abs().max()) == 0.0


def test_softmax_ce_on_a_column_slice_and_on_3d_logits(dev):
    """A column slice reaches ce_fwd_kernel / ce_bwd_kernel with ld > Q; [B, T, Q] logits come back with a [B, T, Q] gradient."""
    from parrot_amd import ops
    g = torch.Generator().manual_seed(12)
    B, T, Q = 3, 7, 65
    for shape, sl in (((B * T, Q + 8), (slice(None), slice(4, 4 + Q))), ((B, T, Q), (slice(None), slice(None), slice(None)))):
        wide = torch.randn(*shape, generator=g, dtype=torch.float64) * 4
        t = torch.randint(0, Q, shape[:-1], generator=g)
        w = torch.rand(*shape[:-1], generator=g, dtype=torch.float64)
        wr = wide.clone().requires_grad_()
        xr = wr[sl]
        ref = torch.logsumexp(xr, -1) - xr.gather(-1, t[..., None])[..., 0]
        (ref * w).sum().backward()
        wh = wide.float().to(dev).requires_grad_()
        xh = wh[sl]
        ce = ops.softmax_ce(xh, t.to(dev))
        (ce.reshape(shape[:-1]) * w.float().to(dev)).sum().backward()
        assert_close(ce.reshape(shape[:-1]), ref, 2e-6, "cross-entropy %s" % (shape,))
        assert wh.grad.shape == wide.shape
        assert_close(wh.grad, wr.grad, 1e-5, "d logits %s" % (shape,))


def test_weightnorm_fold_of_a_column_slice_through_the_backward(dev):
    """A column-sliced W reaches wn_colsum_kernel<true> and wn_scale_bwd_kernel with ld > N."""
    from parrot_amd import ops
    g0 = torch.Generator().manual_seed(13)
    K, N = 70, 65
    wide = torch.randn(K, N + 40, generator=g0, dtype=torch.float64) * 0.3
    gg = torch.rand(N, generator=g0, dtype=torch.float64) + 0.5
    d = torch.randn(K, N, generator=g0, dtype=torch.float64)
    wr, gr = wide.clone().requires_grad_(), gg.clone().requires_grad_()
    Wr = wr[:, 8:8 + N]
    ref = Wr * (gr / Wr.norm(2, dim=0))
    ref.backward(d)
    wh, gh = wide.float().to(dev).requires_grad_(), gg.float().to(dev).requires_grad_()
    Wh = wh[:, 8:8 + N]
    assert Wh.stride(0) == N + 40
    out = ops.weightnorm_fold(Wh, gh)
    out.backward(d.float().to(dev))
    assert_close(out, ref, 2e-6, "W_eff of a strided W")
    assert_close(wh.grad, wr.grad, 1e-5, "dW of a strided W")
    assert_close(gh.grad, gr.grad, 1e-5, "dg of a strided W")


def test_sum_backward_through_all_four_functions(dev):
    """.sum().backward() hands every autograd function a gradient of stride 0."""
    from parrot_amd import ops
    N, J, Q, EMB, D = 77, 5, 16, 4, 36
    E, W1, wide, idx, _ = _embed_operands(N, J, Q, EMB, D, 14)
    add = wide[:, :D].contiguous()
    r = [t.clone().requires_grad_() for t in (E, W1, add)]
    (r[0][idx.reshape(-1)].reshape(N, J * EMB) @ r[1] + r[2]).sum().backward()
    h = [t.float().to(dev).requires_grad_() for t in (E, W1, add)]
    ops.embed_sum(h[0], h[1], idx.to(dev), h[2]).sum().backward()
    for got, want, n in zip(h, r, ("dE", "dW1", "dadd")):
        assert_close(got.grad, want.grad, 2e-5, "embed_sum: " + n)

    g = torch.Generator().manual_seed(15)
    M, Dm, Qm = 70, 32, 17
    shapes = [(M, Dm), (Dm, Dm), (Dm,), (Dm, Dm), (Dm,), (Dm, Qm), (Qm,)]
    vals = [torch.randn(*s, generator=g, dtype=torch.float64) / (Dm ** 0.5 if len(s) == 2 and s[0] == Dm else 1.0) for s in shapes]
    r = [v.clone().requires_grad_() for v in vals]
    (torch.relu(torch.relu(r[0] @ r[1] + r[2]) @ r[3] + r[4]) @ r[5] + r[6]).sum().backward()
    h = [v.float().to(dev).requires_grad_() for v in vals]
    ops.relu_mlp(*h).sum().backward()
    for got, want, n in zip(h, r, ("dx", "dW2", "db2", "dW3", "db3", "dW4", "db4")):
        assert_close(got.grad, want.grad, 1e-4, "relu_mlp: " + n)

    x = torch.randn(37, 10, generator=g, dtype=torch.float64) * 4
    t = torch.randint(0, 10, (37,), generator=g)
    xr = x.clone().requires_grad_()
    (torch.logsumexp(xr, -1) - xr.gather(1, t[:, None])[:, 0]).sum().backward()
    xh = x.float().to(dev).requires_grad_()
    ops.softmax_ce(xh, t.to(dev)).sum().backward()
    assert_close(xh.grad, xr.grad, 1e-5, "softmax_ce: d logits")

    W = torch.randn(70, 65, generator=g, dtype=torch.float64) * 0.3
    gg = torch.rand(65, generator=g, dtype=torch.float64) + 0.5
    Wr, gr = W.clone().requires_grad_(), gg.clone().requires_grad_()
    (Wr * (gr / Wr.norm(2, dim=0))).sum().backward()
    Wh, gh = W.float().to(dev).requires_grad_(), gg.float().to(dev).requires_grad_()
    ops.weightnorm_fold(Wh, gh).sum().backward()
    assert_close(Wh.grad, Wr.grad, 1e-5, "weightnorm_fold: dW")
    assert_close(gh.grad, gr.grad, 1e-5, "weightnorm_fold: dg")
