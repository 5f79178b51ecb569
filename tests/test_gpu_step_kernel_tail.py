"""The tail of a step-kernel launch (sk_body, from the K loop's exit to the last store): the descriptor fields the epilogue
reads -- epi, act, accumulate, H, colmode, bias, out, o1, o2, mask, the three leading dimensions, N, M -- travel with the
batch at the kernel's entry and stay in scalar registers over the K loop.  One `parrot_step_job` launch per case against the
float64 product (helpers and tolerances of tests/test_gpu_step_kernel_waves.py: TOL_STEP, TOL_STEP_ACT behind tanh / sigmoid),
M = 33 and N = 48 in framed buffers:

  * K totals around a wave's walk of one ring group (eight waves, ring depth 2): 16 and 48 (waves with no chunk at all), 128
    (one chunk each), 144, 256 (exactly one group each), 272 and 384 (a group and a remainder), at tiles 11, 21 and 22;
  * every field the epilogue reads at a non-default value, one at a time: the activations, accumulate, no bias, an additive
    input, a wide leading dimension; gates, candidates with and without c_out, d(r o h), the LSTM cell with and without
    saved gates;
  * the step mask through `parrot_gru_step_fwd` (the candidate launch against the float64 product of the r o h the gate launch
    left), `colmode` through the LSTM schedule-5 window of tests/decoder_scan_cases.py (its tolerances);
  * the same case launched twice into fresh buffers gives the same bits (the K deal and the order of every sum are fixed)."""
import pytest
import torch

from tests import decoder_scan_cases as D
from tests.gemm_cases import NONE, RELU, SIGMOID, TANH, TOL_STEP, TOL_STEP_ACT
from tests.test_gpu_step_kernel_waves import BWD_RH, CAND, FILL, GATES, LINEAR, LSTM, TILED, _gen, _launch, _linear, _operands
from tests.util import assert_close

pytestmark = pytest.mark.gpu

M, N = 33, 48
KS = [16, 48, 128, 144, 256, 272, 384]
ACT64 = {NONE: lambda x: x, RELU: lambda x: x.clamp(min=0), TANH: torch.tanh, SIGMOID: torch.sigmoid}


@pytest.mark.parametrize("tile", [11, 21, 22])
@pytest.mark.parametrize("K", KS)
def test_k_totals_around_one_ring_group(dev, K, tile):
    _linear(dev, M, N, [K], TILED, tile=tile)


def _framed(dev, rows, cols, pad=0, fill=FILL):
    """(buffer, view): `rows` x `cols` inside a frame row on either side and `pad` more columns."""
    buf = torch.full((rows + 2, cols + pad), fill, device=dev)
    return buf, buf[1:rows + 1, :cols]


def _frame_untouched(buf, rows, cols, what):
    got = buf.cpu().clone()
    got[1:rows + 1, :cols] = FILL
    assert bool((got == FILL).all()), what + ": wrote outside its rows / columns"


def _rand(key, *shape):
    return torch.randn(*shape, generator=_gen("tail", key, shape), dtype=torch.float64).float()


def _run_linear(dev, K, tile, act=NONE, accumulate=False, with_bias=True, with_add=False, pad=3):
    a, w, bias, acc = _operands(M, N, [K])
    prev, add = _rand("prev", M, N), _rand("add", M, N)
    buf, view = _framed(dev, M, N, pad)
    if accumulate:
        view.copy_(prev.to(dev))
    addbuf = torch.full((M, N + 5), float("nan"), device=dev)   # the additive input has a leading dimension of its own
    addbuf[:, :N] = add.to(dev)
    _launch(dev, LINEAR, M, N, N, a, w, TILED, tile=tile, act=act, accumulate=accumulate, bias=bias.to(dev) if with_bias else None,
            add=addbuf[:, :N] if with_add else None, out=view, ldo=N + pad)
    want = ACT64[act](acc + (bias.double() if with_bias else 0) + (add.double() if with_add else 0))
    if accumulate:
        want = want + prev.double()
    return buf, view, want


LINEAR_FIELDS = [dict(), dict(act=RELU), dict(act=TANH), dict(act=SIGMOID), dict(accumulate=True), dict(with_bias=False),
                 dict(with_add=True), dict(pad=0), dict(act=TANH, accumulate=True, with_add=True)]


@pytest.mark.parametrize("K", [128, 272])
@pytest.mark.parametrize("fields", LINEAR_FIELDS, ids=lambda f: "-".join("%s=%s" % kv for kv in sorted(f.items())) or "default")
def test_linear_fields_one_at_a_time(dev, fields, K):
    buf, view, want = _run_linear(dev, K, 22, **fields)
    what = "linear K=%d %s" % (K, fields)
    e = assert_close(view, want, TOL_STEP_ACT if fields.get("act") in (TANH, SIGMOID) else TOL_STEP, what)
    print("%s: rel err %.3e" % (what, e))
    _frame_untouched(buf, M, N, what)


@pytest.mark.parametrize("tile", [11, 22])
@pytest.mark.parametrize("K", [128, 272])
def test_gru_gates(dev, K, tile):
    H = N // 2
    a, w, bias, acc = _operands(M, N, [K])
    hp, add = _rand("hp", M, H), _rand("gadd", M, N)
    (zb, z), (rb, r), (rhb, rh) = (_framed(dev, M, H) for _ in range(3))
    _launch(dev, GATES, M, N, H, a, w, TILED, tile=tile, bias=bias.to(dev), add=add.to(dev), out=rh, e0=hp.to(dev), o1=z, o2=r)
    gate = torch.sigmoid(acc + bias.double() + add.double())
    assert_close(z, gate[:, :H], TOL_STEP_ACT, "z")
    assert_close(r, gate[:, H:], TOL_STEP_ACT, "r")
    assert_close(rh, gate[:, H:] * hp.double(), TOL_STEP_ACT, "r * h_prev")
    for b, what in ((zb, "z"), (rb, "r"), (rhb, "r * h_prev")):
        _frame_untouched(b, M, H, what)


@pytest.mark.parametrize("c_out", [True, False])
@pytest.mark.parametrize("K", [128, 272])
def test_gru_candidate(dev, K, c_out):
    H = N
    a, w, bias, acc = _operands(M, H, [K])
    hp, z = _rand("hp", M, H), torch.sigmoid(_rand("z", M, H))
    (cb, c), (hb, hn) = (_framed(dev, M, H) for _ in range(2))
    _launch(dev, CAND, M, H, H, a, w, TILED, tile=22, bias=bias.to(dev), out=hn, e0=hp.to(dev), e1=z.to(dev),
            o1=c if c_out else None)
    cand = torch.tanh(acc + bias.double())
    if c_out:
        assert_close(c, cand, TOL_STEP_ACT, "c")
    assert_close(hn, z.double() * cand + (1 - z.double()) * hp.double(), TOL_STEP_ACT, "h_next")
    _frame_untouched(hb, M, H, "h_next")
    _frame_untouched(cb, M, H if c_out else 0, "c" if c_out else "c (not asked for)")


@pytest.mark.parametrize("K", [128, 272])
def test_backward_rh(dev, K):
    H = N
    a, w, _, acc = _operands(M, H, [K])
    hp, rg, dh0 = _rand("hp", M, H), torch.sigmoid(_rand("r", M, H)), _rand("dh0", M, H)
    gb, _ = _framed(dev, M, 2 * H)                  # the r half of a [M, 2H] buffer
    dG = gb[1:M + 1, H:]
    dhb, dh = _framed(dev, M, H)
    dh.copy_(dh0.to(dev))
    _launch(dev, BWD_RH, M, H, H, a, w, TILED, tile=22, out=dG, ldo=2 * H, e0=hp.to(dev), e1=rg.to(dev), o1=dh)
    assert_close(dG, acc * hp.double() * rg.double() * (1 - rg.double()), TOL_STEP, "dG_r")
    assert_close(dh, dh0.double() + acc * rg.double(), TOL_STEP, "dh_prev")
    got = gb.cpu().clone()
    got[1:M + 1, H:] = FILL
    assert bool((got == FILL).all()), "dG: wrote outside the r half"
    _frame_untouched(dhb, M, H, "dh_prev")


@pytest.mark.parametrize("saved", [True, False])
@pytest.mark.parametrize("K", [128, 272])
def test_lstm_cell(dev, K, saved):
    H = N // 4
    a, w, bias, acc = _operands(M, N, [K])
    cp = _rand("cp", M, H)
    (cnb, cn), (sb, s) = (_framed(dev, M, H) for _ in range(2))
    gb, gates = _framed(dev, M, N)
    _launch(dev, LSTM, M, N, H, a, w, TILED, tile=22, bias=bias.to(dev), out=s, e1=cp.to(dev), o1=cn, o2=gates if saved else None)
    pre = acc + bias.double()
    act = torch.cat([torch.sigmoid(pre[:, :3 * H]), torch.tanh(pre[:, 3 * H:])], 1)   # i | f | o | g
    i, f, o, gg = act.split(H, 1)
    cell = cp.double() * f + gg * i
    if saved:
        assert_close(gates, act, TOL_STEP_ACT, "gate activations")
    assert_close(cn, cell, TOL_STEP_ACT, "c_next")
    assert_close(s, torch.tanh(cell) * o, TOL_STEP_ACT, "s_next")
    _frame_untouched(cnb, M, H, "c_next")
    _frame_untouched(sb, M, H, "s_next")
    _frame_untouched(gb, M, N if saved else 0, "gate activations")


def test_step_mask(dev):
    """`parrot_gru_step_fwd` with a mask: its candidate launch is one step-kernel launch over r o h, held to the float64 product of
    the r o h and z that its gate launch wrote."""
    from parrot_amd import ops
    H = N
    h, x, gx = _rand("mh", M, H), _rand("mx", M, H), _rand("mgx", M, 2 * H)
    Wg, Wc = _rand("mWg", H, 2 * H) / H ** 0.5, _rand("mWc", H, H) / H ** 0.5
    mask = (torch.arange(M) % 3 != 1).float()              # rows that keep their state among rows that move
    mask[0] = 0.25                                         # ... and one blend
    dv = [t.to(dev) for t in (h, x, gx, Wg, Wc)]
    out, (z, r, rh, c) = ops.gru_step_fwd(*dv, mask.to(dev))
    torch.cuda.synchronize()
    gate = torch.sigmoid(h.double() @ Wg.double() + gx.double())
    assert_close(z, gate[:, :H], TOL_STEP_ACT, "z")
    assert_close(rh, gate[:, H:] * h.double(), TOL_STEP_ACT, "r * h_prev")
    cand = torch.tanh(rh.double().cpu() @ Wc.double() + x.double())
    zz, mk = z.double().cpu(), mask.double()[:, None]
    hn = zz * cand + (1 - zz) * h.double()
    assert_close(c, cand, TOL_STEP_ACT, "c")
    assert_close(out, mk * hn + (1 - mk) * h.double(), TOL_STEP_ACT, "h_next under the mask")
    assert torch.equal(out.cpu()[1::3], h[1::3]), "a row the mask holds moved"


def test_colmode_through_the_lstm_schedule_5_window(dev):
    from tests.test_gpu_decoder_scan_edges import _against_reference, _assert_route, _result
    case = D.CASES["paths-s5-lstm-L2-T5-B17-H32-E16-U7"]
    res = _result(dev, case)
    _assert_route(case, res)
    _against_reference(case, res["windows"][0], 0, case.id)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


@pytest.mark.parametrize("tile", [11, 21, 22])
@pytest.mark.parametrize("K", [48, 272, 1280])
def test_same_bits_from_run_to_run(dev, K, tile):
    first = None
    for _ in range(3):
        buf, view, _ = _run_linear(dev, K, tile, act=TANH, with_add=True)
        if first is None:
            first = _bits(buf)
        else:
            assert torch.equal(first, _bits(buf)), "K=%d tile=%d: two launches of one case differ" % (K, tile)
    H = N // 2
    a, w, bias, _ = _operands(M, N, [K])
    hp = _rand("hp", M, H)
    runs = []
    for _ in range(2):
        z, r, rh = (torch.full((M, H), float("nan"), device=dev) for _ in range(3))
        _launch(dev, GATES, M, N, H, a, w, TILED, tile=tile, bias=bias.to(dev), out=rh, e0=hp.to(dev), o1=z, o2=r)
        runs.append(torch.cat([_bits(z), _bits(r), _bits(rh)]))
    assert torch.equal(runs[0], runs[1]), "K=%d tile=%d: two gate launches of one case differ" % (K, tile)
