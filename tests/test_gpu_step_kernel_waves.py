"""The step kernel's K walk (sk_body: chunks of 16 K rows dealt round-robin to the SK_KW waves of a workgroup, a register
ring of depth 2 whose refills are pinned behind the MFMAs they follow): one launch per case through `parrot_step_job`,
against the float64 product, at the K totals around the deal -- of the shipped build (8 waves) and of the 16-wave build
the constant allows.

  K total          chunks         at 8 waves                          at 16 waves
  16, 48           1, 3           waves with no chunk at all          the same
  256, 272         16, 17         two each; one wave has three        one each (the prologue clamps); one has two
  496 / 512 / 528  31 / 32 / 33   around four each                    around two each
  768              48             six each                            three each: a remainder behind the last group
  1280             80             the headline workload's ten         five per wave

plus segment boundaries inside a wave's walk, the generic path (K = 63: unaligned rows), the bf16 ring (chunks of 32), every
row count around the 16-row blocks, the tile shapes a plan can ask for, every fused epilogue, and the step-GEMM jobs inside
the heterogeneous launches (ska_kernel / skb_kernel) of one small GRU training window.  (What the attention blocks of those
launches write is held bit for bit to a recorded build by tests/test_gpu_step_launch_modes.py.)

Tolerances: those of the step-kernel cases of tests/gemm_cases.py section 5 (TOL_STEP; TOL_STEP_ACT behind tanh / sigmoid;
TOL_BF16 against the product of the operands rounded to bf16); the window's buffers follow the rule of
tests/decoder_scan_cases.py (the scan tolerance, or 4 x the buffer's own float32 noise floor where that is larger), with
the floor computed here from the case's float32 reference."""
import ctypes as C
import math
import zlib

import pytest
import torch

from tests import decoder_scan_cases as D
from tests import step_launch_cases as S
from tests.gemm_cases import NONE, TANH, TOL_BF16, TOL_STEP, TOL_STEP_ACT
from tests.util import assert_close, rel_err, rel_err_elem

pytestmark = pytest.mark.gpu

LINEAR, GATES, CAND, BWD_RH, LSTM = 0, 1, 2, 3, 4   # SkEpi
PLAIN, KCONTIG, TILED, TILED_BF16 = 0, 1, 2, 3       # weight layouts of parrot_step_job
FILL = 7.25


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _weights(dev, W, layout, lstm_H=0):
    """(device buffer, ldb) of one segment's weights W [K, N] in the layout."""
    from parrot_amd import _lib, ops
    K, N = W.shape
    Wd = W.to(dev).contiguous()
    if layout == PLAIN:
        return Wd, N
    if layout == KCONTIG:
        return Wd.t().contiguous(), K
    if layout == TILED:
        out = torch.full((K * N,), float("nan"), device=dev)
        _lib.call("parrot_tile_weights", Wd.data_ptr(), K, N, N, out.data_ptr(), 0, lstm_H, ops._stream())
        return out, K // 16 * 256
    out = torch.full((K * N // 2,), float("nan"), device=dev)
    _lib.call("parrot_tile_weights_bf16", Wd.data_ptr(), K, N, N, out.data_ptr(), 0, lstm_H, ops._stream())
    return out, K // 32 * 256


def _launch(dev, epi, M, N, H, a, w, layout, tile=0, act=NONE, accumulate=False, bias=None, add=None, out=None, ldo=None,
            e0=None, e1=None, o1=None, o2=None, lda_pad=0):
    """One parrot_step_job launch; a / w: the segments' operands on the host."""
    from parrot_amd import _lib, ops
    n = len(a)
    keep = []
    A_, B_, lda, ldb = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_int * n)(), (C.c_int * n)()
    Ks = (C.c_int * n)(*[x.shape[1] for x in a])
    for s in range(n):
        K = a[s].shape[1]
        buf = torch.full((M, K + lda_pad), float("nan"), device=dev)
        buf[:, :K] = a[s].to(dev)
        wb, ldb[s] = _weights(dev, w[s], layout, H if epi == LSTM else 0)
        keep += [buf, wb]
        A_[s], B_[s], lda[s] = buf.data_ptr(), wb.data_ptr(), K + lda_pad
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.call("parrot_step_job", epi, M, N, H, n, A_, lda, B_, ldb, Ks, layout, act, int(accumulate), tile, ptr(bias),
              ptr(add), 0 if add is None else add.stride(0), ptr(out), ldo if ldo is not None else out.stride(0), ptr(e0),
              ptr(e1), ptr(o1), ptr(o2), ops._stream())
    torch.cuda.synchronize()
    return keep


def _operands(M, N, Ks, bf16=False):
    """Segments a_s [M, K_s] ~ N(0, 1 / K total), w_s [K_s, N] ~ N(0, 1), bias [N], and the float64 product."""
    g = _gen(M, N, tuple(Ks))
    tot = sum(Ks)
    a = [(torch.randn(M, K, generator=g, dtype=torch.float64) / math.sqrt(tot)).float() for K in Ks]
    w = [torch.randn(K, N, generator=g, dtype=torch.float64).float() for K in Ks]
    bias = torch.randn(N, generator=g, dtype=torch.float64).float()
    rnd = (lambda t: t.to(torch.bfloat16)) if bf16 else (lambda t: t)
    acc = sum(rnd(x).double() @ rnd(y).double() for x, y in zip(a, w))
    return a, w, bias, acc


def _linear(dev, M, N, Ks, layout, tile=0, lda_pad=0):
    bf16 = layout == TILED_BF16
    a, w, bias, acc = _operands(M, N, Ks, bf16)
    out = torch.full((M + 2, N + 3), FILL, device=dev)  # a frame row on either side, a wider leading dimension
    view = out[1:M + 1, :N]
    _launch(dev, LINEAR, M, N, N, a, w, layout, tile=tile, bias=bias.to(dev), out=view, ldo=N + 3, lda_pad=lda_pad)
    got = out.cpu()
    what = "M=%d N=%d K=%s layout=%d tile=%d" % (M, N, Ks, layout, tile)
    e = assert_close(got[1:M + 1, :N], acc + bias.double(), TOL_BF16 if bf16 else TOL_STEP, what)
    print("%s: rel err %.3e" % (what, e))
    got[1:M + 1, :N] = FILL
    assert bool((got == FILL).all()), what + ": wrote outside its [M, N]"


# ---- the deal: K totals around 8 / 16 waves x ring depth 2, at every tile shape a plan can force ---------------------------
@pytest.mark.parametrize("tile", [11, 21, 22])
@pytest.mark.parametrize("K", [16, 48, 256, 272, 496, 512, 528, 768, 1280])
def test_k_totals_around_the_deal(dev, K, tile):
    _linear(dev, 33, 48, [K], TILED, tile=tile)   # 33 rows: a ragged last block; 48 columns: a ragged 32-column workgroup


@pytest.mark.parametrize("layout", [PLAIN, KCONTIG])
@pytest.mark.parametrize("K", [16, 272, 528, 768])
def test_k_totals_plain_weight_layouts(dev, K, layout):
    _linear(dev, 17, 32, [K], layout, tile=22)


@pytest.mark.parametrize("layout", [PLAIN, TILED])
@pytest.mark.parametrize("M", [1, 17, 33, 64])
def test_row_counts_at_the_workload_depth(dev, M, layout):
    _linear(dev, M, 64, [1280], layout)


@pytest.mark.parametrize("layout", [PLAIN, TILED])
@pytest.mark.parametrize("Ks", [(32, 16), (256, 64, 16), (1024, 256)])
def test_segment_boundary_inside_a_waves_walk(dev, Ks, layout):
    _linear(dev, 17, 48, list(Ks), layout, tile=22)


@pytest.mark.parametrize("M,tile", [(5, 11), (33, 21), (48, 31)])
@pytest.mark.parametrize("Ks", [(63,), (272, 63)])
def test_generic_path(dev, Ks, M, tile):
    _linear(dev, M, 30, list(Ks), PLAIN, tile=tile)            # K = 63: rows of 63 floats are not 16-byte aligned


def test_generic_path_by_leading_dimension(dev):
    _linear(dev, 17, 32, [528], PLAIN, lda_pad=1)              # K % 16 == 0, lda % 4 != 0


@pytest.mark.parametrize("tile", [11, 22])
@pytest.mark.parametrize("Ks", [(512,), (544,), (1056,), (512, 32)])
def test_bf16_ring(dev, Ks, tile):
    _linear(dev, 33, 48, list(Ks), TILED_BF16, tile=tile)     # chunks of 32: 16, 17, 33 chunks; a boundary at chunk 16


def test_tiles_of_48_rows(dev):
    _linear(dev, 40, 64, [1280], TILED, tile=32)               # six blocks per workgroup: three waves run the epilogue
    _linear(dev, 40, 64, [272], TILED, tile=31)


# ---- every fused epilogue once, K = 272 + 32 (a segment boundary in wave 1's walk), 32 x 32 tiles --------------------------
EPI_M, EPI_H, EPI_KS = 17, 32, (272, 32)


def _epi_data(N):
    a, w, bias, acc = _operands(EPI_M, N, EPI_KS)
    g = _gen("epi", N)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()
    return a, w, bias, acc, r


def test_epilogue_linear_accumulate(dev):
    N = 48
    a, w, bias, acc, r = _epi_data(N)
    add, c0 = r(EPI_M, N), r(EPI_M, N)
    out = c0.to(dev)
    _launch(dev, LINEAR, EPI_M, N, N, a, w, TILED, tile=22, accumulate=True, bias=bias.to(dev), add=add.to(dev), out=out)
    assert_close(out, acc + bias.double() + add.double() + c0.double(), TOL_STEP, "linear + accumulate")
    out = c0.to(dev)
    _launch(dev, LINEAR, EPI_M, N, N, a, w, TILED, tile=22, act=TANH, bias=bias.to(dev), out=out)
    assert_close(out, torch.tanh(acc + bias.double()), TOL_STEP_ACT, "linear + tanh")


def test_epilogue_gru_gates(dev):
    H = EPI_H
    a, w, bias, acc, r = _epi_data(2 * H)
    hp, add = r(EPI_M, H), r(EPI_M, 2 * H)
    z, rr, rh = (torch.full((EPI_M, H), float("nan"), device=dev) for _ in range(3))
    _launch(dev, GATES, EPI_M, 2 * H, H, a, w, TILED, tile=22, bias=bias.to(dev), add=add.to(dev), out=rh, e0=hp.to(dev), o1=z,
            o2=rr)
    gate = torch.sigmoid(acc + bias.double() + add.double())
    assert_close(z, gate[:, :H], TOL_STEP_ACT, "z")
    assert_close(rr, gate[:, H:], TOL_STEP_ACT, "r")
    assert_close(rh, gate[:, H:] * hp.double(), TOL_STEP_ACT, "r * h_prev")


def test_epilogue_gru_candidate(dev):
    H = EPI_H
    a, w, bias, acc, r = _epi_data(H)
    hp, z = r(EPI_M, H), torch.sigmoid(r(EPI_M, H))
    c, hn = (torch.full((EPI_M, H), float("nan"), device=dev) for _ in range(2))
    _launch(dev, CAND, EPI_M, H, H, a, w, TILED, tile=22, bias=bias.to(dev), out=hn, e0=hp.to(dev), e1=z.to(dev), o1=c)
    cand = torch.tanh(acc + bias.double())
    assert_close(c, cand, TOL_STEP_ACT, "c")
    assert_close(hn, z.double() * cand + (1 - z.double()) * hp.double(), TOL_STEP_ACT, "h_next")


def test_epilogue_backward_rh(dev):
    H = EPI_H
    a, w, _, acc, r = _epi_data(H)
    hp, rg, dh0 = r(EPI_M, H), torch.sigmoid(r(EPI_M, H)), r(EPI_M, H)
    dG = torch.full((EPI_M, 2 * H), FILL, device=dev)   # the r half of a [M, 2H] buffer
    dh = dh0.to(dev)
    _launch(dev, BWD_RH, EPI_M, H, H, a, w, TILED, tile=22, out=dG[:, H:], ldo=2 * H, e0=hp.to(dev), e1=rg.to(dev), o1=dh)
    assert_close(dG[:, H:], acc * hp.double() * rg.double() * (1 - rg.double()), TOL_STEP, "dG_r")
    assert_close(dh, dh0.double() + acc * rg.double(), TOL_STEP, "dh_prev")
    assert bool((dG[:, :H] == FILL).all()), "the z half of dG was written"


@pytest.mark.parametrize("layout", [PLAIN, TILED])
def test_epilogue_lstm_cell(dev, layout):
    H = EPI_H
    a, w, bias, acc, r = _epi_data(4 * H)
    cp = r(EPI_M, H)
    cn, s = (torch.full((EPI_M, H), float("nan"), device=dev) for _ in range(2))
    gates = torch.full((EPI_M, 4 * H), float("nan"), device=dev)
    _launch(dev, LSTM, EPI_M, 4 * H, H, a, w, layout, tile=22, bias=bias.to(dev), out=s, e1=cp.to(dev), o1=cn, o2=gates)
    pre = acc + bias.double()
    act = torch.cat([torch.sigmoid(pre[:, :3 * H]), torch.tanh(pre[:, 3 * H:])], 1)   # i | f | o | g
    i, f, o, gg = act.split(H, 1)
    cell = cp.double() * f + gg * i
    assert_close(gates, act, TOL_STEP_ACT, "gate activations")
    assert_close(cn, cell, TOL_STEP_ACT, "c_next")
    assert_close(s, torch.tanh(cell) * o, TOL_STEP_ACT, "s_next")


# ---- the step-GEMM jobs inside ska_kernel / skb_kernel: one small GRU training window -------------------------------------
def _window_case(B):
    name = "waves-s5-gru-L2-T3-B%d-H64-E32-U7" % B
    return D.Case(name, "waves", D.GRU, 2, 3, B, 64, 32, 3, 7, 0, "l0", 2, True, False, (("PARROT_SCHEDULE", "5"),), "")


_WINDOWS = {}


def _window(dev, B):
    """The case run once (tests/test_gpu_decoder_scan_edges.py's framed plan): route, launch kinds, one window's buffers."""
    if B not in _WINDOWS:
        from tests.test_gpu_decoder_scan_edges import Scan
        case = _window_case(B)
        scan = Scan(dev, case)
        try:
            res = dict(case=case, route=scan.route, kinds=S.plan_modes(scan.plan), window=None)
            if scan.route == D.expected_route(case):
                res["window"] = scan.window()
        finally:
            scan.close()
        _WINDOWS[B] = res
    return _WINDOWS[B]


def _tolerance(case, noise, name, elem=False):
    base = D.TOL_FWD if name in D.forward_names(case.cell, case.L) else D.TOL_BWD
    floor = noise[name + (":elem" if elem else "")]
    return D.NOISE_MARGIN * floor if floor > base / D.NOISE_MARGIN else base


@pytest.mark.parametrize("B", [5, 64])
def test_training_window_on_the_heterogeneous_launches(dev, B):
    from tests.test_gpu_decoder_scan_edges import results_of
    res = _window(dev, B)
    case = res["case"]
    assert res["route"] == dict(schedule=5, tick=8, persistent=0) == D.expected_route(case), res["route"]
    for kernel in ("ska", "skb"):
        assert any(k == kernel for k, _, _ in res["kinds"]), "no %s launch among %s" % (kernel, sorted(res["kinds"]))
    out, bad_fwd, bad_bwd, status = res["window"]
    assert status == 0 and not bad_fwd and not bad_bwd, (status, bad_fwd, bad_bwd)
    ref, noise, got = D.case_reference(case), D.noise_row(case), results_of(case, out)
    problems = []
    for n in D.forward_names(case.cell, case.L) + D.backward_names(case.cell, case.L):
        want = D.representable(ref[n])
        checks = [(rel_err, _tolerance(case, noise, n), "")]
        if n in D.ELEMENTWISE:
            checks.append((rel_err_elem, _tolerance(case, noise, n, elem=True), ":elem"))
        for fn, tol, tag in checks:
            e = fn(got[n], want)
            print("B=%d %s%s: %.3e (bound %.1e)" % (B, n, tag, e, tol))
            if not e <= tol:
                problems.append("%s%s: relative error %.3e > %.1e" % (n, tag, e, tol))
    assert not problems, "\n  ".join(problems)
