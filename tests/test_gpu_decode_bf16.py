"""Decode with bf16 operands (Parrot(decode_dtype='bf16'); ParrotSampleDesc::bf16, PM_GEMM16 units in persist.hip): the
recurrent-layer product of every LSTM layer and step rounds BOTH operands to bf16 (nearest even) where they enter the
product and accumulates in f32; states, cells, biases, additive inputs, the attention window, the composed output product
and the per-call host products stay f32.

The yardstick is the ROUNDED ORACLE: oracle/parrot_ref.py under operand_rounding('bf16') with the products the contract
leaves exact made exact for the duration of a call (R.linear: readouts, output, speaker-to-readout / -output; R.fork for
the speaker_to_* names; h1_to_att is exact already).  Nothing under oracle/ changes.  Parameters are made
f32-representable first, so that the model and the oracle round the same weights."""
import contextlib
import ctypes as C
import functools

import pytest
import torch

from tests.test_gpu_decode_lstm import NAMES, SMALL, _abort_word
from tests.util import assert_close, make_batch, rel_err

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def rounded_oracle():
    from oracle import parrot_ref as R
    lin, frk = R.linear, R.fork

    def linear(p, name, x):
        return x @ p[f'/parrot/{name}.W'] + p[f'/parrot/{name}.b']

    def fork(p, name, x, outs):
        if name.startswith('speaker_to_'):
            return [x @ p[f'/parrot/{name}/fork_{o}.W'] + p[f'/parrot/{name}/fork_{o}.b'] for o in outs]
        return frk(p, name, x, outs)

    R.linear, R.fork = linear, fork
    try:
        with R.operand_rounding('bf16'):
            yield
    finally:
        R.linear, R.fork = lin, frk


def _params(cfg, seed, perturb=False, kappa_bias=None):
    from oracle import parrot_ref as R
    p = R.init_params(cfg, seed=seed, scale_by_fan_in=True)
    if kappa_bias is not None:
        p['/parrot/h1_to_att/fork_kappa.b'].fill_(kappa_bias)
    if perturb:
        g = torch.Generator().manual_seed(21)
        keys = ['/parrot.initial_w'] + [f'/parrot/rnn{l}.{nm}' for l in range(1, cfg['num_layers'] + 1)
                                        for nm in ("initial_state", "initial_cells")]
        for k in keys:
            p[k] = p[k] + 0.5 * torch.randn(p[k].shape, generator=g, dtype=p[k].dtype)
    return {k: v.float().double() for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def _case(kw_items, N, U, S, seed=7, perturb=False, kappa_bias=None, batch_seed=9, with_f32=False):
    """(full kwargs, parameters, batch, exact oracle, rounded oracle[, the rounded oracle accumulated in f32]): computed
    once per case and shared; nothing in it is modified afterwards."""
    from oracle import parrot_ref as R
    full = dict(kw_items)
    cfg = R.default_config(**full)
    p = _params(cfg, seed, perturb, kappa_bias)
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=batch_seed, speaker=cfg['use_speaker'])
    with torch.no_grad():
        exact = R.sample_model(p, cfg, lab, lm, spk, S)
        with rounded_oracle():
            rnd = R.sample_model(p, cfg, lab, lm, spk, S)
            rnd32 = None
            if with_f32:
                p32 = {k: v.float() for k, v in p.items()}
                rnd32 = R.sample_model(p32, cfg, lab, lm.float(), spk, S)
    return full, p, (lab, lm, spk), exact, rnd, rnd32


def _small(**kw):
    return tuple(sorted(dict(SMALL, **kw).items()))


def _engaged_bf16(m, S, N, U):
    """Every test that engages the bf16 plan: it IS the bf16 plan, on the machine, no spin timed out, no launch gave up."""
    from parrot_amd import _lib
    ws = m._sample_ws.get((S, N, U))
    assert ws is not None
    lib = _lib.load()
    assert lib.parrot_sample_is_bf16(ws['plan']) == 1
    assert lib.parrot_sample_is_persistent(ws['plan']) != 0
    assert _abort_word(ws) == 0, "a spin timed out inside the machine"
    assert lib.parrot_sample_status(ws['plan']) == 0
    return ws


def _decode(dev, full, p, batch, N, S, decode_dtype='bf16', reps=1, **extra):
    from parrot_amd.model import Parrot
    lab, lm, spk = batch
    m = Parrot(device=dev, use_graph=True, decode_dtype=decode_dtype, **full, **extra).allocate()
    m.set_parameter_values(p)
    outs = None
    for _ in range(reps):
        outs = [o.clone() for o in m.sample_model_device(lab, lm.float(), spk, N, S)]
    return m, outs


def _check(outs, ref, tol, tag):
    worst = 0.0
    for o, r, n in zip(outs, ref, NAMES):
        assert tuple(o.shape) == tuple(r.shape), n
        e = rel_err(o, r)
        print(f"{tag}: {n} {e:.3e}")
        worst = max(worst, e)
    for o, r, n in zip(outs, ref, NAMES):
        assert_close(o, r, tol[n] if isinstance(tol, dict) else tol, f"{tag}: {n}")
    return worst


# ------------------------------------------------------------------------------------------------ 1. layout
@pytest.mark.parametrize("rows,cols,lstm_h", [(64, 48, 0), (160, 256, 64), (96, 128, 32)])
def test_tile_weights_bf16_machine_layout(dev, rows, cols, lstm_h):
    """parrot_tile_weights_bf16 mode 2, bit for bit: block [ct][c], lane (kk, i) holds K rows 32c + 4kk .. + 3 and
    32c + 16 + 4kk .. + 3 of column col(ct, i) -- what the same lane of two f32 fragment-major blocks holds."""
    from parrot_amd import _lib, ops
    g = torch.Generator().manual_seed(rows * 7 + cols)
    W = torch.randn(rows, cols, generator=g).to(dev)
    out = torch.zeros(rows * cols, dtype=torch.bfloat16, device=dev)
    _lib.call('parrot_tile_weights_bf16', W.data_ptr(), rows, cols, cols, out.data_ptr(), 2, lstm_h, ops._stream())
    torch.cuda.synchronize()
    Wb = W.to(torch.bfloat16).cpu()
    got = out.cpu().view(-1, 64, 8)  # [block][lane][u]
    nch = rows // 32
    exp = torch.empty_like(got)
    for ct in range(cols // 16):
        for c in range(nch):
            for lane in range(64):
                i, kk = lane & 15, lane >> 4
                ks = torch.cat([torch.arange(4) + 32 * c + 4 * kk, torch.arange(4) + 32 * c + 16 + 4 * kk])
                col = (i >> 2) * lstm_h + ct * 4 + (i & 3) if lstm_h else ct * 16 + i
                exp[ct * nch + c, lane] = Wb[ks, col]
    assert torch.equal(got.view(torch.int16), exp.view(torch.int16))


# ------------------------------------------------------------------------------------------------ 2. arithmetic pinned
@pytest.mark.parametrize("N", [5, 37])
@pytest.mark.parametrize("kw", [dict(num_layers=1),
                                dict(num_layers=2, weak_feedback=True),
                                dict(num_layers=3, full_feedback=True, use_speaker=True)])
def test_bf16_decode_rounds_the_declared_operands_to_nearest_even(dev, kw, N):
    """S = 2 with perturbed initial state, cells and w: all six outputs within 1e-4 (the project's f32 parity tolerance) of
    the rounded oracle in fp64, while the rounded oracle itself is more than 3e-4 from the exact one on sample_x -- so the
    test tells round-to-nearest-even on exactly the declared operands from anything else (f32 operands, truncation, a
    rounded readout).  On the CPU the f32-accumulated rounded oracle is within 6.4e-7 of the fp64 one on these cases.
    Measured on the MI355X (worst of the six outputs over the six cases): 2.3e-7 against the rounded oracle, which is
    6.4e-4 .. 1.5e-3 away from the exact one on sample_x."""
    U, S = 9, 2
    full, p, batch, exact, rnd, _ = _case(_small(**kw), N, U, S, perturb=True)
    moved = rel_err(rnd[0], exact[0])
    print(f"rounded vs exact oracle, sample_x: {moved:.3e}")
    assert moved > 3e-4, "the rounded and the exact oracle are too close on this case to tell the two arithmetics apart"
    m, outs = _decode(dev, full, p, batch, N, S)
    _engaged_bf16(m, S, N, U)
    _check(outs, rnd, 1e-4, f"L={full['num_layers']} N={N} vs rounded oracle")
    m.close()


# ------------------------------------------------------------------------------------------------ 3. trajectories
@pytest.mark.parametrize("kw", [dict(num_layers=1),
                                dict(num_layers=2, weak_feedback=True),
                                dict(num_layers=3, full_feedback=True, use_speaker=True),
                                dict(num_layers=2, weak_feedback=True, sharpening_coeff=1.2, timing_coeff=0.9,
                                     attention_type='softmax')])
def test_bf16_decode_trajectories(dev, kw):
    """N = 5, U = 9, S = 14: every output within 2e-3 of the rounded oracle (the bar for two bf16 paths with the same rounding
    points, tests/test_gpu_bf16.py) and within 2e-2 of the exact oracle (the mode's tolerance); sample_x is more than 1e-4
    away from the f32 decode of the same model.  On the CPU: f32-accumulated rounded oracle vs the fp64 one at most 8.8e-5,
    rounded vs exact oracle 0.5e-3 to 4.2e-3.  Measured on the MI355X (worst output, four cases): 2.7e-7 against the rounded
    oracle, 4.2e-3 against the exact one; sample_x 2.2e-3 .. 2.7e-3 away from the f32 decode."""
    N, U, S = 5, 9, 14
    full, p, batch, exact, rnd, _ = _case(_small(**kw), N, U, S)
    m, outs = _decode(dev, full, p, batch, N, S, reps=2)
    _engaged_bf16(m, S, N, U)
    _check(outs, rnd, 2e-3, "vs rounded oracle")
    _check(outs, exact, 2e-2, "vs exact oracle")
    m.close()
    m32, outs32 = _decode(dev, full, p, batch, N, S, decode_dtype='float32')
    from parrot_amd import _lib
    assert _lib.load().parrot_sample_is_bf16(m32._sample_ws.get((S, N, U))['plan']) == 0
    m32.close()
    d = rel_err(outs[0], outs32[0])
    print(f"bf16 vs f32 decode, sample_x: {d:.3e}")
    assert d > 1e-4, "decode_dtype='bf16' did not change the arithmetic"


# ------------------------------------------------------------------------------------------------ 4. row blocks
@pytest.mark.parametrize("B", [16, 24, 37, 64])
def test_bf16_decode_row_blocks(dev, B):
    """1, 2, 4 and 4 row blocks at L = 2, S = 10, padding rows never waited for; the library's size query equals the
    workspace.  (CPU floor at B = 37: 7.6e-4.)  Measured on the MI355X, worst output against the rounded / exact oracle:
    B 16 2.6e-7 / 4.6e-3, B 24 2.8e-6 / 4.0e-3, B 37 4.0e-4 / 5.3e-3, B 64 8.6e-4 / 7.6e-3 (beyond B = 16 an operand lands on
    the other bf16 neighbour somewhere within the ten steps)."""
    from parrot_amd import _lib
    U, S = 9, 10
    full, p, batch, exact, rnd, _ = _case(_small(num_layers=2, weak_feedback=True), B, U, S)
    m, outs = _decode(dev, full, p, batch, B, S)
    ws = _engaged_bf16(m, S, B, U)
    _check(outs, rnd, 2e-3, f"B={B} vs rounded oracle")
    _check(outs, exact, 2e-2, f"B={B} vs exact oracle")
    n = _lib.load().parrot_sample_persist_floats(C.byref(ws['desc']))
    assert 0 < n == ws['pm']['ws'].numel()
    m.close()


# ------------------------------------------------------------------------------------------------ 5. barrier == dataflow
def test_bf16_dataflow_mode_matches_the_barrier_mode_bit_for_bit(dev, monkeypatch):
    """L = 3, N = 37, S = 9.  Measured on the MI355X: both modes 9.4e-7 from the rounded oracle (worst output), equal bit for bit."""
    N, U, S = 37, 11, 9
    full, p, batch, exact, rnd, _ = _case(_small(num_layers=3, weak_feedback=True), N, U, S, seed=4, batch_seed=5)
    got = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("PARROT_PM_DATAFLOW", mode)
        m, got[mode] = _decode(dev, full, p, batch, N, S)
        _engaged_bf16(m, S, N, U)
        _check(got[mode], rnd, 2e-3, f"dataflow={mode} vs rounded oracle")
        m.close()
    for a, b, n in zip(got["0"], got["1"], NAMES):
        assert torch.equal(a, b), n


# ------------------------------------------------------------------------------------------------ 6. replay and refresh
def test_bf16_replay_and_refreshed_weight_copies(dev):
    """Two calls on one workspace are equal; after set_parameter_values with other parameters the next call equals a fresh
    model's output bit for bit (a stale bf16 copy would not)."""
    from oracle import parrot_ref as R
    N, U, S = 5, 9, 8
    full, p, batch, _, rnd, _ = _case(_small(num_layers=2, weak_feedback=True), N, U, S)
    cfg = R.default_config(**full)
    p2 = _params(cfg, seed=8)
    m, a = _decode(dev, full, p, batch, N, S)
    lab, lm, spk = batch
    b = [o.clone() for o in m.sample_model_device(lab, lm.float(), spk, N, S)]
    for x, y, n in zip(a, b, NAMES):
        assert torch.equal(x, y), n
    m.set_parameter_values(p2)
    c = [o.clone() for o in m.sample_model_device(lab, lm.float(), spk, N, S)]
    _engaged_bf16(m, S, N, U)
    m.close()
    fresh_m, fresh = _decode(dev, full, p2, batch, N, S)
    _engaged_bf16(fresh_m, S, N, U)
    fresh_m.close()
    assert rel_err(c[0], a[0]) > 1e-3, "the second parameter set must decode differently"
    for x, y, n in zip(c, fresh, NAMES):
        assert torch.equal(x, y), n


# ------------------------------------------------------------------------------------------------ 7 / 8. wide stacks
def _wide(dev, full_kw, seed, batch_seed, N, U, S, tag):
    full, p, batch, exact, rnd, rnd32 = _case(tuple(sorted(full_kw.items())), N, U, S, seed=seed, kappa_bias=-1.0,
                                              batch_seed=batch_seed, with_f32=True)
    # the rounded oracle is itself unsteady at these widths: its f32-accumulated twin against the fp64 one, per output
    floor = {n: rel_err(a, b) for a, b, n in zip(rnd32, rnd, NAMES)}
    print(f"{tag}: floors {floor}")
    assert max(floor.values()) <= 5e-3, f"the rounded oracle is too unsteady on this input to judge by: {floor}"
    # factor 4: a summation order (8-way K split, 32-deep MFMA) that differs from torch's
    tol = {n: max(2e-3, 4 * f) for n, f in floor.items()}
    m, outs = _decode(dev, full, p, batch, N, S, reps=2)
    ws = _engaged_bf16(m, S, N, U)
    _check(outs, exact, 2e-2, f"{tag} vs exact oracle")
    _check(outs, rnd, tol, f"{tag} vs rounded oracle")
    m.close()
    return ws


def test_bf16_decode_streamed_and_resident_units(dev):
    """3 x LSTM-1024, E = 512, B = 16, U = 40, S = 16: one unit per workgroup and phase; a workgroup's three slabs need 7744
    bf16 K-rows against the 4608 it holds, so resident and streamed bf16 units run in one launch, beside the streamed f32
    output tiles.  2e-2 against the exact oracle; against the rounded oracle max(2e-3, 4 x floor), floor = the error of
    the f32-accumulated rounded oracle against the fp64 one, per output, computed here (up to 2.5e-3 on phi); the test
    fails instead of widening if a floor exceeds 5e-3.  Measured on the MI355X (worst output, pi_att): 1.4e-3 against the
    rounded oracle (its floor 1.5e-3), 7.0e-3 against the exact one."""
    kw = dict(num_layers=3, encoder_type='bidirectional', encoder_dim=256, cell_type='lstm', rnn_h_dim=1024,
              readouts_dim=1024, weak_feedback=True)
    _wide(dev, kw, 29, 31, 16, 40, 16, "3x1024")


def test_bf16_decode_cfg4_width_two_units_per_workgroup(dev):
    """3 x LSTM-1536, readouts 1536, B = 16, U = 100, S = 16: 384 tiles per layer on 256 workgroups, two units per workgroup
    and phase, barriers.  Same tolerances as the 3 x 1024 test (floor up to 1.9e-3 on the CPU).  Measured on the MI355X
    (worst output, pi_att): 1.7e-3 against the rounded oracle (its floor 2.0e-3), 5.6e-3 against the exact one."""
    kw = dict(num_layers=3, encoder_type='bidirectional', cell_type='lstm', rnn_h_dim=1536, readouts_dim=1536,
              weak_feedback=True)
    _wide(dev, kw, 29, 31, 16, 100, 16, "3x1536")


# ------------------------------------------------------------------------------------------------ 9. refusals
@pytest.mark.parametrize("kw,env", [(dict(cell_type='gru'), None),
                                    (dict(which_cost='GMM', k_gmm=3), None),
                                    (dict(layer_norm=True), None),
                                    (dict(rnn_h_dim=48), None),
                                    (dict(), ("PARROT_SAMPLE_PERSIST", "0"))])
def test_bf16_decode_refuses_what_it_does_not_cover(dev, monkeypatch, kw, env):
    """No silent f32 decode: a ValueError that names the reason when the workspace is made, and no plan is left behind."""
    from oracle import parrot_ref as R
    from parrot_amd.model import Parrot
    if env:
        monkeypatch.setenv(*env)
    full = dict(SMALL, num_layers=2, weak_feedback=True, **kw)
    cfg = R.default_config(**full)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    N, U, S = 4, 9, 6
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=9)
    m = Parrot(device=dev, use_graph=True, decode_dtype='bf16', **full).allocate()
    m.set_parameter_values(p)
    with pytest.raises(ValueError, match="decode_dtype='bf16'"):
        m.sample_model_device(lab, lm.float(), spk, N, S)
    assert len(m._sample_ws) == 0
    m.close()


# ------------------------------------------------------------------------------------------------ 10. default untouched
def test_default_decode_of_a_bf16_trained_model_keeps_f32_operands(dev):
    """compute_dtype='bf16' without decode_dtype: the f32 machine, outputs within 1e-4 of the exact oracle, as before
    (measured on the MI355X: 2.1e-7)."""
    from parrot_amd import _lib
    from parrot_amd.model import Parrot
    N, U, S = 5, 9, 14
    full, p, batch, exact, _, _ = _case(_small(num_layers=2, weak_feedback=True), N, U, S)
    lab, lm, spk = batch
    m = Parrot(device=dev, use_graph=True, compute_dtype='bf16', **full).allocate()
    m.set_parameter_values(p)
    outs = m.sample_model_device(lab, lm.float(), spk, N, S)
    ws = m._sample_ws.get((S, N, U))
    assert _lib.load().parrot_sample_is_bf16(ws['plan']) == 0
    assert _lib.load().parrot_sample_is_persistent(ws['plan']) != 0
    _check(outs, exact, 1e-4, "default decode vs exact oracle")
    m.close()
