"""GRU decoders with bf16 operands on the decode machine (PARROT_PM_GRU_BF16=1 with Parrot(decode_dtype='bf16');
ParrotSampleDesc::bf16 with cell = 0, PM_GEMM16 layer units in both GRU programs, pm_kernel<MB, DF, false, true, EOU, false>):
the gate and the candidate product of every layer and step round BOTH operands to bf16 (nearest even) where they enter the
product -- r * h where it enters the candidate product -- and accumulate in f32; gate activations, the state blend, the
attention window, the readout / output tiles and the per-call host products stay f32.  The fed-back-frame composition and
the attention fold are not taken under bf16.

The yardstick is the rounded oracle of tests/test_gpu_decode_bf16.py (oracle/parrot_ref.py under operand_rounding('bf16')
with the products the contract leaves exact made exact); its helpers are imported from there.  Where a tolerance follows
the oracle's own unsteadiness it is max(2e-3, 4 x floor) per output, floor = the f32-accumulated rounded oracle against the
fp64 one, computed in the test, which fails instead of widening if a floor exceeds 5e-3 (the rule of _wide in that file).
The CPU figures quoted below are the oracle's own behaviour on the CPU."""
import ctypes as C
import functools

import pytest
import torch

from tests.test_gpu_decode_bf16 import _case, _check, _decode, _engaged_bf16, _wide, rounded_oracle
from tests.test_gpu_decode_lstm import NAMES, SMALL
from tests.util import make_batch, rel_err

pytestmark = pytest.mark.gpu

SWITCH = "PARROT_PM_GRU_BF16"
GRU = dict(SMALL, cell_type='gru')   # H 64, E 32, R 48


@pytest.fixture
def on(monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    return monkeypatch


def _small(**kw):
    return tuple(sorted(dict(GRU, **kw).items()))


def _params(cfg, seed, perturb=False):
    """f32-representable parameters; perturb: non-zero initial_w and initial_state (a GRU has no initial_cells)."""
    from oracle import parrot_ref as R
    p = R.init_params(cfg, seed=seed, scale_by_fan_in=True)
    if perturb:
        g = torch.Generator().manual_seed(21)
        keys = ['/parrot.initial_w'] + [f'/parrot/rnn{l}.initial_state' for l in range(1, cfg['num_layers'] + 1)]
        for k in keys:
            p[k] = p[k] + 0.5 * torch.randn(p[k].shape, generator=g, dtype=p[k].dtype)
    return {k: v.float().double() for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def _perturbed_case(kw_items, N, U, S, batch_seed=9):
    """(full kwargs, parameters, batch, exact oracle, rounded oracle, the rounded oracle accumulated in f32) with perturbed
    initial states: computed once per case and shared; nothing in it is modified afterwards."""
    from oracle import parrot_ref as R
    full = dict(kw_items)
    cfg = R.default_config(**full)
    p = _params(cfg, 7, perturb=True)
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=batch_seed, speaker=cfg['use_speaker'])
    with torch.no_grad():
        exact = R.sample_model(p, cfg, lab, lm, spk, S)
        with rounded_oracle():
            rnd = R.sample_model(p, cfg, lab, lm, spk, S)
            rnd32 = R.sample_model({k: v.float() for k, v in p.items()}, cfg, lab, lm.float(), spk, S)
    return full, p, (lab, lm, spk), exact, rnd, rnd32


def _floor_tol(rnd32, rnd, tag):
    floor = {n: rel_err(a, b) for a, b, n in zip(rnd32, rnd, NAMES)}
    print(f"{tag}: floors {floor}")
    assert max(floor.values()) <= 5e-3, f"the rounded oracle is too unsteady on this input to judge by: {floor}"
    return {n: max(2e-3, 4 * f) for n, f in floor.items()}


def _program(m, S, N, U):
    from parrot_amd import _lib
    return _lib.load().parrot_sample_is_persistent(m._sample_ws[(S, N, U)]['plan'])


# ------------------------------------------------------------------------------------------------ 1. arithmetic pinned
L1 = dict(num_layers=1)
L2 = dict(num_layers=2, weak_feedback=True)
L3 = dict(num_layers=3, full_feedback=True, use_speaker=True)


@pytest.mark.parametrize("pieces", ["1", "0"])
@pytest.mark.parametrize("kw,N,batch_seed", [(L1, 5, 9), (L2, 5, 9), (L3, 5, 9), (L1, 17, 9), (L2, 17, 9), (L3, 17, 10)])
def test_bf16_gru_decode_rounds_the_declared_operands_to_nearest_even(dev, on, kw, N, batch_seed, pieces):
    """S = 2 with perturbed initial states and w, on the step cut along K and on the whole-K phases: all six outputs within
    1e-4 (the project's f32 parity tolerance) of the rounded oracle in fp64, while the rounded oracle itself is more than
    3e-4 from the exact one on sample_x (CPU: 1.4e-3 to 2.6e-3) -- round-to-nearest-even on exactly the declared operands,
    r * h among them, and nothing else.  The cases were chosen so that the f32-accumulated rounded oracle stays within 1e-5
    of the fp64 one (within 5e-7 on all six on the CPU that chose them); L3 at N = 17 with batch_seed 9 does not (9.9e-4: an
    operand lands on the other bf16 neighbour) and is left out on purpose, batch_seed 10 takes its place.  That figure is
    printed, not asserted: it depends on the summation order of the host's f32 matrix product (another CPU gave 1.3e-3 for
    L1 at N = 17), while the bar itself is against the fp64 oracle.  Measured on the MI355X (worst of the six outputs over the
    twelve cases): 3.1e-7 against the rounded oracle."""
    U, S = 9, 2
    on.setenv("PARROT_PM_PIECES", pieces)
    full, p, batch, exact, rnd, rnd32 = _perturbed_case(_small(**kw), N, U, S, batch_seed)
    moved = rel_err(rnd[0], exact[0])
    steady = max(rel_err(a, b) for a, b in zip(rnd32, rnd))
    print(f"rounded vs exact oracle, sample_x: {moved:.3e}; f32-accumulated vs fp64 rounded oracle: {steady:.3e}")
    assert moved > 3e-4, "the rounded and the exact oracle are too close on this case to tell the two arithmetics apart"
    m, outs = _decode(dev, full, p, batch, N, S)
    _engaged_bf16(m, S, N, U)
    assert _program(m, S, N, U) == (2 if pieces == "1" else 1)
    _check(outs, rnd, 1e-4, f"L={full['num_layers']} N={N} pieces={pieces} vs rounded oracle")
    m.close()


# ------------------------------------------------------------------------------------------------ 2. trajectories
@pytest.mark.parametrize("kw", [L1, L2, L3,
                                dict(num_layers=2, weak_feedback=True, sharpening_coeff=1.2, timing_coeff=0.9,
                                     attention_type='softmax')])
def test_bf16_gru_decode_trajectories(dev, on, kw):
    """N = 5, U = 9, S = 14: every output within max(2e-3, 4 x floor) of the rounded oracle (CPU floors: 4e-7 for three cases,
    1.6e-3 for the softmax one) and within 2e-2 of the exact oracle (the mode's tolerance; on the CPU the rounded oracle itself
    is 8.7e-3 to 1.22e-2 away); sample_x is more than 1e-4 from the f32 decode of the same model.  Measured on the MI355X
    (worst output, four cases): 4.4e-7 against the rounded oracle, 1.22e-2 against the exact one; sample_x 5.4e-3 .. 9.1e-3
    away from the f32 decode."""
    from parrot_amd import _lib
    N, U, S = 5, 9, 14
    full, p, batch, exact, rnd, rnd32 = _case(_small(**kw), N, U, S, with_f32=True)
    tol = _floor_tol(rnd32, rnd, "trajectory")
    m, outs = _decode(dev, full, p, batch, N, S, reps=2)
    _engaged_bf16(m, S, N, U)
    _check(outs, rnd, tol, "vs rounded oracle")
    _check(outs, exact, 2e-2, "vs exact oracle")
    m.close()
    m32, outs32 = _decode(dev, full, p, batch, N, S, decode_dtype='float32')
    assert _lib.load().parrot_sample_is_bf16(m32._sample_ws.get((S, N, U))['plan']) == 0
    m32.close()
    d = rel_err(outs[0], outs32[0])
    print(f"bf16 vs f32 decode, sample_x: {d:.3e}")
    assert d > 1e-4, "decode_dtype='bf16' did not change the arithmetic"


# ------------------------------------------------------------------------------------------------ 3. row blocks
@pytest.mark.parametrize("B", [16, 24, 37, 64])
def test_bf16_gru_decode_row_blocks(dev, on, B):
    """1, 2, 4 and 4 row blocks at L = 2, S = 4, padding rows never waited for; the library's size query equals the workspace.
    Against the rounded oracle by the floor rule (CPU floors at S = 4: 8.6e-6, 8.6e-7, 5.5e-7, 3.0e-4).  No comparison with the
    exact oracle: the rounded oracle itself is 1.0e-2 to 2.3e-2 from it on these inputs, already at S = 4.  Measured on the
    MI355X (worst output): 5.3e-7, 4.3e-7, 6.0e-7 and 1.2e-4 against the rounded oracle."""
    from parrot_amd import _lib
    U, S = 9, 4
    full, p, batch, exact, rnd, rnd32 = _case(_small(**L2), B, U, S, with_f32=True)
    tol = _floor_tol(rnd32, rnd, f"B={B}")
    m, outs = _decode(dev, full, p, batch, B, S)
    ws = _engaged_bf16(m, S, B, U)
    _check(outs, rnd, tol, f"B={B} vs rounded oracle")
    n = _lib.load().parrot_sample_persist_floats(C.byref(ws['desc']))
    assert 0 < n == ws['pm']['ws'].numel()
    m.close()


# ------------------------------------------------------------------------------------------------ 4. barrier == dataflow
def test_bf16_gru_dataflow_mode_matches_the_barrier_mode_bit_for_bit(dev, on):
    """L = 3, N = 37, U = 11, S = 9 (CPU floor 2.6e-3): both modes within the floor rule of the rounded oracle, equal bit for bit.
    Measured on the MI355X: both modes 4.6e-6 from the rounded oracle (worst output)."""
    N, U, S = 37, 11, 9
    full, p, batch, exact, rnd, rnd32 = _case(_small(num_layers=3, weak_feedback=True), N, U, S, seed=4, batch_seed=5,
                                              with_f32=True)
    tol = _floor_tol(rnd32, rnd, "dataflow")
    got = {}
    for mode in ("0", "1"):
        on.setenv("PARROT_PM_DATAFLOW", mode)
        m, got[mode] = _decode(dev, full, p, batch, N, S)
        _engaged_bf16(m, S, N, U)
        _check(got[mode], rnd, tol, f"dataflow={mode} vs rounded oracle")
        m.close()
    for a, b, n in zip(got["0"], got["1"], NAMES):
        assert torch.equal(a, b), n


# ------------------------------------------------------------------------------------------------ 5. replay and refresh
def test_bf16_gru_replay_and_refreshed_weight_copies(dev, on):
    """Two calls on one workspace are equal; after set_parameter_values with other parameters the next call equals a fresh
    model's output bit for bit (a stale bf16 copy of either group would not)."""
    from oracle import parrot_ref as R
    N, U, S = 5, 9, 8
    full, p, batch, _, rnd, _ = _case(_small(**L2), N, U, S)
    p2 = _params(R.default_config(**full), seed=8)
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


# ------------------------------------------------------------------------------------------------ 6. stop at the end
def test_bf16_gru_program_stops_at_the_end_of_the_utterance(dev, on):
    """Case A of tests/test_gpu_decode_stop.py (2 x GRU-64, E 32, weak feedback, N 5, S 48) with bf16 operands: the stopped run
    equals the first steps_run steps of the full-length bf16 decode bit for bit.  The bf16 decode is another function of the
    weights, so its lengths are checked against its own unstopped run only."""
    from parrot_amd import _lib
    from tests import test_gpu_decode_stop as T
    c = T._case('A')
    m = T._model(dev, c, decode_dtype='bf16')
    lengths = T._stopped_against_plain(m, c, oracle=False)
    assert max(lengths) < c['S']
    for key in ((c['S'], c['N'], c['U']), ('stop', c['S'], c['N'], c['U'], T.EXTRA)):
        assert _lib.load().parrot_sample_is_bf16(m._sample_ws[key]['plan']) == 1
    m.close()


# ------------------------------------------------------------------------------------------------ 7. wide stack
def test_bf16_gru_decode_streamed_and_resident_units(dev, on):
    """2 x GRU-1024, E = 512, readouts 1024, B = 16, U = 40, S = 16: a workgroup's four layer slabs need about 8300 bf16 K-rows
    against the 4608 it holds, so resident and streamed bf16 units run in one launch, beside the f32 output tiles.  2e-2
    against the exact oracle (CPU: the rounded oracle is at most 8.0e-3 away, worst phi); against the rounded oracle
    max(2e-3, 4 x floor) (CPU floors up to 3.4e-3 .. 4.4e-3 depending on the host, worst phi or pi_att).  Measured on the MI355X
    (worst output, pi_att): 2.7e-3 against the rounded oracle (its floor 3.2e-3), 8.0e-3 against the exact one (phi)."""
    kw = dict(num_layers=2, encoder_type='bidirectional', encoder_dim=256, cell_type='gru', rnn_h_dim=1024,
              readouts_dim=1024, weak_feedback=True)
    _wide(dev, kw, 29, 31, 16, 40, 16, "2x1024 gru")


# ------------------------------------------------------------------------------------------------ 8. refusals, defaults
def _refused(dev, full, N=4, U=9, S=6):
    from oracle import parrot_ref as R
    from parrot_amd.model import Parrot
    cfg = R.default_config(**full)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=9)
    m = Parrot(device=dev, use_graph=True, decode_dtype='bf16', **full).allocate()
    m.set_parameter_values(p)
    with pytest.raises(ValueError, match="decode_dtype='bf16'"):
        m.sample_model_device(lab, lm.float(), spk, N, S)
    assert len(m._sample_ws) == 0
    m.close()


@pytest.mark.parametrize("value", [None, "0"])
def test_bf16_gru_decode_is_refused_without_the_switch(dev, monkeypatch, value):
    """No silent f32 decode and no workspace left behind."""
    if value is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, value)
    _refused(dev, dict(GRU, **L2))


@pytest.mark.parametrize("kw,env", [(dict(which_cost='GMM', k_gmm=3), None),
                                    (dict(which_cost='GMM', k_gmm=3), ("PARROT_PM_GMM", "1")),
                                    (dict(layer_norm=True), None),
                                    (dict(rnn_h_dim=48), None),
                                    (dict(), ("PARROT_SAMPLE_PERSIST", "0"))])
def test_bf16_gru_decode_refuses_what_it_does_not_cover(dev, on, kw, env):
    if env:
        on.setenv(*env)
    _refused(dev, dict(GRU, **L2, **kw))


def test_f32_gru_decode_does_not_see_the_switch(dev, monkeypatch):
    """An f32 decode of a GRU model with the switch set is bit-identical to the same decode with the switch unset (the
    default program: the step cut along K with fold and composition)."""
    N, U, S = 5, 9, 14
    full, p, batch, _, _, _ = _case(_small(**L2), N, U, S)
    got = {}
    for value in (None, "1"):
        if value is None:
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, value)
        m, got[value] = _decode(dev, full, p, batch, N, S, decode_dtype='float32')
        assert _program(m, S, N, U) == 3
        m.close()
    for a, b, n in zip(got[None], got["1"], NAMES):
        assert torch.equal(a, b), n
