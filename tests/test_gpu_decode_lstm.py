"""LSTM decoders on the persistent phase machine (plans_decode.hip build_persist_lstm, persist.hip PM_EPI_LSTM): the
whole sample_model loop as one resident kernel, L + 2 phases per step.  Every output against the fp64 oracle, the machine
really engaged, replay on the same workspace, and the per-step launch path (PARROT_SAMPLE_PERSIST=0) as the second
witness."""
import ctypes as C

import pytest
import torch

from tests.util import assert_close, make_batch

pytestmark = pytest.mark.gpu

SMALL = dict(rnn_h_dim=64, readouts_dim=48, encoder_dim=16, input_dim=24, speaker_dim=8, num_speakers=5,
             encoder_type='bidirectional', cell_type='lstm')
NAMES = ("sample_x", "k", "w", "pi", "phi", "pi_att")


def _abort_word(ws):
    return int(ws['pm']['ws'][832:833].view(torch.int32).item())


def _engaged(m, S, N, U, want=True):
    """The plan the workspace holds runs on the machine (or not), no launch gave up, no spin timed out."""
    from parrot_amd import _lib
    ws = m._sample_ws.get((S, N, U))
    assert ws is not None
    got = _lib.load().parrot_sample_is_persistent(ws['plan'])
    if want:
        assert got != 0, "the LSTM decoder did not run on the persistent machine"
        assert _abort_word(ws) == 0, "a spin timed out inside the machine"
    else:
        assert got == 0
    assert _lib.load().parrot_sample_status(ws['plan']) == 0
    return ws


def _run(dev, full, p, lab, lm, spk, N, S, ref, tag, reps=2):
    from parrot_amd.model import Parrot
    m = Parrot(device=dev, use_graph=True, **full).allocate()
    m.set_parameter_values(p)
    for rep in range(reps):
        outs = m.sample_model_device(lab, lm.float(), spk, N, S)
        for o, r, n in zip(outs, ref, NAMES):
            assert tuple(o.shape) == tuple(r.shape), n
            assert_close(o, r, 1e-4, f"{tag} pass {rep}: {n}")
    return m, [o.clone() for o in outs]


@pytest.mark.parametrize("kw", [dict(num_layers=1),
                                dict(num_layers=2, weak_feedback=True),
                                dict(num_layers=3, full_feedback=True, use_speaker=True),
                                dict(num_layers=2, weak_feedback=True, sharpening_coeff=1.2, timing_coeff=0.9,
                                     attention_type='softmax')])
def test_lstm_decode_on_the_persistent_machine(dev, monkeypatch, kw):
    """N = 5 (padding rows), U = 9, S = 14: all six outputs at 1e-4 vs the fp64 oracle on the machine (one plan: whole-K,
    parrot_sample_is_persistent == 1) and on the launches, two calls per workspace, and machine vs launches at 2e-5.
    Measured on the MI355X (worst of the six outputs, four cases): launches vs oracle 3.5e-7, machine vs oracle 3.0e-7,
    machine vs launches 4.0e-7."""
    from oracle import parrot_ref as R
    full = dict(SMALL, **kw)
    cfg = R.default_config(**full)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    N, U, S = 5, 9, 14
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=9, speaker=cfg['use_speaker'])
    with torch.no_grad():
        ref = R.sample_model(p, cfg, lab, lm, spk, S)
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("PARROT_SAMPLE_PERSIST", mode)
        m, res[mode] = _run(dev, full, p, lab, lm, spk, N, S, ref, f"persist={mode}")
        _engaged(m, S, N, U, want=mode == "1")
        m.close()
    for a, b, n in zip(res["1"], res["0"], NAMES):
        assert_close(a, b, 2e-5, f"machine vs launches: {n}")


@pytest.mark.parametrize("B", [16, 24, 37, 64])
def test_lstm_decode_row_blocks(dev, B):
    """1, 2, 4 and 4 row blocks (B <= 16 / 32 / 64) at L = 2: parity, machine engaged (dataflow mode is the default: a
    padding row that was waited for would end in the abort word), workspace size reported by the library."""
    from oracle import parrot_ref as R
    from parrot_amd import _lib
    full = dict(SMALL, num_layers=2, weak_feedback=True)
    cfg = R.default_config(**full)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    U, S = 9, 10
    _, _, lab, lm, spk = make_batch(cfg, 2, B, U, seed=9)
    with torch.no_grad():
        ref = R.sample_model(p, cfg, lab, lm, spk, S)
    m, _ = _run(dev, full, p, lab, lm, spk, B, S, ref, f"B={B}")
    ws = _engaged(m, S, B, U)
    lib = _lib.load()
    lib.parrot_sample_persist_floats.restype = C.c_longlong
    n = lib.parrot_sample_persist_floats(C.byref(ws['desc']))
    assert 0 < n == ws['pm']['ws'].numel()
    m.close()


def test_lstm_dataflow_mode_matches_the_barrier_mode_bit_for_bit(dev, monkeypatch):
    from oracle import parrot_ref as R
    full = dict(SMALL, num_layers=3, weak_feedback=True)
    cfg = R.default_config(**full)
    p = R.init_params(cfg, seed=4, scale_by_fan_in=True)
    N, U, S = 37, 11, 9
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=5)
    with torch.no_grad():
        ref = R.sample_model(p, cfg, lab, lm, spk, S)
    got = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("PARROT_PM_DATAFLOW", mode)
        m, got[mode] = _run(dev, full, p, lab, lm, spk, N, S, ref, f"dataflow={mode}")
        _engaged(m, S, N, U)
        m.close()
    for a, b in zip(got["0"], got["1"]):
        assert torch.equal(a, b)


def test_lstm_decode_starts_from_initial_state_and_cells(dev):
    """Non-zero initial_state AND initial_cells parameters: the first frame already depends on both."""
    from oracle import parrot_ref as R
    full = dict(SMALL, num_layers=2, weak_feedback=True)
    cfg = R.default_config(**full)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    g = torch.Generator().manual_seed(21)
    for l in (1, 2):
        for nm in ("initial_state", "initial_cells"):
            k = f'/parrot/rnn{l}.{nm}'
            p[k] = p[k] + 0.5 * torch.randn(p[k].shape, generator=g, dtype=p[k].dtype)
    N, U, S = 5, 9, 8
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=9)
    with torch.no_grad():
        ref = R.sample_model(p, cfg, lab, lm, spk, S)
        p0 = dict(p)
        for l in (1, 2):
            p0[f'/parrot/rnn{l}.initial_cells'] = torch.zeros_like(p[f'/parrot/rnn{l}.initial_cells'])
        ref0 = R.sample_model(p0, cfg, lab, lm, spk, S)
    assert float((ref[0][0] - ref0[0][0]).abs().max()) > 1e-4, "the first frame must depend on the initial cells"
    m, _ = _run(dev, full, p, lab, lm, spk, N, S, ref, "initial state")
    _engaged(m, S, N, U)
    m.close()


def test_lstm_decode_cfg4_width(dev, monkeypatch):
    """3 x LSTM-1536, readouts 1536, weak feedback, B = 16, U = 100, S = 60: 384 tiles per layer on 256 workgroups (two
    units per workgroup and phase) and streamed weights.  Launch path first (the yardstick that fixes S), then the machine
    forced on: both at 1e-4 against the fp64 oracle over all S frames.  Measured on the MI355X at S = 60 (worst output,
    phi): launch path (its arithmetic is the parent commit's) 2.9e-6, machine 2.1e-6, machine vs launches 1.4e-6."""
    from oracle import parrot_ref as R
    full = dict(num_layers=3, encoder_type='bidirectional', cell_type='lstm', rnn_h_dim=1536, readouts_dim=1536,
                weak_feedback=True)
    cfg = R.default_config(**full)
    p = R.init_params(cfg, seed=29, scale_by_fan_in=True)
    p['/parrot/h1_to_att/fork_kappa.b'].fill_(-1.0)
    N, U, S = 16, 100, 60
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=31)
    with torch.no_grad():
        ref = R.sample_model(p, cfg, lab, lm, spk, S)
    monkeypatch.setenv("PARROT_SAMPLE_PERSIST", "0")
    m, _ = _run(dev, full, p, lab, lm, spk, N, S, ref, "launches", reps=1)
    _engaged(m, S, N, U, want=False)
    m.close()
    monkeypatch.setenv("PARROT_SAMPLE_PERSIST", "1")   # (the default: the machine wherever the shape qualifies)
    m, _ = _run(dev, full, p, lab, lm, spk, N, S, ref, "machine", reps=2)
    _engaged(m, S, N, U)
    m.close()


@pytest.mark.parametrize("kw,tol", [(dict(num_layers=2, weak_feedback=True, which_cost='GMM', k_gmm=3), 2e-4),
                                    (dict(num_layers=2, weak_feedback=True, layer_norm=True), 3e-4)])
def test_lstm_fallbacks_still_fall_back(dev, kw, tol):
    """GMM head / layer_norm are not covered by the machine: the launches run and match the oracle as before."""
    from oracle import parrot_ref as R
    from parrot_amd import _lib
    from parrot_amd.model import Parrot
    full = dict(SMALL, **kw)
    cfg = R.default_config(**full)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    N, U, S = 4, 9, 10
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=9)
    g = torch.Generator().manual_seed(11)
    unif = torch.rand(S, N, generator=g, dtype=torch.float64)
    noise = torch.randn(S, N, cfg['output_dim'], generator=g, dtype=torch.float64)
    with torch.no_grad():
        ref = R.sample_model(p, cfg, lab, lm, spk, S, unif=unif, noise=noise)
    m = Parrot(device=dev, use_graph=True, **full).allocate()
    m.set_parameter_values(p)
    outs = m.sample_model_device(lab, lm.float(), spk, N, S, unif=unif.float(), noise=noise.float())
    for o, r, n in zip(outs, ref, NAMES):
        assert_close(o, r, tol, n)
    ws = m._sample_ws.get((S, N, U))
    assert 'pm' not in ws and _lib.load().parrot_sample_is_persistent(ws['plan']) == 0
    m.close()
