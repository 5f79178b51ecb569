"""GMM-head models on the persistent phase machine (PARROT_PM_GMM=1; plans_decode.hip gmm_eligible, persist.hip
pm_sample_row): LSTM stacks on L + 3 phases, GRU stacks on the 2L + 3 whole-K phases, the composed head
Wr . [W_mu | W_sig | W_co] as plain column tiles and one sampling unit per batch row.  Every output against the fp64
oracle with explicit randomness, the launches (switch unset) as the second witness, the machine really engaged, both
hand-off modes, replay, the end-of-utterance stop and the refusals.  The cases and their premise (the oracle's pick is no
coin flip): tests/decode_gmm_cases.py, tests/test_decode_gmm_cpu.py."""
import ctypes as C

import pytest
import torch

from tests import decode_gmm_cases as G
from tests.util import assert_close, make_batch, rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-4  # the tolerance of the GMM decode on the launches at these shapes (test_gpu_decode_lstm.py, test_gpu_parrot.py)


def _model(dev, c, params=True, **kw):
    from parrot_amd.model import Parrot
    m = Parrot(device=dev, use_graph=True, **dict(c['full'], **kw)).allocate()
    if params:
        m.set_parameter_values(c['p'])
    return m


def _decode(m, c):
    outs = m.sample_model_device(c['lab'], c['lm'].float(), c['spk'], c['N'], c['S'], unif=c['unif'].float(),
                                 noise=c['noise'].float())
    return [o.clone() for o in outs]


def _abort_word(ws):
    return int(ws['pm']['ws'][832:833].view(torch.int32).item())


def _on_machine(m, c, want=True):
    """The plan of the case's workspace runs on the machine (or on the launches); nothing gave up."""
    from parrot_amd import _lib
    lib = _lib.load()
    ws = m._sample_ws[(c['S'], c['N'], c['U'])]
    if want:
        assert 'pm' in ws
        assert lib.parrot_sample_is_persistent(ws['plan']) == 1
        assert _abort_word(ws) == 0, "a spin timed out inside the machine"
        assert m.decode_path == 'machine'
    else:
        assert 'pm' not in ws
        assert lib.parrot_sample_is_persistent(ws['plan']) == 0
        assert m.decode_path == 'launches'
    assert lib.parrot_sample_status(ws['plan']) == 0
    return ws


def _against(outs, ref, tag):
    worst = 0.0
    for o, r, n in zip(outs, ref, G.NAMES):
        assert tuple(o.shape) == tuple(r.shape), n
        e = rel_err(o, r)
        print(f"{tag}: {n} {e:.3e}")
        worst = max(worst, e)
    for o, r, n in zip(outs, ref, G.NAMES):
        assert_close(o, r, TOL, f"{tag}: {n}")
    return worst


@pytest.mark.parametrize("name", G.PARITY)
def test_gmm_decode_on_the_machine_matches_the_oracle_and_the_launches(dev, monkeypatch, name):
    """LSTM L = 1, 2, 3 and GRU L = 1, 2, each with K = 1, 3, 20 and N = 4, 17 (U = 9, S = 10), a speaker model, full
    feedback, sampling_bias = 0.5: all six outputs at 2e-4 against the fp64 oracle on the machine and on the launches, and
    machine against launches at 2e-4.  Measured on the MI355X, worst output over the 33 cases: machine 2.0e-5
    (lstm3_k3_n17), launches 1.3e-5 (lstm2_k3_n17), machine against launches 1.7e-5; the one-layer stacks and the damped
    two-layer GRU stacks stay below 4e-6 on both paths."""
    c = G.case(name)
    monkeypatch.setenv("PARROT_PM_GMM", "1")
    m = _model(dev, c)
    on = _decode(m, c)
    _on_machine(m, c)
    m.close()
    monkeypatch.delenv("PARROT_PM_GMM")
    m = _model(dev, c)
    off = _decode(m, c)
    _on_machine(m, c, want=False)
    m.close()
    e_on = _against(on, c['ref'], f"{name} machine vs oracle")
    e_off = _against(off, c['ref'], f"{name} launches vs oracle")
    e_x = _against(on, off, f"{name} machine vs launches")
    print(f"WORST {name}: machine {e_on:.3e} launches {e_off:.3e} machine-vs-launches {e_x:.3e}")


@pytest.mark.parametrize("name", ["lstm2_k3_n4", "gru2_k20_n17"])
def test_the_switch_engages_the_machine_and_its_absence_does_not(dev, monkeypatch, name):
    c = G.case(name)
    monkeypatch.setenv("PARROT_PM_GMM", "1")
    m = _model(dev, c)
    assert m.decode_path is None
    _decode(m, c)
    _on_machine(m, c)
    m.close()
    for off in (None, "0"):
        if off is None:
            monkeypatch.delenv("PARROT_PM_GMM")
        else:
            monkeypatch.setenv("PARROT_PM_GMM", off)
        m = _model(dev, c)
        _decode(m, c)
        _on_machine(m, c, want=False)
        m.close()


@pytest.mark.parametrize("mode", ["0", "1"])
@pytest.mark.parametrize("name", ["lstm3_k3_n17", "gru2_k3_n17", "lstm2_k20_n4"])
def test_both_hand_off_modes(dev, monkeypatch, name, mode):
    """Grid barriers (0) and per-slot polling (1): both programs have both; same bits either way (compared through the
    oracle here, bit for bit in test_hand_off_modes_agree_bit_for_bit)."""
    c = G.case(name)
    monkeypatch.setenv("PARROT_PM_GMM", "1")
    monkeypatch.setenv("PARROT_PM_DATAFLOW", mode)
    m = _model(dev, c)
    outs = _decode(m, c)
    _on_machine(m, c)
    _against(outs, c['ref'], f"{name} dataflow={mode}")
    m.close()


@pytest.mark.parametrize("name", ["lstm3_k3_n17", "gru2_k3_n17"])
def test_hand_off_modes_agree_bit_for_bit(dev, monkeypatch, name):
    c = G.case(name)
    monkeypatch.setenv("PARROT_PM_GMM", "1")
    got = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("PARROT_PM_DATAFLOW", mode)
        m = _model(dev, c)
        got[mode] = _decode(m, c)
        _on_machine(m, c)
        m.close()
    for a, b, n in zip(got["0"], got["1"], G.NAMES):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("name", ["lstm2_k3_n4", "gru2_k3_n4"])
def test_replay_follows_the_new_randomness(dev, monkeypatch, name):
    """Three calls on one workspace (one captured graph): the second, with other unif / noise, matches ITS oracle run (the
    head history is emptied per launch, nothing of the first call's picks survives); the third repeats the first bit for
    bit."""
    c1, c2 = G.case(name), G.case(name + '_again')
    assert not torch.equal(c1['unif'], c2['unif'])
    assert float((c1['ref'][0] - c2['ref'][0]).abs().max()) > 1e-2
    monkeypatch.setenv("PARROT_PM_GMM", "1")
    m = _model(dev, c1)
    first = _decode(m, c1)
    second = _decode(m, c2)
    third = _decode(m, c1)
    _on_machine(m, c1)
    assert len(m._sample_ws) == 1
    _against(first, c1['ref'], "first call")
    _against(second, c2['ref'], "second call")
    for a, b, n in zip(third, first, G.NAMES):
        assert torch.equal(a, b), n
    m.close()


# the texts and the window bias of case 'A' of tests/test_gpu_decode_stop.py (copied: its helpers are private)
STOP = dict(N=5, U=9, S=48, texts=[9, 7, 5, 8, 3], kappa_bias=-1.0, extra=8, seed=3)


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_stop_at_the_end_of_the_utterance(dev, monkeypatch, cell):
    """sample_until_end_device on a GMM head (K = 3, fixed unif / noise): the six tensors equal the first steps_run steps
    of the unstopped machine run bit for bit, and lengths is end_of_utterance on that run's full-length phi."""
    from oracle import parrot_ref as R
    from parrot_amd import _lib
    from parrot_amd.utils import end_of_utterance
    full = dict(G.SMALL, cell_type=cell, num_layers=2, weak_feedback=True, k_gmm=3)
    N, U, S, extra = STOP['N'], STOP['U'], STOP['S'], STOP['extra']
    cfg = R.default_config(**full)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    p['/parrot/h1_to_att/fork_kappa.b'].fill_(STOP['kappa_bias'])
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=9)
    for i in range(N):
        lm[i, STOP['texts'][i]:] = 0
    unif, noise = G.randomness(N, cfg['output_dim'], STOP['seed'], steps=S)
    c = dict(full=full, p=p, lab=lab, lm=lm, spk=spk, N=N, U=U, S=S, unif=unif, noise=noise)
    monkeypatch.setenv("PARROT_PM_GMM", "1")
    m = _model(dev, c)
    plain = _decode(m, c)
    _on_machine(m, c)
    outs, lengths = m.sample_until_end_device(lab, lm.float(), spk, N, S, extra=extra, unif=unif.float(), noise=noise.float())
    assert m.decode_path == 'machine'
    ph = plain[4].cpu().numpy()
    own = [end_of_utterance(ph[:, i], min(int(lm[i].sum()), U - 1), S, extra) for i in range(N)]
    print(f"lengths {lengths.tolist()}  rule on the unstopped phi {own}")
    assert lengths.tolist() == own
    assert max(own) < S, "the case no longer ends before the cap"
    steps_run = max(own)
    ws = m._sample_ws[('stop', S, N, U, extra)]
    lib = _lib.load()
    assert lib.parrot_sample_is_persistent(ws['plan']) == 1 and lib.parrot_sample_stops_early(ws['plan']) == 1
    steps = C.c_int(-1)
    assert lib.parrot_sample_steps_run(ws['plan'], C.byref(steps)) == 0 and steps.value == steps_run
    for o, r, n in zip(outs, plain, G.NAMES):
        assert o.shape[0] == steps_run, n
        assert torch.equal(o, r[:steps_run]), f"{n}: the stopped run differs from the unstopped run's first {steps_run} steps"
    assert _abort_word(ws) == 0 and lib.parrot_sample_status(ws['plan']) == 0
    m.close()


def test_stop_is_still_refused_without_the_switch(dev, monkeypatch):
    monkeypatch.delenv("PARROT_PM_GMM", raising=False)
    c = G.case('gru2_k3_n4')
    m = _model(dev, c, params=False)
    with pytest.raises(ValueError, match='GMM'):
        m.sample_until_end_device(c['lab'], c['lm'].float(), c['spk'], c['N'], c['S'], extra=8)
    assert not m._sample_ws
    m.close()


def test_bf16_with_a_gmm_head_stays_refused(dev, monkeypatch):
    monkeypatch.setenv("PARROT_PM_GMM", "1")
    c = G.case('lstm2_k3_n4')
    m = _model(dev, c, params=False, decode_dtype='bf16')
    with pytest.raises(ValueError, match="decode_dtype='bf16'"):
        _decode(m, c)
    assert not m._sample_ws
    m.close()


def test_layer_norm_keeps_the_launches_with_the_switch_on(dev, monkeypatch):
    monkeypatch.setenv("PARROT_PM_GMM", "1")
    c = G.case('layer_norm')
    m = _model(dev, c)
    outs = _decode(m, c)
    _on_machine(m, c, want=False)
    _against(outs, c['ref'], "layer_norm on the launches")
    m.close()
