"""Per-utterance decode controls on the GPU (Parrot.sample_model*(timing_coeffs=, sharpening_coeffs=, sampling_biases=,
speaker_weights=); parrot_sample_set_row_controls; pm_att_row / pm_sample_row with ROW, att_fwd_rows_kernel,
gmm_sample_kernel<true>): every output against the fp64 oracle with column-tensor controls on every decode program and on
the launches, the same row giving the same bits as a model built with its scalars, equal values being the scalar, replay
without stale values, the end-of-utterance stop, the speaker blend, the C entry point and sample.py.  The cases and their
premise: tests/decode_row_controls_cases.py, tests/test_decode_row_controls_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from tests import decode_row_controls_cases as RC
from tests.util import assert_close, make_batch, rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-4  # the project's decode tolerance at these shapes (tests/test_gpu_decode_gmm.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = 10001
SWITCHES = ("PARROT_PM_GMM", "PARROT_PM_PIECES", "PARROT_PM_FBC", "PARROT_PM_ATTFOLD", "PARROT_PM_DATAFLOW", "PARROT_SAMPLE_PERSIST")


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _model(dev, c, **kw):
    from parrot_amd.model import Parrot
    m = Parrot(device=dev, use_graph=True, **dict(c['full'], **kw)).allocate()
    m.set_parameter_values(c['p'])
    return m


def _kw(ctl):
    if ctl is None:
        return {}
    return dict(timing_coeffs=ctl['timing'], sharpening_coeffs=ctl['sharpening'], sampling_biases=ctl.get('bias'))


def _decode(m, c, ctl=None, **extra):
    outs = m.sample_model_device(c['lab'], c['lm'].float(), c['spk'], c['N'], c['S'], unif=c['unif'].float(),
                                 noise=c['noise'].float(), **_kw(ctl), **extra)
    return [o.clone() for o in outs]


def _abort_word(ws):
    return int(ws['pm']['ws'][832:833].view(torch.int32).item())


def _on_path(m, c, path, key=None):
    """The last call ran on `path` ('machine' / 'launches'), nothing gave up."""
    from parrot_amd import _lib
    lib = _lib.load()
    ws = m._sample_ws[key or (c['S'], c['N'], c['U'])]
    assert m.decode_path == path
    assert (lib.parrot_sample_is_persistent(ws['plan']) != 0) == (path == 'machine')
    if path == 'machine':
        assert _abort_word(ws) == 0, "a spin timed out inside the machine"
    assert lib.parrot_sample_status(ws['plan']) == 0
    return ws


def _against(outs, ref, tag, tol=TOL):
    for o, r, n in zip(outs, ref, RC.NAMES):
        assert tuple(o.shape) == tuple(r.shape), n
        print(f"{tag}: {n} {rel_err(o, r):.3e}")
    for o, r, n in zip(outs, ref, RC.NAMES):
        assert_close(o, r, tol, f"{tag}: {n}")


def _same_bits(a, b, tag, rows=None):
    for x, y, n in zip(a, b, RC.NAMES):
        if rows is not None:
            x, y = x[:, rows], y[:, rows]
        assert torch.equal(x, y), f"{tag}: {n} differs"


# ------------------------------------------------------------------------------------------------ 1. oracle parity
GMM_ON = {"PARROT_PM_GMM": "1"}
PARITY = [(n, {}, 'machine') for n in RC.MSE_MACHINE]
PARITY += [(n, GMM_ON, 'machine') for n in RC.GMM] + [(n, {}, 'launches') for n in RC.GMM]
PARITY += [
    ('gru2_mse_n5', {"PARROT_PM_PIECES": "0"}, 'machine'),  # the whole-K phases
    ('gru3_mse_n5', {"PARROT_PM_PIECES": "0"}, 'machine'),
    ('gru2_mse_n17', {"PARROT_PM_PIECES": "0"}, 'machine'),
    ('gru2_mse_n5', {"PARROT_PM_FBC": "0"}, 'machine'),     # the cut along K with the fed-back frame on the chain
    ('gru2_mse_n17', {"PARROT_PM_FBC": "0"}, 'machine'),
    ('gru1_mse_n5', {"PARROT_PM_ATTFOLD": "0"}, 'machine'),
    ('gru2_mse_n5', {"PARROT_PM_ATTFOLD": "0"}, 'machine'),
    ('gru2_mse_n5', {"PARROT_PM_ATTFOLD": "1"}, 'machine'),
    ('gru2_mse_n5', {"PARROT_PM_DATAFLOW": "0"}, 'machine'),
    ('gru2_mse_n5', {"PARROT_PM_DATAFLOW": "1"}, 'machine'),
    ('gru2_mse_n17', {"PARROT_PM_DATAFLOW": "0", "PARROT_PM_PIECES": "0"}, 'machine'),
    ('gru2_mse_n17', {"PARROT_PM_DATAFLOW": "1", "PARROT_PM_PIECES": "0"}, 'machine'),
    ('lstm2_mse_n17', {"PARROT_PM_DATAFLOW": "0"}, 'machine'),
    ('lstm2_mse_n17', {"PARROT_PM_DATAFLOW": "1"}, 'machine'),
    ('lstm2_k3_n5', dict(GMM_ON, PARROT_PM_DATAFLOW="0"), 'machine'),
    ('lstm2_k3_n5', dict(GMM_ON, PARROT_PM_DATAFLOW="1"), 'machine'),
    ('gru1_k3_n5', dict(GMM_ON, PARROT_PM_DATAFLOW="0"), 'machine'),
    ('gru2_mse_n5', {"PARROT_SAMPLE_PERSIST": "0"}, 'launches'),
    ('gru2_mse_n17', {"PARROT_SAMPLE_PERSIST": "0"}, 'launches'),
    ('lstm2_mse_n17', {"PARROT_SAMPLE_PERSIST": "0"}, 'launches'),
    ('layer_norm', {}, 'launches'),
]


@pytest.mark.parametrize("name, env, path", PARITY, ids=[f"{n}-{'-'.join(k[7:] + v for k, v in e.items()) or 'default'}-{p}"
                                                         for n, e, p in PARITY])
def test_row_controls_match_the_oracle(dev, monkeypatch, name, env, path):
    """All six outputs within 2e-4 of the fp64 oracle with column-tensor controls, on the path the case names.  The oracle's
    run with the model's scalars is 0.2 .. 1.2 away from it (CPU test), so a kernel that ignored the arrays fails here."""
    c = RC.case(name)
    _env(monkeypatch, env)
    m = _model(dev, c)
    outs = _decode(m, c, c['ctl'])
    _on_path(m, c, path)
    _against(outs, c['ref'], f"{name} {env} {path}")
    m.close()


def test_row_controls_with_bf16_operands(dev, monkeypatch):
    """decode_dtype='bf16' (LSTM, L = 2): against the rounded oracle with the same column-tensor controls, at the tolerance
    tests/test_gpu_decode_bf16.py holds its trajectories to (2e-3), and 2e-2 against the exact oracle."""
    from oracle import parrot_ref as R
    from parrot_amd import _lib
    from tests.test_gpu_decode_bf16 import rounded_oracle
    _env(monkeypatch, {})
    c = dict(RC.case('lstm2_mse_n5'))
    c['p'] = {k: v.float().double() for k, v in c['p'].items()}  # (f32-representable: model and oracle round the same weights)
    with torch.no_grad():
        exact = R.sample_model(c['p'], c['cfg'], c['lab'], c['lm'], c['spk'], c['S'])
        with rounded_oracle():
            rnd = R.sample_model(c['p'], c['cfg'], c['lab'], c['lm'], c['spk'], c['S'])
    m = _model(dev, c, decode_dtype='bf16')
    outs = _decode(m, c, c['ctl'])
    ws = _on_path(m, c, 'machine')
    assert _lib.load().parrot_sample_is_bf16(ws['plan']) == 1
    _against(outs, rnd, "bf16 vs rounded oracle", 2e-3)
    _against(outs, exact, "bf16 vs exact oracle", 2e-2)
    m.close()


# ------------------------------------------------------------------------------------------------ 2. / 3. bits
BITS = [('gru2_mse_n5', {}, 'machine'), ('lstm2_k3_n5', GMM_ON, 'machine'),
        ('gru2_mse_n5', {"PARROT_SAMPLE_PERSIST": "0"}, 'launches'), ('lstm2_k3_n5', {}, 'launches')]
BITS_IDS = [f"{n}-{p}" for n, _, p in BITS]


@pytest.mark.parametrize("name, env, path", BITS, ids=BITS_IDS)
def test_same_row_same_bits(dev, monkeypatch, name, env, path):
    """Rows 1 and 2 of the mixed call are bit-identical to the same rows of a call on a model built with that row's three
    values as its scalars (same labels, same randomness), all six outputs."""
    c = RC.case(name)
    _env(monkeypatch, env)
    m = _model(dev, c)
    mixed = _decode(m, c, c['ctl'])
    _on_path(m, c, path)
    m.close()
    for i in (1, 2):
        kw = dict(timing_coeff=c['ctl']['timing'][i], sharpening_coeff=c['ctl']['sharpening'][i])
        if c['gmm']:
            kw['sampling_bias'] = c['ctl']['bias'][i]
        mi = _model(dev, c, **kw)
        alone = _decode(mi, c)
        _on_path(mi, c, path)
        mi.close()
        _same_bits(mixed, alone, f"row {i}", rows=i)
        assert not torch.equal(mixed[0][:, 0], alone[0][:, 0]), "row 0 has other values: the twin must differ there"


@pytest.mark.parametrize("name, env, path", BITS, ids=BITS_IDS)
def test_equal_values_are_the_scalar(dev, monkeypatch, name, env, path):
    """Arrays filled with the model's own scalars and a call without controls give the same bits."""
    c = RC.case(name)
    _env(monkeypatch, env)
    kw = dict(timing_coeff=0.8, sharpening_coeff=1.5, **({'sampling_bias': 0.5} if c['gmm'] else {}))
    N = c['N']
    m = _model(dev, c, **kw)
    plain = _decode(m, c)
    filled = _decode(m, c, dict(timing=[0.8] * N, sharpening=[1.5] * N, bias=[0.5] * N if c['gmm'] else None))
    _on_path(m, c, path)
    _same_bits(plain, filled, "scalars vs arrays of the scalars")
    m.close()


def test_one_hot_speaker_weights_are_the_indexed_speaker(dev, monkeypatch):
    c = RC.case('speaker')
    _env(monkeypatch, {})
    m = _model(dev, c)
    indexed = _decode(m, c, c['ctl'])
    one_hot = torch.nn.functional.one_hot(c['spk'][:, 0].long(), c['full']['num_speakers']).float().numpy()
    blended = _decode(m, c, c['ctl'], speaker_weights=one_hot)
    _on_path(m, c, 'machine')
    _same_bits(indexed, blended, "indexed vs one-hot")
    _against(indexed, c['ref'], "speaker model with controls")
    m.close()


# ------------------------------------------------------------------------------------------------ 4. replay
@pytest.mark.parametrize("name, env, path", BITS, ids=BITS_IDS)
def test_replay_carries_no_stale_values(dev, monkeypatch, name, env, path):
    """One model, one workspace, one captured graph: controls A, controls B, none, A again.  Each equals a fresh model's
    result bit for bit, the fourth equals the first, nothing gave up."""
    cA, cB = RC.case(name), RC.case(name, 'B')
    assert cA['ctl'] != cB['ctl']
    _env(monkeypatch, env)
    m = _model(dev, cA)
    got = [_decode(m, cA, cA['ctl']), _decode(m, cA, cB['ctl']), _decode(m, cA), _decode(m, cA, cA['ctl'])]
    assert len(m._sample_ws) == 1
    _on_path(m, cA, path)
    m.close()
    for i, ctl in enumerate((cA['ctl'], cB['ctl'], None)):
        f = _model(dev, cA)
        fresh = _decode(f, cA, ctl)
        _on_path(f, cA, path)
        f.close()
        _same_bits(got[i], fresh, f"call {i + 1} vs a fresh model")
    _same_bits(got[3], got[0], "fourth vs first")
    if not cA['gmm']:  # (the GMM seeds are conditioned on the first set only: its second set is held to the fresh model's bits)
        _against(got[1], cB['ref'], "second call vs its oracle")
    assert rel_err(got[2][0], got[0][0]) > 0.05, "the call without controls kept the first call's values"


# ------------------------------------------------------------------------------------------------ 5. stop
STOP = dict(N=5, U=9, S=48, texts=[7, 7, 5, 8, 7], kappa_bias=-1.0, extra=8, timing=[1.0, 0.5, 1.25, 0.8, 0.5])


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_stop_at_the_end_of_the_utterance_follows_the_rate(dev, monkeypatch, cell):
    """sample_until_end_device(timing_coeffs=..): lengths are end_of_utterance on the full-length phi of sample_model_device
    with the same controls, the outputs its bit-identical prefix; rows 0, 1 and 4 carry the same labels, mask and
    sharpening, and the two that divide the window's step by 0.5 end earlier than their twin at 1.0.  (Compared in length
    only: through the literal encoder equal label rows do not give equal context rows, in the oracle either.)"""
    from oracle import parrot_ref as R
    from parrot_amd import _lib
    from parrot_amd.utils import end_of_utterance
    _env(monkeypatch, {})
    full = dict(RC.SMALL, cell_type=cell, num_layers=2, weak_feedback=True, which_cost='MSE')
    N, U, S, extra = STOP['N'], STOP['U'], STOP['S'], STOP['extra']
    cfg = R.default_config(**full)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    p['/parrot/h1_to_att/fork_kappa.b'].fill_(STOP['kappa_bias'])
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=9)
    lab[1], lab[4] = lab[0], lab[0]
    for i in range(N):
        lm[i, STOP['texts'][i]:] = 0
    unif, noise = RC.G.randomness(N, cfg['output_dim'], 3, steps=S)
    c = dict(full=full, p=p, lab=lab, lm=lm, spk=spk, N=N, U=U, S=S, unif=unif, noise=noise)
    ctl = dict(timing=STOP['timing'], sharpening=RC.cycle(RC.SHARPENING, N))
    ctl['sharpening'][1] = ctl['sharpening'][4] = ctl['sharpening'][0]
    m = _model(dev, c)
    plain = _decode(m, c, ctl)
    _on_path(m, c, 'machine')
    outs, lengths = m.sample_until_end_device(lab, lm.float(), spk, N, S, extra=extra, **_kw(ctl))
    ws = _on_path(m, c, 'machine', key=('stop', S, N, U, extra))
    ph = plain[4].cpu().numpy()
    own = [end_of_utterance(ph[:, i], min(int(lm[i].sum()), U - 1), S, extra) for i in range(N)]
    print(f"lengths {lengths.tolist()}  rule on the unstopped phi {own}")
    assert lengths.tolist() == own
    assert own[1] < own[0] and own[4] < own[0]
    assert own[0] < S, "the twin at timing 1.0 no longer ends before the cap"
    steps_run = max(own)
    steps = C.c_int(-1)
    lib = _lib.load()
    assert lib.parrot_sample_stops_early(ws['plan']) == 1
    assert lib.parrot_sample_steps_run(ws['plan'], C.byref(steps)) == 0 and steps.value == steps_run
    for o, r, n in zip(outs, plain, RC.NAMES):
        assert o.shape[0] == steps_run, n
        assert torch.equal(o, r[:steps_run]), f"{n}: the stopped run differs from the unstopped run's first {steps_run} steps"
    m.close()


# ------------------------------------------------------------------------------------------------ 6. speaker blend
@pytest.mark.parametrize("env, path", [({}, 'machine'), ({"PARROT_SAMPLE_PERSIST": "0"}, 'launches')])
def test_speaker_blend_matches_the_oracle(dev, monkeypatch, env, path):
    """speaker_weights with a one-hot row, a 50 / 50 row and a row that does not sum to 1: the oracle gets the table
    speaker_weights @ W as its lookuptable.W and speaker = arange(N); all six outputs within 2e-4, controls included."""
    from oracle import parrot_ref as R
    c = RC.case('speaker')
    _env(monkeypatch, env)
    SW = torch.tensor(RC.SPEAKER_WEIGHTS, dtype=torch.float64)
    assert SW[0].tolist().count(1.0) == 1 and SW[1].tolist().count(0.5) == 2 and abs(float(SW[2].sum()) - 1) > 0.1
    p2 = dict(c['p'])
    p2['/parrot/lookuptable.W'] = SW @ c['p']['/parrot/lookuptable.W']
    with torch.no_grad():
        ref = R.sample_model(p2, c['cfg'], c['lab'], c['lm'], torch.arange(c['N']).unsqueeze(1), c['S'])
    assert rel_err(ref[0], c['ref'][0]) > 1e-3, "the blend must decode differently from the indexed speakers"
    m = _model(dev, c)
    outs = _decode(m, c, c['ctl'], speaker_weights=SW.float().numpy())
    _on_path(m, c, path)
    _against(outs, ref, f"speaker blend on the {path}")
    m.close()


# ------------------------------------------------------------------------------------------------ 7. the C entry point
def test_the_symbol_is_declared_and_bound():
    from parrot_amd import _lib
    assert 'parrot_sample_set_row_controls' in _lib.SIGNATURES
    with open(os.path.join(ROOT, 'include', 'parrot_hip.h')) as f:
        assert 'int parrot_sample_set_row_controls(void* plan, const float* timing, const float* sharpening, ' \
               'const float* sampling_bias);' in f.read()


@pytest.mark.parametrize("name, env", [('gru2_mse_n5', {}), ('lstm2_k3_n5', GMM_ON)])
def test_a_plan_without_controls_is_the_scalar_decode_and_the_entry_refuses_late_calls(dev, monkeypatch, name, env):
    """A second plan made from the workspace's own descriptor and never given controls (the kernels without them) decodes
    the same bits as the model's call without controls (the kernels with them, arrays of the scalars).  After its run
    parrot_sample_set_row_controls is refused with PARROT_ERR_BADARG; a bias array on a plan without a GMM head, too."""
    from parrot_amd import _lib, ops
    lib = _lib.load()
    c = RC.case(name)
    _env(monkeypatch, env)
    m = _model(dev, c, timing_coeff=0.8, sharpening_coeff=1.5)
    plain = _decode(m, c)
    ws = _on_path(m, c, 'machine')
    arr = torch.ones(c['N'], device=dev)
    assert lib.parrot_sample_set_row_controls(ws['plan'], arr.data_ptr(), None, None) == BADARG  # (the model's plan has run)
    plan = C.c_void_p()
    assert lib.parrot_sample_create(C.byref(ws['desc']), C.byref(plan)) == 0
    try:
        assert lib.parrot_sample_set_row_controls(None, None, None, None) == BADARG
        if not c['gmm']:
            assert lib.parrot_sample_set_row_controls(plan, None, None, arr.data_ptr()) == BADARG
        assert lib.parrot_sample_set_row_controls(plan, None, None, None) == 0  # (all null: no controls)
        # (the machine leaves the entering states where they were: the outputs are cleared, the inputs are still in place)
        for k in ('phi', 'a') + (('pi_out',) if c['gmm'] else ()):
            ws[k].zero_()
        for k in ('x', 'kappa', 'w'):
            ws[k][1:].zero_()
        assert lib.parrot_sample_run(plan, ops._stream()) == 0
        assert lib.parrot_sample_status(plan) == 0 and _abort_word(ws) == 0
        sx = ws['x'][1:, :, :plain[0].shape[2]]
        again = [sx, ws['kappa'][1:], ws['w'][1:], ws['pi_out'] if c['gmm'] else sx, ws['phi'], ws['a']]
        _same_bits(plain, again, "plan without controls vs the model's call")
        assert lib.parrot_sample_set_row_controls(plan, arr.data_ptr(), arr.data_ptr(), None) == BADARG  # after a run
    finally:
        lib.parrot_sample_destroy(plan)
    m.close()


def test_partial_controls_through_the_entry(dev, monkeypatch):
    """Only `timing` given: sharpening stays the descriptor's scalar (the plan's own array of it)."""
    from parrot_amd import _lib, ops
    lib = _lib.load()
    c = RC.case('gru2_mse_n5')
    _env(monkeypatch, {})
    m = _model(dev, c, sharpening_coeff=1.5)
    want = _decode(m, c, dict(timing=c['ctl']['timing'], sharpening=[1.5] * c['N']))
    ws = _on_path(m, c, 'machine')
    timing = torch.tensor(c['ctl']['timing'], device=dev)
    plan = C.c_void_p()
    assert lib.parrot_sample_create(C.byref(ws['desc']), C.byref(plan)) == 0
    try:
        assert lib.parrot_sample_set_row_controls(plan, timing.data_ptr(), None, None) == 0
        for k in ('phi', 'a'):
            ws[k].zero_()
        for k in ('x', 'kappa', 'w'):
            ws[k][1:].zero_()
        assert lib.parrot_sample_run(plan, ops._stream()) == 0
        assert lib.parrot_sample_status(plan) == 0
        sx = ws['x'][1:, :, :want[0].shape[2]]
        _same_bits(want, [sx, ws['kappa'][1:], ws['w'][1:], sx, ws['phi'], ws['a']], "timing only")
    finally:
        lib.parrot_sample_destroy(plan)
    m.close()


# ------------------------------------------------------------------------------------------------ 8. sample.py
def _experiment(tmp_path, monkeypatch, name, extra):
    monkeypatch.setenv("RESULTS_DIR", str(tmp_path))
    sys.path.insert(0, ROOT)
    import importlib
    train = importlib.import_module("train")
    train.main(["--experiment_name", name, "--rnn_h_dim", "64", "--readouts_dim", "64", "--batch_size", "4", "--seq_size", "20",
                "--num_layers", "1", "--labels_type", "text", "--synthetic_examples", "8", "--save_every", "2", "--max_steps", "2",
                "--save_dir", str(tmp_path), "--weak_feedback", "1"] + extra)
    return importlib.import_module("sample")


def _api_model(tmp_path, name, dev, N, S):
    """The model and the batch sample.py builds for the experiment, through the same calls."""
    import pickle

    from parrot_amd.checkpoint import load_parameters
    from parrot_amd.datasets import parrot_stream
    from parrot_amd.model import Parrot
    with open(os.path.join(str(tmp_path), 'vctk', 'config', name + '.pkl'), 'rb') as f:
        sa = pickle.load(f)
    params = load_parameters(os.path.join(str(tmp_path), 'vctk', 'pkl', 'best_' + name + '.tar'))
    stream = parrot_stream('vctk', sa.use_speaker, ('test',), N, S, sorting_mult=1, labels_type=sa.labels_type, raw_data=False,
                           num_examples=64)
    data = next(stream.get_epoch_iterator(as_dict=True))
    m = Parrot(input_dim=sa.input_dim, output_dim=sa.output_dim, rnn_h_dim=sa.rnn_h_dim, readouts_dim=sa.readouts_dim,
               weak_feedback=sa.weak_feedback, full_feedback=sa.full_feedback, feedback_noise_level=None, layer_norm=sa.layer_norm,
               use_speaker=sa.use_speaker, num_speakers=sa.num_speakers, speaker_dim=sa.speaker_dim, which_cost=sa.which_cost,
               num_characters=sa.num_characters, attention_type=sa.attention_type, attention_alignment=sa.attention_alignment,
               sampling_bias=1., sharpening_coeff=1., timing_coeff=1., encoder_type=sa.encoder_type, name='parrot',
               num_layers=getattr(sa, 'num_layers', 3), cell_type=getattr(sa, 'cell_type', 'gru'), encoder_literal=bool(getattr(sa, 'encoder_literal', 1)),
               device=dev).allocate()
    m.set_parameter_values(params)
    return m, data


def test_sample_py_passes_the_list_flags(dev, tmp_path, monkeypatch):
    _env(monkeypatch, {})
    sample = _experiment(tmp_path, monkeypatch, "rows", [])
    N, S = 3, 24
    base = ["--experiment_name", "rows", "--num_samples", str(N), "--num_steps", str(S), "--save_dir", str(tmp_path)]
    plain, _ = sample.main(base)
    got, _ = sample.main(base + ["--timing_coeffs", "1,0.5,2", "--sharpening_coeffs", "1,1.5,0.7"])
    assert got.shape == plain.shape == (N, S, 63)
    assert np.array_equal(got[0], plain[0]) and not np.array_equal(got[1], plain[1]) and not np.array_equal(got[2], plain[2])
    m, data = _api_model(tmp_path, "rows", dev, N, S)
    api = m.sample_model(data['labels'], data['labels_mask'], data.get('features_mask'), data.get('speaker_index'), N, S,
                         timing_coeffs=[1, 0.5, 2], sharpening_coeffs=[1, 1.5, 0.7])[0].swapaxes(0, 1)
    assert np.array_equal(got, api)
    m.close()
    with pytest.raises(SystemExit, match="2 values"):
        sample.main(base + ["--timing_coeffs", "1,0.5"])


def test_sample_py_honours_mix(dev, tmp_path, monkeypatch, capsys):
    from parrot_amd.utils import mix_speaker_weights
    _env(monkeypatch, {})
    sample = _experiment(tmp_path, monkeypatch, "spk", ["--use_speaker", "1", "--num_speakers", "22", "--speaker_dim", "16"])
    N, S = 3, 24
    base = ["--experiment_name", "spk", "--num_samples", str(N), "--num_steps", str(S), "--save_dir", str(tmp_path)]
    plain, _ = sample.main(base)
    capsys.readouterr()
    mixed, _ = sample.main(base + ["--mix", "0.5"])
    assert "0.5 * speaker 15 + 0.5 * speaker 11" in capsys.readouterr().out
    assert not np.array_equal(mixed, plain)
    m, data = _api_model(tmp_path, "spk", dev, N, S)
    table = m._p('/lookuptable.W').clone()
    api = m.sample_model(data['labels'], data['labels_mask'], data.get('features_mask'), data.get('speaker_index'), N, S,
                         speaker_weights=mix_speaker_weights(0.5, (15, 11), 22, N))[0].swapaxes(0, 1)
    assert np.array_equal(mixed, api)
    assert torch.equal(table, m._p('/lookuptable.W')), "the speaker table was modified"
    m.close()
    other, _ = sample.main(base + ["--mix", "0.5", "--mix_speakers", "3,7"])
    assert not np.array_equal(other, mixed)
