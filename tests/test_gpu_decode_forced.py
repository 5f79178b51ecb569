"""Forced frames on the GPU (Parrot.sample_model*(forced_frames=, n_forced=); ParrotSampleForcedDesc::forced / n_forced / own_x;
pm_gemm / pm_sample_row with FRC in persist_forced.hip, frame_force_kernel on the launches): all seven outputs against the
forced fp64 oracle on every decode program and on the launches, a decode that ignored the forcing caught, the fixed point
that shows every slab copy holds the row-major frame's bits, replay without stale values, the end-of-utterance stop, the
row controls on top, sample.py --prime_frames.  The cases and their premise: tests/decode_forced_cases.py,
tests/test_decode_forced_cpu.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import decode_forced_cases as FC
from tests import decode_row_controls_cases as RC
from tests.test_gpu_decode_row_controls import TOL, _abort_word, _api_model, _env, _experiment, _model
from tests.util import assert_close, make_batch, rel_err

pytestmark = pytest.mark.gpu

GMM_ON = {"PARROT_PM_GMM": "1"}
OFF = {"PARROT_SAMPLE_PERSIST": "0"}
# (case, switches, path): every path that decodes the cases -- the machine for the MSE cases (the cut along K; LSTM stacks),
# the machine with PARROT_PM_GMM=1 for the GMM cases, the launches under PARROT_SAMPLE_PERSIST=0 and for layer_norm; then the
# other programs and hand-offs of the machine: the whole-K GRU phases, grid barriers and dataflow each way
RUNS = [(n, {}, 'machine') for n in FC.MSE_MACHINE]
RUNS += [(n, GMM_ON, 'machine') for n in FC.GMM]
RUNS += [('gru2_mse_n5', OFF, 'launches'), ('lstm2_mse_n17', OFF, 'launches'), ('gru1_k3_n5', OFF, 'launches'),
         ('lstm2_k3_n5', OFF, 'launches'), ('layer_norm', {}, 'launches')]
RUNS += [
    ('gru2_mse_n5', {"PARROT_PM_PIECES": "0"}, 'machine'),
    ('gru2_mse_n17', {"PARROT_PM_PIECES": "0", "PARROT_PM_DATAFLOW": "1"}, 'machine'),
    ('gru2_mse_n17', {"PARROT_PM_DATAFLOW": "0"}, 'machine'),
    ('gru2_mse_n5', {"PARROT_PM_ATTFOLD": "0"}, 'machine'),
    ('lstm2_mse_n17', {"PARROT_PM_DATAFLOW": "0"}, 'machine'),
    ('lstm2_k3_n5', dict(GMM_ON, PARROT_PM_DATAFLOW="0"), 'machine'),
    ('gru1_k3_n5', dict(GMM_ON, PARROT_PM_DATAFLOW="1"), 'machine'),
]
IDS = [f"{n}-{'-'.join(k[7:] + v for k, v in e.items()) or 'default'}-{p}" for n, e, p in RUNS]
runs = pytest.mark.parametrize("name, env, path", RUNS, ids=IDS)


def _key(c, forced, stop=0):
    k = ('stop', c['S'], c['N'], c['U'], stop) if stop else (c['S'], c['N'], c['U'])
    return (('forced',) + k) if forced else k


def _decode(m, c, frames=None, n=None):
    """One call; frames None: without forcing (six outputs), else seven."""
    kw = {} if frames is None else dict(forced_frames=frames, n_forced=n)
    outs = m.sample_model_device(c['lab'], c['lm'].float(), c['spk'], c['N'], c['S'], unif=c['unif'].float(),
                                 noise=c['noise'].float(), **kw)
    assert len(outs) == (6 if frames is None else 7)
    return [o.clone() for o in outs]


def _on_path(m, c, path, forced=True, stop=0):
    from parrot_amd import _lib
    lib = _lib.load()
    ws = m._sample_ws[_key(c, forced, stop)]
    assert m.decode_path == path
    assert (lib.parrot_sample_is_persistent(ws['plan']) != 0) == (path == 'machine')
    if path == 'machine':
        assert _abort_word(ws) == 0, "a spin timed out inside the machine"
    assert lib.parrot_sample_status(ws['plan']) == 0
    return ws


def _against(outs, ref, tag, tol=TOL):
    assert len(outs) == len(ref)
    for o, r, n in zip(outs, ref, FC.NAMES):
        assert tuple(o.shape) == tuple(r.shape), n
        print(f"{tag}: {n} {rel_err(o, r):.3e}")
    for o, r, n in zip(outs, ref, FC.NAMES):
        assert_close(o, r, tol, f"{tag}: {n}")


def _same_bits(a, b, tag):
    assert len(a) == len(b)
    for x, y, n in zip(a, b, FC.NAMES):
        assert torch.equal(x, y), f"{tag}: {n} differs"


_RUN = {}  # (case, switches) -> the seven outputs of the forced run with set 'A': tests 1 and 2 look at the same run


def _forced_run(dev, monkeypatch, name, env, path):
    key = (name, tuple(sorted(env.items())))
    if key not in _RUN:
        c = FC.case(name)
        _env(monkeypatch, env)
        m = _model(dev, c)
        outs = _decode(m, c, c['forced'].float(), c['n'])
        _on_path(m, c, path)
        m.close()
        _RUN[key] = [o.cpu() for o in outs]
    return _RUN[key]


# ------------------------------------------------------------------------------------------------ 1. oracle parity
@runs
def test_forced_run_matches_the_forced_oracle(dev, monkeypatch, name, env, path):
    """All seven outputs within 2e-4 of the forced fp64 oracle; under the prompt sample_x is the given frames exactly."""
    c = FC.case(name)
    outs = _forced_run(dev, monkeypatch, name, env, path)
    _against(outs, c['ref'], f"{name} {env} {path}")
    under = ~FC.free_region(c)
    assert torch.equal(outs[0][under], c['forced'].float()[under]), "sample_x under the prompt is not the given frames"
    assert torch.equal(outs[0][~under], outs[6][~under]), "behind the prompt sample_x is the model's own frame"


# ------------------------------------------------------------------------------------------------ 2. ignored forcing is caught
@runs
def test_forced_run_is_far_from_the_free_oracle(dev, monkeypatch, name, env, path):
    """The same run against the oracle WITHOUT forcing: more than 0.05 away on sample_x, and behind the prompt alone -- so a
    build that ignored the arguments could not pass test 1."""
    c = FC.case(name)
    outs = _forced_run(dev, monkeypatch, name, env, path)
    free = FC.free_region(c)
    e_all, e_free = rel_err(outs[0], c['free'][0]), rel_err(outs[0][free], c['free'][0][free])
    print(f"{name} {env} {path}: sample_x vs the free oracle {e_all:.3e}, behind the prompt {e_free:.3e}")
    assert e_all > 0.05 and e_free > 0.05


# ------------------------------------------------------------------------------------------------ 3. fixed point
@runs
def test_forcing_a_run_with_its_own_frames_is_a_fixed_point(dev, monkeypatch, name, env, path):
    """A forced plan with all n = 0, then the same plan with forced = its own_x and n = S: all seven outputs bit-identical.
    The layers of the second run read the forced frame from the slab copies, so every copy holds the row-major frame's bits."""
    c = FC.case(name)
    _env(monkeypatch, env)
    m = _model(dev, c)
    first = _decode(m, c, c['forced'].float(), [0] * c['N'])
    assert torch.equal(first[6], first[0])
    second = _decode(m, c, first[6], [c['S']] * c['N'])
    assert len(m._sample_ws) == 1
    _on_path(m, c, path)
    m.close()
    _same_bits(first, second, "n = 0 vs forced with its own frames")
    _against(first[:6], c['free'], f"{name} {env} {path}: the forced plan with n = 0 vs the free oracle")


# ------------------------------------------------------------------------------------------------ 4. replay
@runs
def test_replay_carries_no_stale_values(dev, monkeypatch, name, env, path):
    """One model: set A, set B (other frames, other lengths) on the same plan, then a call without forcing, then A again.
    Each run is held to its own oracle, the fourth equals the first bit for bit."""
    cA, cB = FC.case(name), FC.case(name, 'B')
    assert cA['n'] != cB['n'] and not torch.equal(cA['forced'], cB['forced'])
    _env(monkeypatch, env)
    m = _model(dev, cA)
    a1 = _decode(m, cA, cA['forced'].float(), cA['n'])
    b = _decode(m, cA, cB['forced'].float(), cB['n'])
    _on_path(m, cA, path)
    free = _decode(m, cA)
    _on_path(m, cA, path, forced=False)
    a2 = _decode(m, cA, cA['forced'].float(), cA['n'])
    assert sorted(map(str, m._sample_ws)) == sorted(map(str, (_key(cA, True), _key(cA, False))))
    m.close()
    _against(a1, cA['ref'], "first call")
    _against(b, cB['ref'], "second call")
    _against(free, cA['free'], "call without forcing")
    _same_bits(a1, a2, "fourth vs first")
    under = ~FC.free_region(cB)
    assert torch.equal(b[0].cpu()[under], cB['forced'].float()[under])


# ------------------------------------------------------------------------------------------------ 5. stop
STOP = dict(N=5, U=9, S=48, texts=[7, 7, 5, 8, 7], kappa_bias=-1.0, extra=8)


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_stop_at_the_end_of_the_utterance_with_forcing(dev, monkeypatch, cell):
    """sample_until_end_device(forced_frames=..): lengths are end_of_utterance on the phi of the unstopped forced run (the
    rule reads phi only), the seven outputs its bit-identical prefix."""
    from oracle import parrot_ref as R
    from parrot_amd import _lib
    from parrot_amd.utils import end_of_utterance
    _env(monkeypatch, {})
    full = dict(FC.SMALL, cell_type=cell, num_layers=2, weak_feedback=True, which_cost='MSE')
    N, U, S, extra = STOP['N'], STOP['U'], STOP['S'], STOP['extra']
    cfg = R.default_config(**full)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    p['/parrot/h1_to_att/fork_kappa.b'].fill_(STOP['kappa_bias'])
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=9)
    for i in range(N):
        lm[i, STOP['texts'][i]:] = 0
    unif, noise = FC.G.randomness(N, cfg['output_dim'], 3, steps=S)
    c = dict(full=full, p=p, lab=lab, lm=lm, spk=spk, N=N, U=U, S=S, unif=unif, noise=noise)
    g = torch.Generator().manual_seed(5)
    frames = torch.randn(S, N, cfg['output_dim'], generator=g) * 0.5
    n = [0, 4, 1, 20, 12]
    m = _model(dev, c)
    plain = _decode(m, c, frames, n)
    _on_path(m, c, 'machine')
    outs, lengths = m.sample_until_end_device(lab, lm.float(), spk, N, S, extra=extra, forced_frames=frames, n_forced=n)
    ws = _on_path(m, c, 'machine', stop=extra)
    ph = plain[4].cpu().numpy()
    own = [end_of_utterance(ph[:, i], min(int(lm[i].sum()), U - 1), S, extra) for i in range(N)]
    print(f"lengths {lengths.tolist()}  rule on the unstopped phi {own}")
    assert lengths.tolist() == own
    assert max(own) < S, "no row ends before the cap: the stop is not exercised"
    steps_run, steps = max(own), C.c_int(-1)
    lib = _lib.load()
    assert lib.parrot_sample_stops_early(ws['plan']) == 1
    assert lib.parrot_sample_steps_run(ws['plan'], C.byref(steps)) == 0 and steps.value == steps_run
    assert len(outs) == 7
    for o, r, nm in zip(outs, plain, FC.NAMES):
        assert o.shape[0] == steps_run, nm
        assert torch.equal(o, r[:steps_run]), f"{nm}: the stopped run differs from the unstopped run's first {steps_run} steps"
    k = min(12, steps_run)
    assert torch.equal(outs[0][:k, 4], frames[:k, 4].to(dev)), "row 4's prompt is not in the stopped run's frames"
    m.close()


# ------------------------------------------------------------------------------------------------ 6. row controls on top
@pytest.mark.parametrize("env, path", [({}, 'machine'), (OFF, 'launches')])
def test_row_controls_together_with_forcing(dev, monkeypatch, env, path):
    c = FC.case_with_controls('gru2_mse_n5')
    _env(monkeypatch, env)
    m = _model(dev, c)
    ctl = c['ctl']
    outs = m.sample_model_device(c['lab'], c['lm'].float(), c['spk'], c['N'], c['S'], timing_coeffs=ctl['timing'],
                                 sharpening_coeffs=ctl['sharpening'], forced_frames=c['forced'].float(), n_forced=c['n'])
    _on_path(m, c, path)
    _against(outs, c['ref'], f"controls and forcing on the {path}")
    m.close()


# ------------------------------------------------------------------------------------------------ 7. sample.py
def test_sample_py_prime_frames(dev, tmp_path, monkeypatch):
    """--prime_frames 3 on the synthetic dataset: the frames sample.py returns and writes start with each utterance's own
    first three feature frames, the rest is the call's through the API; with --phrase the flag is an error."""
    from parrot_amd.utils import prime_frames
    _env(monkeypatch, {})
    sample = _experiment(tmp_path, monkeypatch, "prime", [])
    N, S = 3, 24
    base = ["--experiment_name", "prime", "--num_samples", str(N), "--num_steps", str(S), "--save_dir", str(tmp_path)]
    plain, _ = sample.main(base)
    got, lengths = sample.main(base + ["--prime_frames", "3"])
    m, data = _api_model(tmp_path, "prime", dev, N, S)
    feats = np.asarray(data['features'], dtype=np.float32)
    assert got.shape == plain.shape == (N, S, 63) and feats.shape[0] >= 3
    for i in range(N):
        assert np.array_equal(got[i, :3], feats[:3, i]), f"utterance {i} does not start with its own frames"
        assert not np.array_equal(got[i, 3:], plain[i, 3:]), f"utterance {i} continues as if it had not been primed"
        written = np.load(os.path.join(str(tmp_path), 'vctk', 'samples', f'best_sample_{i}.npy'))
        k = min(3, lengths[i])
        assert written.shape[0] == lengths[i] and np.array_equal(written[:k], feats[:k, i])
    fr, n = prime_frames(data['features'], data['features_mask'], 3, S)
    assert n.tolist() == [3] * N
    api = m.sample_model(data['labels'], data['labels_mask'], data.get('features_mask'), data.get('speaker_index'), N, S,
                         forced_frames=fr, n_forced=n)
    assert len(api) == 7 and np.array_equal(got, api[0].swapaxes(0, 1))
    m.close()
    with pytest.raises(SystemExit, match="--phrase"):
        sample.main(base + ["--prime_frames", "3", "--phrase", "abc"])
