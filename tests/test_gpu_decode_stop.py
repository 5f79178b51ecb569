"""Decode that stops at the end of the utterance inside the persistent machine (persist.hip: PmAtt::eou_*, the stop word of
the sync area; Parrot.sample_until_end_device).  A stopped launch executes a prefix of the ticks of the unstopped one, so
every check here is exact: the lengths are end_of_utterance's on the unstopped run's own phi (and the fp64 oracle's -- the
deciding comparisons have relative margins of 5e-3 and more, thousands of times the f32 decode error), the kernel really
left at T_stop (parrot_sample_steps_run), and every returned tensor equals the unstopped run's first T_stop steps bit for
bit, in every machine program."""
import ctypes as C
import functools

import pytest
import torch

from tests.test_gpu_decode_lstm import NAMES, SMALL
from tests.util import make_batch

pytestmark = pytest.mark.gpu

EXTRA = 8
GRU = dict(SMALL, cell_type='gru')
# name -> (model keywords, N, U, S, text lengths (cycled over the rows), fork_kappa.b, lengths of the rows on the oracle)
CASES = {
    'A': (dict(GRU, num_layers=2, weak_feedback=True), 5, 9, 48, [9, 7, 5, 8, 3], -1.0, [20, 29, 15, 32, 12]),
    'B': (dict(SMALL, num_layers=2, weak_feedback=True), 5, 9, 48, [9, 7, 5, 8, 3], -1.0, [22, 22, 18, 29, 13]),
    'C': (dict(GRU, num_layers=1), 5, 9, 48, [9, 7, 5, 8, 3], -1.0, [26, 38, 19, 48, 15]),
    'D': (dict(GRU, num_layers=3, full_feedback=True, use_speaker=True), 5, 9, 48, [9, 7, 5, 8, 3], -1.0,
          [20, 18, 19, 28, 12]),
    'E': (dict(GRU, num_layers=2, weak_feedback=True), 37, 12, 64, [12, 10, 7, 4, 11, 2, 1], -1.0, None),
    'F': (dict(GRU, num_layers=2, weak_feedback=True), 5, 9, 48, [9, 7, 5, 8, 3], -3.0, [48, 48, 48, 48, 48]),
}


def _lengths_of(phi, lm, S):
    """end_of_utterance, as sample.py applies it, on a time-major phi [S, N, U]."""
    from parrot_amd.utils import end_of_utterance
    ph = phi.detach().cpu().numpy()
    U = ph.shape[2]
    return [end_of_utterance(ph[:, i], min(int(lm[i].sum()), U - 1), S, EXTRA) for i in range(ph.shape[1])]


@functools.lru_cache(maxsize=None)
def _case(name, text=None):
    """Parameters, batch and the oracle's row lengths of a case (computed once per session, never modified)."""
    from oracle import parrot_ref as R
    full, N, U, S, lens, bias, want = CASES[name]
    lens = list(text) if text is not None else lens
    cfg = R.default_config(**full)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    p['/parrot/h1_to_att/fork_kappa.b'].fill_(bias)
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=9, speaker=cfg['use_speaker'])
    for i in range(N):
        lm[i, lens[i % len(lens)]:] = 0
    with torch.no_grad():
        ref = R.sample_model(p, cfg, lab, lm, spk, S)
    return dict(full=full, p=p, lab=lab, lm=lm, spk=spk, N=N, U=U, S=S, oracle=_lengths_of(ref[4], lm, S),
                want=want if text is None else None)


def _model(dev, c, params=True, **kw):
    from parrot_amd.model import Parrot
    m = Parrot(device=dev, use_graph=True, **dict(c['full'], **kw)).allocate()
    if params:
        m.set_parameter_values(c['p'])
    return m


def _stopped_against_plain(m, c, oracle=True):
    """One unstopped and one stopped call on `m`; every assertion of the module's docstring.  Returns the lengths."""
    from parrot_amd import _lib
    N, U, S = c['N'], c['U'], c['S']
    lm = c['lm'].float()
    plain = [o.clone() for o in m.sample_model_device(c['lab'], lm, c['spk'], N, S)]
    outs, lengths = m.sample_until_end_device(c['lab'], lm, c['spk'], N, S, extra=EXTRA)
    lengths = lengths.tolist()
    own = _lengths_of(plain[4], c['lm'], S)
    print(f"lengths {lengths}  rule on the unstopped phi {own}  oracle {c['oracle']}")
    assert lengths == own
    if oracle:
        assert lengths == c['oracle']
    T_stop = max(own)
    ws = m._sample_ws[('stop', S, N, U, EXTRA)]
    lib = _lib.load()
    assert lib.parrot_sample_is_persistent(ws['plan']) != 0 and lib.parrot_sample_stops_early(ws['plan']) == 1
    steps = C.c_int(-1)
    assert lib.parrot_sample_steps_run(ws['plan'], C.byref(steps)) == 0
    assert steps.value == T_stop, "the kernel did not leave at T_stop"
    for o, r, n in zip(outs, plain, NAMES):
        assert o.shape[0] == T_stop, n
        assert torch.equal(o, r[:T_stop]), f"{n}: the stopped run differs from the unstopped run's first {T_stop} steps"
    assert int(ws['pm']['ws'][832:833].view(torch.int32).item()) == 0, "a spin timed out inside the machine"
    assert lib.parrot_sample_status(ws['plan']) == 0
    plain_ws = m._sample_ws[(S, N, U)]
    assert lib.parrot_sample_stops_early(plain_ws['plan']) == 0
    assert lib.parrot_sample_steps_run(plain_ws['plan'], C.byref(steps)) == 0 and steps.value == S
    return lengths


def _premise(c):
    if c['want'] is not None:
        assert c['oracle'] == c['want'], "the case no longer ends where it was designed to"


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_stopped_run_is_a_bit_identical_prefix(dev, name):
    """A, B, D: every row fires before the cap.  C: one row reaches the cap (steps_run == S).  E: 37 rows in three row
    blocks, a text of one character fires at step 0, T_stop 46 of 64."""
    c = _case(name)
    _premise(c)
    if name == 'E':
        assert min(c['oracle']) == 8 and max(c['oracle']) == 46 and all(n < c['S'] for n in c['oracle'])
    m = _model(dev, c)
    lengths = _stopped_against_plain(m, c)
    assert max(lengths) == {'A': 32, 'B': 29, 'C': 48, 'D': 28, 'E': 46}[name]
    m.close()


@pytest.mark.parametrize("env", [("PARROT_PM_FBC", "0"), ("PARROT_PM_PIECES", "0"), ("PARROT_PM_DATAFLOW", "0"),
                                 ("PARROT_PM_DATAFLOW", "1")])
def test_every_gru_program_stops_at_the_same_tick(dev, monkeypatch, env):
    """Case A on the step cut along K without the fed-back frame out of the chain, on the whole-K phases, with and without
    grid barriers: each against its own unstopped run."""
    from parrot_amd import _lib
    monkeypatch.setenv(*env)
    c = _case('A')
    _premise(c)
    m = _model(dev, c)
    assert max(_stopped_against_plain(m, c)) == 32
    kind = _lib.load().parrot_sample_is_persistent(m._sample_ws[('stop', c['S'], c['N'], c['U'], EXTRA)]['plan'])
    if env == ("PARROT_PM_FBC", "0"):
        assert kind == 2
    if env == ("PARROT_PM_PIECES", "0"):
        assert kind == 1
    m.close()


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_lstm_programs_stop(dev, dtype):
    """Case B with f32 and with bf16 operands.  The bf16 decode is another function of the weights, so its lengths are
    checked against its own unstopped run only."""
    c = _case('B')
    _premise(c)
    m = _model(dev, c, decode_dtype=dtype)
    lengths = _stopped_against_plain(m, c, oracle=dtype == 'float32')
    assert max(lengths) < c['S']
    m.close()


LONG = dict(rnn_h_dim=1024, readouts_dim=1024, encoder_type='bidirectional', cell_type='gru', num_layers=2,
            weak_feedback=True)
LONG_TEXTS = [300, 200, 150, 260, 130]


@functools.lru_cache(maxsize=None)
def _long_text_case():
    from oracle import parrot_ref as R
    N, U, S = 5, 300, 64
    cfg = R.default_config(**LONG)
    p = R.init_params(cfg, seed=7, scale_by_fan_in=True)
    p['/parrot/h1_to_att/fork_kappa.b'].fill_(2.0)
    _, _, lab, lm, spk = make_batch(cfg, 2, N, U, seed=9)
    for i in range(N):
        lm[i, LONG_TEXTS[i]:] = 0
    return dict(full=LONG, p=p, lab=lab, lm=lm, spk=spk, N=N, U=U, S=S, oracle=None, want=None)


def test_long_texts_where_the_row_shares_its_lds_with_the_next_unit(dev, monkeypatch):
    """U = 300, texts of 130 .. 300 characters: the rule compares positions far beyond 112, the part of the row's phi in LDS
    that the split-K partial tiles of the workgroup's NEXT unit overwrite (waves 1 .. 3 write lds_red from float 320 on, phi
    starts at 208).  2 x GRU-1024: 388 critical GEMM units on at most 256 workgroups, so every workgroup that owns an
    attention row also owns GEMM units, and the program runs without grid barriers (the default of the step cut along K):
    only the row's own last barrier keeps the other waves off its phi until the predicate has read it.
    The reference is the unstopped run of the same program, exactly; the fp64 oracle is none here: with the window moving
    this fast through a randomly initialised 1024-wide decoder the decode is chaotic -- the f32 paths, machine and per-step
    launches alike, leave the oracle by a factor of ~20 every four steps (kappa: 1e-7 at step 0, 4e-3 at step 16, measured
    on the MI355X), so the oracle's firing steps (lengths 51, 49, 43, 45, 37) are not the f32 decode's (50, 31, 33, 45, 37
    on the machine, 50, 40, 43, 64, 37 on the launches)."""
    from parrot_amd import _lib
    from parrot_amd.utils import end_of_utterance_args
    monkeypatch.delenv("PARROT_PM_DATAFLOW", raising=False)
    c = _long_text_case()
    pos, ncmp = end_of_utterance_args(c['lm'].numpy(), c['U'])
    assert ncmp.min() > 112 and pos.min() > 112
    m = _model(dev, c)
    lengths = _stopped_against_plain(m, c, oracle=False)
    assert max(lengths) < c['S'], "no row-dependent stop: the case no longer ends before the cap"
    ws = m._sample_ws[('stop', c['S'], c['N'], c['U'], EXTRA)]
    # (the step cut along K; it runs without grid barriers unless PARROT_PM_DATAFLOW says otherwise)
    assert _lib.load().parrot_sample_is_persistent(ws['plan']) >= 2
    m.close()


def test_rows_that_never_fire_run_to_the_cap(dev):
    """Case F: four rows never fire, so no stop tick is ever published: S frames, bit-identical to the plain run."""
    c = _case('F')
    _premise(c)
    m = _model(dev, c)
    assert _stopped_against_plain(m, c) == [48] * 5
    m.close()


def test_replay_on_one_workspace_follows_the_new_texts(dev):
    """Two stopped calls on one workspace (one captured graph) with different text lengths: the second call's lengths
    follow the new texts (the launch preamble resets the rows' first steps, the stop word and the tick record).  The plain
    decode of the same model is untouched by the stopping plan beside it."""
    c1, c2 = _case('A'), _case('A', text=(4, 9, 6, 3, 8))
    assert c1['oracle'] != c2['oracle']
    m = _model(dev, c1)
    before = [o.clone() for o in m.sample_model_device(c1['lab'], c1['lm'].float(), c1['spk'], c1['N'], c1['S'])]
    l1 = _stopped_against_plain(m, c1)
    l2 = _stopped_against_plain(m, c2)
    assert l1 == c1['oracle'] and l2 == c2['oracle']
    assert len([k for k in m._sample_ws if k[0] == 'stop']) == 1
    after = m.sample_model_device(c1['lab'], c1['lm'].float(), c1['spk'], c1['N'], c1['S'])
    for a, b, n in zip(after, before, NAMES):
        assert torch.equal(a, b), n
    m.close()


@pytest.mark.parametrize("kw,env,extra,word", [
    (dict(which_cost='GMM', k_gmm=3), None, EXTRA, 'GMM'),
    (dict(layer_norm=True), None, EXTRA, 'layer_norm'),
    (dict(), ("PARROT_SAMPLE_PERSIST", "0"), EXTRA, 'PARROT_SAMPLE_PERSIST'),
    (dict(), None, 4, 'extra >= 8'),
    (dict(), None, 0, 'extra >= 8'),
])
def test_refusals_raise_and_leave_no_workspace(dev, monkeypatch, kw, env, extra, word):
    if env:
        monkeypatch.setenv(*env)
    c = _case('A')
    m = _model(dev, c, params=False, **kw)  # (refused before any parameter is read)
    with pytest.raises(ValueError, match=word):
        m.sample_until_end_device(c['lab'], c['lm'].float(), c['spk'], c['N'], c['S'], extra=extra)
    assert not m._sample_ws
    m.close()


def test_the_library_refuses_what_python_would_let_through(dev, monkeypatch):
    """The C ABI itself refuses a descriptor that asks for the stop and gets no machine plan (here: extra below the bound),
    instead of running all S steps or the per-step launches."""
    c = _case('A')
    m = _model(dev, c)
    monkeypatch.setattr(m, '_decode_stop_refusal', lambda N, extra: '')
    with pytest.raises(ValueError, match='did not build'):
        m.sample_until_end_device(c['lab'], c['lm'].float(), c['spk'], c['N'], c['S'], extra=4)
    assert not m._sample_ws
    m.close()
