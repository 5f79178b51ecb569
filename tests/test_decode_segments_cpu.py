"""The premise of tests/test_gpu_decode_segments.py, and everything of the resumable decode that needs no device: the carry
oracle of tests/decode_segment_cases.py chained over any cut IS the one-piece loop; the state's width; the new entries of
the C ABI; a carry workspace plans the program that keeps the fed-back frame on the chain and every other configuration's
own; DecodeState; the refusals, before anything is allocated; the segment-level end-of-utterance rule against
utils.end_of_utterance; sample.py's flag."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import decode_forced_cases as FC
from tests import decode_plan_cases as P
from tests import decode_segment_cases as SC
from tests import decode_workspace_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("parrot_sample_state_floats", "parrot_sample_save_state", "parrot_sample_load_state")


# ---------------------------------------------------------------------------------------------------- the carry oracle
@pytest.mark.parametrize("name", ["gru2_mse_n5", "lstm2_k3_n5", "layer_norm"])
def test_without_an_entering_carry_the_loop_is_forced_loop(name):
    c = FC.case(name)
    free, _, _ = SC.one_piece(name)
    forced, _, _ = SC.one_piece(name, forced=True)
    for a, b, n in zip(free[:6], c['free'], SC.NAMES):
        assert torch.equal(a, b), n
    for a, b, n in zip(forced, c['ref'], SC.NAMES):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("name", ["gru2_mse_n5", "gru1_k3_n5", "lstm2_k3_n5", "lstm2_mse_n17", "layer_norm"])
@pytest.mark.parametrize("cuts", [SC.CUTS, [4, 8, 10], [3, 10]], ids=["1-4-10", "4-8-10", "3-10"])
@pytest.mark.parametrize("forced", [False, True], ids=["free", "forced"])
def test_chained_segments_equal_the_one_piece_loop(name, cuts, forced):
    """float64, torch.equal: every output and the leaving carry.  Set 'A' has prompts of 4, 1, S and S - 1 frames, so with
    the cut at 3 (and at 1, 4, 8) prompts straddle cuts."""
    c = FC.case(name)
    assert any(0 < t < n for n in c['n'] for t in cuts), "no prompt straddles a cut"
    ref, carry, packed = SC.one_piece(name, forced)
    outs, last = SC.chain(c, cuts, forced)
    for a, b, n in zip(outs, ref, SC.NAMES):
        assert torch.equal(a, b), n
    assert torch.equal(SC.pack(last, c['cfg']), packed)
    assert packed.shape == (c['N'], SC.state_floats(c['cfg']))


def test_the_packed_carry_is_in_the_library_order():
    c = FC.case('lstm2_mse_n5')
    _, carry, packed = SC.one_piece('lstm2_mse_n5')
    H, E, A, O = (c['cfg'][k] for k in ('rnn_h_dim', 'encoded_input_dim', 'attention_size', 'output_dim'))
    ldx = (O + 3) // 4 * 4
    assert torch.equal(packed[:, :O], carry['x']) and not packed[:, O:ldx].any()
    assert torch.equal(packed[:, ldx:ldx + A], carry['k']) and torch.equal(packed[:, ldx + A:ldx + A + E], carry['w'])
    o = ldx + A + E
    assert torch.equal(packed[:, o + H:o + 2 * H], carry['h'][1][0]) and torch.equal(packed[:, o + 3 * H:], carry['h'][1][1])


# ---------------------------------------------------------------------------------------------------- the C ABI
def _model(name, **kw):
    from parrot_amd.model import Parrot
    return Parrot(device=torch.device('cpu'), **dict(FC.CASES[name][0], **kw))


@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_state_floats(name):
    """parrot_sample_state_floats = ldx + A + E + L H (1 + lstm), from the descriptor's integers alone; Parrot agrees."""
    from oracle import parrot_ref as R
    from parrot_amd import _lib
    full, _ = FC.CASES[name]
    cfg = R.default_config(**full)
    lstm = full['cell_type'] == 'lstm'
    d = _lib.SampleDesc()
    d.H, d.E, d.A, d.L, d.O = cfg['rnn_h_dim'], cfg['encoded_input_dim'], cfg['attention_size'], cfg['num_layers'], cfg['output_dim']
    d.ldx, d.cell, d.S, d.B = (d.O + 3) // 4 * 4, int(lstm), 10, 5
    want = d.ldx + d.A + d.E + d.L * d.H * (1 + int(lstm))
    assert _lib.load().parrot_sample_state_floats(C.byref(d)) == want == SC.state_floats(cfg)
    assert _model(name).decode_state_floats() == want
    assert _lib.load().parrot_sample_state_floats(None) == 0


def test_entries_are_exported_and_declared():
    from parrot_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert name + "(" in header and name in guide
    assert "long long parrot_sample_state_floats(const ParrotSampleDesc* desc);" in header
    assert "int parrot_sample_save_state(void* plan, float* state, void* stream);" in header
    assert "int parrot_sample_load_state(void* plan, const float* state, void* stream);" in header
    assert "decode_state.hip" in open(os.path.join(ROOT, "parrot_amd", "build.py")).read()


def test_entries_refuse_null_arguments():
    from parrot_amd import _lib
    lib, buf = _lib.load(), (C.c_float * 4)()
    assert lib.parrot_sample_save_state(None, buf, None) == P.BADARG
    assert lib.parrot_sample_load_state(None, buf, None) == P.BADARG


# ---------------------------------------------------------------------------------------------------- carry plans, dry
def _normalised(d):
    """A copy of the workspace's descriptor with every pointer that is set replaced by the made-up address of its field
    (decode_plan_cases._addr): the dry digest then tells the programs of two workspaces apart, not their allocations."""
    from parrot_amd import _lib
    out = type(d)()
    C.memmove(C.byref(out), C.byref(d), C.sizeof(d))
    base = out.base if isinstance(out, _lib.SampleForcedDesc) else out
    for field, ctype in base._fields_:
        v = getattr(base, field)
        if ctype is C.c_void_p:
            if v is not None:
                setattr(base, field, P._addr(base, field))
        elif isinstance(v, C.Array) and v._type_ is C.c_void_p:
            for l in range(len(v)):
                if v[l] is not None:
                    v[l] = P._addr(base, field, l)
    return out


def _dry(name, monkeypatch, env, carry, N=5):
    """(info16, digest) of the dry plan of the case's workspace -- default or carry -- built on the CPU under `env`."""
    from parrot_amd import _lib
    W.set_switches(monkeypatch, env)
    with monkeypatch.context() as mp:
        W.install_stubs(mp)
        m = _model(name).allocate()
        ws = m._sample_workspace(SC.S, N, SC.U, carry=carry)
        assert list(m._sample_ws) == [(('carry',) if carry else ()) + (SC.S, N, SC.U)]
        d = _normalised(ws['desc'])
    lib, info, dig = _lib.load(), (C.c_int * 16)(), C.c_ulonglong(0)
    assert lib.parrot_sample_plan_pieces_dry(C.byref(d), 256, info) == 0
    assert lib.parrot_sample_plan_digest_dry(C.byref(d), 256, C.byref(dig)) == 0 and dig.value
    return list(info), dig.value


def test_the_gru_mse_carry_plan_is_the_program_without_the_composed_feedback(monkeypatch):
    """gru2_mse: the carry workspace plans, under the default switches, what the default workspace plans under
    PARROT_PM_FBC=0 -- same digest --, info16[15] bit 0 (the composition) is clear and the fold (bit 1) stays."""
    info_c, dig_c = _dry('gru2_mse_n5', monkeypatch, {}, carry=True)
    info_d, dig_d = _dry('gru2_mse_n5', monkeypatch, {}, carry=False)
    info_0, dig_0 = _dry('gru2_mse_n5', monkeypatch, {"PARROT_PM_FBC": "0"}, carry=False)
    assert info_d[15] & 1 == 1, "the default plan of the case composes the feedback: else the test shows nothing"
    assert info_c[15] & 1 == 0 and info_c[15] & 2 == info_d[15] & 2
    assert (info_c, dig_c) == (info_0, dig_0) and dig_c != dig_d
    assert info_c[0] == info_d[0] + 1   # 2L + 2 phases against 2L + 1


@pytest.mark.parametrize("name, env", [('lstm2_mse_n5', {}), ('gru1_mse_n5', {}), ('gru1_k3_n5', {"PARROT_PM_GMM": "1"}),
                                       ('lstm2_k3_n5', {"PARROT_PM_GMM": "1"}), ('gru2_mse_n5', {"PARROT_PM_PIECES": "0"})])
def test_every_other_configuration_keeps_its_program(name, env, monkeypatch):
    assert _dry(name, monkeypatch, env, carry=True) == _dry(name, monkeypatch, env, carry=False)


def test_workspace_keys():
    from parrot_amd.model import Parrot
    k = Parrot._sample_ws_key
    assert k(10, 5, 9, 0, False) == (10, 5, 9) and k(10, 5, 9, 0, False, True) == ('carry', 10, 5, 9)
    assert k(10, 5, 9, 0, True, True) == ('carry', 'forced', 10, 5, 9) and k(10, 5, 9, 8, True) == ('forced', 'stop', 10, 5, 9, 8)


# ---------------------------------------------------------------------------------------------------- DecodeState
def test_decode_state_views_reset_and_clone():
    """initial_decode_state is the oracle's initial carry, packed; the views are views; reset_rows touches its rows only."""
    from oracle import parrot_ref as R
    c = FC.case('lstm2_mse_n5')
    m = _model('lstm2_mse_n5').allocate()
    m.set_parameter_values(c['p'])
    st = m.initial_decode_state(4)
    init = R.initial_carry(c['p'], c['cfg'], 4)
    want = SC.pack(dict(init, x=torch.zeros(4, c['cfg']['output_dim'], dtype=torch.float64)), c['cfg']).float()
    assert st.tensor.dtype == torch.float32 and torch.equal(st.tensor, want)
    assert st.frames_done.tolist() == [0] * 4 and len(st.h) == len(st.c) == 2
    assert st.x.shape == (4, 64) and st.kappa.shape == (4, c['cfg']['attention_size']) and st.h[1].shape == (4, c['cfg']['rnn_h_dim'])
    assert st.tensor.shape[1] == m.decode_state_floats() == sum(v.shape[1] for v in [st.x, st.kappa, st.w] + st.h + st.c)
    st.c[1][2, 3] = 7.
    assert st.tensor[2, -c['cfg']['rnn_h_dim'] + 3] == 7.
    other = st.clone()
    st.tensor.add_(1.)
    st.frames_done[:] = 6
    assert other.tensor[2, -c['cfg']['rnn_h_dim'] + 3] == 7. and other.frames_done.tolist() == [0] * 4
    st.reset_rows([1, 3])
    assert torch.equal(st.tensor[[1, 3]], want[[1, 3]]) and torch.equal(st.tensor[[0]], want[[0]] + 1.)
    assert st.frames_done.tolist() == [6, 0, 6, 0]
    assert len(_model('gru2_mse_n5').allocate().initial_decode_state(2).c) == 0


# ---------------------------------------------------------------------------------------------------- refusals
def test_bad_states_are_refused_before_anything_is_allocated():
    from parrot_amd.decode import DecodeState
    m = _model('lstm2_mse_n5').allocate()
    Wd = m.decode_state_floats()
    lab, lm = np.zeros((3, 4), dtype='int64'), np.ones((3, 4), dtype='float32')
    good = m.initial_decode_state(3)
    nan = good.clone()
    nan.h[0][1, 2] = float('nan')
    inf = good.clone()
    inf.x[0, 0] = float('inf')
    bad = [(m.initial_decode_state(2), "N = 3"), (DecodeState(m, torch.zeros(3, Wd + 4)), f"W = {Wd}"),
           (DecodeState(m, torch.zeros(3, Wd, device='meta')), "device"), (nan, "finite"), (inf, "finite"),
           (good.tensor, "DecodeState"), (DecodeState(m, torch.zeros(3, Wd, dtype=torch.float64)), "float32")]
    for state, match in bad:
        for call in (lambda: m.sample_model_device(lab, lm, None, 3, 6, state=state),
                     lambda: m.sample_model(lab, lm, None, None, 3, 6, state=state),
                     lambda: m.decode_segments(lab, lm, None, 3, 6, 4, state=state)):
            with pytest.raises(ValueError, match=match):
                call()
    for kw in (dict(state=good), dict(return_state=True)):
        with pytest.raises(ValueError, match="does not resume"):
            m.sample_until_end_device(lab, lm, None, 3, 6, **kw)
        with pytest.raises(ValueError, match="does not resume"):
            m.sample_until_end(lab, lm, None, None, 3, 6, **kw)
    with pytest.raises(ValueError, match="segment_frames"):
        m.decode_segments(lab, lm, None, 3, 6, 0)
    with pytest.raises(ValueError, match="P <= 6"):   # (the other refusals of the decode calls hold for the segments too)
        m.decode_segments(lab, lm, None, 3, 6, 4, forced_frames=np.zeros((7, 3, 63)), n_forced=[0, 1, 2])
    assert not m._sample_ws and m.decode_path is None


def test_streaming_decoder_refuses_bad_arguments():
    from parrot_amd.decode import StreamingDecoder
    with pytest.raises(ValueError, match="encoder_literal"):
        StreamingDecoder(_model('gru2_mse_n5'), 2, 4, 9, 20)
    m = _model('gru2_mse_n5', encoder_literal=False)
    for kw in (dict(slots=0), dict(segment_frames=0), dict(max_text=0), dict(max_frames=0), dict(extra=-1)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            StreamingDecoder(m, **dict(dict(slots=2, segment_frames=4, max_text=9, max_frames=20), **kw))
    sd = StreamingDecoder(m, 2, 4, 9, 20)
    with pytest.raises(ValueError, match="max_text"):
        sd.submit(np.zeros(10, dtype='int64'))
    with pytest.raises(ValueError, match="max_text"):
        sd.submit([])
    with pytest.raises(ValueError, match="timing_coeffs"):
        sd.submit([1, 2], timing_coeff=0.)
    with pytest.raises(ValueError, match="P <= 20"):
        sd.submit([1, 2], forced_frames=np.zeros((21, 63)))
    assert sd.submit([1, 2, 3]) == 0 and sd.submit([4], timing_coeff=1.5, forced_frames=np.zeros((3, 63))) == 1
    assert not m._sample_ws


# ---------------------------------------------------------------------------------------------------- the rule, per segment
def _chained_first(phi, lm, cuts):
    from parrot_amd.decode import segment_end_of_utterance
    from parrot_amd.utils import end_of_utterance_args
    pos, ncmp = (torch.from_numpy(a) for a in end_of_utterance_args(lm, phi.shape[2]))
    first, t0 = torch.full((phi.shape[1],), -1, dtype=torch.long), 0
    for t1 in cuts:
        first = segment_end_of_utterance(torch.from_numpy(phi[t0:t1]), pos, ncmp, first, t0)
        t0 = t1
    return first.tolist()


def _lengths(first, S, extra):
    return [S if f < 0 else min(f + extra, S) for f in first]


@pytest.mark.parametrize("cuts", [[10], SC.CUTS, [4, 8, 10]], ids=["whole", "1-4-10", "4-8-10"])
def test_the_segment_rule_is_end_of_utterance(cuts):
    """Random windows for every text length 0 .. U (the slicing corner at length 1 and the clamp at U included), and the
    edges: never fires, fires at frame 0, on the last frame of a segment, on the first of the next, a tie (strict: no)."""
    from parrot_amd.utils import end_of_utterance
    S, U, extra = 10, SC.U, 3
    rng = np.random.RandomState(3)
    N = 4 * (U + 1)
    lengths = np.arange(N) % (U + 1)
    lm = (np.arange(U)[None, :] < lengths[:, None]).astype('float32')
    phi = rng.rand(S, N, U).astype('float32')
    first = _chained_first(phi, lm, cuts)
    want = [end_of_utterance(phi[:, i], min(int(lengths[i]), U - 1), S, extra) for i in range(N)]
    assert _lengths(first, S, extra) == want
    assert any(f < 0 for f in first) and any(f == 0 for f in first) and any(f > 0 for f in first)
    # the edges, on a text of 4 characters: the rule compares phi[:, 4] with phi[:, :3]
    fire = {0: None, 1: 0, 2: 3, 3: 4, 4: 9, 5: None}
    phi = np.zeros((S, 6, U), dtype='float32')
    phi[:, :, :3] = 0.5
    phi[:, :, 3] = 9.   # (position 3 is not compared)
    for row, t in fire.items():
        if t is not None:
            phi[t:, row, 4] = 0.75
    phi[:, 5, 4] = 0.5  # a tie with every compared position: never fires
    lm = np.zeros((6, U), dtype='float32')
    lm[:, :4] = 1
    first = _chained_first(phi, lm, cuts)
    assert first == [-1, 0, 3, 4, 9, -1]
    assert _lengths(first, S, extra) == [end_of_utterance(phi[:, i], 4, S, extra) for i in range(6)] == [10, 3, 6, 7, 10, 10]


def test_the_segment_rule_counts_every_row_from_its_own_frame():
    from parrot_amd.decode import segment_end_of_utterance
    phi = torch.zeros(4, 2, SC.U)
    phi[2:, :, 3] = 1.
    pos, ncmp = torch.tensor([3, 3], dtype=torch.int32), torch.tensor([2, 2], dtype=torch.int32)
    first = segment_end_of_utterance(phi, pos, ncmp, torch.tensor([-1, 5]), torch.tensor([8, 12]))
    assert first.tolist() == [10, 5]


# ---------------------------------------------------------------------------------------------------- sample.py's flag
def test_segment_frames_flag():
    from parrot_amd.utils import sample_parse
    assert sample_parse([]).segment_frames == 0 and sample_parse(["--segment_frames", "4"]).segment_frames == 4
    with pytest.raises(SystemExit, match="--sample_one_step"):
        sample_parse(["--segment_frames", "4", "--sample_one_step", "1"])
    with pytest.raises(SystemExit, match="negative"):
        sample_parse(["--segment_frames", "-1"])
