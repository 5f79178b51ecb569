"""Forced samples and per-sample log-probabilities of the SampleRNN generator (samplernn_generate_set_forced,
samplernn_generate_set_log_probs), as far as they can be checked without a GPU: the float64 reference the GPU tests lean on
(tests/samplernn_forced_cases.py::log_probs) against oracle.samplernn_ref.compute_cost, the host validation in front of
any device call, the packed layout of prompts, the runner contract of StreamingGenerator, the header and the signatures."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import samplernn_ref as S
from tests import samplernn_forced_cases as FC
from tests import samplernn_packed_cases as PC
from tests import samplernn_sampling_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tt():
    from parrot_amd.sampleRNN.models.conditional import three_tier
    return three_tier


# ---- 1. the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [dict(RNN_TYPE='GRU', N_RNN=1), dict(RNN_TYPE='LSTM', N_RNN=2)], ids=["gru1", "lstm2"])
def test_reference_is_what_compute_cost_averages(cfg):
    """The per-sample log-probabilities, averaged and in bits, are compute_cost of the same sequences to 1e-10 (the mean
    with compute_cost's own denominator: it guards the sample count with + 1e-5)."""
    c = S.config(DIM=32, EMB_SIZE=8, **cfg)
    p = S.init_params(c, seed=5, perturb=0.25)
    B, T = 3, 3
    feats = SC.features(T, B, 6).double()
    seq = FC.codes(B, T, seed=7)
    lp = FC.log_probs(p, c, seq, feats)
    assert lp.shape == (B, 80 * (T - 1)) and lp.dtype == torch.float64 and bool((lp < 0).all())
    want = FC.cost_bits(p, c, seq, feats)
    got = FC.mean_bits(lp.numpy())
    print(f"FORCED-CPU {cfg}: {got:.12f} bits against compute_cost {want:.12f}")
    assert abs(got - want) <= 1e-10
    assert 4.0 < want < 16.0          # random codes under a random model: near log2(256), and no degenerate zero
    # the helper follows the sequence: another code at one place moves that sample's value and only later ones
    seq2 = seq.copy()
    seq2[1, 97] = (seq2[1, 97] + 1) % 256
    lp2 = FC.log_probs(p, c, seq2, feats)
    assert torch.equal(lp2[0], lp[0]) and torch.equal(lp2[1, :17], lp[1, :17]) and lp2[1, 17] != lp[1, 17]
    assert not torch.equal(lp2[1, 18:], lp[1, 18:])


# ---- 2. host validation --------------------------------------------------------------------------------------------------
def _bare_plan(tt, forcing, packed=False, B=2, T=3):
    """A DeviceGenerator without a device behind it: what generate() checks before it stages anything."""
    gen = object.__new__(tt.DeviceGenerator)
    gen.B, gen.T, gen.packed, gen.utterance_draws, gen._has_run, gen.top_k, gen.top_p = B, T, packed, False, False, 0, 0.0
    gen.forcing, gen.log_probs = forcing, False
    return gen


def _no_device(monkeypatch):
    from parrot_amd import _lib
    from parrot_amd.sampleRNN import lib

    def no_device(*a, **k):
        raise AssertionError("a device call in front of the check")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(lib, "device", no_device)


def test_generate_refuses_bad_forced_in_front_of_the_device(tt, monkeypatch):
    _no_device(monkeypatch)
    feats = np.zeros((3, 2, 63), dtype=np.float32)
    good = np.full((2, 240), -1, dtype=np.int32)
    with pytest.raises(ValueError):                       # forced without forcing=True
        _bare_plan(tt, False).generate(feats, forced=good)
    with pytest.raises(ValueError):                       # and the reverse
        _bare_plan(tt, True).generate(feats)
    on = _bare_plan(tt, True)
    bad_value = good.copy()
    bad_value[1, 100] = 256
    low = good.copy()
    low[0, 239] = -2
    for bad in (good[:, :160], good[:1], good.reshape(-1), good.astype(np.float32), good.astype(bool), bad_value, low,
                [[0.5] * 240] * 2):
        with pytest.raises(ValueError):
            on.generate(feats, forced=bad)
    # a segment: [B, 80 rows] for the rows of this call -- k + 1 with the prefix, k when it resumes
    with pytest.raises(ValueError):
        on.generate(feats[:2], n_frames=1, forced=good)
    on._has_run = True
    with pytest.raises(ValueError):
        on.generate(feats[:1], resume=True, n_frames=1, forced=good[:, :160])
    # values and dtypes that pass: every code, -1, any integer type
    assert tt.forced_array(np.array([[-1, 0, 255]], dtype=np.int64), (1, 3)).dtype == np.int32
    assert tt.forced_array(np.array([[0, 255]], dtype=np.uint8), (1, 2)).tolist() == [[0, 255]]
    assert inspect.signature(tt.DeviceGenerator.__init__).parameters["forcing"].default is False
    assert inspect.signature(tt.DeviceGenerator.__init__).parameters["log_probs"].default is False
    assert inspect.signature(tt.DeviceGenerator.generate).parameters["forced"].default is None


def test_prompts_are_checked_in_front_of_the_device(tt, monkeypatch):
    _no_device(monkeypatch)
    utt = np.zeros((3, 63), dtype=np.float32)             # generates 160 samples
    for bad in ([np.zeros(161, dtype=np.int32)],         # longer than its utterance
                [np.array([0, 256])], [np.array([-1, 3])], [np.array([0.5, 1.0])], [np.zeros((2, 2), dtype=np.int32)],
                [None, None]):                            # one prompt too many
        with pytest.raises(ValueError):
            tt.generate_packed([utt], n_streams=2, prompts=bad)
    with pytest.raises(ValueError):                       # the prefix slot alone generates nothing
        tt.generate_packed([utt[:1]], n_streams=2, prompts=[np.array([3])])
    with pytest.raises(ValueError):
        tt.score_utterances([utt], [np.zeros(100, dtype=np.int32)])
    with pytest.raises(ValueError):
        tt.score_utterances([utt], [np.full(160, 256)])
    with pytest.raises(ValueError):
        tt.score_utterances([utt, utt], [np.zeros(160, dtype=np.int32)])
    tt.configure(SKIP_CONN=True)                          # skip-connection stacks stay refused, as before
    try:
        with pytest.raises(NotImplementedError):
            tt.generate_packed([utt], n_streams=2, prompts=[None])
        with pytest.raises(NotImplementedError):
            tt.DeviceGenerator(2, 3, forcing=True, log_probs=True)
    finally:
        tt.configure(SKIP_CONN=False)
    got = tt._per_utterance_prompts([None, np.arange(5), []], [2, 2, 1])
    assert [g.tolist() for g in got] == [[], [0, 1, 2, 3, 4], []] and all(g.dtype == np.int32 for g in got)
    assert tt.generate_packed([], prompts=[], log_probs=True) == ([], [])


def test_submit_checks_the_prompt(tt):
    runner = lambda features, starts, resume, **kw: np.zeros((2, 80 * features.shape[0]), dtype=np.int32)
    sg = tt.StreamingGenerator(2, 2, run_segment=runner)
    utt = np.zeros((2, 63), dtype=np.float32)
    for bad in (np.zeros(81, dtype=np.int32), np.array([256]), np.array([-1]), np.array([1.5])):
        with pytest.raises(ValueError):
            sg.submit(utt, prompt=bad)
    assert sg.submit(utt, prompt=np.arange(80)) == 0


# ---- 3. the packed layout ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["GRU_PACKING", "GROUPS_PACKING", "STACKED_PACKING"])
def test_packed_prompts_unpack_to_the_prompts(tt, name):
    case = getattr(PC, name)
    rng = np.random.RandomState(3)
    n = len(case.lengths)
    prompts = []
    for i, frames in enumerate(case.lengths):
        room = 80 * (frames - 1)
        size = (None, room, 0, 1, room // 2 + 3)[i % 5]       # none, fully forced, empty, one code, ending mid-frame
        prompts.append(None if size is None else rng.randint(0, 256, size=size))
    forced = tt.build_packed_prompts(prompts, case.lengths, case.stream, case.first_slot, case.T, case.B)
    assert forced.shape == (case.B, 80 * case.T) and forced.dtype == np.int32
    pieces = tt.unpack_samples(forced, case.lengths, case.stream, case.first_slot)
    busy = np.zeros(forced.shape, dtype=bool)
    for i in range(n):
        b, s, frames = case.stream[i], case.first_slot[i], case.lengths[i]
        want = np.full(80 * (frames - 1), -1, dtype=np.int32)
        if prompts[i] is not None:
            want[:len(prompts[i])] = prompts[i]
        assert np.array_equal(pieces[i][80:], want), i
        assert (forced[b, 80 * s:80 * (s + 1)] == -1).all(), f"prefix slot of utterance {i}"
        busy[b, 80 * (s + 1):80 * (s + frames)] = True
    assert (forced[~busy] == -1).all()                        # prefix slots and idle slots
    assert (forced[busy] >= 0).sum() == sum(len(p) for p in prompts if p is not None)
    lp = np.arange(forced.size, dtype=np.float32).reshape(forced.shape)
    for i, piece in enumerate(tt.unpack_log_probs(lp, case.lengths, case.stream, case.first_slot)):
        b, s = case.stream[i], case.first_slot[i]
        assert piece.dtype == np.float32 and np.array_equal(piece, lp[b, 80 * (s + 1):80 * (s + case.lengths[i])])
    with pytest.raises(ValueError):
        tt.build_packed_prompts([np.zeros(81, dtype=np.int32)], [2], [0], [0], 2, 1)


# ---- 4. the runner contract of StreamingGenerator ------------------------------------------------------------------------
def test_prompt_is_cut_across_segments(tt):
    """One stream, segments of two slots, an utterance of a prefix slot and three frames with a prompt of 100 codes: it is
    longer than the first segment has room for and ends 20 samples into its second frame."""
    seen = []

    def runner(features, starts, resume, forced=None):
        seen.append(forced.copy())
        out = np.where(forced >= 0, forced, 7).astype(np.int32)
        return out, np.where(forced >= 0, np.float32(-1.0), np.float32(-2.0))

    prompt = np.arange(100) + 100
    sg = tt.StreamingGenerator(1, 2, run_segment=runner, log_probs=True)
    sg.submit(np.zeros((4, 63), dtype=np.float32), prompt=prompt)
    chunks = sg.drain()
    assert len(seen) == 2 and all(f.shape == (1, 160) and f.dtype == np.int32 for f in seen)
    assert (seen[0][0, :80] == -1).all() and np.array_equal(seen[0][0, 80:], prompt[:80])       # prefix slot | frame 1
    assert np.array_equal(seen[1][0, :20], prompt[80:]) and (seen[1][0, 20:] == -1).all()       # frame 2 | frame 3
    (t0, c0, l0, d0), (t1, c1, l1, d1) = chunks
    assert (t0, t1, d0, d1) == (0, 0, False, True)
    assert (c0[:80] == 128).all() and np.array_equal(c0[80:], prompt[:80]) and np.array_equal(c1[:20], prompt[80:])
    assert (c1[20:] == 7).all()
    assert l0.dtype == np.float32 and (l0[:80] == 0).all() and (l0[80:] == -1).all()
    assert (l1[:20] == -1).all() and (l1[20:] == -2).all()
    with pytest.raises(ValueError):                                      # log_probs=True wants (samples, logp)
        bad = tt.StreamingGenerator(1, 2, run_segment=lambda f, s, r, **kw: np.zeros((1, 80 * f.shape[0]), dtype=np.int32),
                                    log_probs=True)
        bad.submit(np.zeros((2, 63), dtype=np.float32))
        bad.step()


def test_a_second_utterance_takes_its_own_columns(tt):
    """Two streams: the utterance without a prompt leaves its row free, the prompt of the other starts behind its own
    prefix slot wherever that lies in the segment."""
    seen = []

    def runner(features, starts, resume, forced=None):
        seen.append(forced.copy())
        return np.zeros(forced.shape, dtype=np.int32)

    sg = tt.StreamingGenerator(2, 3, run_segment=runner)
    sg.submit(np.zeros((2, 63), dtype=np.float32), prompt=np.arange(10))     # stream 0, slots 1 .. 2
    sg.submit(np.zeros((3, 63), dtype=np.float32))                           # stream 1, slots 1 .. 3
    sg.submit(np.zeros((2, 63), dtype=np.float32), prompt=np.arange(80))     # stream 0: prefix at slot 3, frame 1 next segment
    sg.drain()
    assert len(seen) == 2
    want = np.full((2, 240), -1, dtype=np.int32)
    want[0, 80:90] = np.arange(10)
    assert np.array_equal(seen[0], want)
    assert np.array_equal(seen[1][0, :80], np.arange(80)) and (seen[1][1] == -1).all()


def test_without_prompts_the_runner_is_called_as_before(tt):
    calls = []

    def three(features, starts, resume):                   # exactly today's arguments: anything more would be a TypeError
        calls.append((features.shape, starts.shape, resume))
        return np.zeros((2, 80 * features.shape[0]), dtype=np.int32)

    sg = tt.StreamingGenerator(2, 2, run_segment=three)
    sg.submit(np.zeros((3, 63), dtype=np.float32))
    sg.submit(np.zeros((2, 63), dtype=np.float32))
    out = sg.drain()
    assert calls and all(len(item) == 3 for item in out)   # (ticket, chunk, done), as before
    sg.submit(np.zeros((2, 63), dtype=np.float32), prompt=np.array([5]))    # from the first prompt on: one more keyword
    with pytest.raises(TypeError):
        sg.step()


# ---- 5. the ABI ----------------------------------------------------------------------------------------------------------
def test_header_and_signatures():
    from parrot_amd import _lib
    txt = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    assert re.search(r"int samplernn_generate_set_forced\(void\* plan, const int\* forced\);", txt)
    assert re.search(r"int samplernn_generate_set_log_probs\(void\* plan, float\* logp\);", txt)
    assert _lib.SIGNATURES["samplernn_generate_set_forced"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert _lib.SIGNATURES["samplernn_generate_set_log_probs"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert C.sizeof(_lib.SampleRnnGenDesc) == 936            # the descriptor did not change
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "samplernn_generate_set_forced" in doc and "samplernn_generate_set_log_probs" in doc


def test_c_entries_refuse_null_arguments():
    from parrot_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 4)()
    assert lib.samplernn_generate_set_forced(None, C.addressof(buf)) == 10001       # PARROT_ERR_BADARG, no device call
    assert lib.samplernn_generate_set_log_probs(None, C.addressof(buf)) == 10001
    assert lib.samplernn_generate_set_forced(C.addressof(buf), None) == 10001       # (the plan is only looked at after the pointer)
    assert lib.samplernn_generate_set_log_probs(C.addressof(buf), None) == 10001


def test_new_names_are_reexported(tt):
    from parrot_amd.sampleRNN.generation import inputs, serving
    for name in ("build_packed_prompts", "forced_array", "unpack_log_probs", "_per_utterance_prompts"):
        assert getattr(tt, name) is getattr(inputs, name), name
    assert tt.score_utterances is serving.score_utterances
