"""Packing utterances of unequal length into the streams of one SampleRNN generation plan (three_tier.pack_utterances,
build_packed_inputs, generate_packed; SampleRnnGenDesc::starts), as far as it can be checked without a GPU: the packing
itself, the features / starts it turns into, and the descriptor fields in the header and in _lib."""
import os
import re

import numpy as np
import pytest

from tests import samplernn_packed_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tt():
    from parrot_amd.sampleRNN.models.conditional import three_tier as tt
    return tt


def _check_packing(lengths, B):
    stream, first, T = _tt().pack_utterances(lengths, B)
    assert len(stream) == len(first) == len(lengths)
    used = {}
    for n, b, s in zip(lengths, stream, first):
        assert 0 <= b < B and s >= 0
        slots = set(range(s, s + n))
        assert not (used.setdefault(b, set()) & slots), "two utterances share a slot of stream %d" % b
        used[b] |= slots
    longest = max(max(v) + 1 for v in used.values())
    for b, v in used.items():          # no holes: a stream's utterances follow one another from slot 0
        assert v == set(range(len(v)))
    assert T == max(2, longest)
    assert longest <= -(-sum(lengths) // B) + max(lengths)   # longest first onto the least-loaded stream
    return stream, first, T


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("B", [1, 3, 5, 32])
def test_slots_never_overlap_and_T_is_bounded(seed, B):
    rng = np.random.RandomState(seed)
    lengths = [int(n) for n in rng.randint(1, 40, size=rng.randint(1, 70))]
    _check_packing(lengths, B)


def test_deterministic_and_ties():
    tt = _tt()
    lengths = [3, 5, 5, 2, 5, 3, 1]
    a, b = tt.pack_utterances(lengths, 3), tt.pack_utterances(list(lengths), 3)
    assert a == b
    stream, first, T = a
    # longest first, the lower utterance index first among equals, onto the lower of the least-loaded streams:
    # 5 (1) -> s0, 5 (2) -> s1, 5 (4) -> s2, 3 (0) -> s0 @5, 3 (5) -> s1 @5, 2 (3) -> s2 @5, 1 (6) -> s2 @7
    assert stream == [0, 0, 1, 2, 2, 1, 2]
    assert first == [5, 0, 0, 5, 0, 5, 7]
    assert T == 8
    assert tt.pack_utterances(np.asarray(lengths), 3) == a     # any sequence of integers


def test_fewer_utterances_than_streams_single_and_ones():
    tt = _tt()
    assert tt.pack_utterances([4, 7], 5) == ([1, 0], [0, 0], 7)
    assert tt.pack_utterances([6], 32) == ([0], [0], 6)
    assert tt.pack_utterances([1], 4) == ([0], [0], 2)               # a plan has at least two frames
    assert tt.pack_utterances([1, 1, 1], 2) == ([0, 1, 0], [0, 0, 1], 2)
    _check_packing([1] * 9, 4)
    _check_packing([1, 9, 1, 1], 2)


@pytest.mark.parametrize("bad", [[0], [3, 0, 2], [-1, 4], [2, -5]])
def test_lengths_below_one_raise(bad):
    with pytest.raises(ValueError):
        _tt().pack_utterances(bad, 4)


def test_features_and_starts_are_built_as_specified():
    tt = _tt()
    rng = np.random.RandomState(3)
    lengths = [3, 5, 1, 2, 4, 1]
    utts = [rng.randn(n, 63).astype(np.float32) for n in lengths]
    B = 2
    stream, first, T = tt.pack_utterances(lengths, B)
    feats, starts = tt.build_packed_inputs(utts, stream, first, T, B)
    assert feats.shape == (T, B, 63) and feats.dtype == np.float32
    assert starts.shape == (T, B) and starts.dtype == np.int32
    want_f, want_s = np.zeros_like(feats), np.zeros_like(starts)
    for u, b, s in zip(utts, stream, first):
        for j in range(u.shape[0]):
            want_f[s + j, b] = u[j]
        if s + 1 < T:
            want_s[s + 1, b] = 1
    assert np.array_equal(feats, want_f) and np.array_equal(starts, want_s)
    assert not starts[0].any()                      # slot 0 is a prefix, never a start
    assert starts.sum() == sum(1 for s in first if s + 1 < T)
    with pytest.raises(ValueError):                 # an utterance that runs past T
        tt.build_packed_inputs(utts, stream, first, T - 1, B)


def test_the_required_case_is_what_it_claims():
    """The hand-made packing of the GPU tests: 11 utterances of 2..5 frames on 5 streams, T = 10; streams 0 and 1 begin
    an utterance in one period while stream 2 (same team of four) goes on; starts inside the eight-period chunk graph
    and in the single period behind it."""
    for case in (PC.GRU_PACKING, PC.GROUPS_PACKING, PC.STACKED_PACKING):
        lengths, stream, first, T, B = case.lengths, case.stream, case.first_slot, case.T, case.B
        used = {}
        for n, b, s in zip(lengths, stream, first):
            assert 0 <= b < B and s + n <= T and case.min_len <= n <= case.max_len
            assert not (used.setdefault(b, set()) & set(range(s, s + n)))
            used[b] |= set(range(s, s + n))
        for b, v in used.items():
            assert v == set(range(len(v)))
    c = PC.GRU_PACKING
    assert (c.B, len(c.lengths), c.T) == (5, 11, 10)
    flags = {(s + 1, b) for b, s in zip(c.stream, c.first_slot) if s + 1 < c.T}
    assert (6, 0) in flags and (6, 1) in flags and (6, 2) not in flags
    assert any(f <= 8 and f > 1 for f, _ in flags) and any(f == 9 for f, _ in flags)
    g = PC.GROUPS_PACKING
    gflags = {(s + 1, b) for b, s in zip(g.stream, g.first_slot) if s + 1 > 1}
    assert g.B == 37 and any(b == 36 for _, b in gflags) and any(32 <= b < 36 for _, b in gflags)
    # rectangles: the k-th utterances of all streams, each in its own stream
    for case in (PC.GRU_PACKING, PC.GROUPS_PACKING, PC.STACKED_PACKING):
        seen = sorted(i for rect in PC.rectangles(case) for i in rect.values())
        assert seen == list(range(len(case.lengths)))


def test_descriptor_fields_are_last_in_header_and_lib():
    from parrot_amd import _lib
    names = [f[0] for f in _lib.SampleRnnGenDesc._fields_]
    assert names[-3:] == ["starts", "big_h0", "frm_h0"]
    assert names[-5:-3] == ["persist_ws", "persist_ws_floats"]
    txt = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    body = txt[txt.index("typedef struct SampleRnnGenDesc {"):txt.index("} SampleRnnGenDesc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [re.sub(r"\[.*", "", d.strip().split()[-1].lstrip("*")) for d in body.split("{", 1)[1].split(";") if d.strip()]
    assert decl[-5:] == ["persist_ws", "persist_ws_floats", "starts", "big_h0", "frm_h0"], decl[-6:]
    assert re.search(r"const int\*\s+starts;", body) and re.search(r"const float\*\s+big_h0;\s*const float\*\s+frm_h0;", body)


def test_generator_refuses_skip_connections_and_mismatched_starts():
    tt = _tt()
    tt.configure(SKIP_CONN=True)
    try:
        with pytest.raises(NotImplementedError):
            tt.generate_packed([np.zeros((2, 63), np.float32)], n_streams=2, temperature=0.0)
    finally:
        tt.configure(SKIP_CONN=False)
    assert tt.generate_packed([], n_streams=2) == []


def test_unpack_gives_every_piece_its_prefix():
    tt = _tt()
    lengths = [3, 1, 2, 1]
    stream, first, T = tt.pack_utterances(lengths, 2)      # 3 -> s0, 2 -> s1, 1 (1) -> s1 @2, 1 (3) -> s0 @3; T = 4
    assert (stream, first, T) == ([0, 1, 1, 0], [0, 2, 0, 3], 4)
    samples = np.arange(2 * 80 * T, dtype=np.int32).reshape(2, 80 * T)
    pieces = tt.unpack_samples(samples, lengths, stream, first)
    assert [p.shape[0] for p in pieces] == [240, 80, 160, 80]
    assert np.array_equal(pieces[0], samples[0, :240]) and np.array_equal(pieces[1], samples[1, 160:240])
    assert np.array_equal(pieces[2], samples[1, :160])
    # the one-frame utterance in the plan's last slot: no period follows that would write its prefix
    assert (pieces[3] == 128).all()
