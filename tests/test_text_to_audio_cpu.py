"""Text to audio in one stream, as far as it can be checked without a GPU: StreamingGenerator(open_utterances=True) on a
fake segment runner whose samples name the frame each slot was handed -- the six scheduling rules of the class's docstring
one by one --, the default generator's trace against a replay of schedule_segment, and the argument refusals of
DeviceGenerator.generate(gather=) (on a stubbed library), feed, TextToAudio and sample.py --stream_audio."""
import numpy as np
import pytest
import torch

BFS, F = 80, 63


def _tt():
    from parrot_amd.sampleRNN.models.conditional import three_tier as tt
    return tt


def _code(ticket, frame):
    return 1 + 16 * ticket + frame   # (0: an idle slot; < 256 for the tickets and lengths below)


def _utt(ticket, n):
    """[n, 63] frames whose every row names (ticket, frame) in column 0 and carries other columns too."""
    u = np.zeros((n, F), dtype=np.float32)
    u[:, 0] = [_code(ticket, f) for f in range(n)]
    u[:, 1:] = np.arange(1, F, dtype=np.float32)[None] * 0.5 + ticket
    return u


class Fake:
    """run_segment: every sample of slot r, stream b is feats[r, b, 0], the code of the frame the slot was handed."""

    def __init__(self):
        self.calls = []

    def __call__(self, feats, starts, resume, **kw):
        assert feats.dtype == np.float32 and feats.shape[1:] == (starts.shape[1], F) and feats.shape[0] == starts.shape[0]
        self.calls.append((feats.copy(), starts.copy(), resume, kw))
        return np.repeat(feats[:, :, 0].T.astype(np.int32), BFS, axis=1)

    def timeline(self, B):
        """Per stream, the codes of all slots run so far, in order."""
        return [np.concatenate([c[0][:, b, 0] for c in self.calls]).astype(int).tolist() if self.calls else [] for b in range(B)]


def _gen(B, S, fake, **kw):
    return _tt().StreamingGenerator(B, S, run_segment=fake, open_utterances=True, **dict(dict(max_frames=16), **kw))


def _collect(chunks, into, done):
    for ticket, chunk, d in chunks:
        assert ticket not in done, "a chunk behind done"
        assert chunk.dtype == np.int32 and chunk.size % BFS == 0
        into.setdefault(ticket, []).append(chunk)
        if d:
            done.append(ticket)


def _expected(ticket, n):
    want = np.repeat(np.array([_code(ticket, f) for f in range(n)], dtype=np.int32), BFS)
    want[:BFS] = _tt().Q_ZERO
    return want


def _rules_hold(fake, B, lengths, fed_at_call):
    """Rules 1 and 2 on the runner's record: every utterance's frames lie in consecutive slots of one stream, in order, once
    -- none unfed (fed_at_call[k][ticket] = the frames it had been fed when segment k ran)."""
    for k, (feats, _, _, _) in enumerate(fake.calls):
        for code in feats[:, :, 0].astype(int).ravel():
            if code:
                ticket, frame = divmod(code - 1, 16)
                assert frame < fed_at_call[k].get(ticket, 0), f"segment {k} ran frame {frame} of utterance {ticket} unfed"
    seen = {}
    for b, line in enumerate(fake.timeline(B)):
        for pos, code in enumerate(line):
            if code:
                ticket, frame = divmod(code - 1, 16)
                seen.setdefault(ticket, []).append((b, pos, frame))
    for ticket, n in lengths.items():
        got = seen[ticket]
        assert [f for _, _, f in got] == list(range(n)), f"utterance {ticket}: frames {[f for _, _, f in got]}"
        assert len({b for b, _, _ in got}) == 1, "an utterance changed its stream"
        assert [p for _, p, _ in got] == list(range(got[0][1], got[0][1] + n)), f"utterance {ticket} idles inside"


def _drive(B, S, lengths, plan, late_close=()):
    """Opens len(lengths) utterances and, before step k, feeds plan[k] = {ticket: frames to add}; an utterance is closed with
    its last frames unless it is in late_close (then after the step that placed its last frame).  Steps until everything is
    done."""
    fake = Fake()
    sg = _gen(B, S, fake)
    tickets = [sg.open() for _ in lengths]
    assert tickets == list(range(len(lengths)))
    utts = [_utt(t, n) for t, n in enumerate(lengths)]
    fed, chunks, done, fed_at_call, starved_steps, to_close = [0] * len(lengths), {}, [], [], 0, list(late_close)
    k = 0
    while not sg.idle():
        for t in [t for t in to_close if sum(c.size for c in chunks.get(t, [])) == BFS * lengths[t]]:
            sg.close(t)
            to_close.remove(t)
        for t, add in (plan[k] if k < len(plan) else {t: lengths[t] - fed[t] for t in tickets if fed[t] < lengths[t]}).items():
            add = min(add, lengths[t] - fed[t])
            if add == 0:
                continue
            last = fed[t] + add == lengths[t]
            sg.feed(t, utts[t][fed[t]:fed[t] + add], last=last and t not in late_close)
            fed[t] += add
        calls = len(fake.calls)
        out = sg.step()
        if len(fake.calls) > calls:
            fed_at_call.append(dict(enumerate(fed)))
            assert sg.starved is None
        else:
            assert all(c.size == 0 for _, c, _ in out), "chunks without a segment"
            starved_steps += sg.starved is not None
        _collect(out, chunks, done)
        k += 1
        assert k < 200
    assert sorted(done) == tickets
    for t, n in enumerate(lengths):
        assert np.array_equal(np.concatenate(chunks[t]), _expected(t, n)), f"utterance {t}"
    _rules_hold(fake, B, dict(enumerate(lengths)), fed_at_call)
    assert sg.free_rows == 2 * B and sg.step() == []
    return sg, fake, chunks, starved_steps


# ---- rules 1, 2, 3: pieces, whole, and starvation --------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 4])
def test_fed_one_frame_at_a_time(S):
    """1 + 1 + ...: one frame before every step, two streams and three utterances; no step starves (every running utterance
    has one new frame) and, while two open utterances run, every segment is cut to one slot (the last utterance has
    collected frames while it was queued and runs them in longer segments once it is alone)."""
    lengths = [5, 3, 4]
    plan = [{0: 1, 1: 1, 2: 1}] * 5
    sg, fake, chunks, starved = _drive(2, S, lengths, plan)
    assert starved == 0
    assert all(c[0].shape[0] == 1 for c in fake.calls[:3]), "a segment longer than what the open utterances could supply"
    assert sg.record[0][0] != sg.record[1][0] and sg.record[2][0] == sg.record[1][0], "the third follows the shortest"


@pytest.mark.parametrize("S", [1, 4])
def test_fed_whole_equals_submit(S):
    """Rule 4: everything closed before its first placement -- the runner sees the calls, and the caller the chunks, of the
    default generator, whose placements are schedule_segment's."""
    tt = _tt()
    lengths = [5, 3, 4, 1, 6]
    fake, ref = Fake(), Fake()
    sg = _gen(2, S, fake, store_utterances=len(lengths))
    plain = tt.StreamingGenerator(2, S, run_segment=ref)
    for t, n in enumerate(lengths):
        assert sg.open() == t
        sg.feed(t, _utt(t, n)[:2])
        sg.feed(t, torch.from_numpy(_utt(t, n)[2:]), last=True)   # (a host tensor is taken like an array)
        assert plain.submit(_utt(t, n)) == t
    got, want = sg.drain(), plain.drain()
    assert len(got) == len(want)
    for (t1, c1, d1), (t2, c2, d2) in zip(got, want):
        assert (t1, d1) == (t2, d2) and np.array_equal(c1, c2)
    assert len(fake.calls) == len(ref.calls)
    for (f1, s1, r1, k1), (f2, s2, r2, k2) in zip(fake.calls, ref.calls):
        assert np.array_equal(f1, f2) and np.array_equal(s1, s2) and r1 == r2 and k1 == k2 == {}
    assert sg.record == plain.record
    # and submit() on the open generator is open + feed + close
    fake2 = Fake()
    sg2 = _gen(2, S, fake2, store_utterances=len(lengths))
    assert [sg2.submit(_utt(t, n)) for t, n in enumerate(lengths)] == list(range(len(lengths)))
    again = sg2.drain()
    assert all(a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1]) for a, b in zip(again, want))
    assert sg2.record == plain.record


@pytest.mark.parametrize("S", [1, 4])
def test_starved_step_runs_nothing_and_a_late_feed_resumes(S):
    """Rule 2: utterance 0 runs out of frames while open -> step() == [], starved says why, the runner is not called; the
    feed that arrives afterwards is run from the next step on, in the same stream, without a gap."""
    lengths = [6, 4, 5]
    plan = [{0: 2, 1: 4, 2: 5}, {}, {}, {}, {0: 4}]
    sg, fake, chunks, starved = _drive(2, S, lengths, plan)
    assert starved >= 1
    fake = Fake()
    sg = _gen(2, 4, fake)
    a = sg.open()
    assert sg.step() == [] and "frame 0" in sg.starved and not fake.calls          # rule 3: nothing to place
    sg.feed(a, _utt(a, 3)[:1])
    out = sg.step()                                                                # the prefix slot alone
    assert [(t, c.size, d) for t, c, d in out] == [(a, BFS, False)] and sg.starved is None and len(fake.calls) == 1
    assert sg.step() == [] and "utterance 0" in sg.starved and len(fake.calls) == 1
    with pytest.raises(RuntimeError, match="drain"):
        sg.drain()
    sg.feed(a, _utt(a, 3)[1:], last=True)
    out = sg.drain()
    assert [(t, c.size, d) for t, c, d in out] == [(a, 2 * BFS, True)] and sg.idle() and sg.starved is None


def test_a_later_utterance_with_frames_passes_one_without():
    """Rule 3: ticket 0 has no frame yet; ticket 1 is placed, in stream 0."""
    fake = Fake()
    sg = _gen(1, 4, fake)
    a, b = sg.open(), sg.open()
    sg.feed(b, _utt(b, 2), last=True)
    out = sg.step()
    assert [(t, d) for t, _, d in out] == [(b, True)] and sg.record[b] == (0, 1)
    sg.feed(a, _utt(a, 2), last=True)
    out = sg.drain()
    assert [(t, d) for t, _, d in out] == [(a, True)] and sg.record[a] == (0, 3)


# ---- rule 5 and 6: a late close ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 4])
def test_late_close_is_reported_with_an_empty_chunk(S):
    lengths = [4, 3, 2]
    sg, fake, chunks, starved = _drive(2, S, lengths, [{0: 4, 1: 3, 2: 2}], late_close=(0, 2))
    for t in (0, 2):
        assert chunks[t][-1].size == 0, "the close behind the last frame is an empty chunk with done"
    assert chunks[1][-1].size > 0


def test_drain_terminates_once_everything_is_closed():
    fake = Fake()
    sg = _gen(2, 4, fake)
    ts = [sg.open() for _ in range(3)]
    for t in ts:
        sg.feed(t, _utt(t, 3 + t)[:2])
    out = sg.step()
    for t in ts:
        sg.feed(t, _utt(t, 3 + t)[2:])
        sg.close(t)
    chunks, done = {}, []
    _collect(out + sg.drain(), chunks, done)
    assert sorted(done) == ts and sg.idle()
    for t in ts:
        assert np.array_equal(np.concatenate(chunks[t]), _expected(t, 3 + t))


# ---- the default generator ---------------------------------------------------------------------------------------------
def test_default_generator_is_the_class_as_it_was():
    """open / feed / close raise; the runner's calls and the chunks are those a replay of schedule_segment gives."""
    tt = _tt()
    fake = Fake()
    sg = tt.StreamingGenerator(2, 3, run_segment=fake)
    assert sg.open_utterances is False and sg.free_rows == 0 and sg.starved is None
    for call in (lambda: sg.open(), lambda: sg.feed(0, _utt(0, 1)), lambda: sg.close(0)):
        with pytest.raises(ValueError, match="open_utterances=True"):
            call()
    lengths = [4, 2, 5, 1]
    utts = [_utt(t, n) for t, n in enumerate(lengths)]
    trace = []
    for t in (0, 1):
        assert sg.submit(utts[t]) == t
    trace.append(sg.step())
    for t in (2, 3):
        assert sg.submit(utts[t]) == t
    while not sg.idle():
        trace.append(sg.step())
    assert sg.step() == []
    # the replay
    running, queue, calls, want = [None, None], [(0, 4), (1, 2)], [], []
    arrivals = {1: [(2, 5), (3, 1)]}
    k = 0
    while queue or any(r is not None for r in running) or k in arrivals:
        queue = queue + arrivals.pop(k, []) if k in arrivals else queue
        placements, starts, n, running, queue = tt.schedule_segment(running, queue, 2, 3)
        feats, flags, out = np.zeros((n, 2, F), np.float32), np.zeros((n, 2), np.int32), []
        for ticket, b, slot, frame, count in placements:
            feats[slot - 1:slot - 1 + count, b] = utts[ticket][frame:frame + count]
            out.append((ticket, _expected(ticket, lengths[ticket])[BFS * frame:BFS * (frame + count)],
                        frame + count == lengths[ticket]))
        for slot, b in starts:
            flags[slot - 1, b] = 1
        calls.append((feats, flags))
        want.append(out)
        k += 1
    assert len(trace) == len(want) and len(fake.calls) == len(calls)
    for got, exp in zip(trace, want):
        assert [(t, d) for t, _, d in got] == [(t, d) for t, _, d in exp]
        assert all(np.array_equal(a[1], b[1]) for a, b in zip(got, exp))
    for k, ((f1, s1, resume, kw), (f2, s2)) in enumerate(zip(fake.calls, calls)):
        assert np.array_equal(f1, f2) and np.array_equal(s1, s2) and resume == (k > 0) and kw == {}


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_feed_and_open_refusals():
    fake = Fake()
    sg = _gen(1, 2, fake, max_frames=4, store_utterances=2)
    a = sg.open()
    with pytest.raises(ValueError, match=r"\[k, 63\]"):
        sg.feed(a, np.zeros((2, 64), np.float32))
    with pytest.raises(ValueError, match=r"\[k, 63\]"):
        sg.feed(a, np.zeros(63, np.float32))
    with pytest.raises(ValueError, match="float32"):
        sg.feed(a, torch.zeros(1, 63, dtype=torch.float64))
    with pytest.raises(ValueError, match="at least one frame"):
        sg.close(a)
    sg.feed(a, _utt(a, 3))
    with pytest.raises(ValueError, match="overflow"):
        sg.feed(a, _utt(a, 2))
    sg.feed(a, _utt(a, 4)[3:], last=True)            # exactly max_frames
    with pytest.raises(ValueError, match="not an open utterance"):
        sg.feed(a, _utt(a, 1))
    with pytest.raises(ValueError, match="not an open utterance"):
        sg.feed(7, _utt(a, 1))
    with pytest.raises(ValueError, match="overflows"):
        sg.submit(_utt(1, 5))
    b = sg.open()
    assert sg.free_rows == 0
    with pytest.raises(RuntimeError, match="store"):
        sg.open()
    with pytest.raises(RuntimeError, match="store"):
        sg.submit(_utt(2, 2))
    for kw in (dict(seed=3), dict(temperature=0.5), dict(top_k=4), dict(top_p=0.5), dict(min_p=0.1)):
        with pytest.raises(ValueError, match="utterance_draws=True"):
            sg.open(**kw)
    sg.feed(b, _utt(b, 2), last=True)
    assert np.array_equal(np.concatenate([c for t, c, _ in sg.drain() if t == a]), _expected(a, 4)) and sg.free_rows == 2
    drawn = _gen(1, 2, Fake(), utterance_draws=True)
    with pytest.raises(ValueError, match="utterance_draws=True"):
        drawn.open()
    assert drawn.open(seed=5, temperature=0.7, top_k=3) == 0
    with pytest.raises(ValueError, match="log_probs"):
        _gen(1, 2, Fake(), log_probs=True).open()
    for kw in (dict(max_frames=0), dict(store_utterances=0)):
        with pytest.raises(ValueError, match="at least 1"):
            _gen(1, 2, Fake(), **kw)


def test_open_utterances_carry_their_draws_to_the_runner():
    """utterance_draws: the seed and temperature of an open utterance land on the row of its start flag, as submit's do."""
    fake = Fake()
    sg = _gen(2, 4, fake, utterance_draws=True)
    a = sg.open(seed=11, temperature=0.5)
    b = sg.open(seed=2 ** 63 + 5)
    sg.feed(a, _utt(a, 1))
    sg.feed(b, _utt(b, 3), last=True)
    sg.step()                                         # cut to one slot: a's prefix and b's
    sg.feed(a, _utt(a, 3)[1:], last=True)
    sg.drain()
    (_, s0, _, k0), (_, s1, _, k1) = fake.calls
    assert s0.shape == (1, 2) and not s0.any() and s1[0].tolist() == [1, 1]
    assert k1['seeds'][0].tolist() == [11, 2 ** 63 + 5] and k1['temperatures'][0].tolist() == [0.5, 0.0]


def _bare_plan(B, T, packed=False):
    """A DeviceGenerator around no plan: what generate() touches before and while it stages."""
    from parrot_amd.sampleRNN.generation.device import DeviceGenerator
    gen = DeviceGenerator.__new__(DeviceGenerator)
    gen.B, gen.T, gen.packed, gen.utterance_draws, gen._has_run, gen.persistent = B, T, packed, False, False, False
    gen.ws = dict(features=torch.zeros(T, B, F), samples=torch.zeros(B, BFS * T, dtype=torch.int32))
    gen.plan = 0x1234
    return gen


def test_generate_gather_refusals(monkeypatch):
    """Every refusal comes before anything is staged: the stubbed library records no call."""
    from parrot_amd import _lib
    from parrot_amd.sampleRNN.generation import device
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(device.hip, "_stream", lambda: 0)
    monkeypatch.setattr(device.DeviceGenerator, "_init_run", lambda self: None)
    B, T = 3, 5
    gen = _bare_plan(B, T)
    src, idx = torch.zeros(7, 64), np.zeros((T, B), np.int32)
    bad = [
        dict(features=np.zeros((T, B, F), np.float32), gather=(src, idx)),            # both
        dict(),                                                                        # neither
        dict(gather=src),                                                              # no pair
        dict(gather=(src.numpy(), idx)),                                               # src: no tensor
        dict(gather=(src.double(), idx)),                                              # src: dtype
        dict(gather=(torch.zeros(7, 62), idx)),                                        # ld < FEAT_DIM
        dict(gather=(torch.zeros(64, 7).t(), idx)),                                    # column stride
        dict(gather=(torch.zeros(0, 64), idx)),                                        # no rows
        dict(gather=(torch.zeros(2, 7, 64), idx)),                                     # rank
        dict(gather=(torch.zeros(7, 64, device='meta'), idx)),                         # another device
        dict(gather=(src, idx.astype(np.int64))),                                      # index: dtype
        dict(gather=(src, idx[:-1])),                                                  # index: rows
        dict(gather=(src, idx[:, :-1])),                                               # index: streams
        dict(gather=(src, idx), n_frames=2),                                           # k + 1 = 3 rows wanted
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            gen.generate(**kw)
    assert calls == []
    # and the call that passes stages through the entry: (plan, src, R, ld, index, first, rows, stream)
    gen.generate(gather=(src[:, :63], idx))
    assert [c[0] for c in calls] == ['samplernn_generate_stage_features', 'samplernn_generate_run']
    plan, ptr, R, ld, _, first, rows, stream = calls[0][1]
    assert (plan, ptr, R, ld, first, rows) == (0x1234, src.data_ptr(), 7, 64, 0, T)
    calls.clear()
    gen.generate(gather=(torch.zeros(4, 63), idx[:3]), n_frames=2)
    assert calls[0][1][2:4] == (4, 63) and calls[0][1][5:7] == (0, 3)
    calls.clear()
    gen.generate(gather=(src, idx[:2]), n_frames=2, resume=True)
    assert calls[0][1][5:7] == (1, 2)


class _NoModel:
    output_dim, encoder_type, encoder_literal, which_cost = 63, 'bidirectional', False, 'MSE'


def test_text_to_audio_refusals():
    from parrot_amd.decode import TextToAudio
    args = (2, 4, 9, 48, 2, 2)
    wide = _NoModel()
    wide.output_dim = 64
    with pytest.raises(ValueError, match="output_dim"):
        TextToAudio(wide, *args, run_segment=Fake())
    literal = _NoModel()
    literal.encoder_literal = True
    with pytest.raises(ValueError, match="encoder_literal=False"):
        TextToAudio(literal, *args, run_segment=Fake())
    with pytest.raises(ValueError, match="segment_frames"):
        TextToAudio(_NoModel(), 2, 0, 9, 48, 2, 2, run_segment=Fake())
    with pytest.raises(ValueError, match="pool_utterances"):
        TextToAudio(_NoModel(), *args, pool_utterances=0, run_segment=Fake())
    tta = TextToAudio(_NoModel(), *args, run_segment=Fake())
    assert tta.vocoder.open_utterances and tta.vocoder.free_rows == 4 and tta.vocoder.max_frames == 48
    assert (tta.decoder.slots, tta.decoder.segment_frames, tta.vocoder.B, tta.vocoder.S) == (2, 4, 2, 2)
    with pytest.raises(ValueError, match="utterance_draws=True"):
        tta.submit([1, 2, 3], seed=4)
    assert not tta._pending and not tta.decoder.busy


def test_sample_py_stream_audio_refusals():
    """The parser's refusals (an experiment without --raw_output is refused by sample.py itself, which reads the saved
    configuration: tests/test_gpu_text_to_audio.py)."""
    from parrot_amd.utils import sample_parse
    base = ["--experiment_name", "x"]
    ok = sample_parse(base + ["--stream_audio", "1", "--segment_frames", "4", "--stream_frames", "2", "--pack_streams", "3",
                              "--utterance_seed", "5", "--draw_mode", "scan", "--top_k", "9", "--timing_coeffs",
                              "1,1,1,1,1,1,1,1,1,1"])
    assert ok.stream_audio == 1 and sample_parse(base).stream_audio == 0
    for argv, what in [
        (["--stream_audio", "1", "--stream_frames", "2"], "--segment_frames F > 0"),
        (["--stream_audio", "1", "--segment_frames", "4"], "--stream_frames S > 0"),
        (["--stream_audio", "1", "--segment_frames", "4", "--stream_frames", "2", "--sample_one_step", "True"],
         "--sample_one_step"),
        (["--stream_audio", "2", "--segment_frames", "4", "--stream_frames", "2"], "0 or 1"),
    ]:
        with pytest.raises(SystemExit, match=what):
            sample_parse(base + argv)
