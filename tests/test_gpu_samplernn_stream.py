"""SampleRNN generation in resumable segments (samplernn_generate_run_segment, sr_resume_kernel in samplernn.hip;
three_tier.DeviceGenerator.generate(resume=, n_frames=), generate_stream) and continuous admission on one packed plan
(three_tier.StreamingGenerator, schedule_segment): the segments of a run are, bit for bit, the run in one piece -- greedy
and seeded, through the captured graphs and eagerly, on the persistent sample kernel (one and two row groups), on the
launch path and with stacked tiers -- and an utterance admitted while the plan runs computes what a plain plan computes
for it in the same stream.
References: tests/samplernn_groups_cases.py; packings: tests/samplernn_packed_cases.py."""
import numpy as np
import pytest

from oracle import samplernn_ref as S
from tests import samplernn_groups_cases as GC
from tests import samplernn_packed_cases as PC
from tests import samplernn_sampling_cases as SC
from tests.test_gpu_samplernn import _greedy_follows_oracle
from tests.test_gpu_samplernn_groups import _model, _plan
from tests.test_gpu_samplernn_packed import _equal_pieces, _pieces_follow_oracle, _standalone, _utterances

pytestmark = pytest.mark.gpu

SWITCH = "PARROT_SR_PERSIST_GROUPS"
BADARG = 10001   # PARROT_ERR_BADARG
B, N = 5, 10     # the greedy cases: five streams (one team of the persistent kernel and one stream of the next), ten frames


def _feats(feats, n, b):
    return np.asarray(feats[:n, :b], dtype=np.float32)


def _one_shot(tt, feats, groups, **kw):
    with _plan(tt, feats.shape[1], feats.shape[0], groups, **kw) as gen:
        out = gen.generate(feats).cpu().numpy().copy()
        return out, gen.ws['logits'].detach().cpu().numpy().copy()


def _in_segments(tt, feats, groups, lens, slots=None, **kw):
    """The run of `feats` as calls of lens[0], lens[1], ... frames on one plan of `slots` slots (default: the longest
    call + 1): (samples [B, 80 N], last step's logits)."""
    assert sum(lens) == feats.shape[0] - 1
    with _plan(tt, feats.shape[1], slots or max(lens) + 1, groups, **kw) as gen:
        parts = [gen.generate(feats[:lens[0] + 1], n_frames=lens[0]).cpu().numpy()]
        done = lens[0] + 1
        for k in lens[1:]:
            parts.append(gen.generate(feats[done:done + k], resume=True, n_frames=k).cpu().numpy())
            assert parts[-1].shape == (feats.shape[1], 80 * k) and parts[-1].dtype == np.int32
            done += k
        return np.concatenate(parts, axis=1), gen.ws['logits'].detach().cpu().numpy().copy()


def _same(got, want, what):
    assert got[0].shape == want[0].shape
    assert np.array_equal(got[0], want[0]), f"{what}: {(got[0] != want[0]).sum()} samples differ, first at " \
                                             f"{np.argwhere(got[0] != want[0])[0].tolist()}"
    assert np.array_equal(got[1], want[1]), f"{what}: the last step's logits differ"


# ---- 1. segments == the run in one piece, greedy ------------------------------------------------------------------------
SEGMENTINGS = {"S1": ([1] * 9, None), "S3": ([3, 3, 3], None), "S4": ([4, 4, 1], None), "S8": ([8, 1], None),
               "mixed": ([2, 4, 1, 2], 5)}
_greedy = {}


def _greedy_one_shot(tt, feats, use_graph):
    if use_graph not in _greedy:
        _greedy[use_graph] = _one_shot(tt, feats, 1, temperature=0.0, use_graph=use_graph)
    return _greedy[use_graph]


@pytest.mark.parametrize("use_graph", [True, False])
def test_segments_equal_one_shot(dev, use_graph, monkeypatch):
    """S = 1: every period behind a boundary; S = 8: the chunk graph, then the single period; mixed: the tail slot of a
    five-slot ring differs from call to call.  (Scratch builds that recomputed gpre at a boundary, or invalidated the
    carry instead of re-keying it, still passed at this width: what they change is the last bit of one step's
    pre-activations, and no argmax turned on it.  The build without the draw origin fails test_seeded_draws.)"""
    p, feats, _, _ = GC.gru_reference()
    feats = _feats(feats, N, B)
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p) as tt:
        want = _greedy_one_shot(tt, feats, use_graph)
        assert want[0].shape == (B, 80 * N) and (want[0][:, :80] == 128).all()
        for name, (lens, slots) in SEGMENTINGS.items():
            got = _in_segments(tt, feats, 1, lens, slots, temperature=0.0, use_graph=use_graph)
            _same(got, want, f"{name}, use_graph={use_graph}")
        _same(_greedy_one_shot(tt, feats, True), _greedy_one_shot(tt, feats, False), "graph against eager")


# ---- 2. seeded draws ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("persist", [True, False])
def test_seeded_draws(dev, persist, monkeypatch):
    """The draw of a sample is keyed by its index in the whole run (the draw origin), not by its place in the ring."""
    c = S.config(DIM=GC.DIM, EMB_SIZE=GC.EMB)
    p = S.init_params(c, seed=GC.DRAW_PARAM_SEED, perturb=0.25)
    feats = SC.features(N, B, GC.DRAW_FEAT_SEED).numpy().astype(np.float32)
    monkeypatch.delenv(SWITCH, raising=False)
    if not persist:
        monkeypatch.setenv("PARROT_SR_PERSIST", "0")
    g = 1 if persist else 0
    with _model(dev, p) as tt:
        want = _one_shot(tt, feats, g, temperature=1.0, seed=GC.DRAW_SEEDS[0])
        got = _in_segments(tt, feats, g, [3, 3, 3], temperature=1.0, seed=GC.DRAW_SEEDS[0])
        other = _in_segments(tt, feats, g, [3, 3, 3], temperature=1.0, seed=GC.DRAW_SEEDS[1])
    _same(got, want, f"seeded, persistent={persist}")
    assert not np.array_equal(other[0], got[0])
    assert len(np.unique(got[0][:, 80:])) > 20 and got[0].min() >= 0 and got[0].max() <= 255


# ---- 3. row groups ------------------------------------------------------------------------------------------------------
def test_row_groups(dev, monkeypatch):
    p, feats, _, _ = GC.gru_reference()
    feats = _feats(feats, N, 37)
    monkeypatch.setenv(SWITCH, "2")
    with _model(dev, p) as tt:
        want = _one_shot(tt, feats, 2, temperature=0.0)
        _same(_in_segments(tt, feats, 2, [4, 4, 1], temperature=0.0), want, "two row groups")


# ---- 4. the launch path, a narrow model ---------------------------------------------------------------------------------
def test_launch_path(dev, monkeypatch):
    p, feats, _, _ = GC.gru_reference()
    feats = _feats(feats, N, B)
    monkeypatch.setenv("PARROT_SR_PERSIST", "0")
    with _model(dev, p) as tt:
        want = _one_shot(tt, feats, 0, temperature=0.0)
        _same(_in_segments(tt, feats, 0, [3, 3, 3], temperature=0.0), want, "launch path")


def test_dim32(dev, monkeypatch):
    c = S.config(DIM=32, EMB_SIZE=8)
    p = S.init_params(c, seed=GC.GRU_SEEDS[0], perturb=0.25)
    feats = SC.features(4, 3, GC.GRU_SEEDS[1]).numpy().astype(np.float32)
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p, DIM=32, EMB_SIZE=8) as tt:
        want = _one_shot(tt, feats, 0, temperature=0.0)
        _same(_in_segments(tt, feats, 0, [1, 1, 1], temperature=0.0), want, "DIM 32")


# ---- 5. stacked LSTM tiers ----------------------------------------------------------------------------------------------
def test_stacked_lstm_tiers(dev, monkeypatch):
    p, feats, _, _ = GC.stacked_reference()
    feats = _feats(feats, 3, B)
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p, RNN_TYPE='LSTM', N_RNN=2) as tt:
        want = _one_shot(tt, feats, 1, temperature=0.0)
        _same(_in_segments(tt, feats, 1, [1, 1], temperature=0.0), want, "stacked LSTM")


# ---- 6. along the float64 oracle ----------------------------------------------------------------------------------------
def test_segments_follow_oracle(dev, monkeypatch):
    p, feats, ref, ref_logits = GC.gru_reference()
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p) as tt:
        out, _ = _in_segments(tt, _feats(feats, N, B), 1, [3, 3, 3], temperature=0.0)
    assert (out[:, :80] == 128).all()
    _greedy_follows_oracle(out, ref[:B, :80 * N], ref_logits[:B, :80 * (N - 1)], B, slack_rows=1)


# ---- 7. nothing leaks ---------------------------------------------------------------------------------------------------
def test_nothing_leaks(dev, monkeypatch):
    p, feats, _, _ = GC.gru_reference()
    feats = _feats(feats, N, B)
    feats2 = SC.features(N, B, GC.FEAT_SEED_2).numpy().astype(np.float32)
    T = 7
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p) as tt:
        want = _greedy_one_shot(tt, feats, True)
        with _plan(tt, B, T, 1, temperature=0.0) as gen:
            # a plain run of T frames, then three more: the run of T + 3 in one piece
            head = gen.generate(feats[:T]).cpu().numpy().copy()
            tail = gen.generate(feats[T:T + 3], resume=True, n_frames=3).cpu().numpy()
            assert np.array_equal(np.concatenate([head, tail], axis=1), want[0])
            assert np.array_equal(gen.ws['logits'].detach().cpu().numpy(), want[1])
            # and a plain run on the plan that has run segments: a fresh plan's
            again = gen.generate(feats2[:T]).cpu().numpy().copy()
        with _plan(tt, B, T, 1, temperature=0.0) as gen:
            fresh = gen.generate(feats2[:T]).cpu().numpy().copy()
    assert np.array_equal(again, fresh) and not np.array_equal(again, head)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(dev, monkeypatch):
    from parrot_amd import _lib
    from parrot_amd import ops as hip
    p, feats, _, _ = GC.gru_reference()
    feats = _feats(feats, N, B)
    T = 4
    run_segment = _lib.load().samplernn_generate_run_segment
    monkeypatch.delenv(SWITCH, raising=False)

    def untouched(gen, call, *a, **kw):
        before = gen.ws['samples'].clone(), gen.ws['tbase'].clone(), gen.ws['features'].clone()
        with pytest.raises(ValueError):
            call(*a, **kw)
        after = gen.ws['samples'], gen.ws['tbase'], gen.ws['features']
        assert all(bool((x == y).all()) for x, y in zip(before, after))

    with _model(dev, p) as tt:
        with _plan(tt, B, T, 1, temperature=0.0) as gen:
            untouched(gen, gen.generate, feats[:2], resume=True, n_frames=2)        # nothing to resume
            assert run_segment(gen.plan, 2, 1, hip._stream()) == BADARG
            for k in (0, T):
                untouched(gen, gen.generate, feats[:k + 1], n_frames=k)
                assert run_segment(gen.plan, k, 0, hip._stream()) == BADARG
            untouched(gen, gen.generate, feats[:2], n_frames=2)                     # rows: 3 wanted
            gen.generate(feats[:3], n_frames=2)
            for k in (0, T):
                untouched(gen, gen.generate, feats[:k], resume=True, n_frames=k)
                assert run_segment(gen.plan, k, 1, hip._stream()) == BADARG
            untouched(gen, gen.generate, feats[:3], resume=True, n_frames=2)        # rows: 2 wanted
            untouched(gen, gen.generate, feats[:2], np.zeros((2, B), np.int32), resume=True, n_frames=2)  # not packed
            assert gen.generate(feats[3:5], resume=True, n_frames=2).shape == (B, 160)
        with _plan(tt, B, T, 1, temperature=0.0, packed=True) as gen:
            gen.generate(feats[:3], np.zeros((3, B), np.int32), n_frames=2)
            untouched(gen, gen.generate, feats[:2], resume=True, n_frames=2)        # starts missing
            untouched(gen, gen.generate, feats[:2], np.zeros((3, B), np.int32), resume=True, n_frames=2)


# ---- 9. continuous admission --------------------------------------------------------------------------------------------
def _admit(tt, case, utts, first, steps_between, segment_frames, **kw):
    """Submits utts[:first], runs `steps_between` steps, submits the rest and drains: (pieces per ticket, the Packing the
    scheduler's record amounts to)."""
    sg = tt.StreamingGenerator(case.B, segment_frames, temperature=0.0, **kw)
    try:
        assert sg.gen.persistent and sg.gen.persist_groups == 1
        chunks = {}
        assert [sg.submit(u) for u in utts[:first]] == list(range(first))
        got = []
        for _ in range(steps_between):
            got += sg.step()
        assert [sg.submit(u) for u in utts[first:]] == list(range(first, len(utts)))
        got += sg.drain()
        assert sg.idle() and sg.step() == []
        finished = []
        for ticket, chunk, done in got:
            assert chunk.dtype == np.int32 and chunk.ndim == 1 and chunk.size % 80 == 0 and chunk.size > 0
            assert ticket not in finished, "chunks after done"
            chunks.setdefault(ticket, []).append(chunk)
            if done:
                finished.append(ticket)
        assert sorted(finished) == list(range(len(utts))), "done exactly once per ticket"
        pieces = [np.concatenate(chunks[i]) for i in range(len(utts))]
        stream = tuple(sg.record[i][0] for i in range(len(utts)))
        slot = tuple(sg.record[i][1] for i in range(len(utts)))
    finally:
        sg.close()
    for piece, u in zip(pieces, utts):
        assert piece.shape == (80 * u.shape[0],) and (piece[:80] == 128).all()
    T = max(s + n for s, n in zip(slot, case.lengths))
    return pieces, PC.Packing(case.lengths, stream, slot, T, case.B, case.min_len, case.max_len)


def test_continuous_admission(dev, monkeypatch):
    case = PC.GRU_PACKING
    p, feats, ref, ref_logits = GC.gru_reference()
    utts = _utterances(feats, case)
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p) as tt:
        pieces, own = _admit(tt, case, utts, 6, 2, 4)
        _equal_pieces(pieces, _standalone(tt, own, utts, 1), "continuous admission")
    _pieces_follow_oracle(pieces, ref, ref_logits, "continuous admission")


def test_continuous_admission_stacked_gru(dev, monkeypatch):
    case = PC.STACKED_PACKING
    p = S.init_params(S.config(DIM=GC.DIM, EMB_SIZE=GC.EMB, RNN_TYPE='GRU', N_RNN=2), seed=GC.STACKED_SEEDS[0], perturb=0.25)
    feats = SC.features(case.max_len, len(case.lengths), GC.STACKED_SEEDS[1]).numpy()
    utts = _utterances(feats, case)
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p, RNN_TYPE='GRU', N_RNN=2) as tt:
        pieces, own = _admit(tt, case, utts, 8, 2, 4)
        _equal_pieces(pieces, _standalone(tt, own, utts, 1), "continuous admission, stacked GRU")


# ---- 10. entry points ---------------------------------------------------------------------------------------------------
def test_entry_points(dev, monkeypatch, tmp_path):
    case = PC.GRU_PACKING
    p, feats, _, _ = GC.gru_reference()
    n = len(case.lengths)
    rect = _feats(feats, case.max_len, n)
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p) as tt:
        pieces = tt.generate_and_save_samples("t", path_to_save=str(tmp_path), features=rect, features_length=case.lengths,
                                              temperature=0.0, stream_frames=4, pack_streams=5)
        want, _ = _admit(tt, case, _utterances(feats, case), n, 0, 4)
        _equal_pieces(pieces, want, "generate_and_save_samples(stream_frames=4)")
        assert sorted(f.name for f in tmp_path.iterdir()) == sorted("sample_t_%d.wav" % i for i in range(n))
        # generate_stream over a rectangle longer than its plan
        full = _feats(feats, N, B)
        chunks = list(tt.generate_stream(full, 4, temperature=0.0))
        assert [c.shape for c in chunks] == [(B, 400), (B, 320), (B, 80)]
        assert np.array_equal(np.concatenate(chunks, axis=1), _greedy_one_shot(tt, full, True)[0])
