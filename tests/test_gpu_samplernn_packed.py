"""Several utterances one after the other in each stream of ONE SampleRNN generation plan (SampleRnnGenDesc::starts,
sr_start_kernel in samplernn.hip; three_tier.DeviceGenerator(packed=True), generate_packed): a stream that begins an
utterance inside the loop computes what a run of that utterance on its own computes -- bit for bit against a plain plan
that carries the utterance in the same stream, and along the float64 oracle -- on the persistent sample kernel (one and
two row groups), on the launch path and with stacked tiers, through the captured graphs and eagerly.
Packings: tests/samplernn_packed_cases.py (premises checked by tests/test_samplernn_packed_cpu.py); references:
tests/samplernn_groups_cases.py."""
import numpy as np
import pytest

from oracle import samplernn_ref as S
from tests import samplernn_groups_cases as GC
from tests import samplernn_packed_cases as PC
from tests import samplernn_sampling_cases as SC
from tests.test_gpu_samplernn import _greedy_follows_oracle
from tests.test_gpu_samplernn_groups import _model, _plan

pytestmark = pytest.mark.gpu

SWITCH = "PARROT_SR_PERSIST_GROUPS"


def _utterances(feats, case):
    feats = np.asarray(feats, dtype=np.float32)
    return [feats[:n, i].copy() for i, n in enumerate(case.lengths)]


def _packed(tt, case, utts, groups, clear=(), **kw):
    """(samples [B, 80 T], pieces) of the packed run; `clear`: (frame, stream) start flags taken out again."""
    features, starts = tt.build_packed_inputs(utts, case.stream, case.first_slot, case.T, case.B)
    for f, b in clear:
        assert starts[f, b] == 1
        starts[f, b] = 0
    with _plan(tt, case.B, case.T, groups, temperature=0.0, packed=True, **kw) as gen:
        samples = gen.generate(features, starts).cpu().numpy().copy()
    return samples, tt.unpack_samples(samples, case.lengths, case.stream, case.first_slot)


def _standalone(tt, case, utts, groups, **kw):
    """Every utterance from a plain plan of the same batch, carried in the stream that carries it in the packed run: the
    streams' k-th utterances together as rectangle k."""
    pieces = [None] * len(case.lengths)
    for rect in PC.rectangles(case):
        T = max(2, max(case.lengths[i] for i in rect.values()))
        feats = np.zeros((T, case.B, 63), dtype=np.float32)
        for b, i in rect.items():
            feats[:case.lengths[i], b] = utts[i]
        with _plan(tt, case.B, T, groups, temperature=0.0, **kw) as gen:
            out = gen.generate(feats).cpu().numpy().copy()
        for b, i in rect.items():
            pieces[i] = out[b, :80 * case.lengths[i]]
    return pieces


def _equal_pieces(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == np.int32, (i, a.shape, b.shape)
        assert np.array_equal(a, b), f"{what}: utterance {i} differs in {(a != b).sum()} of {a.size} samples, first at " \
                                     f"{int(np.nonzero(a != b)[0][0])}"


def _pieces_follow_oracle(pieces, ref, ref_logits, what):
    """Per utterance the rule of _greedy_follows_oracle (an utterance may leave the float64 trajectory only at a near-tie of
    the oracle's top two logits); at most one utterance per started 16 may leave it."""
    left = 0
    for i, piece in enumerate(pieces):
        n = piece.shape[0] // 80
        assert (piece[:80] == 128).all() and piece.min() >= 0 and piece.max() <= 255
        exact = _greedy_follows_oracle(piece[None], ref[i:i + 1, :80 * n], ref_logits[i:i + 1, :80 * (n - 1)], 1, slack_rows=1)
        left += 1 - len(exact)
    print(f"PACKED-GPU {what}: utterances identical {len(pieces) - left} of {len(pieces)}")
    assert left <= PC.slack_utterances(len(pieces)), f"{left} of {len(pieces)} utterances leave the oracle"


def _checks_1_and_2(tt, case, utts, ref, ref_logits, groups, what, **kw):
    samples, pieces = _packed(tt, case, utts, groups, **kw)
    _equal_pieces(pieces, _standalone(tt, case, utts, groups, **kw), what)
    if ref is not None:
        _pieces_follow_oracle(pieces, ref, ref_logits, what)
    return samples, pieces


# ---- 1. packed == standalone, bit for bit -------------------------------------------------------------------------------
def test_packed_equals_standalone(dev, monkeypatch):
    case = PC.GRU_PACKING
    p, feats, _, _ = GC.gru_reference()
    utts = _utterances(feats, case)
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p) as tt:
        samples, pieces = _packed(tt, case, utts, 1)
        _equal_pieces(pieces, _standalone(tt, case, utts, 1), "persistent, one group")
        # two starts in one period inside one team (streams 0 and 1) beside a stream of that team that goes on: stream 2
        # computes what it computes without them (its team's carry is invalidated in that period, its history is not)
        without, _ = _packed(tt, case, utts, 1, clear=[(6, 0), (6, 1)])
        assert np.array_equal(samples[2], without[2]), f"{(samples[2] != without[2]).sum()} samples of stream 2 differ"
        assert np.array_equal(samples[3:], without[3:])
        assert np.array_equal(samples[:2, :400], without[:2, :400])
        # the public entry point, with the packing it chooses itself: utterance by utterance the same samples
        got = tt.generate_packed(utts, n_streams=case.B, temperature=0.0)
        stream, first, T = tt.pack_utterances(case.lengths, case.B)
        own = PC.Packing(case.lengths, tuple(stream), tuple(first), T, case.B, case.min_len, case.max_len)
        _equal_pieces(got, _standalone(tt, own, utts, 1), "generate_packed")


# ---- 2. packed follows the oracle ---------------------------------------------------------------------------------------
def test_packed_follows_oracle(dev, monkeypatch):
    case = PC.GRU_PACKING
    p, feats, ref, ref_logits = GC.gru_reference()
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p) as tt:
        _, pieces = _packed(tt, case, _utterances(feats, case), 1)
        _pieces_follow_oracle(pieces, ref, ref_logits, "persistent, one group")


# ---- 3. graph == eager, a plan used twice repeats itself ----------------------------------------------------------------
def test_graph_equals_eager_and_replay_equals_fresh(dev, monkeypatch):
    case = PC.GRU_PACKING
    p, feats, _, _ = GC.gru_reference()
    utts = _utterances(feats, case)
    # another packing of the same plan shape: the utterances in reverse order, placed by pack_utterances
    utts2 = utts[::-1]
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p) as tt:
        stream2, first2, T2 = tt.pack_utterances([u.shape[0] for u in utts2], case.B)
        assert T2 <= case.T
        in1 = tt.build_packed_inputs(utts, case.stream, case.first_slot, case.T, case.B)
        in2 = tt.build_packed_inputs(utts2, stream2, first2, case.T, case.B)
        assert not np.array_equal(in1[1], in2[1])
        outs = {}
        for use_graph in (True, False):
            with _plan(tt, case.B, case.T, 1, temperature=0.0, packed=True, use_graph=use_graph) as gen:
                outs[use_graph] = [gen.generate(*x).cpu().numpy().copy() for x in (in1, in2, in1)]
            assert np.array_equal(outs[use_graph][2], outs[use_graph][0]), "the plan's third call differs from its first"
        for a, b in zip(outs[True], outs[False]):
            assert np.array_equal(a, b), f"{(a != b).sum()} samples differ between graph replay and eager launches"
        assert not np.array_equal(outs[True][0], outs[True][1])
        with _plan(tt, case.B, case.T, 1, temperature=0.0, packed=True) as gen:
            fresh = gen.generate(*in2).cpu().numpy().copy()
        assert np.array_equal(fresh, outs[True][1]), f"{(fresh != outs[True][1]).sum()} samples differ from a fresh plan's"
        for use_graph in (True, False):
            got = tt.generate_packed(utts, n_streams=case.B, temperature=0.0, use_graph=use_graph)
            outs[("pieces", use_graph)] = got
        _equal_pieces(outs[("pieces", True)], outs[("pieces", False)], "generate_packed graph / eager")
        with pytest.raises(ValueError):
            with _plan(tt, case.B, case.T, 1, temperature=0.0, packed=True) as gen:
                gen.generate(in1[0])
        with pytest.raises(ValueError):
            with _plan(tt, case.B, case.T, 1, temperature=0.0) as gen:
                gen.generate(*in1)


# ---- 4. row groups ------------------------------------------------------------------------------------------------------
def test_row_groups(dev, monkeypatch):
    case = PC.GROUPS_PACKING
    p, feats, ref, ref_logits = GC.gru_reference()
    monkeypatch.setenv(SWITCH, "2")
    with _model(dev, p) as tt:
        with _plan(tt, case.B, case.T, 2, temperature=0.0, packed=True) as gen:
            assert gen.persist_groups == 2
        _checks_1_and_2(tt, case, _utterances(feats, case), ref, ref_logits, 2, "two row groups")


# ---- 5. the launch path and stacked tiers -------------------------------------------------------------------------------
def test_launch_path(dev, monkeypatch):
    case = PC.GRU_PACKING
    p, feats, ref, ref_logits = GC.gru_reference()
    monkeypatch.setenv("PARROT_SR_PERSIST", "0")
    with _model(dev, p) as tt:
        _checks_1_and_2(tt, case, _utterances(feats, case), ref, ref_logits, 0, "launch path")


def test_stacked_lstm_tiers(dev, monkeypatch):
    """Cell states and the [s | c] split of h0; no composed frame input, so the sample kernel's general next_in tail."""
    case = PC.STACKED_PACKING
    p, feats, ref, ref_logits = GC.stacked_reference()
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p, RNN_TYPE='LSTM', N_RNN=2) as tt:
        _checks_1_and_2(tt, case, _utterances(feats, case), ref, ref_logits, 1, "stacked LSTM")


def test_stacked_gru_tiers(dev, monkeypatch):
    case = PC.STACKED_PACKING
    p = S.init_params(S.config(DIM=GC.DIM, EMB_SIZE=GC.EMB, RNN_TYPE='GRU', N_RNN=2), seed=GC.STACKED_SEEDS[0], perturb=0.25)
    feats = SC.features(case.max_len, len(case.lengths), GC.STACKED_SEEDS[1]).numpy()
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p, RNN_TYPE='GRU', N_RNN=2) as tt:
        _checks_1_and_2(tt, case, _utterances(feats, case), None, None, 1, "stacked GRU")


# ---- 6. the default is untouched ----------------------------------------------------------------------------------------
def test_no_starts_is_the_plain_plan(dev, monkeypatch):
    case = PC.GRU_PACKING
    p, feats, _, _ = GC.gru_reference()
    feats = np.asarray(feats[:case.T, :case.B], dtype=np.float32)
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p) as tt:
        with _plan(tt, case.B, case.T, 1, temperature=0.0) as gen:
            plain = gen.generate(feats).cpu().numpy().copy()
            plain_last = gen.ws['logits'].detach().cpu().numpy().copy()
        with _plan(tt, case.B, case.T, 1, temperature=0.0, packed=True) as gen:
            packed = gen.generate(feats, np.zeros((case.T, case.B), dtype=np.int32)).cpu().numpy().copy()
            packed_last = gen.ws['logits'].detach().cpu().numpy().copy()
    assert np.array_equal(packed, plain)
    assert np.array_equal(packed_last, plain_last)


# ---- 7. the learned h0 is really used -----------------------------------------------------------------------------------
def test_a_cleared_start_changes_the_utterance(dev, monkeypatch):
    """perturb = 0.25 gives a non-zero h0, and the stream's history is not Q/2: without its start flag the utterance goes on
    from the state and the samples of the one before it -- a test of this file that passed without any reset would be void."""
    case = PC.GRU_PACKING
    p, feats, _, _ = GC.gru_reference()
    assert float(p['BigFrameLevel.h0'].abs().max()) > 0 and float(p['FrameLevel.h0'].abs().max()) > 0
    utts = _utterances(feats, case)
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p) as tt:
        _, with_flag = _packed(tt, case, utts, 1)
        _, cleared = _packed(tt, case, utts, 1, clear=[(6, 0)])
    i = [k for k in range(len(case.lengths)) if case.stream[k] == 0 and case.first_slot[k] == 5][0]
    assert not np.array_equal(with_flag[i], cleared[i])
    assert (with_flag[i][:80] == 128).all() and not (cleared[i][:80] == 128).all()
    for k in range(len(case.lengths)):
        if k != i:
            assert np.array_equal(with_flag[k], cleared[k]), k


# ---- 8. seeded draws ----------------------------------------------------------------------------------------------------
def test_seeded_draws(dev, monkeypatch):
    case = PC.GRU_PACKING
    p, feats, _, _ = GC.gru_reference()
    utts = _utterances(feats, case)
    utts = utts + [utts[0][:1]]     # and a one-frame utterance: its piece is the prefix alone
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p) as tt:
        outs = [tt.generate_packed(utts, n_streams=case.B, temperature=1.0, seed=seed) for seed in (77, 77, 78)]
    _equal_pieces(outs[0], outs[1], "same seed")
    assert any(not np.array_equal(a, b) for a, b in zip(outs[0], outs[2]))
    for piece, u in zip(outs[0], utts):
        assert piece.shape == (80 * u.shape[0],) and (piece[:80] == 128).all()
        assert piece.min() >= 0 and piece.max() <= 255
    assert len(np.unique(np.concatenate([x[80:] for x in outs[0]]))) > 20


# ---- 9. the host surface: generate_and_save_samples(pack_streams=N) ------------------------------------------------------
def test_generate_and_save_samples_packs(dev, monkeypatch, tmp_path):
    p, feats, _, _ = GC.gru_reference()
    lengths = [3, 5, 2, 4, 2, 5, 2]
    feats = np.asarray(feats[:5, :len(lengths)], dtype=np.float32)
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p) as tt:
        pieces = tt.generate_and_save_samples("t", path_to_save=str(tmp_path), features=feats, features_length=lengths,
                                              temperature=0.0, pack_streams=3)
        want = tt.generate_packed([feats[:n, i] for i, n in enumerate(lengths)], n_streams=3, temperature=0.0)
        rect = tt.generate_and_save_samples("r", features=feats, features_length=lengths, temperature=0.0)
    _equal_pieces(pieces, want, "generate_and_save_samples")
    assert [x.shape[0] for x in pieces] == [80 * n for n in lengths]
    assert sorted(f.name for f in tmp_path.iterdir()) == ["sample_t_%d.wav" % i for i in range(len(lengths))]
    assert isinstance(rect, np.ndarray) and rect.shape == (len(lengths), 400)     # the default: today's rectangle


# ---- 10. the descriptor's argument rule ---------------------------------------------------------------------------------
def test_starts_without_h0_is_refused(dev, monkeypatch):
    import ctypes as C
    from parrot_amd import _lib
    p, _, _, _ = GC.gru_reference()
    monkeypatch.delenv(SWITCH, raising=False)
    with _model(dev, p) as tt:
        with _plan(tt, 5, 3, 1, temperature=0.0, packed=True) as gen:
            assert gen.desc.starts and gen.desc.big_h0 and gen.desc.frm_h0
            for missing in ("big_h0", "frm_h0"):
                d = _lib.SampleRnnGenDesc.from_buffer_copy(gen.desc)
                d.persist_ws, d.persist_ws_floats = None, 0     # (a workspace belongs to one plan)
                setattr(d, missing, None)
                plan = C.c_void_p()
                assert _lib.load().samplernn_generate_create(C.byref(d), C.byref(plan)) == 10001   # PARROT_ERR_BADARG
                assert not plan.value
