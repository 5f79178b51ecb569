"""Per-utterance seeds and temperatures of the SampleRNN generator (samplernn_generate_set_utterance_draws; the entries of
sr_pick_kernel in samplernn.hip and of srp_kernel's pick in sr_persist.hip; three_tier.DeviceGenerator(utterance_draws=True),
generate_packed(seeds=), StreamingGenerator(utterance_draws=True)).  Every equality is bit for bit on int32 samples: the
new key against the plan's default key, packed and streamed utterances against the same utterance carried alone in the
same stream, resumed segments against the run in one piece; and the drawn utterances along the float64 oracle.
Cases: tests/samplernn_utt_draw_cases.py (premises checked by tests/test_samplernn_utt_draws_cpu.py)."""
import numpy as np
import pytest

from oracle import samplernn_ref as S
from tests import samplernn_groups_cases as GC
from tests import samplernn_packed_cases as PC
from tests import samplernn_sampling_cases as SC
from tests import samplernn_utt_draw_cases as UC
from tests.test_gpu_samplernn import _greedy_follows_oracle
from tests.test_gpu_samplernn_groups import _model, _plan

pytestmark = pytest.mark.gpu

SWITCH = "PARROT_SR_PERSIST_GROUPS"


def _env(monkeypatch, groups, launches=False):
    if groups > 1:
        monkeypatch.setenv(SWITCH, str(groups))
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    if launches:
        monkeypatch.setenv("PARROT_SR_PERSIST", "0")
    else:
        monkeypatch.delenv("PARROT_SR_PERSIST", raising=False)


def _equal_pieces(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == np.int32, (what, i, a.shape, b.shape, a.dtype)
        assert np.array_equal(a, b), f"{what}: utterance {i} differs in {(a != b).sum()} of {a.size} samples, first at " \
                                     f"{int(np.nonzero(a != b)[0][0])}"


def _utterances(feats, lengths):
    feats = np.asarray(feats, dtype=np.float32)
    return [feats[:n, i].copy() for i, n in enumerate(lengths)]


# ---- 1. the new key with seeds[b] = s ^ K2 (b + 1) is the plan's default key ------------------------------------------------
# name: (DIM, EMB, B, T, groups (0: launches), model configuration, plan arguments, [(plan seed, temperature)])
NEW_IS_OLD = {
    "launch-D32-B3": (32, 8, 3, 3, 0, {}, {}, [(234, 0.5), (234, 1.0), (2 ** 63 + 5, 0.5), (2 ** 63 + 5, 1.0)]),
    "launch-D32-B8": (32, 8, 8, 3, 0, {}, {}, [(2 ** 63 + 5, 1.0)]),
    "persist-D256-B5": (256, 32, 5, 3, 1, {}, {}, [(234, 0.5), (234, 1.0), (2 ** 63 + 5, 0.5), (2 ** 63 + 5, 1.0)]),
    "groups-D256-B37": (256, 32, 37, 3, 2, {}, {}, [(234, 1.0), (2 ** 63 + 5, 0.5)]),
    "chunk-D256-B5-T10": (256, 32, 5, 10, 1, {}, {}, [(2 ** 63 + 5, 1.0)]),
    "eager-D256-B5": (256, 32, 5, 3, 1, {}, dict(use_graph=False), [(234, 0.5)]),
    "stacked-lstm-D256-B5": (256, 32, 5, 3, 1, dict(RNN_TYPE='LSTM', N_RNN=2), {}, [(234, 1.0)]),
}


@pytest.mark.parametrize("name", sorted(NEW_IS_OLD))
def test_new_mode_equals_old_mode(dev, name, monkeypatch):
    DIM, EMB, B, T, groups, cfg, kw, draws = NEW_IS_OLD[name]
    p = S.init_params(S.config(DIM=DIM, EMB_SIZE=EMB, **cfg), seed=GC.DRAW_PARAM_SEED, perturb=0.25)
    feats = SC.features(T, B, GC.DRAW_FEAT_SEED).numpy().astype(np.float32)
    _env(monkeypatch, groups)
    with _model(dev, p, DIM=DIM, EMB_SIZE=EMB, **cfg) as tt:
        for s, tau in draws:
            with _plan(tt, B, T, groups, temperature=tau, seed=s, **kw) as gen:
                old = gen.generate(feats).cpu().numpy().copy()
            with _plan(tt, B, T, groups, utterance_draws=True, **kw) as gen:
                seeds = [UC.old_key_seed(s, b) for b in range(B)]
                new = gen.generate(feats, seeds=seeds, temperatures=tau).cpu().numpy().copy()
                again = gen.generate(feats, seeds=np.array(seeds, dtype=np.uint64),
                                     temperatures=np.full(B, tau, dtype=np.float32)).cpu().numpy().copy()
            assert (old[:, :80] == 128).all() and len(np.unique(old[:, 80:])) > 20
            assert np.array_equal(new, old), f"{name} seed {s} temperature {tau}: {(new != old).sum()} samples differ, " \
                                             f"rows {sorted(set(np.nonzero(new != old)[0].tolist()))}"
            assert np.array_equal(again, new)


# ---- 2. all temperatures 0 in the mode == the packed run at temperature 0 -----------------------------------------------------
def test_zero_temperatures_are_the_greedy_packed_run(dev, monkeypatch):
    case = PC.GRU_PACKING
    p, feats, _, _ = GC.gru_reference()
    utts = _utterances(feats, case.lengths)
    _env(monkeypatch, 1)
    with _model(dev, p) as tt:
        want = tt.generate_packed(utts, n_streams=case.B, temperature=0.0)
        got = tt.generate_packed(utts, n_streams=case.B, temperature=1.0, seeds=UC.utt_seeds(len(utts)), temperatures=0.0)
    _equal_pieces(got, want, "temperatures 0")


# ---- 3. packed == standalone in the same stream ---------------------------------------------------------------------------------
def _packed(tt, case, utts, seeds, temps, groups, **kw):
    features, starts = tt.build_packed_inputs(utts, case.stream, case.first_slot, case.T, case.B)
    utt_seed, utt_temp = tt.build_packed_draws(seeds, temps, case.stream, case.first_slot, case.T, case.B)
    with _plan(tt, case.B, case.T, groups, packed=True, utterance_draws=True, **kw) as gen:
        samples = gen.generate(features, starts, seeds=utt_seed, temperatures=utt_temp).cpu().numpy().copy()
    return tt.unpack_samples(samples, case.lengths, case.stream, case.first_slot)


def _standalone(tt, B, groups, items, utts, seeds, temps, T, **kw):
    """{i: piece} for items = [(utterance i, stream)]: plain rectangles in the mode on ONE plan of B streams and T slots,
    every utterance carried alone in its stream (the streams never meet), an utterance per stream and rectangle."""
    pieces, left = {}, list(items)
    with _plan(tt, B, T, groups, utterance_draws=True, **kw) as gen:
        while left:
            rect, rest = {}, []
            for i, b in left:
                if b in rect:
                    rest.append((i, b))
                else:
                    rect[b] = i
            left = rest
            feats = np.zeros((T, B, 63), dtype=np.float32)
            sd, tp = [0] * B, np.zeros(B, dtype=np.float32)
            for b, i in rect.items():
                feats[:utts[i].shape[0], b] = utts[i]
                sd[b], tp[b] = seeds[i], temps[i]
            out = gen.generate(feats, seeds=sd, temperatures=tp).cpu().numpy().copy()
            for b, i in rect.items():
                pieces[i] = out[b, :80 * utts[i].shape[0]]
    return pieces


def _rectangles_standalone(tt, case, utts, seeds, temps, groups, **kw):
    """The rectangles of PC.rectangles, each on a plain plan in the mode."""
    pieces = [None] * len(case.lengths)
    for rect in PC.rectangles(case):
        got = _standalone(tt, case.B, groups, [(i, b) for b, i in rect.items()], utts, seeds, temps,
                          max(2, max(case.lengths[i] for i in rect.values())), **kw)
        for i, piece in got.items():
            pieces[i] = piece
    return pieces


def _packed_equals_standalone(tt, case, utts, groups, what, **kw):
    n = len(case.lengths)
    seeds, temps = UC.utt_seeds(n), UC.utt_temperatures(n)
    pieces = _packed(tt, case, utts, seeds, temps, groups, **kw)
    _equal_pieces(pieces, _rectangles_standalone(tt, case, utts, seeds, temps, groups, **kw), what)
    drawn = [i for i in range(n) if temps[i] > 0]
    assert len(np.unique(np.concatenate([pieces[i][80:] for i in drawn]))) > 20
    return pieces, seeds, temps


_PIECES = {}     # what test 3 generated on the two paths of the oracle's packing, for test 6


def test_packed_equals_standalone_persistent(dev, monkeypatch):
    case = PC.GRU_PACKING
    assert case is UC.ORACLE_CASE
    p, feats, _, _ = GC.gru_reference()
    utts = _utterances(feats, case.lengths)
    _env(monkeypatch, 1)
    with _model(dev, p) as tt:
        pieces, seeds, temps = _packed_equals_standalone(tt, case, utts, 1, "persistent, one group")
        assert seeds == UC.ORACLE_SEEDS and temps == UC.ORACLE_TEMPERATURES
        _PIECES["persistent"] = pieces
        # the public entry point, with the packing it chooses itself
        got = tt.generate_packed(utts, n_streams=case.B, seeds=seeds, temperatures=temps)
        stream, first, T = tt.pack_utterances(case.lengths, case.B)
        own = PC.Packing(case.lengths, tuple(stream), tuple(first), T, case.B, case.min_len, case.max_len)
        _equal_pieces(got, _rectangles_standalone(tt, own, utts, seeds, temps, 1), "generate_packed")
        # the same utterance with the same seed first in its stream and behind another one: the same piece
        u, sd, tau = utts[0], seeds[2], 1.0
        first_ = PC.Packing((u.shape[0], 3), (1, 0), (0, 0), 8, case.B, 2, 5)
        later = PC.Packing((u.shape[0], 3, 3), (1, 1, 0), (3, 0, 0), 8, case.B, 2, 5)
        a = _packed(tt, first_, [u, utts[2]], [sd, 7], [tau, 0.5], 1)[0]
        b = _packed(tt, later, [u, utts[2], utts[5][:3]], [sd, 7, 8], [tau, 0.5, 2.0], 1)[0]
        assert np.array_equal(a, b), f"{(a != b).sum()} samples differ between slot 0 and slot 3 of stream 1"
        c = _packed(tt, later, [u, utts[2], utts[5][:3]], [sd + 1, 7, 8], [tau, 0.5, 2.0], 1)[0]
        assert not np.array_equal(a, c), "another seed draws the same utterance"


def test_packed_equals_standalone_launches(dev, monkeypatch):
    case = PC.GRU_PACKING
    p, feats, _, _ = GC.gru_reference()
    _env(monkeypatch, 1, launches=True)
    with _model(dev, p) as tt:
        _PIECES["launches"], _, _ = _packed_equals_standalone(tt, case, _utterances(feats, case.lengths), 0, "launch path")


def test_packed_equals_standalone_two_groups(dev, monkeypatch):
    case = PC.GROUPS_PACKING
    p, feats, _, _ = GC.gru_reference()
    _env(monkeypatch, 2)
    with _model(dev, p) as tt:
        _packed_equals_standalone(tt, case, _utterances(feats, case.lengths), 2, "two row groups")


def test_packed_equals_standalone_stacked(dev, monkeypatch):
    case = PC.STACKED_PACKING
    p, feats, _, _ = GC.stacked_reference()
    _env(monkeypatch, 1)
    with _model(dev, p, RNN_TYPE='LSTM', N_RNN=2) as tt:
        _packed_equals_standalone(tt, case, _utterances(feats, case.lengths), 1, "stacked LSTM")


# ---- 4. streaming -----------------------------------------------------------------------------------------------------------------
def test_streaming_equals_standalone(dev, monkeypatch):
    p, feats, _, _ = GC.gru_reference()
    B, lengths = UC.STREAM_B, UC.STREAM_LENGTHS
    utts = _utterances(feats, lengths)
    seeds, temps = UC.utt_seeds(len(utts)), UC.utt_temperatures(len(utts))
    _env(monkeypatch, 1)
    with _model(dev, p) as tt:
        runs = {}
        for S_ in (2, 5):
            for order in (None, UC.STREAM_ORDER_2):
                sg = tt.StreamingGenerator(B, S_, utterance_draws=True)
                try:
                    assert sg.gen.persistent
                    runs[(S_, order)] = UC.drain(sg, utts, seeds, temps, order)
                finally:
                    sg.close()
        wanted = sorted({(i, b) for _, stream, _ in runs.values() for i, b in stream.items()})
        alone = {}
        for b in range(B):   # (an utterance may be wanted in several streams: one _standalone call per stream keeps them apart)
            items = [(i, bb) for i, bb in wanted if bb == b]
            alone.update({(i, b): piece for i, piece in _standalone(tt, B, 1, items, utts, seeds, temps, max(lengths)).items()})
    for (S_, order), (got, stream, slot) in runs.items():
        for i in range(len(utts)):
            want = alone[(i, stream[i])]
            assert got[i].dtype == np.int32 and got[i].shape == want.shape
            assert np.array_equal(got[i], want), f"segments of {S_}, order {order}: utterance {i} in stream {stream[i]} " \
                                                 f"(prefix slot {slot[i]}) differs in {(got[i] != want).sum()} samples"
    for S_ in (2, 5):
        (a, sa, la), (b, sb, lb) = runs[(S_, None)], runs[(S_, UC.STREAM_ORDER_2)]
        same = [i for i in sa if sa[i] == sb[i]]
        assert [i for i in same if la[i] != lb[i]]
        for i in same:
            assert np.array_equal(a[i], b[i])


# ---- 5. resumed segments of a plain plan in the mode == the run in one piece ----------------------------------------------------
def test_segments_equal_one_piece(dev, monkeypatch):
    p, feats, _, _ = GC.gru_reference()
    B, N, S_ = 5, 7, 2
    feats = np.asarray(feats[:N, :B], dtype=np.float32)
    seeds, temps = UC.utt_seeds(B, salt=50), UC.utt_temperatures(B + 1)[1:]
    _env(monkeypatch, 1)
    with _model(dev, p) as tt:
        with _plan(tt, B, N, 1, utterance_draws=True) as gen:
            whole = gen.generate(feats, seeds=seeds, temperatures=temps).cpu().numpy().copy()
        with _plan(tt, B, S_ + 1, 1, utterance_draws=True) as gen:
            parts = [gen.generate(feats[:S_ + 1], n_frames=S_, seeds=seeds, temperatures=temps).cpu().numpy()]
            done = S_ + 1
            while done < N:
                k = min(S_, N - done)
                parts.append(gen.generate(feats[done:done + k], resume=True, n_frames=k).cpu().numpy())
                done += k
            with pytest.raises(ValueError):     # a plain plan takes seeds with resume=False only
                gen.generate(feats[:S_], resume=True, n_frames=S_, seeds=seeds, temperatures=temps)
    got = np.concatenate(parts, axis=1)
    assert np.array_equal(got, whole), f"{(got != whole).sum()} samples differ, first column {np.nonzero(got != whole)[1].min()}"
    assert len(np.unique(whole[:, 80:])) > 20


# ---- 6. the drawn utterances follow the float64 oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["persistent", "launches"])
def test_pieces_follow_oracle(dev, path, monkeypatch):
    """The pieces test 3 generated for PC.GRU_PACKING (generated here when that test has not run).  A drawn piece may leave
    the oracle's trajectory only at a draw whose u01 is within 2e-5 max|logit| / (2 temperature) + SC.DELTA of a boundary
    of the oracle's CDF (SC.draws_follow_oracle), an arg-max piece only at a near-tie (_greedy_follows_oracle); at most
    SC.traj_slack_rows(n) of the n pieces leave."""
    case = UC.ORACLE_CASE
    pieces = _PIECES.get(path)
    if pieces is None:
        p, feats, _, _ = GC.gru_reference()
        _env(monkeypatch, 1, launches=path == "launches")
        with _model(dev, p) as tt:
            pieces = _packed(tt, case, _utterances(feats, case.lengths), UC.ORACLE_SEEDS, UC.ORACLE_TEMPERATURES,
                             1 if path == "persistent" else 0)
    n, left = len(pieces), []
    for i, piece in enumerate(pieces):
        ref, ref_logits, oseed = UC.oracle_piece(i)
        temp = UC.ORACLE_TEMPERATURES[i]
        assert piece.shape == ref.shape and (piece[:80] == 128).all() and piece.min() >= 0 and piece.max() <= 255
        if temp > 0:
            exact, where = SC.draws_follow_oracle(piece[None], ref[None], ref_logits[None], temp, oseed, 1)
        else:
            exact, where = _greedy_follows_oracle(piece[None], ref[None], ref_logits[None], 1, slack_rows=1), None
        if not exact:
            left.append((i, temp, where))
    print(f"UTT-GPU {path}: {n - len(left)} of {n} utterances identical to the float64 oracle; left: {left}")
    assert len(left) <= SC.traj_slack_rows(n), f"{len(left)} of {n} utterances leave the oracle: {left}"


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(dev, monkeypatch):
    from parrot_amd._lib import HipCallError
    p, feats, _, _ = GC.gru_reference()
    B, T = 5, 3
    feats = np.asarray(feats[:T, :B], dtype=np.float32)
    seeds, temps = UC.utt_seeds(B), np.ones(B, dtype=np.float32)
    _env(monkeypatch, 1)
    with _model(dev, p) as tt:
        with _plan(tt, B, T, 1, utterance_draws=True) as gen:
            gen.set_utterance_draws()                  # before the first run: allowed again
            with pytest.raises(ValueError):
                gen.generate(feats)
            with pytest.raises(ValueError):
                gen.generate(feats, seeds=seeds)
            with pytest.raises(ValueError):
                gen.generate(feats, seeds=seeds[:-1], temperatures=temps)
            gen.generate(feats, seeds=seeds, temperatures=temps)
            with pytest.raises(HipCallError):
                gen.set_utterance_draws()              # the period graphs hold the pointers by value
        with _plan(tt, B, T, 1, temperature=1.0) as gen:
            with pytest.raises(ValueError):
                gen.generate(feats, seeds=seeds, temperatures=temps)
            with pytest.raises(ValueError):
                gen.generate(feats, temperatures=temps)


# ---- 8. the streams, observed -------------------------------------------------------------------------------------------------
def test_streams_observed(dev, monkeypatch):
    """The same utterance, seed and temperature in every stream of one plain plan.  P0: all rows equal at temperature 0
    outside the mode (the parent's behaviour); P1: all rows equal at temperature 1 in the mode.  Where the arithmetic does
    not depend on the row, the key must not either."""
    p, feats, _, _ = GC.gru_reference()
    B, T = 5, 3
    feats = np.repeat(np.asarray(feats[:T, :1], dtype=np.float32), B, axis=1)
    _env(monkeypatch, 1)
    with _model(dev, p) as tt:
        with _plan(tt, B, T, 1, temperature=0.0) as gen:
            greedy = gen.generate(feats).cpu().numpy().copy()
        with _plan(tt, B, T, 1, utterance_draws=True) as gen:
            drawn = gen.generate(feats, seeds=[UC.SEEDS[2]] * B, temperatures=1.0).cpu().numpy().copy()
        with _plan(tt, B, T, 1, temperature=1.0, seed=UC.SEEDS[2]) as gen:
            keyed = gen.generate(feats).cpu().numpy().copy()
    P0 = bool((greedy == greedy[0]).all())
    P1 = bool((drawn == drawn[0]).all())
    print(f"UTT-GPU streams observed: P0 (arg-max rows equal) = {P0}, P1 (drawn rows equal in the mode) = {P1}")
    assert P1 or not P0
    assert len({keyed[b].tobytes() for b in range(B)}) == B   # the default key has its stream term


# ---- 9. the host surface: generate_and_save_samples(utterance_seed=S) ---------------------------------------------------------
def test_generate_and_save_samples_takes_a_seed(dev, monkeypatch):
    p, feats, _, _ = GC.gru_reference()
    lengths = [3, 5, 2, 4, 2]
    feats = np.asarray(feats[:5, :len(lengths)], dtype=np.float32)
    utts = [feats[:n, i] for i, n in enumerate(lengths)]
    _env(monkeypatch, 1)
    with _model(dev, p) as tt:
        seeds = [tt.utterance_seed(99, i) for i in range(len(lengths))]
        packed = tt.generate_and_save_samples("t", features=feats, features_length=lengths, temperature=1.0, pack_streams=3,
                                              utterance_seed=99)
        _equal_pieces(packed, tt.generate_packed(utts, n_streams=3, seeds=seeds, temperatures=1.0), "pack_streams")
        streamed = tt.generate_and_save_samples("t", features=feats, features_length=lengths, temperature=1.0,
                                                pack_streams=3, stream_frames=2, utterance_seed=99)
        assert [x.shape for x in streamed] == [x.shape for x in packed]
        rect = tt.generate_and_save_samples("t", features=feats, features_length=lengths, temperature=1.0, utterance_seed=99)
        with _plan(tt, len(lengths), 5, 1, utterance_draws=True) as gen:
            want = gen.generate(feats, seeds=seeds, temperatures=1.0).cpu().numpy().copy()
        assert np.array_equal(rect, want)
        other = tt.generate_and_save_samples("t", features=feats, features_length=lengths, temperature=1.0, utterance_seed=100)
        assert not np.array_equal(other, rect)
