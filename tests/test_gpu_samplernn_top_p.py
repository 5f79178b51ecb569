"""The top-p (nucleus) truncated draw of the SampleRNN generator (samplernn_generate_set_top_p,
samplernn_generate_set_utterance_top_p; DeviceGenerator(top_p=), generate(..., top_ps=)): `srp_topp_keep` (sr_common.h) in
wave 0 of `sr_pick_kernel` (samplernn.hip) and in waves 0..3 of `srp_kernel`'s pick (sr_persist.hip), in both draw modes,
alone and behind top-k.  Every draw against the float64 oracle of the nucleus and, bit for bit, against the top-k run with
k = the oracle's m; exact cases without tolerance (one big tie, a uniform of exactly 1.0); a small p against the arg-max;
off against the default; per-utterance values inside one team; resumed segments; a real trajectory; the batches above one
team; the refusals of the two setters.  Cases: tests/samplernn_top_p_cases.py (premises: tests/test_samplernn_top_p_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import samplernn_ref as S
from tests import samplernn_groups_cases as GC
from tests import samplernn_packed_cases as PC
from tests import samplernn_sampling_cases as SC
from tests import samplernn_top_k_cases as KC
from tests import samplernn_top_p_cases as NC
from tests import samplernn_utt_draw_cases as UC
from tests.test_gpu_samplernn_groups import _plan
from tests.test_gpu_samplernn_sampling import _check_bias_only_run, _model, _run
from tests.test_gpu_samplernn_top_k import _bias_model, _d256_model, _feats, _same
from tests.test_gpu_samplernn_utt_draws import _env, _equal_pieces, _utterances

pytestmark = pytest.mark.gpu

SEED = SC.SEEDS[1]   # (the one that guards the 64-bit field)


# ---- 1. and 2. draws against the oracle, and against top_k = m ----------------------------------------------------------
@pytest.mark.parametrize("mode", NC.MODES)
@pytest.mark.parametrize("temperature", SC.TEMPERATURES)
@pytest.mark.parametrize("pattern", SC.PATTERNS)
@pytest.mark.parametrize("shape", sorted(SC.BIAS_SHAPES))
def test_nucleus_draws_from_known_logits(dev, shape, pattern, temperature, mode):
    """p in NC.PS alone and behind top_k = 64.  Every pick against the float64 CDF of the oracle's nucleus at
    draw_u01(seed, t, b): inside the nucleus without any excuse; a mismatch only within DELTA (sequential) / DELTA_SCAN
    (scan) of a boundary and in at most 0.5 % of the draws.  And the run equals, bit for bit, the run with
    top_k = min(k, m), m the oracle's (every case lies farther than 2^-14 from a prefix mass: NC.case_m)."""
    s = SC.BIAS_SHAPES[shape]
    b4 = SC.b4_pattern(pattern)
    feats = SC.features(s.T, s.B).numpy()
    u = SC.u01_table(SEED, s.T, s.B)
    kw = dict(temperature=temperature, seed=SEED, draw_mode=mode)
    with _bias_model(dev, s, b4) as tt:
        by_k = {}
        for k in NC.WITH_K:
            for p in NC.PS:
                out, logits = _run(tt, s.B, s.T, feats, s.persistent, top_p=p, top_k=k, **kw)
                _check_bias_only_run(out, logits, b4, s.B)
                m, draws, excused, worst = NC.judge_draws(out[:, 80:], b4, temperature, p, k, u, mode)
                print(f"TOPP-GPU {shape} {pattern} T={temperature} {mode} p={p} k={k}: m {m}, draws {draws}, excused "
                      f"mismatches {excused} (worst {worst:.2e})")
                assert draws == 80 * (s.T - 1) * s.B and 1 <= m <= (k or SC.Q)
                if m not in by_k:
                    by_k[m] = _run(tt, s.B, s.T, feats, s.persistent, top_k=m, **kw)[0]
                _same(out, by_k[m], f"top_p = {p} behind top_k = {k} against top_k = {m}")
    if (pattern, temperature) == ("randn", 1.0):   # (the nucleus is taken of the top-k mass: the combined case discriminates)
        assert NC.nucleus_m(b4, 1.0, 0.9) == 65 and NC.nucleus_m(b4, 1.0, 0.9, 64) == 35
        assert not np.array_equal(by_k[65], by_k[35])


# ---- 3. exact cases, no tolerance ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", NC.MODES)
@pytest.mark.parametrize("shape", sorted(SC.EDGE_SHAPES))
def test_all_equal_logits(dev, shape, mode):
    """Every logit equal and p = 0.25: terms 1.0, integer masses, p 256 exact: m = 64, the kept set is codes 0 .. 63 (the tie
    at the cut-off goes to the low indices) and the pick is floor(64 u01) -- 63, not 255, where u01 is exactly 1.0."""
    s = SC.EDGE_SHAPES[shape]
    b4 = np.full(SC.Q, SC.EDGE_LOGIT, dtype=np.float32)
    feats = SC.features(s.T, s.B).numpy()
    m = NC.equal_logits_m()
    assert m == 64 and NC.nucleus_m(b4, 1.0, NC.EQUAL_P) == 64
    with _bias_model(dev, s, b4) as tt:
        for seed in SC.EDGE_SEEDS + tuple(KC.U1_SEEDS):
            u = SC.u01_table(seed, s.T, s.B)
            out, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=seed, draw_mode=mode, top_p=NC.EQUAL_P)
            _check_bias_only_run(out, logits, b4, s.B)
            want = KC.equal_logits_picks(m, u)
            assert np.array_equal(out[:, 80:], want), f"seed {seed}: {(out[:, 80:] != want).sum()} picks differ"
            assert out[:, 80:].max() == 63
            if seed in KC.U1_SEEDS:
                b, t = KC.U1_SEEDS[seed]
                assert u[b, t - 80] == 1.0 and out[b, t] == 63, f"seed {seed}: u01 == 1.0, pick {out[b, t]}"
        # behind top_k = 128: p of THAT mass -- codes 0 .. 31
        out, _ = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=SC.EDGE_SEEDS[0], draw_mode=mode,
                      top_p=NC.EQUAL_P, top_k=128)
        want = KC.equal_logits_picks(32, SC.u01_table(SC.EDGE_SEEDS[0], s.T, s.B))
        assert np.array_equal(out[:, 80:], want)


@pytest.mark.parametrize("mode", NC.MODES)
@pytest.mark.parametrize("shape", sorted(SC.EDGE_SHAPES))
def test_two_maxima_and_a_uniform_of_one(dev, shape, mode):
    """Maxima at 5, 69, 133, 200 and p = 0.25: the oracle's m is 2 with a margin above 0.05, the nucleus is {5, 69}: the pick
    is 5 where u01 < 0.5, else 69 -- also where u01 is exactly 1.0."""
    s = SC.EDGE_SHAPES[shape]
    b4, _ = SC.tie_pattern(KC.TWO_MAXIMA)
    assert NC.two_maxima_m() == 2
    feats = SC.features(s.T, s.B).numpy()
    with _bias_model(dev, s, b4) as tt:
        for seed in SC.EDGE_SEEDS[:1] + tuple(KC.U1_SEEDS):
            u = SC.u01_table(seed, s.T, s.B)
            out, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=seed, draw_mode=mode,
                               top_p=NC.TWO_MAXIMA_P)
            _check_bias_only_run(out, logits, b4, s.B)
            assert set(np.unique(out[:, 80:]).tolist()) <= {5, 69}
            want = KC.two_maxima_picks(u)
            assert np.array_equal(out[:, 80:], want), f"seed {seed}: {(out[:, 80:] != want).sum()} picks differ"


# ---- 4. a small p is the arg-max ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", NC.MODES)
@pytest.mark.parametrize("shape", sorted(SC.TIE_SHAPES))
def test_small_p_is_the_argmax(dev, shape, mode):
    s = SC.TIE_SHAPES[shape]
    feats = SC.features(s.T, s.B).numpy()
    patterns = [(name,) + SC.tie_pattern(name) for name in SC.TIE_MAXIMA] + [("randn", SC.b4_pattern("randn"), None)]
    for name, b4, want in patterns:
        assert NC.nucleus_m(b4, 1.0, NC.SMALL_P) == 1
        with _bias_model(dev, s, b4) as tt:
            small, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=SEED, draw_mode=mode, top_p=NC.SMALL_P)
            _check_bias_only_run(small, logits, b4, s.B)
            greedy, _ = _run(tt, s.B, s.T, feats, s.persistent, temperature=0.0, draw_mode=mode)
            _same(small, greedy, f"{name}: top_p = 2^-10 at temperature 1 against temperature 0")
            assert np.unique(small[:, 80:]).tolist() == [int(np.argmax(b4)) if want is None else want]


# ---- 5. off is off ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", NC.MODES)
@pytest.mark.parametrize("name", sorted(SC.TRAJ_SHAPES))
def test_off_is_the_default(dev, name, mode):
    s = SC.TRAJ_SHAPES[name]
    p = S.init_params(S.config(DIM=s.DIM, EMB_SIZE=s.EMB), seed=s.param_seed, perturb=0.25)
    feats = SC.features(s.T, s.B, s.feat_seed).numpy()
    kw = dict(temperature=1.0, seed=SC.TRAJ_SEED, draw_mode=mode)
    with _model(dev, s.DIM, s.EMB, p) as tt:
        default, _ = _run(tt, s.B, s.T, feats, s.persistent, **kw)
        for top_p in (0, 0.0, 1.0, 1.5):
            out, _ = _run(tt, s.B, s.T, feats, s.persistent, top_p=top_p, **kw)
            _same(out, default, f"top_p = {top_p} against the keyword left out")
        cut, _ = _run(tt, s.B, s.T, feats, s.persistent, top_p=0.5, **kw)
    assert len(np.unique(default[:, 80:])) > 20 and not np.array_equal(cut, default)


# ---- 6. per utterance ---------------------------------------------------------------------------------------------------
def _packed(tt, case, utts, seeds, temps, ks, ps, groups, **kw):
    features, starts = tt.build_packed_inputs(utts, case.stream, case.first_slot, case.T, case.B)
    utt_seed, utt_temp = tt.build_packed_draws(seeds, temps, case.stream, case.first_slot, case.T, case.B)
    utt_top_k = tt.build_packed_top_k(ks, case.stream, case.first_slot, case.T, case.B)
    utt_top_p = tt.build_packed_top_p(ps, case.stream, case.first_slot, case.T, case.B)
    with _plan(tt, case.B, case.T, groups, packed=True, utterance_draws=True, **kw) as gen:
        samples = gen.generate(features, starts, seeds=utt_seed, temperatures=utt_temp, top_ks=utt_top_k,
                               top_ps=utt_top_p).cpu().numpy().copy()
    return tt.unpack_samples(samples, case.lengths, case.stream, case.first_slot)


def _standalone(tt, B, groups, items, utts, seeds, temps, ks, ps, T, **kw):
    """{i: piece} for items = [(utterance i, stream)]: each utterance carried alone in its stream of a plain plan of B
    streams with its seed, temperature, top_k and top_p."""
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
            sd, tp, tk, pp = [0] * B, np.zeros(B, dtype=np.float32), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.float32)
            for b, i in rect.items():
                feats[:utts[i].shape[0], b] = utts[i]
                sd[b], tp[b], tk[b], pp[b] = seeds[i], temps[i], ks[i], ps[i]
            out = gen.generate(feats, seeds=sd, temperatures=tp, top_ks=tk, top_ps=pp).cpu().numpy().copy()
            for b, i in rect.items():
                pieces[i] = out[b, :80 * utts[i].shape[0]]
    return pieces


def _mixed_utterances():
    case = PC.GRU_PACKING
    n = len(case.lengths)
    assert case.B == 5 and n >= 8     # streams 0 .. 3 form one team of the persistent kernel, stream 4 a partial one
    utts = _utterances(_feats(case.max_len, n), case.lengths)
    ks, temps, ps = KC.utt_top_ks(n), KC.utt_temperatures(n), NC.utt_top_ps(n)
    team0 = [i for i in range(n) if case.stream[i] < 4 and case.first_slot[i] == 0]
    assert len({ps[i] for i in team0}) >= 3 and len({ks[i] for i in team0}) == 4 and len({temps[i] for i in team0}) == 3
    return case, utts, UC.utt_seeds(n), temps, ks, ps


@pytest.mark.parametrize("path,mode", [("persistent", "sequential"), ("persistent", "scan"), ("launches", "sequential")])
def test_packed_utterances_equal_standalone(dev, path, mode, monkeypatch):
    """Utterances with p in {0, 0.9, 2^-10, 0.5, 1}, k in {0, 1, 8, 64} and temperatures in {0.5, 1, 2} mixed inside one
    team: each equals, bit for bit, the plain plan that carries it alone in the same stream with the same values."""
    case, utts, seeds, temps, ks, ps = _mixed_utterances()
    groups = 1 if path == "persistent" else 0
    _env(monkeypatch, 1, launches=path == "launches")
    with _d256_model(dev) as tt:
        pieces = _packed(tt, case, utts, seeds, temps, ks, ps, groups, draw_mode=mode)
        alone = [None] * len(utts)
        for rect in PC.rectangles(case):
            T = max(2, max(case.lengths[i] for i in rect.values()))
            got = _standalone(tt, case.B, groups, [(i, b) for b, i in rect.items()], utts, seeds, temps, ks, ps, T, draw_mode=mode)
            for i, piece in got.items():
                alone[i] = piece
        _equal_pieces(pieces, alone, f"{path}, {mode}")
        # the values reach the draws, each its own utterance: against the same packing without nuclei, p = 0 and p = 1
        # change nothing, and a small p (the arg-max instead of a draw) changes an utterance that was not at k = 1 already
        plain = _packed(tt, case, utts, seeds, temps, ks, [0.0] * len(utts), groups, draw_mode=mode)
        changed = 0
        for i, p in enumerate(ps):
            if p in (0.0, 1.0):
                assert np.array_equal(pieces[i], plain[i]), i
            elif p == NC.SMALL_P and ks[i] != 1:
                assert not np.array_equal(pieces[i], plain[i]), i
                changed += 1
        assert changed >= 1
        # and generate_packed builds the same arrays from its lists
        if path == "persistent":
            got = tt.generate_packed(utts, n_streams=case.B, seeds=seeds, temperatures=temps, top_ks=ks, top_ps=ps, draw_mode=mode)
            stream, first, T = tt.pack_utterances(case.lengths, case.B)
            own = PC.Packing(case.lengths, tuple(stream), tuple(first), T, case.B, case.min_len, case.max_len)
            _equal_pieces(got, _packed(tt, own, utts, seeds, temps, ks, ps, groups, draw_mode=mode), "generate_packed")


def test_plan_top_p_is_the_utterances_default(dev, monkeypatch):
    """Without top_ps every utterance takes the plan's top_p: the run equals the one that names it for every utterance."""
    B, T, p = 5, 3, 0.5
    seeds, feats = UC.utt_seeds(B), _feats(T, B)
    _env(monkeypatch, 1)
    with _d256_model(dev) as tt:
        with _plan(tt, B, T, 1, utterance_draws=True, top_p=p) as gen:
            default = gen.generate(feats, seeds=seeds, temperatures=1.0).cpu().numpy().copy()
        with _plan(tt, B, T, 1, utterance_draws=True) as gen:
            named = gen.generate(feats, seeds=seeds, temperatures=1.0, top_ps=[p] * B).cpu().numpy().copy()
            scalar = gen.generate(feats, seeds=seeds, temperatures=1.0, top_ps=p).cpu().numpy().copy()
            off = gen.generate(feats, seeds=seeds, temperatures=1.0).cpu().numpy().copy()
    _same(default, named, "the plan's top_p against top_ps")
    _same(scalar, named, "one top_p for all against top_ps")
    assert not np.array_equal(off, named)


def test_streaming_submit_takes_a_top_p(dev, monkeypatch):
    case, utts, seeds, temps, ks, ps = _mixed_utterances()
    B = case.B
    _env(monkeypatch, 1)
    with _d256_model(dev) as tt:
        sg = tt.StreamingGenerator(B, 2, utterance_draws=True)
        try:
            assert sg.gen.persistent
            ticket_of = {sg.submit(utts[i], seed=seeds[i], temperature=temps[i], top_k=ks[i], top_p=ps[i]): i
                         for i in range(len(utts))}
            chunks = {i: [] for i in range(len(utts))}
            for ticket, chunk, _ in sg.drain():
                chunks[ticket_of[ticket]].append(chunk)
            stream = {ticket_of[t]: sg.record[t][0] for t in ticket_of}
        finally:
            sg.close()
        got = [np.concatenate(chunks[i]) for i in range(len(utts))]
        alone = {}
        for b in range(B):
            items = [(i, b) for i in range(len(utts)) if stream[i] == b]
            alone.update(_standalone(tt, B, 1, items, utts, seeds, temps, ks, ps, max(case.lengths)))
    _equal_pieces(got, [alone[i] for i in range(len(utts))], "StreamingGenerator.submit(top_p=)")


# ---- 7. segments --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", NC.MODES)
def test_segments_equal_one_piece(dev, mode):
    s = SC.BIAS_SHAPES["persist-D256-B5"]
    N, p = 4, 0.5
    feats = _feats(N, s.B)
    with _d256_model(dev) as tt:
        with _plan(tt, s.B, N, 1, temperature=1.0, seed=SEED, draw_mode=mode, top_p=p) as gen:
            whole = gen.generate(feats).cpu().numpy().copy()
        with _plan(tt, s.B, N, 1, temperature=1.0, seed=SEED, draw_mode=mode) as gen:
            plain = gen.generate(feats).cpu().numpy().copy()
        for S_ in (1, 2):
            pieces = list(tt.generate_stream(feats, S_, temperature=1.0, seed=SEED, draw_mode=mode, top_p=p))
            assert len(pieces) == -(-(N - 1) // S_)
            _same(np.concatenate(pieces, axis=1), whole, f"segments of {S_} against the run in one piece")
    assert len(np.unique(whole[:, 80:])) > 8 and not np.array_equal(whole, plain)


# ---- 8. a real trajectory -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", NC.MODES)
@pytest.mark.parametrize("path", ["persistent", "launches"])
def test_last_pick_lies_in_the_nucleus_of_the_plans_logits(dev, path, mode, monkeypatch):
    """Ordinary parameters: the nucleus follows the device's own float32 logits, so the check uses the plan's logits of
    its last step: every stream's last pick is one of the codes the rule keeps.  (Inside 2^-14 of a prefix mass the device's
    m may be the oracle's neighbour: the next code of the order is admitted there, and there only.)"""
    B, T = 6, 2
    _env(monkeypatch, 1, launches=path == "launches")
    with _d256_model(dev) as tt:
        for p, k in ((NC.SMALL_P, 0), (0.5, 0), (0.9, 0), (0.9, 8)):
            out, logits = _run(tt, B, T, _feats(T, B), path == "persistent", temperature=1.0, seed=SEED, draw_mode=mode,
                               top_p=p, top_k=k)
            lg = logits.float().numpy()
            for b in range(B):
                m = NC.nucleus_m(lg[b], 1.0, p, k)
                if NC.margin(lg[b], 1.0, p, k) <= NC.MARGIN:
                    m = min(m + 1, k or SC.Q)
                assert KC.kept_set(lg[b], m)[out[b, -1]], f"p = {p}, k = {k}, stream {b}: pick {out[b, -1]} outside the nucleus"
            if p == NC.SMALL_P:
                assert np.array_equal(out[:, -1], lg.argmax(axis=1))


# ---- above one team -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", NC.MODES)
@pytest.mark.parametrize("B,groups", [(33, 0), (64, 2)])
def test_batches_above_one_team(dev, B, groups, mode, monkeypatch):
    """B = 33 on the launch path (one stream past the persistent kernel's limit) and B = 64 in two row groups."""
    T, p, k = 2, 0.9, 64
    b4 = SC.b4_pattern("randn")
    feats = SC.features(T, B).numpy().astype(np.float32)
    _env(monkeypatch, groups)
    with _model(dev, GC.DIM, GC.EMB, SC.bias_only_params(S.config(DIM=GC.DIM, EMB_SIZE=GC.EMB), b4)) as tt:
        with _plan(tt, B, T, groups, temperature=1.0, seed=SEED, draw_mode=mode, top_p=p, top_k=k) as gen:
            out = gen.generate(feats).cpu().numpy().copy()
            logits = gen.ws['logits'].detach().cpu().double()
        with _plan(tt, B, T, groups, temperature=1.0, seed=SEED, draw_mode=mode, top_k=35) as gen:
            same = gen.generate(feats).cpu().numpy().copy()
    _check_bias_only_run(out, logits, b4, B)
    m, draws, excused, worst = NC.judge_draws(out[:, 80:], b4, 1.0, p, k, SC.u01_table(SEED, T, B), mode)
    print(f"TOPP-GPU B={B} groups={groups} {mode}: m {m}, draws {draws}, excused mismatches {excused} (worst {worst:.2e})")
    assert draws == 80 * B and m == 35
    _same(out, same, "top_p = 0.9 behind top_k = 64 against top_k = 35")


# ---- 9. refusals of the C entries ---------------------------------------------------------------------------------------
def test_refusals(dev):
    from parrot_amd import _lib
    BADARG, UNSUPPORTED = 10001, 10002
    s = SC.BIAS_SHAPES["launch-D32-B3"]
    p = S.init_params(S.config(DIM=s.DIM, EMB_SIZE=s.EMB), seed=SC.PARAM_SEED, perturb=0.25)
    lib = _lib.load()
    feats = SC.features(s.T, s.B).numpy()
    with _model(dev, s.DIM, s.EMB, p) as tt:
        gen = tt.DeviceGenerator(s.B, s.T, temperature=1.0, top_p=0.5)
        try:
            for bad in (-0.5, -1e-30, float("nan"), float("-inf")):
                assert lib.samplernn_generate_set_top_p(gen.plan, C.c_float(bad)) == BADARG, bad
            assert lib.samplernn_generate_set_top_p(None, C.c_float(0.5)) == BADARG
            for fine in (0.0, 1.0, 7.0, float("inf"), 0.5):
                assert lib.samplernn_generate_set_top_p(gen.plan, C.c_float(fine)) == 0, fine
            # per-utterance values only beside per-utterance draws
            buf = np.zeros((s.T, s.B), dtype=np.float32)
            assert lib.samplernn_generate_set_utterance_top_p(gen.plan, buf.ctypes.data) == BADARG
            gen.generate(feats)
            assert lib.samplernn_generate_set_top_p(gen.plan, C.c_float(0.9)) == BADARG       # the plan has run
        finally:
            gen.close()
        gen = tt.DeviceGenerator(s.B, s.T, utterance_draws=True)
        try:
            assert lib.samplernn_generate_set_utterance_top_p(gen.plan, None) == BADARG
            assert lib.samplernn_generate_set_utterance_top_p(None, gen.ws['utt_top_p'].data_ptr()) == BADARG
            gen.set_utterance_draws()                      # before the first run: allowed again
            gen.generate(feats, seeds=[1, 2, 3], temperatures=1.0, top_ps=[0.0, 0.5, 3.0])
            assert lib.samplernn_generate_set_utterance_top_p(gen.plan, gen.ws['utt_top_p'].data_ptr()) == BADARG
            assert lib.samplernn_generate_set_top_p(gen.plan, C.c_float(0.5)) == BADARG
        finally:
            gen.close()
