"""The min-p truncated draw of the SampleRNN generator (samplernn_generate_set_min_p, samplernn_generate_set_utterance_min_p;
DeviceGenerator(min_p=), generate(..., min_ps=)): `srp_minp_keep` (sr_common.h) in wave 0 of `sr_pick_kernel` (samplernn.hip)
and in waves 0..3 of `srp_kernel`'s pick (sr_persist.hip), in both draw modes, alone and behind top-k and top-p.  Every draw
against the float64 oracle of the kept set and, bit for bit, against the top-k run with k = the oracle's m; exact cases
without tolerance (one big tie, four maxima, a uniform of exactly 1.0); off against the default; per-utterance values inside
one team; the streaming generator; resumed segments; a real trajectory; the batches above one team; the refusals.
Cases: tests/samplernn_min_p_cases.py (premises: tests/test_samplernn_min_p_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import samplernn_ref as S
from tests import samplernn_groups_cases as GC
from tests import samplernn_min_p_cases as MC
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
COMBINED_SHAPE = "persist-D256-B5"


# ---- 1. draws against the oracle, and against top_k = m -----------------------------------------------------------------
@pytest.mark.parametrize("mode", MC.MODES)
@pytest.mark.parametrize("temperature", SC.TEMPERATURES)
@pytest.mark.parametrize("pattern", SC.PATTERNS)
@pytest.mark.parametrize("shape", sorted(SC.BIAS_SHAPES))
def test_min_p_draws_from_known_logits(dev, shape, pattern, temperature, mode):
    """min_p in MC.MIN_PS.  Every pick against the float64 CDF of the oracle's kept set at draw_u01(seed, t, b): inside the
    set without any excuse; a mismatch only within DELTA (sequential) / DELTA_SCAN (scan) of a boundary and in at most 0.5 %
    of the draws.  And the run equals, bit for bit, the run with top_k = m, m the oracle's (every ratio of a case lies
    farther than 2^-18 from min_p: MC.case_m)."""
    s = SC.BIAS_SHAPES[shape]
    b4 = SC.b4_pattern(pattern)
    feats = SC.features(s.T, s.B).numpy()
    u = SC.u01_table(SEED, s.T, s.B)
    kw = dict(temperature=temperature, seed=SEED, draw_mode=mode)
    with _bias_model(dev, s, b4) as tt:
        by_k = {}
        for min_p in MC.MIN_PS:
            out, logits = _run(tt, s.B, s.T, feats, s.persistent, min_p=min_p, **kw)
            _check_bias_only_run(out, logits, b4, s.B)
            m, draws, excused, worst = MC.judge_draws(out[:, 80:], b4, temperature, min_p, u, mode)
            print(f"MINP-GPU {shape} {pattern} T={temperature} {mode} min_p={min_p}: m {m}, draws {draws}, excused "
                  f"mismatches {excused} (worst {worst:.2e})")
            assert draws == 80 * (s.T - 1) * s.B and 1 <= m <= SC.Q
            if m not in by_k:
                by_k[m] = _run(tt, s.B, s.T, feats, s.persistent, top_k=m, **kw)[0]
            _same(out, by_k[m], f"min_p = {min_p} against top_k = {m}")
    if (pattern, temperature) == ("randn", 1.0):
        assert sorted(by_k) == [1, 3, 21, 64]


@pytest.mark.parametrize("mode", MC.MODES)
@pytest.mark.parametrize("pattern", SC.PATTERNS)
def test_min_p_behind_top_k_and_top_p(dev, pattern, mode):
    """(top_k, top_p) in {(64, 0), (0, 0.9), (64, 0.9)} in front of min_p = 0.1, at every temperature: the kept set is the
    shortest of the three prefixes, judged and compared like the draws above."""
    s = SC.BIAS_SHAPES[COMBINED_SHAPE]
    b4 = SC.b4_pattern(pattern)
    feats = SC.features(s.T, s.B).numpy()
    u = SC.u01_table(SEED, s.T, s.B)
    cases = [c for c in MC.combined_cases() if c[0] == pattern]
    assert len(cases) == 9
    with _bias_model(dev, s, b4) as tt:
        by_k = {}
        for _, temperature, k, p in cases:
            kw = dict(temperature=temperature, seed=SEED, draw_mode=mode)
            out, logits = _run(tt, s.B, s.T, feats, s.persistent, min_p=MC.COMBINED_MIN_P, top_k=k, top_p=p, **kw)
            _check_bias_only_run(out, logits, b4, s.B)
            m, draws, excused, worst = MC.judge_draws(out[:, 80:], b4, temperature, MC.COMBINED_MIN_P, u, mode, k=k, p=p)
            print(f"MINP-GPU {pattern} T={temperature} {mode} k={k} p={p} min_p={MC.COMBINED_MIN_P}: m {m}, draws {draws}, "
                  f"excused mismatches {excused} (worst {worst:.2e})")
            if (temperature, m) not in by_k:
                by_k[(temperature, m)] = _run(tt, s.B, s.T, feats, s.persistent, top_k=m, **kw)[0]
            _same(out, by_k[(temperature, m)], f"top_k = {k}, top_p = {p}, min_p = {MC.COMBINED_MIN_P} against top_k = {m}")


# ---- 2. exact cases, no tolerance ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MC.MODES)
@pytest.mark.parametrize("shape", sorted(SC.EDGE_SHAPES))
def test_all_equal_logits(dev, shape, mode):
    """Every logit equal: every term is 1.0f, so any active min_p keeps all 256 and the pick is floor(256 u01) -- on a
    boundary too (SC.EDGE_SEEDS), and 255 where u01 is exactly 1.0."""
    s = SC.EDGE_SHAPES[shape]
    b4 = np.full(SC.Q, SC.EDGE_LOGIT, dtype=np.float32)
    feats = SC.features(s.T, s.B).numpy()
    with _bias_model(dev, s, b4) as tt:
        for seed, min_p in zip(SC.EDGE_SEEDS + tuple(KC.U1_SEEDS), MC.EXACT_MIN_PS + (1.0,)):
            u = SC.u01_table(seed, s.T, s.B)
            out, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=seed, draw_mode=mode, min_p=min_p)
            _check_bias_only_run(out, logits, b4, s.B)
            want = MC.equal_logits_picks(u)
            assert np.array_equal(out[:, 80:], want), f"seed {seed}, min_p {min_p}: {(out[:, 80:] != want).sum()} picks differ"
            if seed in KC.U1_SEEDS:
                b, t = KC.U1_SEEDS[seed]
                assert u[b, t - 80] == 1.0 and out[b, t] == 255


@pytest.mark.parametrize("mode", MC.MODES)
@pytest.mark.parametrize("shape", sorted(SC.EDGE_SHAPES) + sorted(SC.TIE_SHAPES))
def test_four_maxima_and_a_uniform_of_one(dev, shape, mode):
    """Maxima at 5, 69, 133, 200: min_p = 1.0 keeps exactly the four (terms of exactly 1.0), and so does 0.02 (every other
    ratio is below 0.0183): the pick is the floor(4 u01)-th of them -- 200 where u01 is exactly 1.0, not 255."""
    s = SC.EDGE_SHAPES[shape] if shape in SC.EDGE_SHAPES else SC.TIE_SHAPES[shape]
    b4, _ = SC.tie_pattern(MC.FOUR_MAXIMA)
    feats = SC.features(s.T, s.B).numpy()
    seeds = SC.EDGE_SEEDS[:1] + (tuple(KC.U1_SEEDS) if shape in SC.EDGE_SHAPES else ())
    with _bias_model(dev, s, b4) as tt:
        for seed in seeds:
            u = SC.u01_table(seed, s.T, s.B)
            want = MC.four_maxima_picks(u)
            for min_p in MC.FOUR_MIN_PS:
                out, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=seed, draw_mode=mode, min_p=min_p)
                _check_bias_only_run(out, logits, b4, s.B)
                assert set(np.unique(out[:, 80:]).tolist()) <= set(MC.FOUR_CODES)
                assert np.array_equal(out[:, 80:], want), f"seed {seed}, min_p {min_p}: {(out[:, 80:] != want).sum()} picks differ"
            if seed in KC.U1_SEEDS:
                b, t = KC.U1_SEEDS[seed]
                assert u[b, t - 80] == 1.0 and out[b, t] == 200, f"seed {seed}: u01 == 1.0, pick {out[b, t]}"


# ---- 3. off is off ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MC.MODES)
@pytest.mark.parametrize("name", sorted(SC.TRAJ_SHAPES))
def test_off_is_the_default(dev, name, mode):
    s = SC.TRAJ_SHAPES[name]
    p = S.init_params(S.config(DIM=s.DIM, EMB_SIZE=s.EMB), seed=s.param_seed, perturb=0.25)
    feats = SC.features(s.T, s.B, s.feat_seed).numpy()
    with _model(dev, s.DIM, s.EMB, p) as tt:
        for temperature in (0.0, 1.0):
            kw = dict(temperature=temperature, seed=SC.TRAJ_SEED, draw_mode=mode)
            default, _ = _run(tt, s.B, s.T, feats, s.persistent, **kw)
            for min_p in (0, 0.0):
                out, _ = _run(tt, s.B, s.T, feats, s.persistent, min_p=min_p, **kw)
                _same(out, default, f"min_p = {min_p!r} at temperature {temperature} against the keyword left out")
            cut, _ = _run(tt, s.B, s.T, feats, s.persistent, min_p=0.5, **kw)
            if temperature == 0.0:
                _same(cut, default, "min_p at temperature 0: the argmax either way")
            else:
                assert len(np.unique(default[:, 80:])) > 20 and not np.array_equal(cut, default)


# ---- 4. per utterance ---------------------------------------------------------------------------------------------------
def _packed(tt, case, utts, seeds, temps, ks, ps, mps, groups, **kw):
    features, starts = tt.build_packed_inputs(utts, case.stream, case.first_slot, case.T, case.B)
    utt_seed, utt_temp = tt.build_packed_draws(seeds, temps, case.stream, case.first_slot, case.T, case.B)
    utt_top_k = tt.build_packed_top_k(ks, case.stream, case.first_slot, case.T, case.B)
    utt_top_p = tt.build_packed_top_p(ps, case.stream, case.first_slot, case.T, case.B)
    utt_min_p = tt.build_packed_min_p(mps, case.stream, case.first_slot, case.T, case.B)
    with _plan(tt, case.B, case.T, groups, packed=True, utterance_draws=True, **kw) as gen:
        samples = gen.generate(features, starts, seeds=utt_seed, temperatures=utt_temp, top_ks=utt_top_k, top_ps=utt_top_p,
                               min_ps=utt_min_p).cpu().numpy().copy()
    return tt.unpack_samples(samples, case.lengths, case.stream, case.first_slot)


def _standalone(tt, B, groups, items, utts, seeds, temps, ks, ps, mps, T, **kw):
    """{i: piece} for items = [(utterance i, stream)]: each utterance carried alone in its stream of a plain plan of B
    streams with its seed, temperature, top_k, top_p and min_p."""
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
            sd, tp, tk = [0] * B, np.zeros(B, dtype=np.float32), np.zeros(B, dtype=np.int32)
            pp, mp = np.zeros(B, dtype=np.float32), np.zeros(B, dtype=np.float32)
            for b, i in rect.items():
                feats[:utts[i].shape[0], b] = utts[i]
                sd[b], tp[b], tk[b], pp[b], mp[b] = seeds[i], temps[i], ks[i], ps[i], mps[i]
            out = gen.generate(feats, seeds=sd, temperatures=tp, top_ks=tk, top_ps=pp, min_ps=mp).cpu().numpy().copy()
            for b, i in rect.items():
                pieces[i] = out[b, :80 * utts[i].shape[0]]
    return pieces


def _mixed_utterances():
    case = PC.GRU_PACKING
    n = len(case.lengths)
    assert case.B == 5 and n >= 8     # streams 0 .. 3 form one team of the persistent kernel, stream 4 a partial one
    utts = _utterances(_feats(case.max_len, n), case.lengths)
    ks, temps, ps, mps = KC.utt_top_ks(n), KC.utt_temperatures(n), NC.utt_top_ps(n), MC.utt_min_ps(n)
    team0 = [i for i in range(n) if case.stream[i] < 4 and case.first_slot[i] == 0]
    assert len({mps[i] for i in team0}) >= 3 and len({temps[i] for i in team0}) == 3
    return case, utts, UC.utt_seeds(n), temps, ks, ps, mps


@pytest.mark.parametrize("path,mode", [("persistent", "sequential"), ("persistent", "scan"), ("launches", "sequential")])
def test_packed_utterances_equal_standalone(dev, path, mode, monkeypatch):
    """Utterances with min_p in {0, 0.1, 1, 0.5}, p in {0, 0.9, 2^-10, 0.5, 1}, k in {0, 1, 8, 64} and temperatures in
    {0.5, 1, 2} mixed inside one team: each equals, bit for bit, the plain plan that carries it alone in the same stream with
    the same values."""
    case, utts, seeds, temps, ks, ps, mps = _mixed_utterances()
    groups = 1 if path == "persistent" else 0
    _env(monkeypatch, 1, launches=path == "launches")
    with _d256_model(dev) as tt:
        pieces = _packed(tt, case, utts, seeds, temps, ks, ps, mps, groups, draw_mode=mode)
        alone = [None] * len(utts)
        for rect in PC.rectangles(case):
            T = max(2, max(case.lengths[i] for i in rect.values()))
            got = _standalone(tt, case.B, groups, [(i, b) for b, i in rect.items()], utts, seeds, temps, ks, ps, mps, T,
                              draw_mode=mode)
            for i, piece in got.items():
                alone[i] = piece
        _equal_pieces(pieces, alone, f"{path}, {mode}")
        # the values reach the draws, each its own utterance: against the same packing without min_p, 0 changes nothing, and
        # min_p = 1 (the argmax instead of a draw: the logits of ordinary parameters have one maximum) changes an utterance
        # that was not at the argmax already
        plain = _packed(tt, case, utts, seeds, temps, ks, ps, [0.0] * len(utts), groups, draw_mode=mode)
        changed = 0
        for i, m in enumerate(mps):
            if m == 0.0:
                assert np.array_equal(pieces[i], plain[i]), i
            elif m == 1.0 and ks[i] != 1 and ps[i] != NC.SMALL_P:
                assert not np.array_equal(pieces[i], plain[i]), i
                changed += 1
        assert changed >= 1
        # and generate_packed builds the same arrays from its lists
        if path == "persistent":
            got = tt.generate_packed(utts, n_streams=case.B, seeds=seeds, temperatures=temps, top_ks=ks, top_ps=ps, min_ps=mps,
                                     draw_mode=mode)
            stream, first, T = tt.pack_utterances(case.lengths, case.B)
            own = PC.Packing(case.lengths, tuple(stream), tuple(first), T, case.B, case.min_len, case.max_len)
            _equal_pieces(got, _packed(tt, own, utts, seeds, temps, ks, ps, mps, groups, draw_mode=mode), "generate_packed")


# ---- 5. the plan's value is the utterances' default -------------------------------------------------------------------------
def test_plan_min_p_is_the_utterances_default(dev, monkeypatch):
    B, T, m = 5, 3, 0.5
    seeds, feats = UC.utt_seeds(B), _feats(T, B)
    _env(monkeypatch, 1)
    with _d256_model(dev) as tt:
        with _plan(tt, B, T, 1, utterance_draws=True, min_p=m) as gen:
            default = gen.generate(feats, seeds=seeds, temperatures=1.0).cpu().numpy().copy()
        with _plan(tt, B, T, 1, utterance_draws=True) as gen:
            named = gen.generate(feats, seeds=seeds, temperatures=1.0, min_ps=[m] * B).cpu().numpy().copy()
            scalar = gen.generate(feats, seeds=seeds, temperatures=1.0, min_ps=m).cpu().numpy().copy()
            off = gen.generate(feats, seeds=seeds, temperatures=1.0).cpu().numpy().copy()
    _same(default, named, "the plan's min_p against min_ps")
    _same(scalar, named, "one min_p for all against min_ps")
    assert not np.array_equal(off, named)


# ---- 6. the streaming generator ---------------------------------------------------------------------------------------------
def test_streaming_submit_takes_a_min_p(dev, monkeypatch):
    case, utts, seeds, temps, ks, ps, mps = _mixed_utterances()
    B = case.B
    _env(monkeypatch, 1)
    with _d256_model(dev) as tt:
        sg = tt.StreamingGenerator(B, 2, utterance_draws=True)
        try:
            assert sg.gen.persistent
            ticket_of = {sg.submit(utts[i], seed=seeds[i], temperature=temps[i], top_k=ks[i], top_p=ps[i], min_p=mps[i]): i
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
            alone.update(_standalone(tt, B, 1, items, utts, seeds, temps, ks, ps, mps, max(case.lengths)))
    _equal_pieces(got, [alone[i] for i in range(len(utts))], "StreamingGenerator.submit(min_p=)")


# ---- 7. segments --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MC.MODES)
def test_segments_equal_one_piece(dev, mode):
    s = SC.BIAS_SHAPES["persist-D256-B5"]
    N, m = 4, 0.1
    feats = _feats(N, s.B)
    with _d256_model(dev) as tt:
        with _plan(tt, s.B, N, 1, temperature=1.0, seed=SEED, draw_mode=mode, min_p=m) as gen:
            whole = gen.generate(feats).cpu().numpy().copy()
        with _plan(tt, s.B, N, 1, temperature=1.0, seed=SEED, draw_mode=mode) as gen:
            plain = gen.generate(feats).cpu().numpy().copy()
        for S_ in (1, 2):
            pieces = list(tt.generate_stream(feats, S_, temperature=1.0, seed=SEED, draw_mode=mode, min_p=m))
            assert len(pieces) == -(-(N - 1) // S_)
            _same(np.concatenate(pieces, axis=1), whole, f"segments of {S_} against the run in one piece")
    assert len(np.unique(whole[:, 80:])) > 4 and not np.array_equal(whole, plain)


# ---- 8. a real trajectory -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MC.MODES)
@pytest.mark.parametrize("path", ["persistent", "launches"])
def test_last_pick_lies_in_the_kept_set_of_the_plans_logits(dev, path, mode, monkeypatch):
    """Ordinary parameters: the kept set follows the device's own float32 logits, so the check uses the plan's logits of its
    last step: every stream's last pick is a code whose float64 ratio is >= min_p (1 - MARGIN)."""
    B, T = 6, 2
    _env(monkeypatch, 1, launches=path == "launches")
    with _d256_model(dev) as tt:
        for m in (1.0, 0.5, 0.1, 0.02):
            out, logits = _run(tt, B, T, _feats(T, B), path == "persistent", temperature=1.0, seed=SEED, draw_mode=mode, min_p=m)
            lg = logits.float().numpy()
            for b in range(B):
                r = MC.ratios64(lg[b], 1.0)[out[b, -1]]
                assert r >= m * (1.0 - MC.MARGIN), f"min_p = {m}, stream {b}: pick {out[b, -1]} has ratio {r:.6f}"
            if m == 1.0:
                assert np.array_equal(out[:, -1], lg.argmax(axis=1))


# ---- 9. above one team --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MC.MODES)
@pytest.mark.parametrize("B,groups", [(33, 0), (64, 2)])
def test_batches_above_one_team(dev, B, groups, mode, monkeypatch):
    """B = 33 on the launch path (one stream past the persistent kernel's limit) and B = 64 in two row groups."""
    T, m_p = 3, 0.1
    b4 = SC.b4_pattern("randn")
    feats = SC.features(T, B).numpy().astype(np.float32)
    _env(monkeypatch, groups)
    with _model(dev, GC.DIM, GC.EMB, SC.bias_only_params(S.config(DIM=GC.DIM, EMB_SIZE=GC.EMB), b4)) as tt:
        with _plan(tt, B, T, groups, temperature=1.0, seed=SEED, draw_mode=mode, min_p=m_p) as gen:
            out = gen.generate(feats).cpu().numpy().copy()
            logits = gen.ws['logits'].detach().cpu().double()
        with _plan(tt, B, T, groups, temperature=1.0, seed=SEED, draw_mode=mode, top_k=21) as gen:
            same = gen.generate(feats).cpu().numpy().copy()
    _check_bias_only_run(out, logits, b4, B)
    m, draws, excused, worst = MC.judge_draws(out[:, 80:], b4, 1.0, m_p, SC.u01_table(SEED, T, B), mode)
    print(f"MINP-GPU B={B} groups={groups} {mode}: m {m}, draws {draws}, excused mismatches {excused} (worst {worst:.2e})")
    assert draws == 160 * B and m == 21
    _same(out, same, "min_p = 0.1 against top_k = 21")


# ---- 10. refusals -------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from parrot_amd import _lib
    BADARG = 10001
    s = SC.BIAS_SHAPES["launch-D32-B3"]
    p = S.init_params(S.config(DIM=s.DIM, EMB_SIZE=s.EMB), seed=SC.PARAM_SEED, perturb=0.25)
    lib = _lib.load()
    feats = SC.features(s.T, s.B).numpy()
    with _model(dev, s.DIM, s.EMB, p) as tt:
        gen = tt.DeviceGenerator(s.B, s.T, temperature=1.0, min_p=0.5)
        try:
            for bad in (-0.5, -1e-30, float("nan"), float("-inf"), 1.5, float("inf"), float(np.nextafter(np.float32(1), np.float32(2)))):
                assert lib.samplernn_generate_set_min_p(gen.plan, C.c_float(bad)) == BADARG, bad
            assert lib.samplernn_generate_set_min_p(None, C.c_float(0.5)) == BADARG
            for fine in (0.0, 1.0, 1e-40, 0.5):
                assert lib.samplernn_generate_set_min_p(gen.plan, C.c_float(fine)) == 0, fine
            # per-utterance values only beside per-utterance draws
            buf = np.zeros((s.T, s.B), dtype=np.float32)
            assert lib.samplernn_generate_set_utterance_min_p(gen.plan, buf.ctypes.data) == BADARG
            gen.generate(feats)
            assert lib.samplernn_generate_set_min_p(gen.plan, C.c_float(0.9)) == BADARG       # the plan has run
        finally:
            gen.close()
        gen = tt.DeviceGenerator(s.B, s.T, utterance_draws=True)
        try:
            assert lib.samplernn_generate_set_utterance_min_p(gen.plan, None) == BADARG
            assert lib.samplernn_generate_set_utterance_min_p(None, gen.ws['utt_min_p'].data_ptr()) == BADARG
            gen.set_utterance_draws()                      # before the first run: allowed again
            gen.generate(feats, seeds=[1, 2, 3], temperatures=1.0, min_ps=[0.0, 0.5, 1.0])
            assert lib.samplernn_generate_set_utterance_min_p(gen.plan, gen.ws['utt_min_p'].data_ptr()) == BADARG
            assert lib.samplernn_generate_set_min_p(gen.plan, C.c_float(0.5)) == BADARG
        finally:
            gen.close()
        with pytest.raises(ValueError):                    # the literal three-function loop draws among all codes
            tt.generate_and_save_samples("t", features=feats, use_device_loop=False, min_p=0.1)
