"""The top-k truncated draw of the SampleRNN generator (SampleRnnGenDesc::top_k, samplernn_generate_set_utterance_top_k;
DeviceGenerator(top_k=), generate(..., top_ks=)): `srp_topk_keep` (sr_common.h) in wave 0 of `sr_pick_kernel`
(samplernn.hip) and in waves 0..3 of `srp_kernel`'s pick (sr_persist.hip), in both draw modes.  Every draw against the
float64 oracle of the truncated CDF, exact cases without tolerance (ties at the cut-off, a uniform of exactly 1.0), k = 1
against the arg-max, off against the default, per-utterance values inside one team, resumed segments, a real trajectory,
and the batches above one team.  Cases: tests/samplernn_top_k_cases.py (premises: tests/test_samplernn_top_k_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import samplernn_ref as S
from tests import samplernn_groups_cases as GC
from tests import samplernn_packed_cases as PC
from tests import samplernn_sampling_cases as SC
from tests import samplernn_top_k_cases as KC
from tests import samplernn_utt_draw_cases as UC
from tests.test_gpu_samplernn_groups import _plan
from tests.test_gpu_samplernn_sampling import _check_bias_only_run, _model, _run
from tests.test_gpu_samplernn_utt_draws import _env, _equal_pieces, _utterances

pytestmark = pytest.mark.gpu

SEED = SC.SEEDS[1]   # (the one that guards the 64-bit field)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == np.int32
    assert np.array_equal(a, b), f"{what}: {(a != b).sum()} of {a.size} samples differ, rows " \
                                 f"{sorted(set(np.nonzero(a != b)[0].tolist()))}"


def _bias_model(dev, s, b4):
    return _model(dev, s.DIM, s.EMB, SC.bias_only_params(S.config(DIM=s.DIM, EMB_SIZE=s.EMB), b4))


def _d256_model(dev):
    """Ordinary parameters at DIM 256 (no oracle run behind them: these tests compare device runs)."""
    p = S.init_params(S.config(DIM=GC.DIM, EMB_SIZE=GC.EMB), seed=GC.DRAW_PARAM_SEED, perturb=0.25)
    return _model(dev, GC.DIM, GC.EMB, p)


def _feats(T, B):
    return SC.features(T, B, GC.DRAW_FEAT_SEED).numpy().astype(np.float32)


# ---- 1. draws against the oracle ----------------------------------------------------------------------------------------
DRAW_CASES = [(shape, pattern, 1.0) for shape in sorted(SC.BIAS_SHAPES) for pattern in SC.PATTERNS] + \
             [(shape, "randn", tau) for shape in sorted(SC.BIAS_SHAPES) for tau in (0.5, 2.0)]


@pytest.mark.parametrize("mode", KC.MODES)
@pytest.mark.parametrize("shape,pattern,temperature", DRAW_CASES)
def test_truncated_draws_from_known_logits(dev, shape, pattern, temperature, mode):
    """Every pick against the truncated float64 CDF at draw_u01(seed, t, b): inside the kept set without any excuse; a
    mismatch only within DELTA (sequential) / DELTA_SCAN (scan) of the boundary and in at most 0.5 % of the draws."""
    s = SC.BIAS_SHAPES[shape]
    b4 = SC.b4_pattern(pattern)
    feats = SC.features(s.T, s.B).numpy()
    u = SC.u01_table(SEED, s.T, s.B)
    with _bias_model(dev, s, b4) as tt:
        plain, _ = _run(tt, s.B, s.T, feats, s.persistent, temperature=temperature, seed=SEED, draw_mode=mode)
        for k in KC.GPU_KS:
            out, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=temperature, seed=SEED, draw_mode=mode, top_k=k)
            _check_bias_only_run(out, logits, b4, s.B)
            draws, excused, worst = KC.judge_draws(out[:, 80:], b4, temperature, k, u, mode)
            print(f"TOPK-GPU {shape} {pattern} T={temperature} {mode} k={k}: draws {draws}, excused mismatches {excused} "
                  f"(worst {worst:.2e})")
            assert draws == 80 * (s.T - 1) * s.B
            if k == 2:   # (the truncation is in the samples: in every pattern the codes behind the top two hold over 10 % of the mass)
                assert not np.array_equal(out, plain)


# ---- 2. exact cases, no tolerance ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", KC.MODES)
@pytest.mark.parametrize("shape", sorted(SC.EDGE_SHAPES))
def test_all_equal_logits(dev, shape, mode):
    """Every logit equal: the cut-off is one big tie, the kept set is codes 0 .. k-1, and the pick is floor(k u01)."""
    s = SC.EDGE_SHAPES[shape]
    b4 = np.full(SC.Q, SC.EDGE_LOGIT, dtype=np.float32)
    feats = SC.features(s.T, s.B).numpy()
    with _bias_model(dev, s, b4) as tt:
        for seed in SC.EDGE_SEEDS:
            u = SC.u01_table(seed, s.T, s.B)
            for k in KC.EQUAL_KS:
                out, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=seed, draw_mode=mode, top_k=k)
                _check_bias_only_run(out, logits, b4, s.B)
                want = KC.equal_logits_picks(k, u)
                assert np.array_equal(out[:, 80:], want), f"k = {k}, seed {seed}: {(out[:, 80:] != want).sum()} picks differ"


@pytest.mark.parametrize("mode", KC.MODES)
@pytest.mark.parametrize("shape", sorted(SC.EDGE_SHAPES))
def test_tie_at_the_cut_off_and_a_uniform_of_one(dev, shape, mode):
    """Maxima at 5, 69, 133, 200 and k = 2: the kept set is {5, 69}, the pick 5 where u01 < 0.5, else 69 -- also where u01 is
    exactly 1.0 and no code satisfies u < c: the pick is the highest kept code, not 255."""
    s = SC.EDGE_SHAPES[shape]
    b4, _ = SC.tie_pattern(KC.TWO_MAXIMA)
    feats = SC.features(s.T, s.B).numpy()
    with _bias_model(dev, s, b4) as tt:
        for seed in SC.EDGE_SEEDS[:1] + tuple(KC.U1_SEEDS):
            u = SC.u01_table(seed, s.T, s.B)
            out, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=seed, draw_mode=mode, top_k=2)
            _check_bias_only_run(out, logits, b4, s.B)
            if seed in KC.U1_SEEDS:
                b, t = KC.U1_SEEDS[seed]
                assert u[b, t - 80] == 1.0
                assert out[b, t] == 69, f"seed {seed}: u01 == 1.0 at stream {b}, sample {t}: pick {out[b, t]}"
            want = KC.two_maxima_picks(u)
            assert np.array_equal(out[:, 80:], want), f"seed {seed}: {(out[:, 80:] != want).sum()} picks differ"


# ---- 3. k = 1 is the arg-max --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", KC.MODES)
@pytest.mark.parametrize("shape", sorted(SC.TIE_SHAPES))
def test_top_1_is_the_argmax(dev, shape, mode):
    s = SC.TIE_SHAPES[shape]
    feats = SC.features(s.T, s.B).numpy()
    patterns = [(name,) + SC.tie_pattern(name) for name in SC.TIE_MAXIMA] + [("randn", SC.b4_pattern("randn"), None)]
    for name, b4, want in patterns:
        with _bias_model(dev, s, b4) as tt:
            top1, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=SEED, draw_mode=mode, top_k=1)
            _check_bias_only_run(top1, logits, b4, s.B)
            greedy, _ = _run(tt, s.B, s.T, feats, s.persistent, temperature=0.0, draw_mode=mode)
            _same(top1, greedy, f"{name}: top_k = 1 at temperature 1 against temperature 0")
            assert np.unique(top1[:, 80:]).tolist() == [int(np.argmax(b4)) if want is None else want]


# ---- 4. off is off ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", KC.MODES)
@pytest.mark.parametrize("name", sorted(SC.TRAJ_SHAPES))
def test_off_is_the_default(dev, name, mode):
    s = SC.TRAJ_SHAPES[name]
    p = S.init_params(S.config(DIM=s.DIM, EMB_SIZE=s.EMB), seed=s.param_seed, perturb=0.25)
    feats = SC.features(s.T, s.B, s.feat_seed).numpy()
    with _model(dev, s.DIM, s.EMB, p) as tt:
        default, _ = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=SC.TRAJ_SEED, draw_mode=mode)
        for k in (0, 256, 1000):
            out, _ = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=SC.TRAJ_SEED, draw_mode=mode, top_k=k)
            _same(out, default, f"top_k = {k} against the keyword left out")
        cut, _ = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=SC.TRAJ_SEED, draw_mode=mode, top_k=4)
    assert len(np.unique(default[:, 80:])) > 20 and not np.array_equal(cut, default)


# ---- 5. per utterance ---------------------------------------------------------------------------------------------------
def _packed(tt, case, utts, seeds, temps, ks, groups, **kw):
    features, starts = tt.build_packed_inputs(utts, case.stream, case.first_slot, case.T, case.B)
    utt_seed, utt_temp = tt.build_packed_draws(seeds, temps, case.stream, case.first_slot, case.T, case.B)
    utt_top_k = tt.build_packed_top_k(ks, case.stream, case.first_slot, case.T, case.B)
    with _plan(tt, case.B, case.T, groups, packed=True, utterance_draws=True, **kw) as gen:
        samples = gen.generate(features, starts, seeds=utt_seed, temperatures=utt_temp, top_ks=utt_top_k).cpu().numpy().copy()
    return tt.unpack_samples(samples, case.lengths, case.stream, case.first_slot)


def _standalone(tt, B, groups, items, utts, seeds, temps, ks, T, **kw):
    """{i: piece} for items = [(utterance i, stream)]: each utterance carried alone in its stream of a plain plan of B
    streams with its seed, temperature and top_k (tests/test_gpu_samplernn_utt_draws.py::_standalone, with top_ks)."""
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
            for b, i in rect.items():
                feats[:utts[i].shape[0], b] = utts[i]
                sd[b], tp[b], tk[b] = seeds[i], temps[i], ks[i]
            out = gen.generate(feats, seeds=sd, temperatures=tp, top_ks=tk).cpu().numpy().copy()
            for b, i in rect.items():
                pieces[i] = out[b, :80 * utts[i].shape[0]]
    return pieces


def _mixed_utterances():
    case = PC.GRU_PACKING
    n = len(case.lengths)
    assert case.B == 5 and n >= 8     # streams 0 .. 3 form one team of the persistent kernel, stream 4 a partial one
    utts = _utterances(_feats(case.max_len, n), case.lengths)
    ks, temps = KC.utt_top_ks(n), KC.utt_temperatures(n)
    team0 = [i for i in range(n) if case.stream[i] < 4 and case.first_slot[i] == 0]
    assert len({ks[i] for i in team0}) == 4 and len({temps[i] for i in team0}) == 3
    return case, utts, UC.utt_seeds(n), temps, ks


@pytest.mark.parametrize("path,mode", [("persistent", "sequential"), ("persistent", "scan"), ("launches", "sequential")])
def test_packed_utterances_equal_standalone(dev, path, mode, monkeypatch):
    """Utterances with k in {0, 1, 8, 64} and temperatures in {0.5, 1, 2} mixed inside one team: each equals, bit for bit, the
    plain plan that carries it alone in the same stream with the same seed, temperature and k."""
    case, utts, seeds, temps, ks = _mixed_utterances()
    groups = 1 if path == "persistent" else 0
    _env(monkeypatch, 1, launches=path == "launches")
    with _d256_model(dev) as tt:
        pieces = _packed(tt, case, utts, seeds, temps, ks, groups, draw_mode=mode)
        alone = [None] * len(utts)
        for rect in PC.rectangles(case):
            T = max(2, max(case.lengths[i] for i in rect.values()))
            got = _standalone(tt, case.B, groups, [(i, b) for b, i in rect.items()], utts, seeds, temps, ks, T, draw_mode=mode)
            for i, piece in got.items():
                alone[i] = piece
        _equal_pieces(pieces, alone, f"{path}, {mode}")
        # the values reach the draws, each its own utterance: against the same packing without truncation, k = 0 changes
        # nothing and k = 1 (the arg-max instead of a draw) changes the utterance
        plain = _packed(tt, case, utts, seeds, temps, [0] * len(utts), groups, draw_mode=mode)
        for i, k in enumerate(ks):
            if k == 0:
                assert np.array_equal(pieces[i], plain[i]), i
            elif k == 1:
                assert not np.array_equal(pieces[i], plain[i]), i
        # and generate_packed builds the same arrays from its lists
        if path == "persistent":
            got = tt.generate_packed(utts, n_streams=case.B, seeds=seeds, temperatures=temps, top_ks=ks, draw_mode=mode)
            stream, first, T = tt.pack_utterances(case.lengths, case.B)
            own = PC.Packing(case.lengths, tuple(stream), tuple(first), T, case.B, case.min_len, case.max_len)
            _equal_pieces(got, _packed(tt, own, utts, seeds, temps, ks, groups, draw_mode=mode), "generate_packed")


def test_plan_top_k_is_the_utterances_default(dev, monkeypatch):
    """Without top_ks every utterance takes the plan's top_k: the run equals the one that names it for every utterance."""
    B, T, k = 5, 3, 8
    seeds, feats = UC.utt_seeds(B), _feats(T, B)
    _env(monkeypatch, 1)
    with _d256_model(dev) as tt:
        with _plan(tt, B, T, 1, utterance_draws=True, top_k=k) as gen:
            default = gen.generate(feats, seeds=seeds, temperatures=1.0).cpu().numpy().copy()
        with _plan(tt, B, T, 1, utterance_draws=True) as gen:
            named = gen.generate(feats, seeds=seeds, temperatures=1.0, top_ks=[k] * B).cpu().numpy().copy()
            scalar = gen.generate(feats, seeds=seeds, temperatures=1.0, top_ks=k).cpu().numpy().copy()
            off = gen.generate(feats, seeds=seeds, temperatures=1.0).cpu().numpy().copy()
    _same(default, named, "the plan's top_k against top_ks")
    _same(scalar, named, "one top_k for all against top_ks")
    assert not np.array_equal(off, named)


def test_streaming_submit_takes_a_top_k(dev, monkeypatch):
    case, utts, seeds, temps, ks = _mixed_utterances()
    B = case.B
    _env(monkeypatch, 1)
    with _d256_model(dev) as tt:
        sg = tt.StreamingGenerator(B, 2, utterance_draws=True)
        try:
            assert sg.gen.persistent
            ticket_of = {sg.submit(utts[i], seed=seeds[i], temperature=temps[i], top_k=ks[i]): i for i in range(len(utts))}
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
            alone.update(_standalone(tt, B, 1, items, utts, seeds, temps, ks, max(case.lengths)))
    _equal_pieces(got, [alone[i] for i in range(len(utts))], "StreamingGenerator.submit(top_k=)")


# ---- 6. segments --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", KC.MODES)
def test_segments_equal_one_piece(dev, mode):
    s = SC.BIAS_SHAPES["persist-D256-B5"]
    N, k = 4, 8
    feats = _feats(N, s.B)
    with _d256_model(dev) as tt:
        with _plan(tt, s.B, N, 1, temperature=1.0, seed=SEED, draw_mode=mode, top_k=k) as gen:
            whole = gen.generate(feats).cpu().numpy().copy()
        with _plan(tt, s.B, N, 1, temperature=1.0, seed=SEED, draw_mode=mode) as gen:
            plain = gen.generate(feats).cpu().numpy().copy()
        for S_ in (1, 2):
            pieces = list(tt.generate_stream(feats, S_, temperature=1.0, seed=SEED, draw_mode=mode, top_k=k))
            assert len(pieces) == -(-(N - 1) // S_)
            _same(np.concatenate(pieces, axis=1), whole, f"segments of {S_} against the run in one piece")
    assert len(np.unique(whole[:, 80:])) > 8 and not np.array_equal(whole, plain)


# ---- 7. a real trajectory -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", KC.MODES)
@pytest.mark.parametrize("path", ["persistent", "launches"])
def test_last_pick_lies_in_the_kept_set_of_the_plans_logits(dev, path, mode, monkeypatch):
    """Ordinary parameters: the kept set follows the device's own float32 logits, so the check uses the plan's logits of
    its last step: every stream's last pick is one of the k codes the rule keeps."""
    B, T = 6, 2
    _env(monkeypatch, 1, launches=path == "launches")
    with _d256_model(dev) as tt:
        for k in (1, 3, 8):
            out, logits = _run(tt, B, T, _feats(T, B), path == "persistent", temperature=1.0, seed=SEED, draw_mode=mode, top_k=k)
            lg = logits.float().numpy()
            for b in range(B):
                assert KC.kept_set(lg[b], k)[out[b, -1]], f"k = {k}, stream {b}: pick {out[b, -1]} outside the kept set"
            if k == 1:
                assert np.array_equal(out[:, -1], lg.argmax(axis=1))


# ---- 8. above one team --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", KC.MODES)
@pytest.mark.parametrize("B,groups", [(33, 0), (64, 2)])
def test_batches_above_one_team(dev, B, groups, mode, monkeypatch):
    """B = 33 on the launch path (one stream past the persistent kernel's limit) and B = 64 in two row groups."""
    T, k = 2, 64
    b4 = SC.b4_pattern("randn")
    feats = SC.features(T, B).numpy().astype(np.float32)
    _env(monkeypatch, groups)
    with _model(dev, GC.DIM, GC.EMB, SC.bias_only_params(S.config(DIM=GC.DIM, EMB_SIZE=GC.EMB), b4)) as tt:
        with _plan(tt, B, T, groups, temperature=1.0, seed=SEED, draw_mode=mode, top_k=k) as gen:
            out = gen.generate(feats).cpu().numpy().copy()
            logits = gen.ws['logits'].detach().cpu().double()
    _check_bias_only_run(out, logits, b4, B)
    draws, excused, worst = KC.judge_draws(out[:, 80:], b4, 1.0, k, SC.u01_table(SEED, T, B), mode)
    print(f"TOPK-GPU B={B} groups={groups} {mode}: draws {draws}, excused mismatches {excused} (worst {worst:.2e})")
    assert draws == 80 * B


# ---- 9. refusals of the C entries ---------------------------------------------------------------------------------------
def test_refusals(dev):
    from parrot_amd import _lib
    s = SC.BIAS_SHAPES["launch-D32-B3"]
    p = S.init_params(S.config(DIM=s.DIM, EMB_SIZE=s.EMB), seed=SC.PARAM_SEED, perturb=0.25)
    lib = _lib.load()
    with _model(dev, s.DIM, s.EMB, p) as tt:
        gen = tt.DeviceGenerator(s.B, s.T, temperature=1.0, top_k=8)
        try:
            assert gen.desc.top_k == 8 and gen.desc.use_graph == 1 and gen.desc.Q == 256
            for k, Q, want in ((-1, 256, 10001), (8, 512, 10002), (511, 512, 10002)):   # BADARG, UNSUPPORTED
                d = type(gen.desc).from_buffer_copy(gen.desc)
                d.top_k, d.Q = k, Q
                plan = C.c_void_p()
                assert lib.samplernn_generate_create(C.byref(d), C.byref(plan)) == want and not plan.value, (k, Q)
            # per-utterance values only beside per-utterance draws, and not once the plan has run
            buf = np.zeros((s.T, s.B), dtype=np.int32)
            assert lib.samplernn_generate_set_utterance_top_k(gen.plan, buf.ctypes.data) == 10001
        finally:
            gen.close()
        gen = tt.DeviceGenerator(s.B, s.T, utterance_draws=True)
        try:
            gen.set_utterance_draws()                      # before the first run: allowed again
            gen.generate(SC.features(s.T, s.B).numpy(), seeds=[1, 2, 3], temperatures=1.0, top_ks=[0, 8, 300])
            assert lib.samplernn_generate_set_utterance_top_k(gen.plan, gen.ws['utt_top_k'].data_ptr()) == 10001
        finally:
            gen.close()
