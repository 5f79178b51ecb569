"""The wave-parallel seeded draw of the SampleRNN generator (SampleRnnGenDesc::draw_mode = 1, DeviceGenerator(draw_mode=
'scan')): `srp_scan_draw` (sr_common.h) in wave 0 of `sr_pick_kernel` (samplernn.hip) and in waves 0..3 of `srp_kernel`'s
pick (sr_persist.hip).  Against the float64 oracle at the derived tolerance DELTA_SCAN, the two kernel paths against each
other, the pattern that tells the mode from the sequential one, a uniform exactly on a boundary, argmax untouched, a real
trajectory, and the mode under every composition the generator has (graphs, row groups, segments, packing, per-utterance
seeds and temperatures).  Cases: tests/samplernn_draw_scan_cases.py (premises: tests/test_samplernn_draw_scan_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import samplernn_ref as S
from tests import samplernn_draw_scan_cases as DC
from tests import samplernn_groups_cases as GC
from tests import samplernn_packed_cases as PC
from tests import samplernn_sampling_cases as SC
from tests import samplernn_utt_draw_cases as UC
from tests.test_gpu_samplernn_groups import _plan
from tests.test_gpu_samplernn_sampling import _check_bias_only_run, _model, _run
from tests.test_gpu_samplernn_utt_draws import _env, _packed_equals_standalone, _utterances

pytestmark = pytest.mark.gpu

SCAN = dict(draw_mode='scan')
D256 = dict(DIM=GC.DIM, EMB=GC.EMB)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == np.int32
    assert np.array_equal(a, b), f"{what}: {(a != b).sum()} of {a.size} samples differ, rows " \
                                 f"{sorted(set(np.nonzero(a != b)[0].tolist()))}"


def _d256_model(dev):
    """Ordinary parameters at DIM 256 (no oracle run behind them: the composition tests compare device runs)."""
    p = S.init_params(S.config(DIM=GC.DIM, EMB_SIZE=GC.EMB), seed=GC.DRAW_PARAM_SEED, perturb=0.25)
    return _model(dev, GC.DIM, GC.EMB, p)


def _feats(T, B):
    return SC.features(T, B, GC.DRAW_FEAT_SEED).numpy().astype(np.float32)


# ---- 1. draws from known logits -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("temperature", DC.TEMPERATURES)
@pytest.mark.parametrize("pattern", DC.PATTERNS)
@pytest.mark.parametrize("shape", sorted(DC.BIAS_SHAPES))
def test_scan_draws_from_known_logits(dev, shape, pattern, temperature):
    """Every pick against draw_pick(b4, temperature, draw_u01(seed, t, b)): a mismatch only within DELTA_SCAN of the CDF
    boundary between the two picks and in at most 0.5 % of the draws; the histogram follows softmax(b4 / temperature)."""
    s = DC.BIAS_SHAPES[shape]
    b4 = SC.b4_pattern(pattern)
    c = S.config(DIM=s.DIM, EMB_SIZE=s.EMB)
    feats = SC.features(s.T, s.B).numpy()
    probs = np.diff(SC.cdf64(b4, temperature), prepend=0.0)
    with _model(dev, s.DIM, s.EMB, SC.bias_only_params(c, b4)) as tt:
        outs = []
        for seed in DC.SEEDS:
            u = SC.u01_table(seed, s.T, s.B)
            out, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=temperature, seed=seed, **SCAN)
            _check_bias_only_run(out, logits, b4, s.B)
            draws, excused, worst = SC.judge_draws(out[:, 80:], b4, temperature, u, delta=DC.DELTA_SCAN)
            stat, dof, pval = SC.chi_square(out[:, 80:], probs)
            print(f"SCAN-GPU {shape} {pattern} T={temperature} seed={seed}: draws {draws}, excused mismatches {excused} "
                  f"(worst {worst:.2e}), chi2 {stat:.1f} / {dof} dof, p {pval:.3g}")
            assert draws == 80 * (s.T - 1) * s.B
            assert dof >= 2 and pval > SC.CHI2_LEVEL, (stat, dof, pval)
            outs.append(out)
        assert not np.array_equal(outs[0], outs[1])


# ---- 2. the launch path equals the persistent path ----------------------------------------------------------------------
@pytest.mark.parametrize("pattern", DC.PATTERNS)
def test_launch_path_equals_persistent_path(dev, pattern, monkeypatch):
    """Exact logits on both paths (g = 0) and one definition of the sums: identical picks, bit for bit."""
    s = DC.BIAS_SHAPES["persist-D256-B5"]
    b4 = SC.b4_pattern(pattern)
    feats = SC.features(s.T, s.B).numpy()
    with _model(dev, s.DIM, s.EMB, SC.bias_only_params(S.config(DIM=s.DIM, EMB_SIZE=s.EMB), b4)) as tt:
        runs = [(tau, seed) for tau in DC.TEMPERATURES for seed in DC.SEEDS]
        persistent = {k: _run(tt, s.B, s.T, feats, True, temperature=k[0], seed=k[1], **SCAN) for k in runs}
        monkeypatch.setenv("PARROT_SR_PERSIST", "0")
        for k in runs:
            launch, logits = _run(tt, s.B, s.T, feats, False, temperature=k[0], seed=k[1], **SCAN)
            _check_bias_only_run(launch, logits, b4, s.B)
            _check_bias_only_run(persistent[k][0], persistent[k][1], b4, s.B)
            _same(launch, persistent[k][0], f"{pattern} temperature {k[0]} seed {k[1]}: sr_pick_kernel against srp_kernel")


# ---- 3. the mode reaches the kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(DC.ABSORB_SHAPES))
def test_mode_reaches_the_kernel(dev, shape):
    """One logit 0, the rest -16.7: the sequential sum absorbs every other term and picks code 0 for every u01; the tree
    keeps them, and each seed holds one draw whose oracle pick is another code.  A build that ignores draw_mode fails."""
    s = DC.ABSORB_SHAPES[shape]
    b4 = DC.absorb_pattern()
    feats = SC.features(s.T, s.B).numpy()
    with _model(dev, s.DIM, s.EMB, SC.bias_only_params(S.config(DIM=s.DIM, EMB_SIZE=s.EMB), b4)) as tt:
        for seed in DC.ABSORB_SEEDS:
            u = SC.u01_table(seed, s.T, s.B)
            (b, j, want), = DC.absorb_hits(seed, s.T, s.B)
            scan, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=seed, **SCAN)
            _check_bias_only_run(scan, logits, b4, s.B)
            print(f"SCAN-GPU absorption {shape} seed {seed}: stream {b} sample {80 + j}: pick {scan[b, 80 + j]}, oracle {want}")
            assert scan[b, 80 + j] != 0, "the scan mode drew code 0 where the oracle does not: draw_mode did not reach the kernel"
            SC.judge_draws(scan[:, 80:], b4, 1.0, u, delta=DC.DELTA_SCAN)
            seq, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=seed, draw_mode='sequential')
            _check_bias_only_run(seq, logits, b4, s.B)
            assert (seq[:, 80:] == 0).all(), "the sequential mode's sum is exactly 1.0: it picks code 0 everywhere"


# ---- 4. a uniform exactly on a boundary ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SC.EDGE_SHAPES))
def test_uniform_exactly_on_a_boundary(dev, shape):
    """All logits equal: every term is 1 and every tree sum an exact integer, so the pick is floor(256 u01) with no slack,
    on the hits too, where `<=` would be off by one."""
    s = SC.EDGE_SHAPES[shape]
    b4 = np.full(SC.Q, SC.EDGE_LOGIT, dtype=np.float32)
    feats = SC.features(s.T, s.B).numpy()
    with _model(dev, s.DIM, s.EMB, SC.bias_only_params(S.config(DIM=s.DIM, EMB_SIZE=s.EMB), b4)) as tt:
        for seed in SC.EDGE_SEEDS:
            u = SC.u01_table(seed, s.T, s.B)
            want = SC.oracle_picks(b4, 1.0, u)
            hits = SC.edge_hits(seed, s.T, s.B)
            assert hits
            for temperature in (1.0, 0.5):
                out, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=temperature, seed=seed, **SCAN)
                _check_bias_only_run(out, logits, b4, s.B)
                for b, j, m in hits:
                    assert out[b, 80 + j] == m, f"stream {b}, sample {80 + j}: u01 == c_{m - 1}, pick {out[b, 80 + j]}"
                assert np.array_equal(out[:, 80:], want), f"{(out[:, 80:] != want).sum()} picks differ"


# ---- 5. temperature 0 and the one-hot pattern ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SC.TIE_SHAPES))
def test_argmax_is_untouched(dev, shape):
    s = SC.TIE_SHAPES[shape]
    c = S.config(DIM=s.DIM, EMB_SIZE=s.EMB)
    feats = SC.features(s.T, s.B).numpy()
    for name in SC.TIE_MAXIMA:
        b4, want = SC.tie_pattern(name)
        with _model(dev, s.DIM, s.EMB, SC.bias_only_params(c, b4)) as tt:
            scan, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=0.0, **SCAN)
            _check_bias_only_run(scan, logits, b4, s.B)
            seq, _ = _run(tt, s.B, s.T, feats, s.persistent, temperature=0.0)
            _same(scan, seq, f"{name}: argmax in scan mode")
            assert np.unique(scan[:, 80:]).tolist() == [want]
    b4 = SC.one_hot_pattern()
    with _model(dev, s.DIM, s.EMB, SC.bias_only_params(c, b4)) as tt:
        scan, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=SC.TRAJ_SEED, **SCAN)
        _check_bias_only_run(scan, logits, b4, s.B)
        seq, _ = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=SC.TRAJ_SEED)
        _same(scan, seq, "one-hot")
        assert np.unique(scan[:, 80:]).tolist() == [SC.ONE_HOT_CODE]


# ---- 6. along a trajectory ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.TRAJ_SHAPES))
def test_scan_draws_along_a_trajectory(dev, name):
    s = SC.TRAJ_SHAPES[name]
    p, feats, ref, ref_logits = SC.traj_reference(name)
    T, seed = SC.TRAJ_TEMPERATURE, SC.TRAJ_SEED
    with _model(dev, s.DIM, s.EMB, p) as tt:
        out, _ = _run(tt, s.B, s.T, feats.numpy(), s.persistent, temperature=T, seed=seed, **SCAN)
        exact, left = SC.draws_follow_oracle(out, ref, ref_logits, T, seed, s.B)
        print(f"SCAN-GPU trajectory {name}: rows identical {len(exact)} of {s.B}; left "
              f"(row, sample, pick, oracle, distance, allowed): {left}")


# ---- 7. composition: each bit-identical to its plain counterpart in scan mode, DIM 256 ----------------------------------
def test_graph_equals_eager(dev):
    B, T = 5, 3
    with _d256_model(dev) as tt:
        graph, _ = _run(tt, B, T, _feats(T, B), True, temperature=1.0, seed=SC.SEEDS[1], use_graph=True, **SCAN)
        eager, _ = _run(tt, B, T, _feats(T, B), True, temperature=1.0, seed=SC.SEEDS[1], use_graph=False, **SCAN)
    _same(graph, eager, "graph replay against eager launches")
    assert len(np.unique(graph[:, 80:])) > 20


def test_chunk_graph_equals_eager(dev):
    s = SC.REPLAY_SHAPES["persist-D256-B5-T10"]     # nine periods: the eight-period graph, then the one-period graph
    with _d256_model(dev) as tt:
        graph, _ = _run(tt, s.B, s.T, _feats(s.T, s.B), s.persistent, calls=2, temperature=1.0, seed=234, use_graph=True, **SCAN)
        eager, _ = _run(tt, s.B, s.T, _feats(s.T, s.B), s.persistent, temperature=1.0, seed=234, use_graph=False, **SCAN)
    _same(graph, eager, "chunk graph against eager launches")


@pytest.mark.parametrize("B", [33, 37])
def test_row_groups_equal_the_launch_path(dev, B, monkeypatch):
    """Bias-only logits (exact on both paths): streams 32 .. B - 1 draw in the second row group what sr_pick_kernel draws."""
    T = 2
    b4 = SC.b4_pattern("randn")
    feats = SC.features(T, B).numpy()
    with _model(dev, GC.DIM, GC.EMB, SC.bias_only_params(S.config(DIM=GC.DIM, EMB_SIZE=GC.EMB), b4)) as tt:
        _env(monkeypatch, 2)
        with _plan(tt, B, T, 2, temperature=1.0, seed=SC.SEEDS[1], **SCAN) as gen:
            groups = gen.generate(feats.astype(np.float32)).cpu().numpy().copy()
        _env(monkeypatch, 2, launches=True)
        with _plan(tt, B, T, 0, temperature=1.0, seed=SC.SEEDS[1], **SCAN) as gen:
            launch = gen.generate(feats.astype(np.float32)).cpu().numpy().copy()
    _same(groups, launch, f"B = {B}: two row groups against the launch path")
    SC.judge_draws(groups[:, 80:], b4, 1.0, SC.u01_table(SC.SEEDS[1], T, B), delta=DC.DELTA_SCAN)


def test_segments_equal_one_piece(dev):
    B, N, S_ = 5, 7, 2
    feats = _feats(N, B)
    with _d256_model(dev) as tt:
        with _plan(tt, B, N, 1, temperature=1.0, seed=SC.SEEDS[1], **SCAN) as gen:
            whole = gen.generate(feats).cpu().numpy().copy()
        pieces = list(tt.generate_stream(feats, S_, temperature=1.0, seed=SC.SEEDS[1], **SCAN))
    assert len(pieces) == 3
    _same(np.concatenate(pieces, axis=1), whole, "resumed segments against the run in one piece")
    assert len(np.unique(whole[:, 80:])) > 20


def test_packed_equals_standalone(dev, monkeypatch):
    """A packed plan with per-utterance draws (temperatures 0, 0.5, 1 and 2 among them) against plain plans carrying the
    same utterance alone in the same stream, all in scan mode."""
    case = PC.GRU_PACKING
    utts = _utterances(_feats(case.max_len, len(case.lengths)), case.lengths)
    _env(monkeypatch, 1)
    with _d256_model(dev) as tt:
        _packed_equals_standalone(tt, case, utts, 1, "scan mode, persistent", **SCAN)


@pytest.mark.parametrize("path", ["persistent", "launches"])
def test_utterance_seeds_equal_the_plan_key(dev, path, monkeypatch):
    B, T, s, tau = 5, 3, 2 ** 63 + 5, 1.0
    groups = 1 if path == "persistent" else 0
    _env(monkeypatch, 1, launches=path == "launches")
    with _d256_model(dev) as tt:
        with _plan(tt, B, T, groups, temperature=tau, seed=s, **SCAN) as gen:
            old = gen.generate(_feats(T, B)).cpu().numpy().copy()
        with _plan(tt, B, T, groups, utterance_draws=True, **SCAN) as gen:
            new = gen.generate(_feats(T, B), seeds=[UC.old_key_seed(s, b) for b in range(B)], temperatures=tau).cpu().numpy().copy()
    _same(new, old, f"{path}: seeds s ^ K2 (b + 1) against the plan key")
    assert len(np.unique(old[:, 80:])) > 20


@pytest.mark.parametrize("path", ["persistent", "launches"])
def test_one_team_mixes_temperatures(dev, path, monkeypatch):
    """Rows 0 .. 3 (one team of the persistent kernel) at temperatures 0, 0.5, 1 and 2: each row equals the same row of a
    plan whose four rows all run at that row's temperature."""
    B, T = 4, 3
    groups = 1 if path == "persistent" else 0
    temps, seeds = list(UC.TEAM_TEMPERATURES), UC.utt_seeds(B)
    assert temps == [0.0, 0.5, 1.0, 2.0]
    _env(monkeypatch, 1, launches=path == "launches")
    with _d256_model(dev) as tt:
        with _plan(tt, B, T, groups, utterance_draws=True, **SCAN) as gen:
            mixed = gen.generate(_feats(T, B), seeds=seeds, temperatures=temps).cpu().numpy().copy()
            for b in range(B):
                alone = gen.generate(_feats(T, B), seeds=seeds, temperatures=temps[b]).cpu().numpy().copy()
                assert np.array_equal(mixed[b], alone[b]), f"row {b} at temperature {temps[b]}: {(mixed[b] != alone[b]).sum()} differ"
        with _plan(tt, B, T, groups, temperature=0.0) as gen:
            greedy = gen.generate(_feats(T, B)).cpu().numpy().copy()
    assert np.array_equal(mixed[0], greedy[0]), "the argmax row of a mixed team is the sequential plan's argmax"
    assert len(np.unique(mixed[1:, 80:])) > 20


# ---- 8. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from parrot_amd import _lib
    s = SC.BIAS_SHAPES["launch-D32-B3"]
    p = S.init_params(S.config(DIM=s.DIM, EMB_SIZE=s.EMB), seed=SC.PARAM_SEED, perturb=0.25)
    with _model(dev, s.DIM, s.EMB, p) as tt:
        gen = tt.DeviceGenerator(s.B, s.T, temperature=1.0, **SCAN)
        try:
            assert gen.desc.draw_mode == 1 and gen.desc.Q == 256
            for mode, Q in ((2, 256), (-1, 256), (1, 250), (1, 32)):
                d = type(gen.desc).from_buffer_copy(gen.desc)
                d.draw_mode, d.Q = mode, Q
                plan = C.c_void_p()
                rc = _lib.load().samplernn_generate_create(C.byref(d), C.byref(plan))
                assert rc == 10001 and not plan.value, (mode, Q, rc)     # PARROT_ERR_BADARG, no plan
                with pytest.raises(_lib.HipCallError):
                    _lib.call('samplernn_generate_create', C.byref(d), C.byref(plan))
        finally:
            gen.close()


# ---- 9. the default is untouched ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.TRAJ_SHAPES))
def test_default_is_the_sequential_mode(dev, name):
    s = SC.TRAJ_SHAPES[name]
    p = S.init_params(S.config(DIM=s.DIM, EMB_SIZE=s.EMB), seed=s.param_seed, perturb=0.25)
    feats = SC.features(s.T, s.B, s.feat_seed).numpy()
    with _model(dev, s.DIM, s.EMB, p) as tt:
        left_out, _ = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=SC.TRAJ_SEED)
        named, _ = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=SC.TRAJ_SEED, draw_mode='sequential')
    _same(named, left_out, "draw_mode='sequential' against the keyword left out")
    assert len(np.unique(named[:, 80:])) > 20
