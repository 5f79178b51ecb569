"""The SampleRNN generator's pick -- `sr_pick_kernel` (samplernn.hip) and lane 0 of waves 0..3 in `srp_kernel`
(sr_persist.hip) -- against the float64 oracle: seeded multinomial draws from known logits and along a real
trajectory, exact arg-max ties, the eight-period chunk graph with plan reuse, and the batch just past the persistent
kernel's limit.  Cases, references and judging rules: tests/samplernn_sampling_cases.py (premises checked on the CPU by
tests/test_samplernn_sampling_cases_cpu.py); measured figures: profiles/samplernn_sampling.md."""
import contextlib

import numpy as np
import pytest

from oracle import samplernn_ref as S
from tests import samplernn_sampling_cases as SC
from tests.test_gpu_samplernn import _greedy_follows_oracle
from tests.util import assert_close

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _model(dev, DIM, EMB, p, weight_norm=True):
    """The generator's module configured for one width with the parameters p registered."""
    from parrot_amd.sampleRNN import lib
    from parrot_amd.sampleRNN.models.conditional import three_tier as tt
    lib.delete_all_params()
    lib.set_device(dev)
    tt.configure(DIM=DIM, EMB_SIZE=EMB, RNN_TYPE='GRU', N_RNN=1, WEIGHT_NORM=weight_norm)
    try:
        lib.set_params(p)
        yield tt
    finally:
        lib.delete_all_params()
        tt.configure(DIM=1024, EMB_SIZE=256, RNN_TYPE='GRU', N_RNN=1, WEIGHT_NORM=True)


def _run(tt, B, T, feats, persistent, calls=1, **kw):
    """One plan, `calls` generate() calls on it -> the last call's samples (numpy) and last-step logits (float64)."""
    gen = tt.DeviceGenerator(B, T, **kw)
    try:
        assert gen.persistent == persistent, "the persistent sample kernel %s" % (
            "did not engage on a qualifying shape" if persistent else "engaged where it must not")
        for _ in range(calls):
            out = gen.generate(np.asarray(feats, dtype=np.float32)).cpu().numpy().copy()
        return out, gen.ws['logits'].detach().cpu().double()
    finally:
        gen.close()


def _check_bias_only_run(out, logits, b4, B):
    assert out.dtype == np.int32 and (out[:, :80] == 128).all()
    # the premise of the construction: the logits ARE the bias, bit for bit
    assert np.array_equal(logits.float().numpy(), np.broadcast_to(b4, (B, SC.Q))), "logits differ from the bias"


# ---- 2. draws from known logits -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("temperature", SC.TEMPERATURES)
@pytest.mark.parametrize("pattern", SC.PATTERNS)
@pytest.mark.parametrize("shape", sorted(SC.BIAS_SHAPES))
def test_seeded_draws_from_known_logits(dev, shape, pattern, temperature, monkeypatch):
    """Every one of the 80 (T - 1) B picks against draw_pick(b4, temperature, draw_u01(seed, t, b)): a mismatch only within
    DELTA of the CDF boundary between the two picks and in at most 0.5 % of the draws; graph replay == eager launches;
    the histogram follows softmax(b4 / temperature); the persistent kernel and the launch path give identical arrays."""
    s = SC.BIAS_SHAPES[shape]
    b4 = SC.b4_pattern(pattern)
    c = S.config(DIM=s.DIM, EMB_SIZE=s.EMB)
    feats = SC.features(s.T, s.B).numpy()
    probs = np.diff(SC.cdf64(b4, temperature), prepend=0.0)
    with _model(dev, s.DIM, s.EMB, SC.bias_only_params(c, b4)) as tt:
        outs = {}
        for seed in SC.SEEDS:
            u = SC.u01_table(seed, s.T, s.B)
            for use_graph in (True, False):
                out, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=temperature, seed=seed,
                                   use_graph=use_graph)
                _check_bias_only_run(out, logits, b4, s.B)
                draws, excused, worst = SC.judge_draws(out[:, 80:], b4, temperature, u)
                stat, dof, pval = SC.chi_square(out[:, 80:], probs)
                print(f"SAMPLING-GPU {shape} {pattern} T={temperature} seed={seed} graph={int(use_graph)}: draws {draws}, "
                      f"excused mismatches {excused} (worst {worst:.2e}), chi2 {stat:.1f} / {dof} dof, p {pval:.3g}")
                assert draws == 80 * (s.T - 1) * s.B
                assert dof >= 2 and pval > SC.CHI2_LEVEL, (stat, dof, pval)
                outs[seed, use_graph] = out
            assert np.array_equal(outs[seed, True], outs[seed, False]), "graph replay and eager launches draw differently"
        assert not np.array_equal(outs[SC.SEEDS[0], True], outs[SC.SEEDS[1], True])
        if s.persistent:  # the same expression in the same order on identical logits: identical samples
            monkeypatch.setenv("PARROT_SR_PERSIST", "0")
            for seed in SC.SEEDS:
                launch, logits = _run(tt, s.B, s.T, feats, False, temperature=temperature, seed=seed)
                _check_bias_only_run(launch, logits, b4, s.B)
                same = np.array_equal(launch, outs[seed, True])
                print(f"SAMPLING-GPU {shape} {pattern} T={temperature} seed={seed}: persistent == launch path: {same} "
                      f"({int((launch != outs[seed, True]).sum())} differ)")
                assert same, f"{(launch != outs[seed, True]).sum()} picks differ between the persistent kernel and sr_pick_kernel"


def test_seeded_draws_without_weight_norm(dev):
    """The same construction with WEIGHT_NORM off (W = 0): the launch path's logits are the bias here as well."""
    s = SC.BIAS_SHAPES["launch-D32-B3"]
    b4 = SC.b4_pattern("randn")
    c = S.config(DIM=s.DIM, EMB_SIZE=s.EMB, WEIGHT_NORM=False)
    feats = SC.features(s.T, s.B).numpy()
    with _model(dev, s.DIM, s.EMB, SC.bias_only_params(c, b4), weight_norm=False) as tt:
        out, logits = _run(tt, s.B, s.T, feats, False, temperature=1.0, seed=SC.SEEDS[0])
        _check_bias_only_run(out, logits, b4, s.B)
        SC.judge_draws(out[:, 80:], b4, 1.0, SC.u01_table(SC.SEEDS[0], s.T, s.B))


@pytest.mark.parametrize("shape", sorted(SC.EDGE_SHAPES))
def test_uniform_exactly_on_a_boundary(dev, shape):
    """All logits equal: the device's sums are the integers 1..256 and 256 u01 is exact, so every pick equals the
    oracle's with no slack; the seeds put one u01 exactly on a boundary, where the strict `u01 < c_q` decides."""
    s = SC.EDGE_SHAPES[shape]
    b4 = np.full(SC.Q, SC.EDGE_LOGIT, dtype=np.float32)
    c = S.config(DIM=s.DIM, EMB_SIZE=s.EMB)
    feats = SC.features(s.T, s.B).numpy()
    with _model(dev, s.DIM, s.EMB, SC.bias_only_params(c, b4)) as tt:
        for seed in SC.EDGE_SEEDS:
            u = SC.u01_table(seed, s.T, s.B)
            want = SC.oracle_picks(b4, 1.0, u)
            for temperature in (1.0, 0.5):   # (0 / temperature: the same draw)
                out, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=temperature, seed=seed)
                _check_bias_only_run(out, logits, b4, s.B)
                for b, j, m in SC.edge_hits(seed, s.T, s.B):
                    assert out[b, 80 + j] == m, f"stream {b}, sample {80 + j}: u01 == c_{m - 1}, pick {out[b, 80 + j]}"
                assert np.array_equal(out[:, 80:], want), f"{(out[:, 80:] != want).sum()} picks differ"


# ---- 3. draws along a real trajectory -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.TRAJ_SHAPES))
def test_seeded_draws_along_a_trajectory(dev, name):
    """Ordinary parameters, temperature 1: rows equal S.generate(..., temperature, seed); a row may leave only where u01
    is within e / (2 T) + DELTA of a boundary of the oracle's CDF, at most max(1, B // 4) rows do, and the rows that stay
    end with the oracle's logits."""
    s = SC.TRAJ_SHAPES[name]
    p, feats, ref, ref_logits = SC.traj_reference(name)
    T, seed = SC.TRAJ_TEMPERATURE, SC.TRAJ_SEED
    with _model(dev, s.DIM, s.EMB, p) as tt:
        outs = {}
        for use_graph in (True, False):
            out, last = _run(tt, s.B, s.T, feats.numpy(), s.persistent, calls=2, temperature=T, seed=seed,
                             use_graph=use_graph)
            exact, left = SC.draws_follow_oracle(out, ref, ref_logits, T, seed, s.B)
            print(f"SAMPLING-GPU trajectory {name} graph={int(use_graph)}: rows identical {len(exact)} of {s.B}; left "
                  f"(row, sample, pick, oracle, distance, allowed): {left}")
            assert_close(last[exact], ref_logits[exact, -1], 1e-4, "last-step logits")
            outs[use_graph] = out
        assert np.array_equal(outs[True], outs[False])


# ---- 4. exact ties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SC.TIE_SHAPES))
def test_argmax_ties_take_the_lowest_index(dev, shape):
    """Bias-only logits made to tie, temperature 0: every sample of every stream is the lowest index that holds the
    maximum (no slack: the logits are exact); at temperature 1 a code 60 above the rest is drawn every time."""
    s = SC.TIE_SHAPES[shape]
    c = S.config(DIM=s.DIM, EMB_SIZE=s.EMB)
    feats = SC.features(s.T, s.B).numpy()
    for name in SC.TIE_MAXIMA:
        b4, want = SC.tie_pattern(name)
        with _model(dev, s.DIM, s.EMB, SC.bias_only_params(c, b4)) as tt:
            for use_graph in (True, False):
                out, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=0.0, use_graph=use_graph)
                _check_bias_only_run(out, logits, b4, s.B)
                got = np.unique(out[:, 80:])
                assert got.tolist() == [want], f"{name}: picks {got.tolist()}, lowest index of the maximum is {want}"
    b4 = SC.one_hot_pattern()
    with _model(dev, s.DIM, s.EMB, SC.bias_only_params(c, b4)) as tt:
        out, logits = _run(tt, s.B, s.T, feats, s.persistent, temperature=1.0, seed=SC.TRAJ_SEED)
        _check_bias_only_run(out, logits, b4, s.B)
        assert np.unique(out[:, 80:]).tolist() == [SC.ONE_HOT_CODE]


# ---- 5. chunked graph replay and plan reuse -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.REPLAY_SHAPES))
def test_chunk_graph_replay_and_plan_reuse(dev, name):
    """T - 1 >= 8 periods: SrPlan::run replays the eight-period graph and then the one-period graph.  Greedy samples vs
    the float64 oracle, graph == eager launches, and a plan that has run twice gives a fresh plan's samples on other
    features (nothing stale crosses a chunk replay)."""
    s = SC.REPLAY_SHAPES[name]
    Tmax = max(r.T for r in SC.REPLAY_SHAPES.values() if (r.DIM, r.B) == (s.DIM, s.B))
    p, feats, ref, ref_logits = SC.greedy_reference(s.DIM, s.EMB, s.B, Tmax)
    feats, ref, ref_logits = feats[:s.T].numpy(), ref[:, :80 * s.T], ref_logits[:, :80 * (s.T - 1)]
    feats2 = SC.features(s.T, s.B, SC.REPLAY_FEAT_SEED_2).numpy()
    with _model(dev, s.DIM, s.EMB, p) as tt:
        eager, last = _run(tt, s.B, s.T, feats, s.persistent, temperature=0.0, use_graph=False)
        exact = _greedy_follows_oracle(eager, ref, ref_logits, s.B, slack_rows=1)
        assert_close(last[exact], ref_logits[exact, -1], 1e-4, "last-step logits")
        eager2, _ = _run(tt, s.B, s.T, feats2, s.persistent, temperature=0.0, use_graph=False)
        assert not np.array_equal(eager2, eager)
        gen = tt.DeviceGenerator(s.B, s.T, temperature=0.0, use_graph=True)
        try:
            assert gen.persistent == s.persistent
            for call in range(2):
                out = gen.generate(feats).cpu().numpy().copy()
                assert np.array_equal(out, eager), f"call {call}: {(out != eager).sum()} samples differ from eager launches"
            again = gen.generate(feats2).cpu().numpy().copy()
        finally:
            gen.close()
        fresh, _ = _run(tt, s.B, s.T, feats2, s.persistent, temperature=0.0, use_graph=True)
        assert np.array_equal(again, fresh), f"{(again != fresh).sum()} samples differ from a fresh plan's"
        assert np.array_equal(again, eager2), f"{(again != eager2).sum()} samples differ from eager launches"


# ---- 6. just past the persistent kernel's batch limit -------------------------------------------------------------------
def test_batch_past_the_persistent_limit_runs_on_launches(dev):
    s = SC.LIMIT_SHAPE
    p, feats, ref, ref_logits = SC.greedy_reference(s.DIM, s.EMB, s.B, s.T)
    with _model(dev, s.DIM, s.EMB, p) as tt:
        for use_graph in (True, False):
            gen = tt.DeviceGenerator(s.B, s.T, temperature=0.0, use_graph=use_graph)
            try:
                assert not gen.persistent and 'persist_ws' not in gen.ws   # samplernn_persist_floats returned 0
                out = gen.generate(feats.numpy()).cpu().numpy().copy()
                last = gen.ws['logits'].detach().cpu().double()
            finally:
                gen.close()
            exact = _greedy_follows_oracle(out, ref, ref_logits, s.B, slack_rows=1)
            assert_close(last[exact], ref_logits[exact, -1], 1e-4, "last-step logits")
        # one stream fewer takes the persistent kernel
        gen = tt.DeviceGenerator(SC.PERSIST_MAX_B, s.T, temperature=0.0)
        try:
            assert gen.persistent
        finally:
            gen.close()
