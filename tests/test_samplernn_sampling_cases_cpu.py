"""The premises of tests/test_gpu_samplernn_sampling.py, checked without a GPU: the oracle's seeded draw (pieces and
defaults), the float32 restatement of the kernels' arithmetic inside half the caps the GPU test grants, the oracle's own
histograms under the chi-square, the seeds of the trajectory cases, the tie patterns and the replay arithmetic."""
import math

import numpy as np
import pytest
import torch

from oracle import samplernn_ref as S
from tests import samplernn_sampling_cases as SC


def _splitmix_u01(seed, t, b):
    """Independent restatement with numpy uint64 (wrap-around arithmetic instead of masked Python integers)."""
    with np.errstate(over="ignore"):
        u = np.uint64
        x = u(seed) ^ (u(0x9E3779B97F4A7C15) * u(t + 1)) ^ (u(0xBF58476D1CE4E5B9) * u(b + 1))
        x ^= x >> u(30); x *= u(0xBF58476D1CE4E5B9)
        x ^= x >> u(27); x *= u(0x94D049BB133111EB)
        x ^= x >> u(31)
    return float(np.float32(np.float64(int(x) >> 40) + 0.5)) / 2.0 ** 24


def test_draw_u01_pieces():
    for seed in SC.SEEDS + (0, 2 ** 64 - 1):
        for t, b in ((80, 0), (81, 0), (80, 1), (239, 31), (879, 4)):
            u = S.draw_u01(seed, t, b)
            assert u == _splitmix_u01(seed, t, b)
            assert 0.0 < u <= 1.0 and u * 2 ** 25 == round(u * 2 ** 25) and float(np.float32(u)) == u
    # every argument matters, the seed beyond 32 bits too
    base = S.draw_u01(234, 80, 0)
    assert len({base, S.draw_u01(234, 81, 0), S.draw_u01(234, 80, 1), S.draw_u01(235, 80, 0),
                S.draw_u01(234 + 2 ** 32, 80, 0), S.draw_u01(234 + 2 ** 40, 80, 0)}) == 6
    assert S.draw_u01(2 ** 40 + 3, 80, 0) != S.draw_u01(3, 80, 0)
    # (k + 0.5) rounds to even in float32 once k has 24 bits: an odd k goes up, the largest one to 2^24 -> u01 = 1.0
    assert float(np.float32(float(2 ** 24 - 1) + 0.5)) / 2.0 ** 24 == 1.0
    u = SC.u01_table(234, 3, 32)
    assert u.shape == (32, 160) and u[3, 7] == S.draw_u01(234, 87, 3)
    assert abs(u.mean() - 0.5) < 0.02 and u.min() < 0.01 and u.max() > 0.99


def test_draw_pick_and_cdf():
    lg = torch.tensor([0.0, math.log(3.0), 0.0, -1e9])
    c = S.draw_cdf(lg, 1.0)
    assert c.dtype == torch.float64 and torch.allclose(c, torch.tensor([0.2, 0.8, 1.0, 1.0], dtype=torch.float64))
    assert S.draw_pick(lg, 1.0, 0.0) == 0 and S.draw_pick(lg, 1.0, 0.19) == 0
    assert S.draw_pick(lg, 1.0, 0.21) == 1 and S.draw_pick(lg, 1.0, 0.79) == 1 and S.draw_pick(lg, 1.0, 0.81) == 2
    assert S.draw_pick(lg, 1.0, 1.0) == 3          # no q with u01 < c_q: the last code
    u_at = float(c[0])
    assert S.draw_pick(lg, 1.0, u_at) == 1         # u01 == c_q belongs to the next bin (strict <)
    # temperature divides the logits: 3^(1/T) : 1 : 1
    assert torch.allclose(S.draw_cdf(lg, 0.5)[:3], torch.tensor([1 / 11, 10 / 11, 1.0], dtype=torch.float64))
    assert torch.allclose(S.draw_cdf(lg, 2.0)[0], torch.tensor(1 / (2 + 3 ** 0.5), dtype=torch.float64))
    # the vectorised form the GPU test uses is draw_pick
    b4 = SC.b4_pattern("randn")
    u = SC.u01_table(234, 3, 3)
    for T in SC.TEMPERATURES:
        want = SC.oracle_picks(b4, T, u)
        for b in range(3):
            for j in range(0, 160, 7):
                assert want[b, j] == S.draw_pick(torch.from_numpy(b4), T, u[b, j])
    assert SC.oracle_picks(b4, 1.0, np.array([[1.0]]))[0, 0] == SC.Q - 1


def _generate_before(p, c, features, return_logits=False):
    """S.generate as it was before it learnt to draw (greedy only), restated to pin the defaults."""
    BFS, FS, D = c['BIG_FRAME_SIZE'], c['FRAME_SIZE'], c['DIM']
    feats = features.transpose(0, 1)
    B, LENGTH = feats.shape[0], feats.shape[1] * BFS
    samples = torch.zeros(B, LENGTH, dtype=torch.int64)
    samples[:, :BFS] = c['Q_LEVELS'] // 2
    dt = p['FrameLevel.h0'].dtype
    big_h0 = torch.zeros(B, c['N_RNN'], c['H0_MULT'] * c['BIG_DIM'], dtype=dt)
    h0 = torch.zeros(B, c['N_RNN'], c['H0_MULT'] * D, dtype=dt)
    big_out = frame_out = None
    all_logits = []
    for t in range(BFS, LENGTH):
        if t % BFS == 0:
            big_out, big_h0, _ = S.big_frame_level_rnn(p, c, samples[:, t - BFS:t], big_h0, t == BFS,
                                                       feats[:, t // BFS][:, None])
        if t % FS == 0:
            frame_out, h0 = S.frame_level_rnn(p, c, samples[:, t - FS:t],
                                              big_out[:, (t // FS) % (BFS // FS)][:, None], h0, t == BFS)
        logits = S.sample_level_predictor(p, c, frame_out[:, t % FS], samples[:, t - FS:t])
        all_logits.append(logits)
        samples[:, t] = torch.argmax(torch.softmax(logits, -1), -1)
    return samples.to(torch.int32), torch.stack(all_logits, 1)


def test_generate_defaults_unchanged_and_draws_use_the_pieces():
    c = S.config(DIM=32, EMB_SIZE=8)
    p = S.init_params(c, seed=5, perturb=0.2)
    feats = SC.features(3, 2, 2)
    with torch.no_grad():
        want, want_lg = _generate_before(p, c, feats)
        got, got_lg = S.generate(p, c, feats, return_logits=True)
        assert torch.equal(got, want) and torch.equal(got_lg, want_lg)
        assert torch.equal(S.generate(p, c, feats), want)
        assert torch.equal(S.generate(p, c, feats, temperature=0.0, seed=99), want)
        out, lg = S.generate(p, c, feats, return_logits=True, temperature=1.0, seed=77)
    assert out.dtype == torch.int32 and (out[:, :80] == 128).all() and not torch.equal(out, want)
    for b in range(2):
        for t in (80, 81, 159, 160, 239):
            assert int(out[b, t]) == S.draw_pick(lg[b, t - 80], 1.0, S.draw_u01(77, t, b))
    with torch.no_grad():
        assert not torch.equal(S.generate(p, c, feats, temperature=1.0, seed=78), out)


# ---- draws from known logits --------------------------------------------------------------------------------------------
def test_patterns():
    for name in SC.PATTERNS:
        b = SC.b4_pattern(name)
        assert b.dtype == np.float32 and b.shape == (SC.Q,) and np.array_equal(b, SC.b4_pattern(name))
    for T in SC.TEMPERATURES:
        pk = np.diff(SC.cdf64(SC.b4_pattern("peaked"), T), prepend=0.0)
        assert pk[list(SC.PEAKED_CODES)].sum() > 0.99 and pk[list(SC.PEAKED_CODES)].min() > 0.05
        fl = np.diff(SC.cdf64(SC.b4_pattern("flat"), T), prepend=0.0)
        assert fl.max() / fl.min() < 1.2
        rn = np.diff(SC.cdf64(SC.b4_pattern("randn"), T), prepend=0.0)
        assert rn.max() / rn.min() > 100
    # in float32 the bias survives the trip through the float64 parameter dict bit for bit
    c = S.config(DIM=32, EMB_SIZE=8)
    b4 = SC.b4_pattern("randn")
    p = SC.bias_only_params(c, b4)
    assert np.array_equal(p['SampleLevel.Output.b'].float().numpy(), b4)
    x = torch.randn(3, 32, dtype=torch.float64)
    assert torch.equal(S.linear(p, c, 'SampleLevel.Output', x), p['SampleLevel.Output.b'].expand(3, -1))
    c2 = S.config(DIM=32, EMB_SIZE=8, WEIGHT_NORM=False)
    p2 = SC.bias_only_params(c2, b4)
    assert torch.equal(S.linear(p2, c2, 'SampleLevel.Output', x), p2['SampleLevel.Output.b'].expand(3, -1))


@pytest.mark.parametrize("pattern", SC.PATTERNS)
@pytest.mark.parametrize("shape", sorted(SC.BIAS_SHAPES))
def test_emulation_keeps_half_the_cap_and_oracle_passes_chi_square(shape, pattern):
    """What the GPU test grants the kernels -- mismatches only within DELTA of a boundary, at most 0.5 % of the draws -- a
    float32 restatement of their arithmetic keeps with half the cap; and the oracle's own picks follow its
    probabilities."""
    s = SC.BIAS_SHAPES[shape]
    b4 = SC.b4_pattern(pattern)
    for T in SC.TEMPERATURES:
        probs = np.diff(SC.cdf64(b4, T), prepend=0.0)
        for seed in SC.SEEDS:
            u = SC.u01_table(seed, s.T, s.B)
            emu = SC.emulate_picks_f32(b4, T, u)
            draws, excused, worst = SC.judge_draws(emu, b4, T, u, cap=SC.EXCUSED_CAP / 2)
            assert draws == 80 * (s.T - 1) * s.B
            stat, dof, pval = SC.chi_square(SC.oracle_picks(b4, T, u), probs)
            print(f"SAMPLING-CPU {shape} {pattern} T={T} seed={seed}: draws {draws}, emulation mismatches {excused} "
                  f"(worst {worst:.2e}), oracle chi2 {stat:.1f} / {dof} dof, p {pval:.3g}")
            assert dof >= 2 and pval > SC.CHI2_LEVEL, (stat, dof, pval)


def test_judge_and_chi_square_reject_what_they_should():
    b4 = SC.b4_pattern("randn")
    u = SC.u01_table(234, 3, 5)
    good = SC.oracle_picks(b4, 1.0, u)
    assert SC.judge_draws(good, b4, 1.0, u)[1] == 0
    for wrong in (SC.oracle_picks(b4, 2.0, u),                               # temperature ignored / inverted
                  SC.oracle_picks(b4, 1.0, SC.u01_table(235, 3, 5)),         # another seed
                  SC.oracle_picks(b4, 1.0, np.roll(u, 1, axis=1)),           # t off by one
                  SC.oracle_picks(b4, 1.0, np.roll(u, 1, axis=0)),           # b off by one
                  np.minimum(good + 1, SC.Q - 1)):                           # CDF off by one bin
        with pytest.raises(AssertionError):
            SC.judge_draws(wrong, b4, 1.0, u)
    probs = np.diff(SC.cdf64(b4, 1.0), prepend=0.0)
    assert SC.chi_square(good, probs)[2] > SC.CHI2_LEVEL
    assert SC.chi_square(SC.oracle_picks(b4, 2.0, u), probs)[2] < SC.CHI2_LEVEL
    assert SC.chi_square(SC.oracle_picks(b4, 0.5, u), probs)[2] < SC.CHI2_LEVEL
    # pooling: expectations below 5 join their neighbours
    stat, dof, pval = SC.chi_square(np.array([0] * 50 + [1] * 50), np.array([0.5, 0.49, 0.005, 0.005]))
    assert dof == 1 and stat < 0.1 and pval > 0.5
    assert SC.boundary_distance(np.array([0.2, 0.8, 1.0]), 0.25, 0, 1) == pytest.approx(0.05)
    assert SC.boundary_distance(np.array([0.2, 0.8, 1.0]), 0.25, 2, 0) == pytest.approx(0.55)


def test_edge_seeds_put_a_uniform_exactly_on_a_boundary():
    b4 = np.full(SC.Q, SC.EDGE_LOGIT, dtype=np.float32)
    c = SC.cdf64(b4, 1.0)
    assert np.array_equal(c, np.arange(1, SC.Q + 1) / 256.0)        # exact in float64
    for s in SC.EDGE_SHAPES.values():
        for seed in SC.EDGE_SEEDS:
            hits = SC.edge_hits(seed, s.T, s.B)
            assert hits, seed
            u = SC.u01_table(seed, s.T, s.B)
            want = SC.oracle_picks(b4, 1.0, u)
            assert np.array_equal(want, np.floor(u * 256).astype(np.int32).clip(max=255))
            assert np.array_equal(SC.emulate_picks_f32(b4, 1.0, u), want)   # float32 is exact here as well
            for b, j, m in hits:
                assert u[b, j] == c[m - 1] and want[b, j] == m == S.draw_pick(torch.from_numpy(b4), 1.0, u[b, j])
                assert int(np.searchsorted(c, u[b, j], side="left")) == m - 1     # what `u01 <= c_q` would pick
    assert {b for seed in SC.EDGE_SEEDS for b, _, _ in SC.edge_hits(seed, 3, 8)} == {4, 6}


# ---- draws along a real trajectory --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.TRAJ_SHAPES))
def test_trajectory_seeds_keep_half_the_row_allowance(name):
    """The oracle with float32 parameters (float32 arithmetic throughout) against itself in float64: rows that leave
    stay within half of what the GPU test allows -- max(1, B // 4) / 2 < 1 for both shapes, so none may leave."""
    s = SC.TRAJ_SHAPES[name]
    p, feats, ref, logits = SC.traj_reference(name)
    _, _, ref32, logits32 = SC.traj_reference(name, torch.float32)
    assert ref.shape == (s.B, 80 * s.T) and logits.shape == (s.B, 80 * (s.T - 1), SC.Q)
    exact, left = SC.draws_follow_oracle(ref32, ref, logits, SC.TRAJ_TEMPERATURE, SC.TRAJ_SEED, s.B)
    print(f"SAMPLING-CPU trajectory {name}: float32 oracle rows identical {len(exact)} of {s.B}, left {left}")
    assert 2 * (s.B - len(exact)) <= SC.traj_slack_rows(s.B)
    assert float((logits32[exact, -1] - logits[exact, -1]).abs().max()) <= 1e-4 * float(logits[exact, -1].abs().max())
    assert len(np.unique(ref[:, 80:])) > 20     # it really samples
    # the rule bites: the trajectory of another seed leaves at once and is refused
    with torch.no_grad():
        other = S.generate(p, S.config(DIM=s.DIM, EMB_SIZE=s.EMB), feats, temperature=SC.TRAJ_TEMPERATURE,
                           seed=SC.TRAJ_SEED + 1).numpy()
    with pytest.raises(AssertionError):
        SC.draws_follow_oracle(other, ref, logits, SC.TRAJ_TEMPERATURE, SC.TRAJ_SEED, s.B)


# ---- ties ---------------------------------------------------------------------------------------------------------------
def test_tie_patterns():
    for name, (codes, want) in SC.TIE_MAXIMA.items():
        b, w = SC.tie_pattern(name)
        assert w == want == min(codes) and b.dtype == np.float32
        assert np.array_equal(np.nonzero(b == b.max())[0], np.array(sorted(codes)))
        assert int(np.argmax(b)) == want and int(torch.argmax(torch.softmax(torch.from_numpy(b).double(), -1))) == want
        if len(codes) < SC.Q:
            assert np.delete(b, list(codes)).max() < 0
    lane, ps = (lambda q: q % 64), (lambda q: q // 64)
    a = SC.TIE_MAXIMA["one-lane-and-another"][0]
    assert lane(a[0]) == lane(a[1]) == lane(a[2]) != lane(a[3])
    lo, hi = SC.TIE_MAXIMA["later-pass-of-lower-lane"][0]
    assert lane(lo) < lane(hi) and ps(lo) > 0 and lane(hi) == 63
    lo, hi = SC.TIE_MAXIMA["last-lane-first-pass"][0]
    assert lane(lo) == 63 and ps(lo) == 0 and lane(hi) == 0 and ps(hi) > 0
    b = SC.one_hot_pattern()
    c = SC.cdf64(b, 1.0)
    assert c[SC.ONE_HOT_CODE - 1] < 2.0 ** -25 and int(np.argmax(b)) == SC.ONE_HOT_CODE
    for s in SC.TIE_SHAPES.values():  # no u01 of the run is exactly 1.0 (that draw would take the last code)
        u = SC.u01_table(SC.TRAJ_SEED, s.T, s.B)
        assert u.max() < 1.0
        assert (SC.oracle_picks(b, 1.0, u) == SC.ONE_HOT_CODE).all()
        assert (SC.emulate_picks_f32(b, 1.0, u) == SC.ONE_HOT_CODE).all()


# ---- replay arithmetic --------------------------------------------------------------------------------------------------
def test_replay_shapes():
    for name, s in SC.REPLAY_SHAPES.items():
        periods = s.T - 1
        assert (periods // SC.SR_CHUNK, periods % SC.SR_CHUNK) == (s.chunks, s.singles), name
        assert s.chunks >= 1 and s.B <= SC.PERSIST_MAX_B and 80 * periods <= 880
    assert any(s.singles == 0 for s in SC.REPLAY_SHAPES.values())
    assert any(s.singles > 1 for s in SC.REPLAY_SHAPES.values())
    assert any(s.persistent and s.singles for s in SC.REPLAY_SHAPES.values())
    assert SC.LIMIT_SHAPE.B == SC.PERSIST_MAX_B + 1 and SC.LIMIT_SHAPE.DIM == 256


def test_greedy_reference_is_causal():
    """What lets the T = 9 case share the T = 11 oracle run."""
    p, feats, ref, logits = SC.greedy_reference(32, 8, 2, 11)
    with torch.no_grad():
        short = S.generate(p, S.config(DIM=32, EMB_SIZE=8), feats[:3]).numpy()
    assert np.array_equal(short, ref[:, :240])
