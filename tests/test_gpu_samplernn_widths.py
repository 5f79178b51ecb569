"""Every width and both bodies of the SampleRNN persistent sample kernel against float64: the twelve instantiations
`srp_kernel<D, MG>` / `srp_fx_kernel<D, MG>` of sr_persist.hip (D = 256, 512, 1024; MG = the row-group loop), of which
the suites pinned to DIM 256 reach four.  At D = 512 and D = 1024 (the shipped width), at B = 5, 32, 33 and 37:

  a. full forcing (fx body): the log-probability of EVERY sample step against the float64 teacher-forced pass at
     FC.PARITY_TOL, on the persistent kernel (graph replay; eager at B = 37) and on the per-step launch path;
  b. the error gate: on identical inputs the persistent kernel's norm-wise error is at most GATE x max(the launch path's,
     the float32 oracle's).  A kernel that drops one of 1024 terms can stay under 1e-4; it does not stay within a small
     factor of what float32 leaves.  GATE = 4 covers what is legitimately different -- the same D products summed in
     another order (S strided partial sums and a tree, against the launch path's MFMA accumulation);
  c. greedy trajectories (plain body) against the float64 oracle with last-step logits, a second utterance on the same plan
     against a fresh plan bit for bit, graph replay against eager launches at B = 37;
  d. the two bodies agree: a seeded trajectory at temperature 1 is bit-identical between the default plan (plain) and plans
     with forcing (every code -1), log_probs and draw_stats (fx) -- one wrong logit bit changes such a run;
  e. draws on exact logits (the bias-only construction) inside srp_kernel<512, false> and srp_kernel<1024, true>, and the
     draw statistics of one truncated setting inside the fx bodies of the same shapes;
  f. the frame sizes 2 and 16 at D = 256 (fx body, B = 5 and 33): FS = 16 is the loop gather (FS - 1 > SRP_GMAX, no carry,
     the rolled next-frame tail), FS = 2 gathers a single early row (the clamp min(pos, FS - 2) = 0).

Every plan asserts that the persistent kernel engaged in the expected number of groups with the expected facilities, so the
instantiation a case names is the one that ran (DeviceGenerator._launch raises when a team gave up).
Cases and references: tests/samplernn_width_cases.py (premises: tests/test_samplernn_width_cases_cpu.py).

Measured on the MI355X (norm-wise error of the log-probabilities against float64; profiles/samplernn_widths.md):

    DIM  FS   B  groups   persistent   launch path   float32 oracle   gate (of 4)
    512  10   5    1      2.325e-07    1.555e-07     3.266e-07        0.71
    512  10  32    1      2.179e-07    1.852e-07     4.094e-07        0.53
    512  10  33    2      2.179e-07    1.852e-07     4.094e-07        0.53
    512  10  37    2      2.179e-07    1.852e-07     4.094e-07        0.53
   1024  10   5    1      3.148e-07    2.380e-07     3.735e-07        0.84
   1024  10  32    1      3.254e-07    2.324e-07     3.391e-07        0.96
   1024  10  33    2      3.254e-07    2.324e-07     3.531e-07        0.92
   1024  10  37    2      3.254e-07    2.324e-07     3.531e-07        0.92
    256   2   5    1      1.585e-07    1.402e-07     2.015e-07        0.79
    256   2  33    2      1.847e-07    1.870e-07     2.409e-07        0.77
    256  16   5    1      2.012e-07    1.431e-07     2.420e-07        0.83
    256  16  33    2      1.813e-07    1.742e-07     2.263e-07        0.80

Greedy: every stream of every case followed the float64 oracle (the allowance was not used).  Draws on exact logits: 0 excused
mismatches in 800 (D = 512, B = 5) and 5920 (D = 1024, B = 37) draws per pattern and seed; draw_logp within 4.25e-07.
"""
import numpy as np
import pytest

from oracle import samplernn_ref as S
from tests import samplernn_draw_stats_cases as DS
from tests import samplernn_groups_cases as GC
from tests import samplernn_sampling_cases as SC
from tests import samplernn_width_cases as WC
from tests.test_gpu_samplernn_draw_stats import _check_step_stats
from tests.test_gpu_samplernn_forced import _env, _full_forcing_parity, _self_replay
from tests.test_gpu_samplernn_groups import _follows_oracle, _generate, _model, _plan
from tests.test_gpu_samplernn_sampling import _check_bias_only_run

pytestmark = pytest.mark.gpu

GATE = 4.0
T, BFS = WC.REF_T, WC.BFS


def _cfg(DIM, FS=10):
    return dict(DIM=DIM, EMB_SIZE=WC.WIDTHS[DIM], FRAME_SIZE=FS)


def _lands_on(tt, gen, body, DIM, groups, FS=10):
    """The plan runs srp_kernel / srp_fx_kernel <DIM, groups > 1>: srp_launch_width takes the fx body exactly when forced
    codes, log-probabilities or draw statistics are asked for."""
    assert (tt.DIM, tt.FRAME_SIZE, tt.EMB_SIZE) == (DIM, FS, WC.WIDTHS[DIM])
    assert gen.persistent and gen.persist_groups == groups and 'persist_ws' in gen.ws
    assert (gen.forcing or gen.log_probs or gen.draw_stats) == (body == "fx")


def _samples(out):
    return (out[0] if isinstance(out, tuple) else out).cpu().numpy().copy()


def _parity_and_gate(dev, case, monkeypatch):
    """(a) and (b) for one fx case: two calls per plan on the persistent kernel and on the launch path; eager as well at
    B = 37.  Returns (persistent, launch path, float32 oracle) errors."""
    ref = WC.forced_case(case)
    cid = WC.case_id(case)
    with _model(dev, ref[0], **_cfg(case.DIM, case.FS)) as tt:
        _env(monkeypatch, groups=case.groups)
        with _plan(tt, case.B, T, case.groups, forcing=True, log_probs=True) as gen:
            _lands_on(tt, gen, "fx", case.DIM, case.groups, case.FS)
        ep = max(_full_forcing_parity(tt, "gru", case.B, case.groups, f"{cid} persistent", ref=ref))
        if case.B == WC.REF_B:
            _full_forcing_parity(tt, "gru", case.B, case.groups, f"{cid} persistent eager", ref=ref, use_graph=False)
        _env(monkeypatch, groups=case.groups, launches=True)
        el = max(_full_forcing_parity(tt, "gru", case.B, 0, f"{cid} launches", ref=ref))
    e32 = WC.f32_oracle_error(case)
    print(f"WIDTHS-GPU {cid}: error against float64: persistent {ep:.3e}, launch path {el:.3e}, float32 oracle {e32:.3e}; "
          f"gate {ep / max(el, e32):.2f} of {GATE:.0f}")
    assert ep <= GATE * max(el, e32), (f"{cid}: the persistent kernel's error {ep:.3e} is more than {GATE:.0f} x "
                                       f"max(launch path {el:.3e}, float32 oracle {e32:.3e})")
    return ep, el, e32


# ---- a, b. full forcing at every step, and the error gate -----------------------------------------------------------------
@pytest.mark.parametrize("case", WC.cases(body="fx", FS=(10,)), ids=WC.case_id)
def test_full_forcing_follows_the_oracle_and_the_launch_path(dev, case, monkeypatch):
    _parity_and_gate(dev, case, monkeypatch)


# ---- c. greedy trajectories -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WC.cases(body="plain"), ids=WC.case_id)
def test_greedy_follows_the_oracle_and_replays(dev, case, monkeypatch):
    p, feats, ref, ref_logits = WC.greedy_case(case)
    feats2 = SC.features(T, case.B, WC.FEAT_SEED_2).numpy()
    cid = WC.case_id(case)
    _env(monkeypatch, groups=case.groups)
    with _model(dev, p, **_cfg(case.DIM)) as tt:
        outs = {}
        for use_graph in ((True, False) if case.B == WC.REF_B else (True,)):
            with _plan(tt, case.B, T, case.groups, temperature=0.0, use_graph=use_graph) as gen:
                _lands_on(tt, gen, "plain", case.DIM, case.groups)
                for call in range(2):   # the second call meets the carry and the last-step logits the first one left
                    first, last = _generate(gen, feats)
                    _follows_oracle(first, last, ref, ref_logits, case.B, f"{cid} graph={int(use_graph)} call {call}")
                second, _ = _generate(gen, feats2)   # another utterance on the plan: every group's and team's carry is stale
                third, _ = _generate(gen, feats)
                outs[use_graph] = (first, second, third)
            assert np.array_equal(third, first), f"{(third != first).sum()} samples differ on the plan's fourth call"
        assert not np.array_equal(outs[True][0], outs[True][1])
        if False in outs:
            for a, b in zip(outs[True], outs[False]):
                assert np.array_equal(a, b), f"{(a != b).sum()} samples differ between graph replay and eager launches"
        with _plan(tt, case.B, T, case.groups, temperature=0.0) as gen:
            fresh, _ = _generate(gen, feats2)
        assert np.array_equal(fresh, outs[True][1]), f"{(fresh != outs[True][1]).sum()} samples differ from a fresh plan's"


# ---- d. the two bodies agree ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("DIM,B,groups", WC.shapes(), ids=lambda v: str(v))
def test_the_two_bodies_draw_the_same_trajectory(dev, DIM, B, groups, monkeypatch):
    """test_off_is_off of tests/test_gpu_samplernn_forced.py at the new widths: srp_kernel<D, MG> against
    srp_fx_kernel<D, MG> at every step of a drawn trajectory."""
    p, feats, _, _ = WC.greedy_case(WC.Case(DIM, 10, B, groups, "plain"))
    feats = np.asarray(feats, dtype=np.float32)
    free = np.full((B, BFS * T), -1, dtype=np.int32)
    kw = dict(temperature=1.0, seed=WC.DRAW_SEED)
    _env(monkeypatch, groups=groups)
    with _model(dev, p, **_cfg(DIM)) as tt:
        with _plan(tt, B, T, groups, **kw) as gen:
            _lands_on(tt, gen, "plain", DIM, groups)
            default = _samples(gen.generate(feats))
        with _plan(tt, B, T, groups, forcing=True, log_probs=True, **kw) as gen:
            _lands_on(tt, gen, "fx", DIM, groups)
            samples, logp = (o.cpu().numpy().copy() for o in gen.generate(feats, forced=free))
        with _plan(tt, B, T, groups, forcing=True, log_probs=True, draw_stats=True, **kw) as gen:
            _lands_on(tt, gen, "fx", DIM, groups)
            with_stats, logp2, dlogp, kept = (o.cpu().numpy().copy() for o in gen.generate(feats, forced=free))
    assert default.min() >= 0 and default.max() <= 255 and (default[:, :BFS] == 128).all()
    assert len(np.unique(default[:, BFS:])) > 20 and len({default[b].tobytes() for b in range(B)}) == B
    assert np.array_equal(samples, default), f"{(samples != default).sum()} samples differ with forcing (every code -1) and log_probs"
    assert np.array_equal(with_stats, default), f"{(with_stats != default).sum()} samples differ with draw_stats added"
    assert np.array_equal(logp2, logp) and (logp[:, BFS:] < 0).all() and np.isfinite(logp).all()
    # untruncated draws at temperature 1: every code is kept and the draw's distribution is the model's (two float32 sums of
    # the same 256 terms in different orders: each within DS.TOL of the exact value by that bound's own derivation)
    assert (kept[:, BFS:] == SC.Q).all()
    assert float(np.abs(dlogp[:, BFS:].astype(np.float64) - logp[:, BFS:]).max()) <= 2 * DS.TOL


# ---- e. draws on exact logits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", WC.DRAW_PATTERNS)
@pytest.mark.parametrize("shape", WC.DRAW_SHAPES, ids=lambda s: f"D{s.DIM}-B{s.B}-g{s.groups}")
def test_draws_on_exact_logits(dev, shape, pattern, monkeypatch):
    """Bias-only logits: every pick against draw_pick(b4, 1.0, draw_u01(seed, t, b)) under SC.judge_draws, the array identical
    to the launch path's; then kept and draw_logp of the truncated setting on the fx body, both draw modes."""
    DIM, B, groups = shape
    b4 = SC.b4_pattern(pattern)
    p = SC.bias_only_params(S.config(DIM=DIM, EMB_SIZE=WC.WIDTHS[DIM]), b4)
    feats = SC.features(T, B).numpy()
    tau = WC.DRAW_TEMPERATURE
    k, top_p, min_p = WC.DRAW_TRUNCATION
    what = f"D{DIM}-B{B}-g{groups} {pattern}"
    with _model(dev, p, **_cfg(DIM)) as tt:
        outs = {}
        _env(monkeypatch, groups=groups)
        for seed in SC.SEEDS:
            with _plan(tt, B, T, groups, temperature=tau, seed=seed) as gen:
                _lands_on(tt, gen, "plain", DIM, groups)
                out, logits = _generate(gen, feats)
            _check_bias_only_run(out, logits, b4, B)
            draws, excused, worst = SC.judge_draws(out[:, BFS:], b4, tau, SC.u01_table(seed, T, B))
            print(f"WIDTHS-GPU draws {what} seed={seed}: draws {draws}, excused mismatches {excused} (worst {worst:.2e})")
            assert draws == BFS * (T - 1) * B
            outs[seed] = out
        assert not np.array_equal(outs[SC.SEEDS[0]], outs[SC.SEEDS[1]])
        for mode in DS.MODES:
            with _plan(tt, B, T, groups, temperature=tau, seed=SC.SEEDS[1], draw_mode=mode, top_k=k, top_p=top_p, min_p=min_p,
                       draw_stats=True) as gen:
                _lands_on(tt, gen, "fx", DIM, groups)
                samples, dlogp, kept = (o.cpu().numpy().copy() for o in gen.generate(np.asarray(feats, dtype=np.float32)))
            assert (dlogp[:, :BFS] == 0).all() and (kept[:, :BFS] == 0).all()
            m, err = _check_step_stats(samples, dlogp, kept, b4, tau, f"{what} {mode}", k=k, p=top_p, min_p=min_p)
            print(f"WIDTHS-GPU draw stats {what} {mode}: kept {m} at all {samples[:, BFS:].size} steps, draw_logp within {err:.2e}")
        _env(monkeypatch, groups=groups, launches=True)   # the same expression in the same order on identical logits
        for seed in SC.SEEDS:
            with _plan(tt, B, T, 0, temperature=tau, seed=seed) as gen:
                launch, logits = _generate(gen, feats)
            _check_bias_only_run(launch, logits, b4, B)
            assert np.array_equal(launch, outs[seed]), \
                f"{what} seed={seed}: {(launch != outs[seed]).sum()} picks differ between the persistent kernel and sr_pick_kernel"


# ---- f. frame sizes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WC.cases(widths=(256,)), ids=WC.case_id)
def test_frame_sizes(dev, case, monkeypatch):
    """FS = 2 and FS = 16 at D = 256: (a) and (b) as above; forcing a run's own output replays it (prefix lengths 1, 7, 10, 85,
    160 cross frame edges that lie elsewhere than at FS = 10); greedy samples equal the launch path's."""
    assert case.FS != 10 and case.body == "fx"
    _parity_and_gate(dev, case, monkeypatch)
    p, feats, _, _ = WC.forced_case(case)
    cid = WC.case_id(case)
    with _model(dev, p, **_cfg(case.DIM, case.FS)) as tt:
        _env(monkeypatch, groups=case.groups)
        free = _self_replay(tt, case.B, case.groups, "sequential", cid)
        assert len(np.unique(free[case.B - 1, BFS:])) > 10
        with _plan(tt, case.B, T, case.groups, temperature=0.0) as gen:
            _lands_on(tt, gen, "plain", case.DIM, case.groups, case.FS)
            persistent, _ = _generate(gen, feats)
            again, _ = _generate(gen, feats)
        assert np.array_equal(again, persistent)
        _env(monkeypatch, groups=case.groups, launches=True)
        with _plan(tt, case.B, T, 0, temperature=0.0) as gen:
            launches, _ = _generate(gen, feats)
    same = [b for b in range(case.B) if np.array_equal(persistent[b], launches[b])]
    print(f"WIDTHS-GPU {cid}: greedy rows identical to the launch path's {len(same)} of {case.B}")
    assert (persistent[:, :BFS] == 128).all() and persistent.min() >= 0 and persistent.max() <= 255
    assert len(same) >= case.B - GC.slack_rows(case.B), f"only {len(same)} of {case.B} rows equal the launch path's"

