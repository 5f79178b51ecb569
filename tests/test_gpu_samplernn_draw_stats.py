"""What each draw kept (samplernn_generate_set_draw_stats; DeviceGenerator(draw_stats=True), generate_packed(...,
draw_stats=True)): srp_fx_kernel in sr_persist.hip and sr_pick_kernel on the launch path.  With bias-only logits the kept
count of EVERY step against the float64 oracle's m -- the min-p cases, top-k, top-p, all three, none, argmax rows -- and
draw_logp against float64 within SC.DELTA; on a real trajectory, forced onto given codes, draw_logp against the teacher-forced
oracle at the draw's temperature; -inf for a forced code outside the kept set; the same bits from a fresh plan, from segments
and from a packed run; the samples of such a plan are the default plan's; the setter's refusals.
Cases and references: tests/samplernn_draw_stats_cases.py (premises: tests/test_samplernn_draw_stats_cpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import samplernn_ref as S
from tests import samplernn_draw_stats_cases as DS
from tests import samplernn_forced_cases as FC
from tests import samplernn_groups_cases as GC
from tests import samplernn_min_p_cases as MC
from tests import samplernn_packed_cases as PC
from tests import samplernn_sampling_cases as SC
from tests import samplernn_utt_draw_cases as UC
from tests.test_gpu_samplernn_groups import _model as _model256
from tests.test_gpu_samplernn_groups import _plan
from tests.test_gpu_samplernn_sampling import _model
from tests.test_gpu_samplernn_top_k import _bias_model, _d256_model, _feats, _same
from tests.test_gpu_samplernn_utt_draws import _env, _utterances
from tests.util import assert_close

pytestmark = pytest.mark.gpu

SEED = SC.SEEDS[1]


def _host(out):
    return tuple(o.cpu().numpy().copy() for o in out)


def _stats_run(tt, s, feats, **kw):
    """(samples, draw_logp, kept) of one plan with draw_stats on the path the shape names."""
    with _plan(tt, s.B, s.T, 1 if s.persistent else 0, draw_stats=True, **kw) as gen:
        samples, dlogp, kept = _host(gen.generate(np.asarray(feats, dtype=np.float32)))
    assert samples.dtype == np.int32 and dlogp.dtype == np.float32 and kept.dtype == np.int32
    assert dlogp.shape == kept.shape == samples.shape
    assert (dlogp[:, :80] == 0).all() and (kept[:, :80] == 0).all()      # the prefix slot holds zeros
    return samples, dlogp, kept


def _check_step_stats(samples, dlogp, kept, b4, temperature, what, **trunc):
    m = DS.oracle_m(b4, temperature, **trunc)
    assert (kept[:, 80:] == m).all(), f"{what}: kept {np.unique(kept[:, 80:]).tolist()}, the oracle's m is {m}"
    want = DS.draw_logp64(b4, temperature, samples[:, 80:], **trunc)
    assert np.isfinite(want).all(), f"{what}: a sample outside the oracle's kept set"
    err = float(np.abs(dlogp[:, 80:].astype(np.float64) - want).max())
    assert err <= DS.TOL, f"{what}: draw_logp off by {err:.3e} (allowed {DS.TOL:.3e})"
    return m, err


# ---- 1. bias-only logits: the kept set itself at every step -------------------------------------------------------------
@pytest.mark.parametrize("mode", DS.MODES)
@pytest.mark.parametrize("pattern", SC.PATTERNS)
@pytest.mark.parametrize("shape", DS.SHAPES)
def test_kept_counts_and_draw_logp_from_known_logits(dev, shape, pattern, mode):
    s = SC.BIAS_SHAPES[shape]
    b4 = SC.b4_pattern(pattern)
    feats = SC.features(s.T, s.B).numpy()
    with _bias_model(dev, s, b4) as tt:
        for temperature in SC.TEMPERATURES:
            kw = dict(temperature=temperature, seed=SEED, draw_mode=mode)
            settings = [dict(min_p=m) for m in MC.MIN_PS] + [dict(k=k, p=p, min_p=m) for k, p, m in DS.OTHER_TRUNCATIONS]
            for t in settings:
                plan_kw = dict(top_k=t.get("k", 0), top_p=t.get("p", 0.0), min_p=t.get("min_p", 0.0))
                what = f"{shape} {pattern} T={temperature} {mode} {plan_kw}"
                out = _stats_run(tt, s, feats, **plan_kw, **kw)
                m, err = _check_step_stats(*out, b4, temperature, what, **t)
                print(f"DRAWSTATS-GPU {what}: kept {m} at all {out[0][:, 80:].size} steps, draw_logp within {err:.2e}")
                if not any(plan_kw.values()):
                    assert m == SC.Q
        # argmax rows: one code, probability one
        samples, dlogp, kept = _stats_run(tt, s, feats, temperature=0.0, draw_mode=mode, min_p=0.1, top_k=8)
        assert (kept[:, 80:] == 1).all() and (dlogp[:, 80:] == 0).all() and (samples[:, 80:] == int(np.argmax(b4))).all()


def test_rows_of_one_team_mix_argmax_and_truncations(dev, monkeypatch):
    """Per-utterance entries on one plan: an argmax row, an untruncated row, top-k, top-p and min-p rows side by side."""
    s = SC.BIAS_SHAPES["persist-D256-B5"]
    b4 = SC.b4_pattern("randn")
    feats = SC.features(s.T, s.B).numpy().astype(np.float32)
    temps, ks, ps, mps = [0.0, 1.0, 1.0, 1.0, 2.0], [0, 0, 64, 0, 0], [0.0, 0.0, 0.0, 0.9, 0.0], [0.5, 0.0, 0.0, 0.0, 0.1]
    _env(monkeypatch, 1)
    with _bias_model(dev, s, b4) as tt:
        with _plan(tt, s.B, s.T, 1, utterance_draws=True, draw_stats=True) as gen:
            samples, dlogp, kept = _host(gen.generate(feats, seeds=UC.utt_seeds(s.B), temperatures=temps, top_ks=ks, top_ps=ps,
                                                      min_ps=mps))
    for b in range(s.B):
        m, _ = _check_step_stats(samples[b:b + 1], dlogp[b:b + 1], kept[b:b + 1], b4, temps[b], f"row {b}",
                                 k=ks[b], p=ps[b], min_p=mps[b])
    assert kept[:, -1].tolist() == [1, 256, 64, 65, 95]


@pytest.mark.parametrize("mode", DS.MODES)
def test_two_row_groups(dev, mode, monkeypatch):
    B, T, min_p = 64, 3, 0.1
    b4 = SC.b4_pattern("randn")
    feats = SC.features(T, B).numpy().astype(np.float32)
    _env(monkeypatch, 2)
    with _model(dev, GC.DIM, GC.EMB, SC.bias_only_params(S.config(DIM=GC.DIM, EMB_SIZE=GC.EMB), b4)) as tt:
        with _plan(tt, B, T, 2, temperature=1.0, seed=SEED, draw_mode=mode, min_p=min_p, draw_stats=True) as gen:
            samples, dlogp, kept = _host(gen.generate(feats))
    m, err = _check_step_stats(samples, dlogp, kept, b4, 1.0, f"B = 64, two groups, {mode}", min_p=min_p)
    assert m == 21


# ---- 2. a real trajectory, forced ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", DS.MODES)
@pytest.mark.parametrize("path", ["persistent", "launches"])
@pytest.mark.parametrize("temperature", DS.FORCED_TEMPERATURES)
def test_forced_trajectory_follows_the_oracle(dev, temperature, path, mode, monkeypatch):
    """Every step forced onto FC.reference's codes, untruncated: draw_logp against the oracle's log softmax(logits / T)[s].  A
    logit error e moves a log-softmax at temperature T by at most 2 e / T, and FC.PARITY_TOL is the project's bar on these
    logits: the bar is 2 PARITY_TOL / T, compared as tests/test_gpu_samplernn_forced.py compares logp."""
    B = 5
    p, feats, forced, want = DS.forced_case(temperature, B)
    _env(monkeypatch, 1, launches=path == "launches")
    with _model256(dev, p) as tt:
        with _plan(tt, B, FC.REF_T, 1 if path == "persistent" else 0, temperature=temperature, seed=SEED, draw_mode=mode,
                   forcing=True, draw_stats=True) as gen:
            samples, dlogp, kept = _host(gen.generate(feats, forced=forced))
    assert np.array_equal(samples[:, 80:], forced[:, 80:]) and (kept[:, 80:] == SC.Q).all() and (dlogp[:, :80] == 0).all()
    e = assert_close(torch.from_numpy(dlogp[:, 80:]).double(), torch.from_numpy(want), 2 * FC.PARITY_TOL / temperature,
                     f"draw_logp at T = {temperature}, {path}, {mode}")
    print(f"DRAWSTATS-GPU forced T={temperature} {path} {mode}: relative error {e:.3e}, largest difference "
          f"{np.abs(dlogp[:, 80:] - want).max():.3e}")


@pytest.mark.parametrize("path", ["persistent", "launches"])
def test_at_temperature_one_untruncated_it_is_the_models_log_prob(dev, path, monkeypatch):
    B = 5
    p, feats, forced, _ = FC.case("gru", B)
    _env(monkeypatch, 1, launches=path == "launches")
    with _model256(dev, p) as tt:
        with _plan(tt, B, FC.REF_T, 1 if path == "persistent" else 0, temperature=1.0, seed=SEED, forcing=True, log_probs=True,
                   draw_stats=True) as gen:
            samples, logp, dlogp, kept = _host(gen.generate(feats, forced=forced))     # (samples, logp, draw_logp, kept)
    assert logp.dtype == dlogp.dtype == np.float32 and kept.dtype == np.int32 and (kept[:, 80:] == SC.Q).all()
    err = float(np.abs(dlogp.astype(np.float64) - logp.astype(np.float64)).max())
    print(f"DRAWSTATS-GPU {path}: draw_logp against logp at temperature 1: {err:.3e}")
    assert err <= SC.DELTA and (logp[:, 80:] < 0).all()


# ---- 3. a forced sample outside the kept set ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", DS.MODES)
@pytest.mark.parametrize("shape", DS.SHAPES)
def test_forced_code_outside_the_kept_set(dev, shape, mode):
    """`peaked` under top_k = 3: the kept set is codes 0, 130, 255.  Row 0 is forced onto code 1 (dropped): -inf at every
    step; row 1 onto code 0 (kept): finite, the float64 value; the other rows draw freely.  kept is 3 on all of them: a forced
    step reports the set its pick was drawn from."""
    s = SC.BIAS_SHAPES[shape]
    b4 = SC.b4_pattern("peaked")
    feats = SC.features(s.T, s.B).numpy()
    forced = np.full((s.B, 80 * s.T), -1, dtype=np.int32)
    forced[0, 80:], forced[1, 80:] = DS.OUTSIDE_CODE, DS.INSIDE_CODE
    with _bias_model(dev, s, b4) as tt:
        for temperature in (1.0, 2.0):
            with _plan(tt, s.B, s.T, 1 if s.persistent else 0, temperature=temperature, seed=SEED, draw_mode=mode,
                       top_k=DS.OUTSIDE_K, forcing=True, draw_stats=True) as gen:
                samples, dlogp, kept = _host(gen.generate(feats.astype(np.float32), forced=forced))
            assert (samples[0, 80:] == DS.OUTSIDE_CODE).all() and (samples[1, 80:] == DS.INSIDE_CODE).all()
            assert (kept[:, 80:] == DS.OUTSIDE_K).all()
            assert np.isneginf(dlogp[0, 80:]).all(), f"T = {temperature}: {dlogp[0, 80:84]}"
            want = DS.draw_logp64(b4, temperature, samples[1:, 80:], k=DS.OUTSIDE_K)
            assert np.isfinite(want).all() and np.abs(dlogp[1:, 80:] - want).max() <= DS.TOL
        # an argmax row: the argmax (code 0) has probability one, any other forced code none
        with _plan(tt, s.B, s.T, 1 if s.persistent else 0, temperature=0.0, draw_mode=mode, forcing=True, draw_stats=True) as gen:
            samples, dlogp, kept = _host(gen.generate(feats.astype(np.float32), forced=forced))
        assert (kept[:, 80:] == 1).all() and np.isneginf(dlogp[0, 80:]).all() and (dlogp[1:, 80:] == 0).all()
        assert (samples[2:, 80:] == DS.INSIDE_CODE).all()


# ---- 4. the same bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", DS.MODES)
def test_replay_fresh_plan_and_segments_give_the_same_bits(dev, mode):
    s = SC.BIAS_SHAPES["persist-D256-B5"]
    N = 4
    feats = _feats(N, s.B)
    kw = dict(temperature=1.0, seed=SEED, draw_mode=mode, top_k=64, min_p=0.05, draw_stats=True)
    with _d256_model(dev) as tt:
        with _plan(tt, s.B, N, 1, **kw) as gen:
            first = _host(gen.generate(feats))
            again = _host(gen.generate(feats))
        with _plan(tt, s.B, N, 1, **kw) as gen:
            fresh = _host(gen.generate(feats))
            parts = [_host(gen.generate(feats[:3], n_frames=2)), _host(gen.generate(feats[3:], resume=True, n_frames=1))]
    for what, got in (("the same plan again", again), ("a fresh plan", fresh),
                      ("two segments", tuple(np.concatenate([a, b], axis=1) for a, b in zip(*parts)))):
        for name, a, b in zip(("samples", "draw_logp", "kept"), got, first):
            assert a.dtype == b.dtype and np.array_equal(a[:, 80:], b[:, 80:]), f"{what}: {name} differs"
    samples, dlogp, kept = first
    print(f"DRAWSTATS-GPU {mode}: kept sizes on a real trajectory {np.unique(kept[:, 80:]).tolist()}")
    assert 1 <= kept[:, 80:].min() and kept[:, 80:].max() <= 64
    assert np.isfinite(dlogp).all() and (dlogp[:, 80:] <= 0).all()


def test_packed_utterances_equal_standalone(dev, monkeypatch):
    case = PC.GRU_PACKING
    n = len(case.lengths)
    utts = _utterances(_feats(case.max_len, n), case.lengths)
    seeds, mps = UC.utt_seeds(n), MC.utt_min_ps(n)
    _env(monkeypatch, 1)
    with _d256_model(dev) as tt:
        samples, dlogps, kepts = tt.generate_packed(utts, n_streams=case.B, temperature=1.0, seeds=seeds, min_ps=mps, top_k=64,
                                                    draw_stats=True)
        stream, first_slot, _ = tt.pack_utterances(case.lengths, case.B)
        for i in (0, n // 2, n - 1):
            T = max(2, case.lengths[i])
            feats = np.zeros((T, case.B, 63), dtype=np.float32)
            feats[:case.lengths[i], stream[i]] = utts[i]
            sd, mp = [0] * case.B, np.zeros(case.B, dtype=np.float32)
            sd[stream[i]], mp[stream[i]] = seeds[i], mps[i]
            with _plan(tt, case.B, T, 1, utterance_draws=True, top_k=64, draw_stats=True) as gen:
                s1, d1, k1 = _host(gen.generate(feats, seeds=sd, temperatures=1.0, min_ps=mp))
            hi = 80 * case.lengths[i]
            assert samples[i].dtype == np.int32 and dlogps[i].dtype == np.float32 and kepts[i].dtype == np.int32
            assert np.array_equal(samples[i], s1[stream[i], :hi]), i
            assert np.array_equal(dlogps[i], d1[stream[i], 80:hi]) and np.array_equal(kepts[i], k1[stream[i], 80:hi]), i
            if hi > 80:
                assert kepts[i].max() <= 64 and kepts[i].min() >= 1


# ---- 5. the draw's own instructions do not change ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", DS.MODES)
@pytest.mark.parametrize("name", sorted(SC.TRAJ_SHAPES))
def test_samples_equal_the_default_plans(dev, name, mode):
    s = SC.TRAJ_SHAPES[name]
    p = S.init_params(S.config(DIM=s.DIM, EMB_SIZE=s.EMB), seed=s.param_seed, perturb=0.25)
    feats = SC.features(s.T, s.B, s.feat_seed).numpy().astype(np.float32)
    with _model(dev, s.DIM, s.EMB, p) as tt:
        for temperature in (0.0, 1.0):
            for trunc in (dict(), dict(top_k=8, min_p=0.1)):
                kw = dict(temperature=temperature, seed=SC.TRAJ_SEED, draw_mode=mode, **trunc)
                with _plan(tt, s.B, s.T, 1 if s.persistent else 0, **kw) as gen:
                    default = gen.generate(feats).cpu().numpy().copy()
                with _plan(tt, s.B, s.T, 1 if s.persistent else 0, draw_stats=True, **kw) as gen:
                    samples, dlogp, kept = _host(gen.generate(feats))
                _same(samples, default, f"draw_stats=True at temperature {temperature}, {trunc}")
                want = 1 if temperature == 0.0 else None
                assert (kept[:, 80:] == want).all() if want else (kept[:, 80:] >= 1).all()
                assert np.isfinite(dlogp).all()            # (a free pick always lies in the set it was drawn from)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from parrot_amd import _lib
    BADARG = 10001
    s = SC.BIAS_SHAPES["launch-D32-B3"]
    p = S.init_params(S.config(DIM=s.DIM, EMB_SIZE=s.EMB), seed=SC.PARAM_SEED, perturb=0.25)
    lib = _lib.load()
    feats = SC.features(s.T, s.B).numpy().astype(np.float32)
    with _model(dev, s.DIM, s.EMB, p) as tt:
        gen = tt.DeviceGenerator(s.B, s.T, temperature=1.0, draw_stats=True)
        try:
            d, k = gen.ws['draw_logp'].data_ptr(), gen.ws['kept'].data_ptr()
            assert lib.samplernn_generate_set_draw_stats(gen.plan, None, k) == BADARG
            assert lib.samplernn_generate_set_draw_stats(gen.plan, d, None) == BADARG
            assert lib.samplernn_generate_set_draw_stats(None, d, k) == BADARG
            assert lib.samplernn_generate_set_draw_stats(gen.plan, d, k) == 0          # before the first run: allowed again
            out = gen.generate(feats)
            assert isinstance(out, tuple) and len(out) == 3
            assert lib.samplernn_generate_set_draw_stats(gen.plan, d, k) == BADARG     # the plan has run
        finally:
            gen.close()
        gen = tt.DeviceGenerator(s.B, s.T, temperature=1.0)
        try:
            assert not isinstance(gen.generate(feats), tuple)
        finally:
            gen.close()
