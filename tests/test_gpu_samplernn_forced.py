"""Forced samples and per-sample log-probabilities of the device-resident SampleRNN generator
(samplernn_generate_set_forced, samplernn_generate_set_log_probs; srp_kernel<D, MG, true> in sr_persist.hip, sr_pick_kernel on
the launch path).  Under full forcing every sample step of both paths is compared with the float64 oracle at a plain
tolerance; forcing a run's own output replays it bit for bit in every draw setting; a plan that forces nothing returns the
default plan's samples; segments and packed runs equal the run in one piece and the utterance carried alone; row groups.
Cases and the reference: tests/samplernn_forced_cases.py (pinned by tests/test_samplernn_forced_cpu.py)."""
import numpy as np
import pytest
import torch

from oracle import samplernn_ref as S
from tests import samplernn_forced_cases as FC
from tests.test_gpu_samplernn_groups import SWITCH, _model, _plan
from tests.util import assert_close

pytestmark = pytest.mark.gpu


def _env(monkeypatch, groups=1, launches=False):
    if groups > 1:
        monkeypatch.setenv(SWITCH, str(groups))
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    if launches:
        monkeypatch.setenv("PARROT_SR_PERSIST", "0")
    else:
        monkeypatch.delenv("PARROT_SR_PERSIST", raising=False)


def _run(gen, feats, **kw):
    """(samples, logp) as host arrays of their own, or samples alone for a plan without log_probs."""
    out = gen.generate(np.asarray(feats, dtype=np.float32), **kw)
    if isinstance(out, tuple):
        return out[0].cpu().numpy().copy(), out[1].cpu().numpy().copy()
    return out.cpu().numpy().copy()


def _full_forcing_parity(tt, kind, B, groups, what, ref=None, **kw):
    """ref: (params, features, codes, float64 log-probabilities) of another reference than FC.case(kind, B)'s, in its
    layout (tests/samplernn_width_cases.py).  Returns the relative error of each call."""
    p, feats, forced, want = FC.case(kind, B) if ref is None else ref
    assert forced.shape == (B, 80 * FC.REF_T) and want.shape == (B, 80 * (FC.REF_T - 1))
    errs = []
    with _plan(tt, B, FC.REF_T, groups, temperature=0.0, forcing=True, log_probs=True, **kw) as gen:
        assert gen.forcing and gen.log_probs
        for call in range(2):           # the second call meets the carry the first one left
            samples, logp = _run(gen, feats, forced=forced)
            assert samples.dtype == np.int32 and logp.dtype == np.float32 and logp.shape == samples.shape
            assert np.array_equal(samples[:, 80:], forced[:, 80:]) and (samples[:, :80] == 128).all()
            assert (logp[:, :80] == 0).all()                      # the prefix slot is not written
            e = assert_close(torch.from_numpy(logp[:, 80:]).double(), torch.from_numpy(want), FC.PARITY_TOL,
                             f"log-probabilities, {what}")
            print(f"FORCED-GPU {what} call {call}: relative error {e:.3e}, largest difference "
                  f"{np.abs(logp[:, 80:] - want).max():.3e}")
            errs.append(e)
    return errs


# ---- 1. oracle parity under full forcing ---------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["persistent", "launches"])
@pytest.mark.parametrize("kind,B", [("gru", 5), ("gru", 32), ("lstm", 5)])
def test_full_forcing_follows_the_oracle(dev, kind, B, path, monkeypatch):
    _env(monkeypatch, launches=path == "launches")
    p = FC.case(kind, B)[0]
    with _model(dev, p, **FC.model_config(kind)) as tt:
        _full_forcing_parity(tt, kind, B, 1 if path == "persistent" else 0, f"{kind} B={B} {path}")


@pytest.mark.parametrize("path", ["persistent", "launches"])
def test_full_forcing_eager(dev, path, monkeypatch):
    _env(monkeypatch, launches=path == "launches")
    with _model(dev, FC.case("gru", 5)[0]) as tt:
        _full_forcing_parity(tt, "gru", 5, 1 if path == "persistent" else 0, f"gru B=5 {path} eager", use_graph=False)


def test_score_utterances_is_the_training_cost(dev, monkeypatch):
    _env(monkeypatch)
    B = 5
    p, feats, forced, want = FC.case("gru", B)
    c = S.config(DIM=FC.DIM, EMB_SIZE=FC.EMB)
    cost = FC.cost_bits({k: v.double() for k, v in p.items()}, c, forced, torch.from_numpy(feats).double())
    with _model(dev, p) as tt:
        lps = tt.score_utterances([feats[:, b] for b in range(B)], [forced[b] for b in range(B)], n_streams=B)
        short = tt.score_utterances([feats[:2, 1]], [forced[1, 80:160]], n_streams=2)   # without the prefix slot, two frames
    assert len(lps) == B and all(lp.dtype == np.float32 and lp.shape == (80 * (FC.REF_T - 1),) for lp in lps)
    got = FC.mean_bits(np.stack(lps))
    print(f"FORCED-GPU score_utterances: {got:.6f} bits against compute_cost {cost:.6f}")
    assert_close(torch.tensor([got], dtype=torch.float64), torch.tensor([cost], dtype=torch.float64), FC.PARITY_TOL, "bits per sample")
    assert_close(torch.from_numpy(np.stack(lps)).double(), torch.from_numpy(want), FC.PARITY_TOL, "per-sample log-probabilities")
    assert_close(torch.from_numpy(short[0]).double(), torch.from_numpy(want[1, :80]), FC.PARITY_TOL, "a shorter utterance")


# ---- 2. self-replay, bit for bit -----------------------------------------------------------------------------------------
def _self_replay(tt, B, groups, name, what):
    T = FC.REPLAY_T
    feats = FC.case("gru", B)[1]
    kw = dict(FC.REPLAY_SETTINGS[name])
    more = {}
    if kw.get("utterance_draws"):
        more = dict(seeds=[FC.UTT_SEEDS[b % 5] + b // 5 for b in range(B)],
                    temperatures=np.array([FC.UTT_TEMPS[b % 5] for b in range(B)], dtype=np.float32))
    free_forced = np.full((B, 80 * T), -1, dtype=np.int32)
    with _plan(tt, B, T, groups, seed=77, forcing=True, log_probs=True, **kw) as gen:
        free, free_lp = _run(gen, feats, forced=free_forced, **more)
        assert (free_lp[:, 80:] < 0).all() and len(np.unique(free[:, 80:])) > 10
        first = _run(gen, feats, forced=FC.prefix_forced(free, FC.replay_ns(B)), **more)
    with _plan(tt, B, T, groups, seed=77, forcing=True, log_probs=True, **kw) as gen:    # a fresh plan, other lengths per row
        second = _run(gen, feats, forced=FC.prefix_forced(free, FC.replay_ns(B, shift=2)), **more)
    for tag, (samples, logp) in (("same plan", first), ("fresh plan", second)):
        assert np.array_equal(samples, free), f"{what}, {tag}: {(samples != free).sum()} samples differ from the free run"
        assert np.array_equal(logp, free_lp), f"{what}, {tag}: {(logp != free_lp).sum()} log-probabilities differ"
    return free


@pytest.mark.parametrize("name", sorted(FC.REPLAY_SETTINGS))
def test_forcing_a_runs_own_output_replays_it(dev, name, monkeypatch):
    """Rows 0 .. 3 are one team: their forced lengths are 1, 7, 10 and 85 (then 10, 85, 160 and 1 on the fresh plan)."""
    _env(monkeypatch)
    with _model(dev, FC.case("gru", 5)[0]) as tt:
        _self_replay(tt, 5, 1, name, name)


def test_forcing_a_runs_own_output_replays_it_on_launches(dev, monkeypatch):
    _env(monkeypatch, launches=True)
    with _model(dev, FC.case("gru", 5)[0]) as tt:
        _self_replay(tt, 5, 0, "scan-topk-topp", "launches")


# ---- 3. off is off -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["persistent", "launches"])
@pytest.mark.parametrize("temperature", [0.0, 1.0])
def test_off_is_off(dev, temperature, path, monkeypatch):
    _env(monkeypatch, launches=path == "launches")
    B, T = 5, 3
    groups = 1 if path == "persistent" else 0
    p, feats, _, _ = FC.case("gru", B)
    free = np.full((B, 80 * T), -1, dtype=np.int32)
    with _model(dev, p) as tt:
        with _plan(tt, B, T, groups, temperature=temperature, seed=78) as gen:
            default = _run(gen, feats)
        with _plan(tt, B, T, groups, temperature=temperature, seed=78, forcing=True) as gen:
            forcing = _run(gen, feats, forced=free)
        with _plan(tt, B, T, groups, temperature=temperature, seed=78, log_probs=True) as gen:
            scored, logp = _run(gen, feats)
    assert len(np.unique(default[:, 80:])) > 10
    assert np.array_equal(forcing, default), f"{(forcing != default).sum()} samples differ with every code -1"
    assert np.array_equal(scored, default), f"{(scored != default).sum()} samples differ with log_probs=True"
    assert (logp[:, 80:] < 0).all() and np.isfinite(logp).all()


# ---- 4. segments and packing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [1, 2])
def test_segments_equal_the_run_in_one_piece(dev, first, monkeypatch):
    """A T = 4 plan, three frames in segments of (1, 2) or (2, 1); every row's prompt ends inside the second segment."""
    _env(monkeypatch)
    B, T = 5, 4
    p = FC.case("gru", B)[0]
    feats = np.concatenate([FC.case("gru", B)[1], FC.case("gru", B)[1][1:2]])          # four rows of features
    ends = [80 * first + n for n in (5, 20, 37, 80, 1)]
    forced = np.full((B, 80 * T), -1, dtype=np.int32)
    codes = FC.codes(B, T, seed=FC.CODE_SEED + 1)
    for b, n in enumerate(ends):
        forced[b, 80:80 + n] = codes[b, 80:80 + n]
    kw = dict(temperature=1.0, seed=79, forcing=True, log_probs=True)
    with _model(dev, p) as tt:
        with _plan(tt, B, T, 1, **kw) as gen:
            whole, whole_lp = _run(gen, feats, forced=forced)
        with _plan(tt, B, T, 1, **kw) as gen:
            cut = 80 * (first + 1)
            s0, l0 = _run(gen, feats[:first + 1], n_frames=first, forced=forced[:, :cut])
            s1, l1 = _run(gen, feats[first + 1:], resume=True, n_frames=T - 1 - first, forced=forced[:, cut:])
    for b, n in enumerate(ends):
        assert np.array_equal(whole[b, 80:80 + n], codes[b, 80:80 + n])
    assert len(np.unique(whole[:, 80 * 3:])) > 10                                       # the free tail really draws
    samples, logp = np.concatenate([s0, s1], axis=1), np.concatenate([l0, l1], axis=1)
    assert np.array_equal(samples, whole), f"{(samples != whole).sum()} samples differ"
    assert np.array_equal(logp[:, 80:], whole_lp[:, 80:]), f"{(logp != whole_lp).sum()} log-probabilities differ"


def test_packed_prompts_equal_the_utterance_alone(dev, monkeypatch):
    """Four utterances of 3, 2, 3 and 2 frames on two streams, two per stream: without a prompt, fully forced, with a prompt
    that ends mid-frame and with a short one.  Each equals the plain plan that carries it alone in the same stream with
    the same prompt and seed."""
    _env(monkeypatch)
    B = 2
    lengths = [3, 2, 3, 2]
    p, feats, _, _ = FC.case("gru", 4)
    utts = [feats[:n, i] for i, n in enumerate(lengths)]
    codes = FC.codes(4, 3, seed=FC.CODE_SEED + 2)
    prompts = [None, codes[1, :80], codes[2, :93], codes[3, :8]]
    seeds = [2 ** 40 + 21, 22, 23, 24]
    with _model(dev, p) as tt:
        stream, first_slot, T = tt.pack_utterances(lengths, B)
        assert T == 5 and sorted(stream) == [0, 0, 1, 1]
        pieces, lps = tt.generate_packed(utts, n_streams=B, temperature=1.0, seeds=seeds, prompts=prompts, log_probs=True)
        for i, n in enumerate(lengths):
            f = np.zeros((n, B, 63), dtype=np.float32)
            f[:, stream[i]] = utts[i]
            forced = np.full((B, 80 * n), -1, dtype=np.int32)
            if prompts[i] is not None:
                forced[stream[i], 80:80 + len(prompts[i])] = prompts[i]
            sd = [0] * B
            sd[stream[i]] = seeds[i]
            with _plan(tt, B, n, 1, utterance_draws=True, forcing=True, log_probs=True) as gen:
                alone, alone_lp = _run(gen, f, forced=forced, seeds=sd, temperatures=1.0)
            assert np.array_equal(pieces[i], alone[stream[i]]), f"utterance {i}: {(pieces[i] != alone[stream[i]]).sum()} samples differ"
            assert np.array_equal(lps[i], alone_lp[stream[i], 80:]), f"utterance {i}: log-probabilities differ"
            if prompts[i] is not None:
                assert np.array_equal(pieces[i][80:80 + len(prompts[i])], prompts[i])
        assert len(np.unique(pieces[0][80:])) > 10


# ---- 5. row groups -------------------------------------------------------------------------------------------------------
def test_row_groups(dev, monkeypatch):
    _env(monkeypatch, groups=2)
    with _model(dev, FC.case("gru", 33)[0]) as tt:
        _full_forcing_parity(tt, "gru", 33, 2, "gru B=33, two row groups")
        free = _self_replay(tt, 33, 2, "sequential", "two row groups")
    assert len(np.unique(free[32, 80:])) > 10
