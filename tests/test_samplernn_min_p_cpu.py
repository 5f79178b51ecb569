"""The min-p truncated draw of the SampleRNN generator (samplernn_generate_set_min_p, samplernn_generate_set_utterance_min_p),
as far as it can be checked without a GPU: the rule and its composition in the cases module, the premises of the GPU tests'
judging rule (every listed case keeps its margin; the float32 restatement finds the oracle's m and keeps the cap; the exact
cases really are exact), and the interface -- validation, refusals in front of any device call, build_packed_min_p, the
runner contract of StreamingGenerator, the header and the signatures, the flag.  Cases: tests/samplernn_min_p_cases.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import samplernn_min_p_cases as MC
from tests import samplernn_sampling_cases as SC
from tests import samplernn_top_k_cases as KC
from tests import samplernn_top_p_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tt():
    from parrot_amd.sampleRNN.models.conditional import three_tier
    return three_tier


# ---- 1. the rule ----------------------------------------------------------------------------------------------------------------
def test_min_p_rule():
    lg = np.log(np.array([1.0, 4.0, 4.0, 0.5, 4.0, 2.0, 2.0, 0.25], dtype=np.float64)).astype(np.float32)
    # ratios at T = 1: 1/4, 1, 1, 1/8, 1, 1/2, 1/2, 1/16
    for min_p, want in ((1.0, [1, 2, 4]), (0.6, [1, 2, 4]), (0.4, [1, 2, 4, 5, 6]), (0.2, [0, 1, 2, 4, 5, 6]),
                        (0.1, [0, 1, 2, 3, 4, 5, 6]), (0.05, list(range(8)))):
        assert np.nonzero(MC.kept_set(lg, 1.0, min_p=min_p))[0].tolist() == want, min_p
        assert MC.min_p_m(lg, 1.0, min_p) == len(want) >= 1
    # the temperature moves the ratios: at T = 2 they are the square roots
    assert MC.min_p_m(lg, 2.0, 0.6) == 5 and MC.min_p_m(lg, 0.5, 0.2) == 5
    # off: outside (0, 1]
    for min_p in (0.0, -1.0, 1.5):
        assert MC.min_p_m(lg, 1.0, min_p) == 8
    # composition: the shortest of the three prefixes
    assert MC.kept_m(lg, 1.0, k=2, min_p=0.2) == 2 and MC.kept_m(lg, 1.0, k=7, min_p=0.4) == 5
    assert NC.nucleus_m(lg, 1.0, 0.5) == 3 and MC.kept_m(lg, 1.0, p=0.5, min_p=0.2) == 3
    assert NC.nucleus_m(lg, 1.0, 0.95) == 6 and MC.kept_m(lg, 1.0, p=0.95, min_p=0.4) == 5
    assert MC.kept_m(lg, 1.0, k=4, p=0.9, min_p=0.6) == 3
    # the nucleus is found without regard to min_p: of top_k's mass, not of what min-p leaves
    assert NC.nucleus_m(lg, 1.0, 0.7, 5) == 3 and MC.kept_m(lg, 1.0, k=5, p=0.7, min_p=0.05) == 3


def test_every_case_keeps_the_margin():
    assert len(MC.CASES) == 36 and MC.MARGIN == 2.0 ** -18
    closest = min((MC.margin(SC.b4_pattern(pattern), tau, min_p), pattern, tau, min_p) for pattern, tau, min_p in MC.CASES)
    print(f"MINP-CPU closest ratio: {closest[0]:.3e} (relative) at {closest[1:]}")
    assert closest[0] >= 4.2e-5 > MC.MARGIN
    ms = {(pattern, tau, min_p): MC.case_m(SC.b4_pattern(pattern), tau, min_p) for pattern, tau, min_p in MC.CASES}
    assert min(ms.values()) == 1 and max(ms.values()) == 256
    assert [ms[("randn", 1.0, p)] for p in MC.MIN_PS] == [64, 21, 3, 1]
    assert [ms[("flat", tau, 0.98)] for tau in SC.TEMPERATURES] == [4, 38, 205]
    assert all(ms[("flat", tau, p)] == 256 for tau in SC.TEMPERATURES for p in MC.MIN_PS[:3])
    # a bar on top of a ratio is no case, and case_m says so
    b4 = SC.b4_pattern("randn")
    on = float(np.sort(MC.ratios64(b4, 1.0))[-5])
    assert MC.margin(b4, 1.0, on) == 0.0
    with pytest.raises(AssertionError):
        MC.case_m(b4, 1.0, on)


def test_combined_cases():
    cases = MC.combined_cases()
    assert len(cases) == 27      # (none of the listed combinations fails NC.case_m's premise)
    ms = {c: MC.case_m(SC.b4_pattern(c[0]), c[1], MC.COMBINED_MIN_P, c[2], c[3]) for c in cases}
    # each of the three is the binding one somewhere, so the order of application is under test
    assert ms[("randn", 1.0, 64, 0.9)] == 21 and ms[("randn", 2.0, 64, 0.9)] == 52 and ms[("randn", 2.0, 64, 0.0)] == 64
    assert ms[("peaked", 0.5, 0, 0.9)] == 2 and ms[("flat", 1.0, 0, 0.9)] == 230


@pytest.mark.parametrize("mode", MC.MODES)
def test_restatement_finds_the_oracles_m_and_keeps_the_cap(mode):
    """Over every listed case: the float32 compare finds the float64 oracle's m, and the restated draw leaves the oracle's in
    at most EXCUSED_CAP of the draws, only within DELTA / DELTA_SCAN of a boundary, never outside the kept set."""
    worst_frac, worst_dist = 0.0, 0.0
    s = SC.BIAS_SHAPES["persist-D256-B32"]
    u = SC.u01_table(SC.SEEDS[1], s.T, s.B)
    for pattern, tau, min_p in MC.CASES:
        b4 = SC.b4_pattern(pattern)
        m = MC.case_m(b4, tau, min_p)
        assert MC.min_p_m_f32(b4, tau, min_p) == m, (pattern, tau, min_p)
        got = MC.emulate_picks_f32(b4, tau, min_p, u, mode)
        m2, draws, excused, worst = MC.judge_draws(got, b4, tau, min_p, u, mode)
        assert m2 == m and draws == u.size
        worst_frac, worst_dist = max(worst_frac, excused / draws), max(worst_dist, worst)
    print(f"MINP-CPU {mode}: {len(MC.CASES)} cases, worst mismatch fraction {worst_frac:.4%} (cap {SC.EXCUSED_CAP:.1%}), worst "
          f"boundary distance {worst_dist:.2e}")


def test_exact_cases_are_exact():
    # all-equal logits: every float32 term is exactly 1.0, so any active min_p keeps all 256
    b4 = np.full(SC.Q, SC.EDGE_LOGIT, dtype=np.float32)
    for tau in SC.TEMPERATURES:
        e = np.exp((b4 - b4.max()) / np.float32(tau)).astype(np.float32)
        assert (e == 1.0).all()
        for min_p in MC.EXACT_MIN_PS:
            assert MC.min_p_m_f32(b4, tau, min_p) == 256 == MC.min_p_m(b4, tau, min_p)
    # four maxima: their terms are exactly 1.0; every other ratio is below 0.0183, so 0.02 keeps the same four as 1.0
    b4, _ = SC.tie_pattern(MC.FOUR_MAXIMA)
    r = MC.ratios64(b4, 1.0)
    assert np.nonzero(r == 1.0)[0].tolist() == list(MC.FOUR_CODES) and np.sort(r)[-5] < 0.0183
    for min_p in MC.FOUR_MIN_PS:
        assert np.nonzero(MC.kept_set(b4, 1.0, min_p=min_p))[0].tolist() == list(MC.FOUR_CODES)
        assert MC.min_p_m_f32(b4, 1.0, min_p) == 4
    assert MC.margin(b4, 1.0, 0.02) > 0.08
    s = SC.EDGE_SHAPES["launch-D32-B8"]
    for seed in SC.EDGE_SEEDS + tuple(KC.U1_SEEDS):
        u = SC.u01_table(seed, s.T, s.B)
        want4 = MC.four_maxima_picks(u)
        assert set(np.unique(want4).tolist()) <= set(MC.FOUR_CODES)
        for mode in MC.MODES:
            for min_p in MC.FOUR_MIN_PS:
                assert np.array_equal(MC.emulate_picks_f32(b4, 1.0, min_p, u, mode), want4), (seed, mode, min_p)
            flat = np.full(SC.Q, SC.EDGE_LOGIT, dtype=np.float32)
            assert np.array_equal(MC.emulate_picks_f32(flat, 1.0, 0.5, u, mode), MC.equal_logits_picks(u)), (seed, mode)
        if seed in KC.U1_SEEDS:   # a uniform of exactly 1: the fall-through goes to the highest kept code
            b, t = KC.U1_SEEDS[seed]
            assert u[b, t - MC.BFS] == 1.0 and want4[b, t - MC.BFS] == 200
    assert np.array_equal(MC.four_maxima_picks(np.array([0.0, 0.2499, 0.25, 0.5, 0.75, 0.9999, 1.0])),
                          [5, 5, 69, 133, 200, 200, 200])


def test_per_utterance_values_mix():
    n = 12
    mps, ks, ps, temps = MC.utt_min_ps(n), KC.utt_top_ks(n), NC.utt_top_ps(n), KC.utt_temperatures(n)
    assert mps[:4] == list(MC.UTT_MIN_PS) == [0.0, 0.1, 1.0, 0.5]
    combos = {(k > 0, 0.0 < p < 1.0, m > 0) for k, p, m in zip(ks, ps, mps)}
    assert (False, False, False) in combos and any(c[2] and (c[0] or c[1]) for c in combos)
    assert len(set(temps)) == 3


# ---- 2. the interface -----------------------------------------------------------------------------------------------------------
def test_new_names_are_reexported(tt):
    from parrot_amd.sampleRNN.generation import inputs
    for name in ("build_packed_min_p", "min_p_code", "min_p_array", "min_p_active", "_per_utterance_min_p"):
        assert getattr(tt, name) is getattr(inputs, name), name


def test_min_p_values(tt):
    assert tt.min_p_code(0) == 0.0 and tt.min_p_code(0.0) == 0.0 and tt.min_p_code(1) == 1.0 and tt.min_p_code(1.0) == 1.0
    assert tt.min_p_code(0.1) == float(np.float32(0.1)) and tt.min_p_code(np.float32(0.25)) == 0.25
    assert 0.0 < tt.min_p_code(1e-60) < 1e-30                       # a positive value below float32's normal range stays active
    assert [tt.min_p_active(p) for p in (0, 0.0, 1e-60, 0.5, 1.0, 1)] == [False, False, True, True, True, True]
    for bad in (-0.5, -1, 1.5, 2, 1.0000001, float("inf"), float("nan"), np.float32("nan"), float("-inf"), "0.1", None, True, [0.5]):
        with pytest.raises(ValueError):
            tt.min_p_code(bad)
        if not isinstance(bad, list):
            with pytest.raises(ValueError):
                tt.min_p_active(bad)
    a = tt.min_p_array([[0, 0.5], [1.0, 1e-60]], (2, 2))
    assert a.dtype == np.float32 and a[0].tolist() == [0.0, 0.5] and a[1, 0] == 1.0 and 0.0 < a[1, 1] < 1e-30
    assert tt.min_p_array(np.array([0, 1]), (2,)).tolist() == [0.0, 1.0]
    for bad, shape in (([[0, -0.1]], (1, 2)), ([0, 1], (1, 2)), ([[0.5, float("nan")]], (1, 2)), ([[0, 1]], (2, 1)),
                       ([["a", "b"]], (1, 2)), ([[0.5, 1.5]], (1, 2))):
        with pytest.raises(ValueError):
            tt.min_p_array(bad, shape)
    assert tt._per_utterance_min_p(None, 3, 0.5) == [0.5] * 3 and tt._per_utterance_min_p([0.25, 0, 1], 3, 0.5) == [0.25, 0.0, 1.0]
    assert tt._per_utterance_min_p(0.25, 2, 0.5) == [0.25, 0.25]
    with pytest.raises(ValueError):
        tt._per_utterance_min_p([0.5, 0.5], 3, 0)
    with pytest.raises(ValueError):
        tt._per_utterance_min_p([0.5, -0.5, 0.5], 3, 0)
    with pytest.raises(ValueError):
        tt._per_utterance_min_p([0.5, 1.5, 0.5], 3, 0)


def test_build_packed_min_p(tt):
    from parrot_amd.sampleRNN.generation import inputs
    T = 4
    for s in range(T):
        got = tt.build_packed_min_p([0.5], [0], [s], T, 2)
        row = inputs.start_row(s, T)
        want = np.zeros((T, 2), dtype=np.float32)
        if row is not None:
            want[row, 0] = 0.5
        assert got.dtype == np.float32 and np.array_equal(got, want)
    assert tt.build_packed_min_p([1.0, 0.0], [0, 1], [0, 0], T, 2)[inputs.start_row(0, T)].tolist() == [1.0, 0.0]
    assert tt.build_packed_top_p([0.5], [0], [0], T, 2).dtype == np.float32    # its sibling keeps its signature and result
    with pytest.raises(ValueError):
        tt.build_packed_min_p([0.5], [2], [0], T, 2)
    with pytest.raises(ValueError):
        tt.build_packed_min_p([-0.5], [0], [0], T, 2)
    with pytest.raises(ValueError):
        tt.build_packed_min_p([1.5], [0], [0], T, 2)


def test_refusals_come_before_any_device_call(tt, monkeypatch):
    from parrot_amd import _lib
    from parrot_amd.sampleRNN import lib
    from parrot_amd.sampleRNN.generation.device import device_loop_guard

    def no_device(*a, **k):
        raise AssertionError("a device call in front of the min_p check")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(lib, "device", no_device)
    feats = np.zeros((3, 2, 63), dtype=np.float32)
    assert inspect.signature(device_loop_guard).parameters["min_p"].default == 0.0
    assert device_loop_guard("sequential", 0, 0.0, 1.0) == 0 and device_loop_guard("scan", min_p=0.1) == 1
    for bad in (-0.5, 1.5, float("nan"), "0.1", None):
        with pytest.raises(ValueError):
            device_loop_guard("sequential", 0, 0.0, bad)
        with pytest.raises(ValueError):
            tt.DeviceGenerator(2, 3, min_p=bad)
        with pytest.raises(ValueError):
            tt.generate_packed([feats[:, 0]], n_streams=2, min_p=bad)
        with pytest.raises(ValueError):
            next(tt.generate_stream(feats, 2, min_p=bad))
        with pytest.raises(ValueError):
            tt.StreamingGenerator(2, 2, min_p=bad)
        with pytest.raises(ValueError):
            tt.generate_and_save_samples("t", features=feats, min_p=bad)
    with pytest.raises(ValueError):                             # per-utterance values need per-utterance seeds
        tt.generate_packed([feats[:, 0]], n_streams=2, min_ps=[0.5])
    with pytest.raises(ValueError):
        tt.generate_packed([feats[:, 0]], n_streams=2, seeds=[5], min_ps=[0.5, 0.5])
    with pytest.raises(ValueError):
        tt.generate_packed([feats[:, 0]], n_streams=2, seeds=[5], min_ps=[1.5])
    for active in (0.1, 1.0, 1e-60):                            # the literal three-function loop draws among all codes
        with pytest.raises(ValueError):
            tt.generate_and_save_samples("t", features=feats, use_device_loop=False, min_p=active)


def _bare_plan(tt, packed, utterance_draws, B=2, T=3):
    """A DeviceGenerator without a device behind it: what generate() checks before it stages anything."""
    gen = object.__new__(tt.DeviceGenerator)
    gen.B, gen.T, gen.packed, gen.utterance_draws, gen._has_run = B, T, packed, utterance_draws, False
    gen.top_k, gen.top_p, gen.min_p = 0, 0.0, 0.0
    return gen


def test_generate_refuses_min_ps_in_front_of_the_device(tt, monkeypatch):
    from parrot_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("a device call in front of the min_ps check")
    monkeypatch.setattr(_lib, "call", no_device)
    feats = np.zeros((3, 2, 63), dtype=np.float32)
    starts = np.zeros((3, 2), dtype=np.int32)
    sd, tp = np.zeros((3, 2), dtype=np.uint64), np.ones((3, 2), dtype=np.float32)
    with pytest.raises(ValueError):                             # no utterance_draws: no min_ps
        _bare_plan(tt, False, False).generate(feats, min_ps=[0.5, 0.5])
    with pytest.raises(ValueError):
        _bare_plan(tt, True, False).generate(feats, starts, min_ps=np.zeros((3, 2), dtype=np.float32))
    plain, packed = _bare_plan(tt, False, True), _bare_plan(tt, True, True)
    for bad in ([0.5], [[0.5, 0.5]], [0.5, -0.1], [0.5, 1.5], [0.5, float("nan")], -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            plain.generate(feats, seeds=[1, 2], temperatures=1.0, min_ps=bad)
    for bad in ([0.5, 0.5], np.zeros((2, 2), dtype=np.float32), np.full((3, 2), -0.5), np.full((3, 2), 1.5), np.full((3, 2), np.nan)):
        with pytest.raises(ValueError):
            packed.generate(feats, starts, seeds=sd, temperatures=tp, min_ps=bad)
    plain._has_run = True                                       # a plain plan takes them with resume=False only, like seeds
    with pytest.raises(ValueError):
        plain.generate(feats[:2], resume=True, n_frames=2, min_ps=[0.5, 0.5])


def test_submit_takes_a_min_p_with_utterance_draws_only(tt):
    runner = lambda features, starts, resume, **kw: np.zeros((2, 80 * features.shape[0]), dtype=np.int32)
    utt = np.zeros((2, 63), dtype=np.float32)
    off = tt.StreamingGenerator(2, 2, run_segment=runner)
    with pytest.raises(ValueError):
        off.submit(utt, min_p=0.5)
    on = tt.StreamingGenerator(2, 2, run_segment=runner, utterance_draws=True)
    for bad in (-0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            on.submit(utt, seed=1, min_p=bad)
    with pytest.raises(ValueError):
        on.submit(utt, min_p=0.5)                                # the seed is still required
    assert on.submit(utt, seed=1, min_p=0.5) == 0


def test_runner_contract(tt):
    """A runner of the caller's sees min_ps only when the generator uses min-p: its min_p is active, or some utterance was
    submitted with one.  Otherwise it is called as before."""
    seen = []
    zeros = lambda features: np.zeros((2, 80 * features.shape[0]), dtype=np.int32)

    def three(features, starts, resume):
        seen.append(())
        return zeros(features)

    def seven(features, starts, resume, seeds=None, temperatures=None, top_ks=None, top_ps=None):
        seen.append((top_ks, top_ps))
        return zeros(features)

    def eight(features, starts, resume, seeds=None, temperatures=None, top_ks=None, top_ps=None, min_ps=None):
        seen.append((starts.copy(), seeds, temperatures, top_ks, top_ps, min_ps))
        return zeros(features)

    utt = np.zeros((3, 63), dtype=np.float32)
    for off in ({}, dict(min_p=0.0), dict(min_p=0)):            # off: the runner never sees the keyword
        sg = tt.StreamingGenerator(2, 2, run_segment=three, **off)
        sg.submit(utt)
        assert sg.drain() and seen
        sg = tt.StreamingGenerator(2, 2, run_segment=seven, utterance_draws=True, top_p=0.5, top_k=8, **off)
        sg.submit(utt, seed=7)
        assert sg.drain() and seen[-1][0] is not None and seen[-1][1] is not None
    # the generator's own min_p, without per-utterance draws: min_ps on the start rows, nothing else
    del seen[:]
    sg = tt.StreamingGenerator(2, 2, run_segment=eight, min_p=1.0)
    sg.submit(utt)
    sg.submit(utt[:2])
    assert sg.drain()
    for starts, sd, tp, tk, pp, mp in seen:
        assert sd is None and tp is None and tk is None and pp is None and mp.dtype == np.float32 and mp.shape == starts.shape
        assert np.array_equal(mp, np.where(starts != 0, np.float32(1.0), np.float32(0)))
    assert sum(int((s[0] != 0).sum()) for s in seen) == 2
    # per utterance: one submitted with a min_p switches the keyword on; the others take the generator's (here 0)
    del seen[:]
    sg = tt.StreamingGenerator(2, 2, run_segment=eight, utterance_draws=True)
    sg.submit(utt, seed=7)
    assert sg.step() and seen[-1][5] is None
    sg.submit(utt, seed=8, min_p=0.25)
    sg.submit(utt, seed=9, temperature=0.5)
    assert sg.drain()
    got = np.concatenate([mp[starts != 0] for starts, _, _, _, _, mp in seen[1:]])
    assert all(mp is not None and mp.dtype == np.float32 and tk is None and pp is None for _, _, _, tk, pp, mp in seen[1:])
    assert sorted(got.tolist()) == [0.0, 0.25], got


def test_keyword_is_everywhere_top_p_is(tt):
    from parrot_amd.model import SampleRnn
    for fn, names in ((tt.DeviceGenerator.__init__, ("top_p", "min_p")), (tt.DeviceGenerator.generate, ("top_ps", "min_ps")),
                      (tt.generate_packed, ("top_p", "top_ps", "min_p", "min_ps")), (tt.generate_stream, ("top_p", "min_p")),
                      (tt.StreamingGenerator.__init__, ("top_p", "min_p")), (tt.StreamingGenerator.submit, ("top_p", "min_p")),
                      (tt.generate_and_save_samples, ("top_p", "min_p")), (SampleRnn.sample_raw, ("top_p", "min_p"))):
        params = inspect.signature(fn).parameters
        for name in names:
            assert name in params, (fn.__qualname__, name)
    for fn in (tt.DeviceGenerator.__init__, tt.generate_packed, tt.generate_stream, tt.StreamingGenerator.__init__):
        assert inspect.signature(fn).parameters["min_p"].default == 0.0


def test_header_and_signatures():
    from parrot_amd import _lib
    txt = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    assert re.search(r"int samplernn_generate_set_min_p\(void\* plan, float min_p\);", txt)
    assert re.search(r"int samplernn_generate_set_utterance_min_p\(void\* plan, const float\* utt_min_p\);", txt)
    for phrase in ("e_q >= min_p", "temperature -> top-k -> top-p -> min-p", "a draw with top_k = m", "the highest kept code"):
        assert phrase in txt, phrase
    assert _lib.SIGNATURES["samplernn_generate_set_min_p"] == (C.c_int, [C.c_void_p, C.c_float])
    assert _lib.SIGNATURES["samplernn_generate_set_utterance_min_p"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert C.sizeof(_lib.SampleRnnGenDesc) == 936               # the descriptor did not grow: min_p arrives by the setters
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "samplernn_generate_set_min_p" in doc and "samplernn_generate_set_utterance_min_p" in doc


def test_c_entries_refuse_bad_arguments_without_a_device():
    from parrot_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 4)()
    assert lib.samplernn_generate_set_min_p(None, C.c_float(0.5)) == 10001                 # PARROT_ERR_BADARG, no device call
    assert lib.samplernn_generate_set_utterance_min_p(None, C.addressof(buf)) == 10001
    assert lib.samplernn_generate_set_utterance_min_p(C.addressof(buf), None) == 10001    # (the plan is only looked at after the pointer)


def test_parser_has_the_flag():
    from parrot_amd import utils
    from parrot_amd.utils import sample_parse
    assert sample_parse([]).min_p == 0.0
    assert sample_parse(['--min_p', '0.1']).min_p == 0.1
    args = sample_parse(['--min_p', '0.1', '--top_p', '0.9', '--top_k', '64'])
    assert (args.top_k, args.top_p, args.min_p) == (64, 0.9, 0.1)
    with pytest.raises(SystemExit):
        sample_parse(['--min_p', 'some'])
    assert "--min_p" in utils.__doc__


def test_sample_raw_refuses_a_bad_min_p(tt):
    from parrot_amd.model import SampleRnn
    m = object.__new__(SampleRnn)      # (no parameters, no device: the check comes first)
    m.three_tier = tt
    for bad in (-0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            m.sample_raw(None, None, "t", None, min_p=bad)
